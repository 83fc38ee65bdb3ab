"""External wrenches on bodies (he_apply_body_forces, he_apply_body_forces_at_pos) on the
GPU. The fp64 oracle cannot apply a wrench, so the feature is held to it through equivalences that
only the wrench-free kernels and the oracle define:

1. forces m_b a on every body equal gravity g + a, in flight (no contacts) ...
2. ... and standing on 16 contacts;
3. one step's velocity change equals dt A^-1 Q, with Q from finite-difference Jacobians of a numpy
   forward kinematics (tests/test_independent_dynamics.py) and A from the oracle's CRBA;
4. the call semantics (accumulate, clear, hold, the wrench-free kernels afterwards, invalid calls);
5. the gym facade and the env's push option.
Every yardstick is the wrench-free engine's own error against the same reference, measured in the
same test; the measured figures are printed before each assertion and quoted beside it."""
import ctypes as C
import os

import numpy as np
import pytest

from humanoid_amd import _abi
from humanoid_amd.body_sets import BODY_NAMES
from oracle import oracle as O

import cases
from test_independent_dynamics import Body, _jacobians

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NB, ND, NG = 24, 69, 75
ENV, LOCAL, GLOBAL = _abi.SPACE_ENV, _abi.SPACE_LOCAL, _abi.SPACE_GLOBAL
G32 = np.float32(-9.81)


def cu(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    return t if dtype is None else t.to(dtype)


def make_engine(he_model, n, sp):
    from humanoid_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(he_model, n, device=0, sim_params=sp)


def load(eng, root, dof, targets, rb=None):
    n = root.shape[0]
    eng.root_states.copy_(cu(root))
    eng.dof_state.copy_(cu(dof.reshape(n * ND, 2)))
    eng.dof_targets.copy_(cu(targets))
    if rb is not None:
        eng.rb_state.copy_(cu(rb.reshape(n * NB, 13)))


def snap(eng):
    torch.cuda.synchronize()
    return tuple(getattr(eng, k).clone() for k in ("root_states", "dof_state", "rb_state", "contact_forces", "dof_force",
                                                   "contact_cache"))


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def masses(he_model):
    return np.array(he_model.mass[:NB], np.float64)


def shifted_gravity(a):
    """Gravity g + a as the engine holds it (fp32), and the a that makes it exact: the forces are
    formed from gB - gA, so that both sides are the same problem in real arithmetic."""
    gA = np.array([0.0, 0.0, G32], np.float64)
    gB = (gA + np.asarray(a, np.float64)).astype(np.float32)
    return gB, gB.astype(np.float64) - gA


def traj_err(model, eng, d_o, rb_o):
    """Largest joint-angle distance (rad) and CoM distance (m) of the engine's state to the oracle's."""
    n = d_o.shape[0]
    dg = eng.dof_state.view(n, ND, 2).cpu().numpy()
    rbg = eng.rb_state.view(n, NB, 13).cpu().numpy()
    e_q = np.abs(dg[..., 0].astype(np.float64) - d_o[..., 0]).max()
    e_c = np.linalg.norm(cases.center_of_mass(model, rbg) - cases.center_of_mass(model, rb_o), axis=-1).max()
    return max(float(e_q), float(e_c))


SOLVERS = {
    "tgs": lambda **kw: _abi.default_sim_params(**kw),
    "pgs": lambda **kw: _abi.pgs_sim_params(**kw),
    "pgs_explicit": lambda **kw: _abi.pgs_sim_params(bias_midpoint=0, **kw),
}


# ------------------------------------------------------------------ 1. extra gravity, in flight
@pytest.mark.parametrize("solver", ["tgs", "pgs", "pgs_explicit"])
def test_forces_equal_extra_gravity_in_flight(he_model, model, solver):
    """f_b = m_b ms_b a on every body (ENV_SPACE, hold 2, re-applied before each of 10 policy steps)
    against gravity g + a without a wrench, both against the fp64 oracle at g + a: 32 tumbling
    bodies in flight with PD drives holding their initial angles, mass_scale on half the envs (the
    force carries it explicitly: the engine does not scale a wrench). The wrench reaches the
    right-hand side through one more fp32 chain of about the gravity bias's length, hence 2 x.
    Measured on the MI355X (wrench / yardstick, the larger of rad and m over all 10 steps): TGS
    2.146e-6 / 2.147e-6, PGS 1.058e-6 / 1.058e-6, PGS without the midpoint bias 1.440e-6 / 1.441e-6."""
    n = 32
    rng = np.random.default_rng(41)
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), vel=0.5, ang=0.5, tilt=0.8)
    targets = dof[..., 0].copy()
    ms = np.ones((n, NB), np.float32)
    ms[::2] = rng.uniform(0.8, 1.2, (n // 2, NB)).astype(np.float32)
    gB, a = shifted_gravity((1.5, -0.7, 3.0))
    kw = dict(self_collision=0, joint_limits=0)
    spA, spB = SOLVERS[solver](**kw), SOLVERS[solver](**kw)
    spB.gravity[:] = [float(x) for x in gB]
    f = cu((masses(he_model)[None, :, None] * ms.astype(np.float64)[:, :, None] * a[None, None, :]).astype(np.float32))
    A, B = make_engine(he_model, n, spA), make_engine(he_model, n, spB)
    ms_t = cu(ms)
    for eng in (A, B):
        eng.set_env_properties(mass_scale=ms_t)
        load(eng, root, dof, targets)
    r_o, d_o, c_o = root.copy(), dof.copy(), O.new_cache(n)
    eA = eB = 0.0
    for _ in range(10):
        A.apply_body_forces(force=f, space=ENV, hold=2)
        A.simulate(2)
        B.simulate(2)
        out = O.physics_step(he_model, spB, r_o, d_o, targets, 2, mass_scale=ms, cache=c_o)
        torch.cuda.synchronize()
        assert int(A.num_contacts.max()) == 0 and int(B.num_contacts.max()) == 0 and out["num_contacts"].max() == 0
        eA = max(eA, traj_err(model, A, d_o, out["rb_state"]))
        eB = max(eB, traj_err(model, B, d_o, out["rb_state"]))
    print(f"\nflight {solver}: wrench {eA:.3e}  extra gravity (yardstick) {eB:.3e}")
    assert eB < 1e-4 and eA < 1e-4
    assert eA <= 2.0 * eB + 1e-6


# ------------------------------------------------------------------ 2. extra gravity, standing
@pytest.fixture(scope="module")
def standing_case(he_model, model):
    """8 standing bodies, default TGS, 30 policy steps at gravity -9.81 + 2: the oracle's trajectory and
    the wrench-free engine's error against it (the yardstick of test 2 and of the zero wrench)."""
    n = 8
    root, dof = cases.standing_state(model, n, np.random.default_rng(4), xy_jitter=1.0)
    targets = np.zeros((n, ND), np.float32)
    gB, a = shifted_gravity((0.0, 0.0, 2.0))
    spB = _abi.default_sim_params()
    spB.gravity[:] = [float(x) for x in gB]
    B = make_engine(he_model, n, spB)
    load(B, root, dof, targets)
    r_o, d_o, c_o = root.copy(), dof.copy(), O.new_cache(n)
    traj, eB = [], 0.0
    for _ in range(30):
        B.simulate(2)
        out = O.physics_step(he_model, spB, r_o, d_o, targets, 2, cache=c_o)
        torch.cuda.synchronize()
        traj.append((d_o.copy(), out["rb_state"].copy(), out["num_contacts"].copy()))
        eB = max(eB, traj_err(model, B, d_o, out["rb_state"]))
    return dict(n=n, root=root, dof=dof, targets=targets, a=a, traj=traj, eB=eB)


def test_forces_equal_extra_gravity_standing(he_model, model, standing_case):
    """f_b = m_b (0, 0, 2) re-applied each step on bodies standing on their 16 contacts at g, against
    the oracle at -7.81 (every env keeps its 16 contacts throughout, none is left out) and against
    the wrench-free engine at -7.81 by the same 2 x rule.
    Measured on the MI355X (the larger of rad and m over all 30 steps): wrench 5.500e-6, yardstick
    4.129e-6."""
    c = standing_case
    n = c["n"]
    A = make_engine(he_model, n, _abi.default_sim_params())
    load(A, c["root"], c["dof"], c["targets"])
    f = cu(np.broadcast_to((masses(he_model)[:, None] * c["a"][None, :]).astype(np.float32), (n, NB, 3)))
    eA = 0.0
    for d_o, rb_o, nc_o in c["traj"]:
        A.apply_body_forces(force=f, space=ENV, hold=2)
        A.simulate(2)
        torch.cuda.synchronize()
        assert (nc_o == 16).all() and (A.num_contacts.cpu().numpy() == 16).all()
        eA = max(eA, traj_err(model, A, d_o, rb_o))
    print(f"\nstanding: wrench {eA:.3e}  extra gravity (yardstick) {c['eB']:.3e}")
    assert eA < 1e-4 and c["eB"] < 1e-4
    assert eA <= 2.0 * c["eB"] + 1e-6


# ------------------------------------------------------------------ 3. dt A^-1 Q
KW3 = dict(substeps=1, angular_damping=0.0, joint_limits=0, self_collision=0, kd_scale=0.0)
SOLVERS3 = {
    "pgs_explicit": lambda **kw: _abi.pgs_sim_params(bias_midpoint=0, **kw),
    "pgs": lambda **kw: _abi.pgs_sim_params(**kw),
    "tgs4": lambda **kw: _abi.default_sim_params(solver_iterations=4, **kw),
}
BODIES3 = ("Pelvis", "Torso", "L_Knee", "Head", "R_Hand")


@pytest.fixture(scope="module")
def rest_case(he_model):
    """6 bodies at rest in flight, their rigid-body rows, the oracle's joint-space inertia and the
    finite-difference Jacobians of the independent numpy kinematics."""
    n = 6
    root, dof = cases.random_state(n, np.random.default_rng(7), height=(3.0, 4.0), vel=0.5, ang=0.5, tilt=0.8)
    root[:, 7:] = 0.0
    dof[..., 1] = 0.0
    rb = O.forward_kinematics(he_model, root, dof)
    H, _ = O.dynamics_terms(he_model, _abi.default_sim_params(), root, dof)
    arm = np.concatenate([np.zeros(6), np.array(he_model.armature[:ND], np.float64)])
    Bm = Body(he_model)
    jac = [_jacobians(Bm, root[e], dof[e]) for e in range(n)]
    R = cases._qmat(rb[..., 3:7])                                          # [n,24,3,3]
    com = rb[..., :3].astype(np.float64) + np.einsum("nbij,bj->nbi", R, Bm.com)  # world CoMs
    return dict(n=n, root=root, dof=dof, rb=rb, H=H, arm=arm, jac=jac, R=R, com=com)


def _velocity_after(he_model, sp, c, targets, apply=None):
    """Generalized velocity [n,75] (root w, root v, joint rates) after one simulate() from rest."""
    n = c["n"]
    eng = make_engine(he_model, n, sp)
    load(eng, c["root"], c["dof"], targets, rb=c["rb"])
    if apply is not None:
        apply(eng)
    eng.simulate(1)
    torch.cuda.synchronize()
    r = eng.root_states.cpu().numpy().astype(np.float64)
    d = eng.dof_state.view(n, ND, 2).cpu().numpy().astype(np.float64)
    return np.concatenate([r[:, 10:13], r[:, 7:10], d[..., 1]], axis=1)


def _predict(c, dt, Q, diag=None):
    out = np.zeros_like(Q)
    for e in range(c["n"]):
        A = c["H"][e] + np.diag(c["arm"] + (0.0 if diag is None else diag))
        out[e] = dt * np.linalg.solve(A, Q[e])
    return out


_yard3 = {}


def _drive_yardstick(he_model, c, solver):
    """The wrench-free kernels on the same formula: kp_scale 1e-6, target offsets U(-400, 400) rad
    give Q_i = kp_i dtgt_i on the joint dofs (hs coef on A's diagonal). Relative error of the
    step's velocity change, largest |du - pred| over largest |pred| (fp64 oracle: 3e-6 .. 1.2e-5)."""
    if solver not in _yard3:
        sp = SOLVERS3[solver](kp_scale=1e-6, **KW3)
        dt = sp.dt / sp.substeps
        hs = dt / sp.solver_iterations if sp.solver_type == 1 else dt
        off = np.random.default_rng(17).uniform(-400.0, 400.0, (c["n"], ND))
        q = c["dof"][..., 0]
        kp = np.array(he_model.stiffness[:ND], np.float64) * 1e-6
        du = (_velocity_after(he_model, sp, c, (q + off).astype(np.float32))
              - _velocity_after(he_model, sp, c, q.copy()))
        dq = (q + off).astype(np.float32).astype(np.float64) - q  # the offsets as fp32 targets hold them
        Q = np.concatenate([np.zeros((c["n"], 6)), kp[None, :] * dq], axis=1)
        pred = _predict(c, dt, Q, diag=np.concatenate([np.zeros(6), hs * hs * kp]))
        _yard3[solver] = float(np.abs(du - pred).max() / np.abs(pred).max())
    return _yard3[solver]


@pytest.mark.parametrize("kind", ["env", "local", "at_pos"])
@pytest.mark.parametrize("solver", ["pgs_explicit", "pgs", "tgs4"])
def test_one_step_velocity_change_is_dt_Ainv_Q(he_model, rest_case, solver, kind):
    """du = u(with the wrench) - u(without) after one physics step from rest equals dt A^-1 Q with
    A = H + diag(armature) (the oracle's CRBA) and Q = sum_b Jv_b^T f_b + Jo_b^T tau_b (independent
    finite-difference Jacobians). Envs 0-4: a wrench on one body (Pelvis, Torso, L_Knee, Head,
    R_Hand); env 5: on every body; each env's scaled to a predicted largest |du| of 0.2 rad/s. Inputs:
    ENV force + torque; LOCAL force + torque (the prediction rotates them by the body's rotation);
    force at a point (the prediction adds (x - c) x f). The wrench also crosses s x f and a subtree
    sum that a joint torque does not, hence 4 x the drive yardstick's relative error.
    Measured on the MI355X, relative error of the wrench (env / local / at_pos) against the yardstick:
    PGS without the midpoint bias 1.82e-5 / 1.88e-5 / 1.62e-5 against 3.32e-5; PGS 8.59e-4 / 7.42e-4 /
    1.44e-3 against 4.44e-4; TGS 4.29e-4 / 3.72e-4 / 7.20e-4 against 2.25e-4 (with the midpoint bias
    both sides carry the velocity-product terms of a 0.2 rad/s change, which the linear prediction
    leaves out)."""
    c = rest_case
    n = c["n"]
    sp = SOLVERS3[solver](kp_scale=0.0, **KW3)
    dt = sp.dt / sp.substeps
    rng = np.random.default_rng(23)
    f = np.zeros((n, NB, 3))
    t = np.zeros((n, NB, 3))
    offs = rng.uniform(-0.1, 0.1, (n, NB, 3))
    for e in range(n):
        bodies = [BODY_NAMES.index(BODIES3[e])] if e < len(BODIES3) else list(range(NB))
        f[e, bodies] = rng.normal(size=(len(bodies), 3))
        t[e, bodies] = 0.1 * rng.normal(size=(len(bodies), 3))
    R = c["R"]
    if kind == "env":
        fw, tw = f, t
    elif kind == "local":
        fw, tw = np.einsum("nbij,nbj->nbi", R, f), np.einsum("nbij,nbj->nbi", R, t)
    else:
        fw, tw = f, np.cross(offs, f)

    def gen_force(fw, tw):
        return np.stack([sum(c["jac"][e][0][b].T @ fw[e, b] + c["jac"][e][1][b].T @ tw[e, b] for b in range(NB))
                         for e in range(n)])

    scale = 0.2 / np.abs(_predict(c, dt, gen_force(fw, tw))).max(axis=1)  # per env
    f32_ = lambda x: (x * scale[:, None, None]).astype(np.float32)  # noqa: E731
    f_in, t_in = f32_(f), f32_(t)
    x_in = (c["com"] + offs).astype(np.float32)
    # the prediction from the inputs as fp32 holds them
    f64, t64 = f_in.astype(np.float64), t_in.astype(np.float64)
    if kind == "env":
        Q = gen_force(f64, t64)
    elif kind == "local":
        Q = gen_force(np.einsum("nbij,nbj->nbi", R, f64), np.einsum("nbij,nbj->nbi", R, t64))
    else:
        Q = gen_force(f64, np.cross(x_in.astype(np.float64) - c["com"], f64))
    pred = _predict(c, dt, Q)

    def apply(eng):
        if kind == "at_pos":
            eng.apply_body_forces_at_pos(cu(f_in), cu(x_in), space=ENV)
        else:
            eng.apply_body_forces(force=cu(f_in), torque=cu(t_in), space=ENV if kind == "env" else LOCAL)

    q = c["dof"][..., 0].copy()
    du = _velocity_after(he_model, sp, c, q, apply) - _velocity_after(he_model, sp, c, q)
    rel = float(np.abs(du - pred).max() / np.abs(pred).max())
    yard = _drive_yardstick(he_model, c, solver)
    print(f"\ndt A^-1 Q {solver} {kind}: wrench {rel:.3e}  drive yardstick {yard:.3e}  (largest |pred| "
          f"{np.abs(pred).max():.3f} rad/s)")
    assert abs(np.abs(pred).max() - 0.2) < 1e-3
    assert rel <= 4.0 * yard


# ------------------------------------------------------------------ 4. semantics
def _standing(he_model, model, n=8, **kw):
    root, dof = cases.standing_state(model, n, np.random.default_rng(4), xy_jitter=1.0)
    eng = make_engine(he_model, n, _abi.default_sim_params(**kw))
    load(eng, root, dof, np.zeros((n, ND), np.float32))
    return eng


def _torso_push(n, newtons=300.0):
    f = torch.zeros(n, NB, 3, device="cuda:0")
    f[:, BODY_NAMES.index("Torso"), 0] = newtons
    return f


def test_apply_then_clear_runs_the_wrench_free_step(he_model, model):
    a, b = _standing(he_model, model), _standing(he_model, model)
    a.apply_body_forces(force=_torso_push(8), torque=_torso_push(8, 20.0), hold=3)
    a.clear_body_forces()
    for _ in range(5):
        a.simulate(2)
        b.simulate(2)
    assert same_bits(snap(a), snap(b))


def test_hold_counts_simulate_calls(he_model, model):
    """hold = 1 (Isaac Gym's rule): simulate(2) applies the wrench in its first simulate() only, the
    bits of simulate(1) twice; hold = 2 differs."""
    outs = []
    for hold, calls in ((1, (2,)), (1, (1, 1)), (2, (2,))):
        eng = _standing(he_model, model)
        eng.apply_body_forces(force=_torso_push(8), hold=hold)
        for k in calls:
            eng.simulate(k)
        outs.append(snap(eng))
    assert same_bits(outs[0], outs[1])
    assert not torch.equal(outs[0][0], outs[2][0])


def test_used_up_wrench_leaves_the_wrench_free_kernels(he_model, model):
    """After the hold is used up the engine steps as a second engine does that is loaded with its state
    and contact cache and never saw a wrench."""
    a = _standing(he_model, model)
    a.apply_body_forces(force=_torso_push(8), hold=2)
    a.simulate(2)
    s = snap(a)
    b = _standing(he_model, model)
    b.root_states.copy_(s[0])
    b.dof_state.copy_(s[1])
    b.contact_cache.copy_(s[5])
    for _ in range(3):
        a.simulate(2)
        b.simulate(2)
    assert not torch.equal(s[0], a.root_states)
    assert same_bits(snap(a), snap(b))


def test_calls_accumulate(he_model, model):
    n = 8
    rng = np.random.default_rng(5)
    f1, t1, f2 = (cu(rng.normal(0, s, (n, NB, 3)).astype(np.float32)) for s in (20.0, 2.0, 20.0))
    a, b, none = _standing(he_model, model), _standing(he_model, model), _standing(he_model, model)
    a.apply_body_forces(force=f1, torque=t1, hold=2)
    a.apply_body_forces(force=f2, hold=2)
    b.apply_body_forces(force=f1 + f2, torque=t1, hold=2)
    for eng in (a, b, none):
        eng.simulate(2)
    sa, sb, sn = snap(a), snap(b), snap(none)
    assert not torch.equal(sa[1], sn[1])
    for x, y in zip(sa[:3], sb[:3]):
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())


def test_zero_wrench_stays_within_the_standing_yardstick(he_model, model, standing_case):
    n = 8
    a, b = _standing(he_model, model), _standing(he_model, model)
    a.apply_body_forces(force=torch.zeros(n, NB, 3, device="cuda:0"), torque=torch.zeros(n * NB, 3, device="cuda:0"), hold=2)
    a.simulate(2)
    b.simulate(2)
    torch.cuda.synchronize()
    d = traj_err(model, a, b.dof_state.view(n, ND, 2).cpu().numpy().astype(np.float64),
                 b.rb_state.view(n, NB, 13).cpu().numpy())
    print(f"\nzero wrench against none: {d:.3e}  (standing yardstick {standing_case['eB']:.3e})")
    assert d <= standing_case["eB"]  # measured 0 (the same bits) against 4.129e-6


def _env_step_run(he_model, model, golden, fused, steps=4, legs=None):
    from humanoid_amd.model import pd_action_offset_scale
    from test_gpu_parity import tables_from_golden
    g = golden("env_step")
    n = 24
    if legs is not None:
        os.environ["HE_TGS_LEGS"] = legs
    try:
        eng = make_engine(he_model, n, _abi.default_sim_params())
    finally:
        os.environ.pop("HE_TGS_LEGS", None)
    eng.set_fused_step(fused)
    eng.load_motions(tables_from_golden(g))
    off, sc = pd_action_offset_scale(model)
    eng.set_pd_params(off, sc, None)
    root, _ = cases.standing_state(model, n)
    eng.root_states.copy_(cu(root))
    st = cu(g["start_times"]); so = torch.zeros(n, device="cuda:0"); go = torch.zeros(n, 3, device="cuda:0")
    prog = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    em = eng.env_motion(torch.arange(n, device="cuda:0"), st, so, go, prog)
    bufs = [torch.zeros(n, 934, device="cuda:0"), torch.zeros(n, device="cuda:0"), torch.zeros(n, 5, device="cuda:0"),
            torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.uint8, device="cuda:0")]
    rng = np.random.default_rng(31)
    push = _torso_push(n)
    for k in range(steps):
        a = cu(rng.uniform(-0.3, 0.3, (n, 69)).astype(np.float32))
        eng.apply_body_forces(force=push, hold=2)
        eng.env_step(_abi.imitation_params(), em, a, *bufs, seed=7, step_index=k)
    return snap(eng) + tuple(b.clone() for b in bufs)


def test_env_step_with_a_wrench_fused_equals_two_launches(he_model, model, golden):
    assert same_bits(_env_step_run(he_model, model, golden, 1), _env_step_run(he_model, model, golden, 0))


def test_leg_class_with_a_wrench_leaves_the_step_unchanged(he_model, model, golden):
    assert same_bits(_env_step_run(he_model, model, golden, 1, legs="0"), _env_step_run(he_model, model, golden, 1, legs="1"))


def test_invalid_calls_are_refused_with_a_reason(he_model, model):
    from humanoid_amd.engine import EngineError, load_library
    eng = _standing(he_model, model)
    f = _torso_push(8)
    for call, reason in (
            (lambda: eng.apply_body_forces(force=f, space=3), "space"),
            (lambda: eng.apply_body_forces(force=f, space=-1), "space"),
            (lambda: eng.apply_body_forces(force=f, hold=0), "hold"),
            (lambda: eng.apply_body_forces_at_pos(f, None), "both"),
            (lambda: eng.apply_body_forces_at_pos(None, f), "both"),
            (lambda: eng.apply_body_forces(force=f[:, :5]), "contiguous"),
            (lambda: eng.apply_body_forces(force=torch.zeros(8, NB, 4, device="cuda:0")), "[num_envs,24,3]")):
        with pytest.raises(EngineError) as ei:
            call()
        assert reason in str(ei.value), str(ei.value)
    lib = load_library()
    assert lib.he_apply_body_forces(None, None, None, 0, 1, None) != 0 and b"null handle" in lib.he_last_error()
    h = C.c_void_p()
    sp = _abi.default_sim_params()
    assert lib.he_create(C.byref(sp), 0, C.byref(h)) == 0
    assert lib.he_apply_body_forces_at_pos(h, C.c_void_p(f.data_ptr()), C.c_void_p(f.data_ptr()), 0, 1, None) != 0
    assert b"no envs" in lib.he_last_error()
    lib.he_destroy(h)
    # nothing was left pending and the engine still steps: the bits of an engine that was never called
    ref = _standing(he_model, model)
    eng.simulate(2)
    ref.simulate(2)
    assert same_bits(snap(eng), snap(ref))
    assert bool(torch.isfinite(eng.root_states).all())


# ------------------------------------------------------------------ 5. facade and env
def test_facade_applies_the_engines_wrench(he_model):
    from humanoid_amd.engine import Engine
    from humanoid_amd.isaacgym import gymapi, gymtorch
    from test_facade_env import _facade_sim
    n = 8
    gym, sim = _facade_sim(n)
    rng = np.random.default_rng(9)
    r0, d0 = cases.random_state(n, rng, height=(0.9, 1.1))
    src_r, src_d = cu(r0), cu(d0.reshape(n * ND, 2))
    rb0 = cu(O.forward_kinematics(he_model, r0, d0).reshape(n * NB, 13))
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_r), gymtorch.unwrap_tensor(ids), n)
    gym.set_dof_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_d), gymtorch.unwrap_tensor(ids), n)
    gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim)).copy_(rb0)
    f = cu(rng.normal(0, 30.0, (n * NB, 3)).astype(np.float32))
    t = cu(rng.normal(0, 3.0, (n * NB, 3)).astype(np.float32))
    x = (rb0[:, :3] + 0.05).contiguous()
    eng = Engine(he_model, n, device=0, sim_params=_abi.default_sim_params())
    eng.root_states.copy_(src_r)
    eng.dof_state.copy_(src_d)
    eng.rb_state.copy_(rb0)
    for step in range(3):
        if step == 0:
            assert gym.apply_rigid_body_force_tensors(sim, gymtorch.unwrap_tensor(f), gymtorch.unwrap_tensor(t), gymapi.LOCAL_SPACE)
            eng.apply_body_forces(f, t, LOCAL, hold=1)
        elif step == 1:
            assert gym.apply_rigid_body_force_tensors(sim, gymtorch.unwrap_tensor(f), None, gymapi.ENV_SPACE)
            eng.apply_body_forces(f, None, ENV, hold=1)
        else:
            assert gym.apply_rigid_body_force_at_pos_tensors(sim, gymtorch.unwrap_tensor(f), gymtorch.unwrap_tensor(x),
                                                             gymapi.GLOBAL_SPACE)
            eng.apply_body_forces_at_pos(f, x, GLOBAL, hold=1)
        gym.simulate(sim)
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        eng.simulate(2)
    torch.cuda.synchronize()
    assert same_bits(snap(sim.engine), snap(eng))
    plain = Engine(he_model, n, device=0, sim_params=_abi.default_sim_params())
    plain.root_states.copy_(src_r)
    plain.dof_state.copy_(src_d)
    for _ in range(3):
        plain.simulate(2)
    assert not torch.equal(plain.root_states, eng.root_states)


def test_env_push_option(model):
    from humanoid_amd.env import EnvConfig, HumanoidPHC, PHCPufferEnv
    from test_facade_env import _clip_dict
    n = 16
    clips = _clip_dict(model)

    def run(cls=PHCPufferEnv, eval_flag=False, **kw):
        env = cls(EnvConfig(num_envs=n, motion_file=clips, seed=3, **kw))
        env.reset()
        if eval_flag:
            env.flag_test = True  # the push gate only (the imitation parameters stay the training ones)
        rng = np.random.default_rng(2)
        obs = []
        for _ in range(10):
            a = rng.uniform(-0.2, 0.2, (n, 69)).astype(np.float32)
            o = env.step(a if cls is PHCPufferEnv else cu(a))[0]
            obs.append(o.clone())
        env.close()
        return torch.stack(obs)

    push = dict(push_interval=4, push_duration=2, push_force=200.0)
    a, b = run(**push), run(**push)
    off, default = run(**dict(push, push_force=0.0)), run()
    assert torch.equal(a, b), "one seed, one run"
    assert torch.equal(off, default)
    assert torch.equal(a[:4], off[:4]) and not torch.equal(a[4], off[4]), "the first push starts at policy step 4"
    assert not torch.equal(a, off)
    # HumanoidPHC.step pushes too; in test / eval mode only with push_in_eval
    h_on, h_off = run(HumanoidPHC, **push), run(HumanoidPHC)
    assert not torch.equal(h_on, h_off)
    assert torch.equal(run(HumanoidPHC, eval_flag=True, **push), h_off)
    assert torch.equal(run(HumanoidPHC, eval_flag=True, push_in_eval=True, **push), h_on)
