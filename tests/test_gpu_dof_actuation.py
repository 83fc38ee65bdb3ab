"""Torque control on the GPU (he_set_dof_drive_modes, he_set_dof_actuation_forces). The fp64
oracle cannot apply a joint force, so the feature is held to references the tests build themselves:

G1  one step's velocity change equals dt A^-1 (0, tau) (A from the oracle's CRBA), by the yardstick of
    the body-forces tests: the untouched kernels' own error on the same formula;
G2  a joint torque equals the pair of body torques that tests/test_dof_actuation.py shows to be the same
    generalized force, applied through he_apply_body_forces;
G3  M a + c = (0, tau) with libhumanoid_dynamics' M and c and the step's acceleration;
G4  the call semantics, bit for bit;  G5  the drive modes;  G6  HE_BUF_DOF_FORCE;  G7  invalid calls;
G8  the gym facade.
The measured figures are printed before each assertion and quoted beside it
(profiles/r11/gpu_tests_r11.log has the run)."""
import ctypes as C
import os

import numpy as np
import pytest

from humanoid_amd import _abi
from humanoid_amd.body_sets import BODY_NAMES

import cases
from test_gpu_body_forces import (ENV, KW3, SOLVERS, SOLVERS3, _drive_yardstick, _predict, _standing, _velocity_after, cu,
                                  load, make_engine, rest_case, same_bits, snap, standing_case, traj_err)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NB, ND, NG = 24, 69, 75
NONE, POS, EFFORT = _abi.DOF_MODE_NONE, _abi.DOF_MODE_POS, _abi.DOF_MODE_EFFORT
ALL_EFFORT = [EFFORT] * ND
ARM0 = 3 * (BODY_NAMES.index("L_Thorax") - 1)  # the arms' dofs: L_Thorax .. R_Hand, bodies 14..23
ARM_MODES = [POS] * ARM0 + [EFFORT] * (ND - ARM0)


def _effort(he_model):
    return np.array(he_model.effort[:ND], np.float64)


def _parents(he_model):
    return np.array(he_model.parents[:NB])


# ------------------------------------------------------------------ G1 / G2: dt A^-1 (0, tau), the wrench pair
JOINTS1 = ("L_Hip", "Spine", "L_Shoulder", "R_Hand", "L_Knee")
ALLOW_ACT = {"pgs_explicit": 2.0, "pgs": 4.0, "tgs4": 4.0}
ALLOW_WRENCH = 4.0  # test_one_step_velocity_change_is_dt_Ainv_Q's allowance, every solver
_runs1 = {}


def _tau_case(he_model, c):
    """tau [6,69] (fp32): envs 0-4 on one joint each (hip, spine, shoulder, hand, knee), env 5 on every
    dof, each env's scaled to a predicted largest |du| of 0.2 rad/s; and the pair of world torques
    [6,24,3] (fp32) with the same generalized force: +tau_k R_child e_k on the child, the opposite on
    the parent."""
    n = c["n"]
    rng = np.random.default_rng(29)
    tau = np.zeros((n, ND))
    for e in range(n):
        if e < len(JOINTS1):
            d = 3 * (BODY_NAMES.index(JOINTS1[e]) - 1)
            tau[e, d:d + 3] = rng.normal(size=3)
        else:
            tau[e] = rng.normal(size=ND)
    dt = _abi.default_sim_params().dt  # KW3: substeps 1
    Q = np.concatenate([np.zeros((n, 6)), tau], axis=1)
    tau *= (0.2 / np.abs(_predict(c, dt, Q)).max(axis=1))[:, None]
    tau32 = tau.astype(np.float32)
    assert (np.abs(tau32) < _effort(he_model)[None, :]).all(), "the clamp must stay out of the prediction"
    par = _parents(he_model)
    pair = np.zeros((n, NB, 3))
    for e in range(n):
        for d in np.nonzero(tau32[e])[0]:
            b, k = d // 3 + 1, d % 3
            t = float(tau32[e, d]) * c["R"][e, b][:, k]
            pair[e, b] += t
            pair[e, par[b]] -= t
    return tau32, pair.astype(np.float32)


def _runs(he_model, c, solver):
    """The step's velocity change from rest under the actuation, under the torque pair (ENV space, held
    over the launch), under both with the pair reversed, and the prediction: once per solver."""
    if solver not in _runs1:
        sp = SOLVERS3[solver](kp_scale=0.0, **KW3)
        dt = sp.dt / sp.substeps
        tau, pair = _tau_case(he_model, c)
        q = c["dof"][..., 0].copy()

        def act(eng):
            eng.set_dof_drive_modes(ALL_EFFORT)
            eng.set_dof_actuation_forces(cu(tau))

        def wrench(eng, sign=1.0):
            eng.apply_body_forces(torque=cu(sign * pair), space=ENV, hold=1)

        def both(eng):
            act(eng)
            wrench(eng, -1.0)

        u_none = _velocity_after(he_model, sp, c, q)
        pred = _predict(c, dt, np.concatenate([np.zeros((c["n"], 6)), tau.astype(np.float64)], axis=1))
        _runs1[solver] = dict(pred=pred, du_act=_velocity_after(he_model, sp, c, q, act) - u_none,
                              du_wrench=_velocity_after(he_model, sp, c, q, wrench) - u_none,
                              du_both=_velocity_after(he_model, sp, c, q, both) - u_none)
    return _runs1[solver]


@pytest.mark.parametrize("solver", ["pgs_explicit", "pgs", "tgs4"])
def test_one_step_velocity_change_is_dt_Ainv_tau(he_model, rest_case, solver):
    """du = u(with the actuation) - u(without) after one physics step from rest equals dt A^-1 (0, tau),
    A = H + diag(armature) (the oracle's CRBA): 6 bodies at rest in flight, every dof in EFFORT mode,
    no drive gains. The yardstick is the untouched kernels' relative error on the same formula through
    the PD drive (test_gpu_body_forces._drive_yardstick, measured in the same run). Without the
    midpoint bias the actuation enters the right-hand side through the drive torque's own chain and
    the prediction is exact for the explicit bias: 2 x. With it (PGS, TGS) both sides carry the
    velocity-product terms of a 0.2 rad/s change that the linear prediction leaves out: 4 x, the wrench
    test's allowance (its measured worst ratio 3.2 x).
    Measured on the MI355X, relative error of the actuation against the yardstick: PGS without the
    midpoint bias 1.66e-5 against 3.32e-5; PGS 6.45e-4 against 4.44e-4; TGS 3.21e-4 against 2.25e-4."""
    r = _runs(he_model, rest_case, solver)
    pred = r["pred"]
    rel = float(np.abs(r["du_act"] - pred).max() / np.abs(pred).max())
    yard = _drive_yardstick(he_model, rest_case, solver)
    print(f"\ndt A^-1 tau {solver}: actuation {rel:.3e}  drive yardstick {yard:.3e}  (largest |pred| "
          f"{np.abs(pred).max():.3f} rad/s)")
    assert abs(np.abs(pred).max() - 0.2) < 1e-3
    assert rel <= ALLOW_ACT[solver] * yard


@pytest.mark.parametrize("solver", ["pgs_explicit", "pgs", "tgs4"])
def test_joint_torque_equals_its_wrench_pair(he_model, rest_case, solver):
    """The same states and tau, once through he_set_dof_actuation_forces and once as the torque pair on
    child and parent through he_apply_body_forces: the two velocity changes differ by no more than
    the sum of the two paths' allowances against the prediction (actuation 2 x / 4 x, wrench 4 x the
    drive yardstick) times the largest |pred|. And the actuation with the reversed pair on top stays
    within the same bound of the untouched run. This pins the dof coordinate to the wrench path, which
    independent Jacobians pin (test_one_step_velocity_change_is_dt_Ainv_Q).
    Measured on the MI355X (rad/s; actuation against pair / actuation + reversed pair against none /
    bound): PGS without the midpoint bias 2.10e-7 / 1.45e-7 / 3.99e-5; PGS 1.98e-7 / 1.45e-7 / 7.10e-4;
    TGS 6.18e-7 / 1.45e-7 / 3.60e-4."""
    r = _runs(he_model, rest_case, solver)
    yard = _drive_yardstick(he_model, rest_case, solver)
    bound = (ALLOW_ACT[solver] + ALLOW_WRENCH) * yard * float(np.abs(r["pred"]).max())
    d = float(np.abs(r["du_act"] - r["du_wrench"]).max())
    z = float(np.abs(r["du_both"]).max())
    print(f"\nactuation against wrench pair {solver}: {d:.3e}  actuation + reversed pair against none: {z:.3e}  "
          f"bound {bound:.3e} rad/s")
    assert float(np.abs(r["du_wrench"]).max()) > 0.1  # the pair did act
    assert d <= bound
    assert z <= bound


# ------------------------------------------------------------------ G3: inverse-dynamics closure
def test_step_acceleration_closes_inverse_dynamics(he_model):
    """M a + c = (0, tau) with libhumanoid_dynamics' M (armature included) and c at the state before the
    step and a = (u1 - u0) / dt over one explicit PGS step: 8 tumbling bodies in flight, every dof in
    EFFORT mode, random tau within +-200. The figure is max |M a + c - (0, tau)| over
    max (|M| |a| + |c| + |tau|); the yardstick the same figure with no actuation set (the kernel without
    the wrench code, the same states); 2 x for one more fp32 add in the chain.
    Measured on the MI355X: 7.84e-8 with the actuation, 2.06e-7 without."""
    from humanoid_amd.dynamics import Dynamics
    n = 8
    rng = np.random.default_rng(43)
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), vel=0.5, ang=0.5)
    tau = rng.uniform(-200.0, 200.0, (n, ND)).astype(np.float32)
    # +-200 N m moves a hand by up to 170 rad/s in one step: the velocity clamps (both 100 rad/s by
    # default) are no part of M a + c = tau and are moved out of reach, like the other terms set to 0
    sp = _abi.pgs_sim_params(bias_midpoint=0, substeps=1, angular_damping=0.0, joint_limits=0, self_collision=0,
                             max_joint_velocity=1e6, max_angular_velocity=1e6)
    figs = []
    for t in (tau, None):
        eng = make_engine(he_model, n, sp)
        load(eng, root, dof, dof[..., 0].copy())
        eng.set_dof_drive_modes(ALL_EFFORT)
        if t is not None:
            eng.set_dof_actuation_forces(cu(t))
        dyn = Dynamics(eng)
        dyn.refresh()
        M = dyn.mass_matrix.cpu().numpy().astype(np.float64)
        c = dyn.bias.cpu().numpy().astype(np.float64)
        u0 = dyn.generalized_velocity().cpu().numpy().astype(np.float64)
        eng.simulate(1)
        torch.cuda.synchronize()
        assert int(eng.num_contacts.max()) == 0
        u1 = dyn.generalized_velocity().cpu().numpy().astype(np.float64)
        a = (u1 - u0) / float(sp.dt)
        Q = np.zeros((n, NG))
        if t is not None:
            Q[:, 6:] = t.astype(np.float64)
        res = np.einsum("nij,nj->ni", M, a) + c - Q
        mag = np.einsum("nij,nj->ni", np.abs(M), np.abs(a)) + np.abs(c) + np.abs(Q)
        figs.append(float(np.abs(res).max() / mag.max()))
    print(f"\ninverse-dynamics closure: actuation {figs[0]:.3e}  no actuation (yardstick) {figs[1]:.3e}")
    assert figs[1] < 1e-4
    assert figs[0] <= 2.0 * figs[1]


# ------------------------------------------------------------------ G4: semantics, bit for bit
def _arm_tau(n, seed, scale=20.0):
    t = np.zeros((n, ND), np.float32)
    t[:, ARM0:] = np.random.default_rng(seed).uniform(-scale, scale, (n, ND - ARM0)).astype(np.float32)
    return cu(t)


def _standing_arms(he_model, model, n=8, **kw):
    eng = _standing(he_model, model, n, **kw)
    eng.set_dof_drive_modes(ARM_MODES)
    return eng


def test_set_then_clear_runs_the_untouched_step(he_model, model):
    a, b = _standing_arms(he_model, model), _standing_arms(he_model, model)
    c, d = _standing(he_model, model), _standing(he_model, model)
    for eng in (a, c):
        eng.set_dof_actuation_forces(_arm_tau(8, 1))
        eng.clear_dof_actuation_forces()
    for _ in range(5):
        for eng in (a, b, c, d):
            eng.simulate(2)
    assert same_bits(snap(a), snap(b))
    assert same_bits(snap(c), snap(d))  # an engine that was never called at all


def test_actuation_persists_over_simulate_calls(he_model, model):
    """The actuation is a setting: set once, simulate(2) gives the bits of simulate(1) twice, and both
    differ from the run without it.
    One launch of two simulate() calls and two launches of one are not the same bits in this engine
    whatever acts, without an actuation too: a launch's first physics step takes the joints' rotations
    from their exp-map angles, a later step of the same launch the integrator's own (he_physics.hip,
    kinematics' `cached`). Only the end of a wrench's hold restarts a launch's step the way a new launch
    starts (physics_body's `first`), which is what makes test_hold_counts_simulate_calls' comparison one
    of bits. So the comparison here runs with a ZERO wrench of hold 1 pending as well: it adds exact
    zeros to the generalized force and puts that restart where the two launches are split, and the
    actuation is then compared bit for bit in the launch's second simulate() and in a later launch.
    Measured on the MI355X without that wrench (printed, not asserted), the largest dof-state difference
    of simulate(2) against simulate(1) twice: 6.58e-5 with the actuation (arms under +-20 N m), 2.38e-7
    without any."""
    def run(calls, tau, zero_wrench):
        eng = _standing_arms(he_model, model)
        if tau:
            eng.set_dof_actuation_forces(_arm_tau(8, 1))
        if zero_wrench:
            eng.apply_body_forces(torque=torch.zeros(8, NB, 3, device="cuda:0"), hold=1)
        for k in calls:
            eng.simulate(k)
        return snap(eng)

    for tau in (True, False):
        d = float((run((2,), tau, False)[1] - run((1, 1), tau, False)[1]).abs().max())
        print(f"\nsimulate(2) against simulate(1) twice, no restart, {'with' if tau else 'without'} an actuation: "
              f"largest dof-state difference {d:.3e}")
    one, two, none = run((2,), True, True), run((1, 1), True, True), run((2,), False, True)
    assert not torch.equal(one[1], none[1])
    assert same_bits(one, two)
    # and the second simulate() did feel it: clearing between the two launches gives another state
    eng = _standing_arms(he_model, model)
    eng.set_dof_actuation_forces(_arm_tau(8, 1))
    eng.simulate(1)
    eng.clear_dof_actuation_forces()
    eng.simulate(1)
    assert not torch.equal(snap(eng)[1], two[1])


def test_replacement_takes_effect(he_model, model):
    a, b, c = (_standing_arms(he_model, model) for _ in range(3))
    t1, t2 = _arm_tau(8, 1), _arm_tau(8, 2)
    a.set_dof_actuation_forces(t1)
    a.set_dof_actuation_forces(t2.view(-1))  # [N*69] is accepted too
    b.set_dof_actuation_forces(t2)
    c.set_dof_actuation_forces(t1)
    for eng in (a, b, c):
        eng.simulate(2)
    assert same_bits(snap(a), snap(b))
    assert not torch.equal(a.dof_state, c.dof_state)


def test_indexed_write_equals_the_merged_full_write(he_model, model):
    a, b, c, d = (_standing_arms(he_model, model) for _ in range(4))
    t1, t2 = _arm_tau(8, 1), _arm_tau(8, 2)
    ids = torch.tensor([1, 4, 6], dtype=torch.int32, device="cuda:0")
    merged = t1.clone()
    merged[ids.long()] = t2[ids.long()]
    a.set_dof_actuation_forces(t1)
    a.set_dof_actuation_forces_indexed(t2, ids)
    b.set_dof_actuation_forces(merged)
    # with nothing set before, the other rows are zero
    from_zero = torch.zeros_like(t2)
    from_zero[ids.long()] = t2[ids.long()]
    c.set_dof_actuation_forces_indexed(t2, ids)
    d.set_dof_actuation_forces(from_zero)
    for eng in (a, b, c, d):
        eng.simulate(2)
    assert same_bits(snap(a), snap(b))
    assert same_bits(snap(c), snap(d))
    assert not torch.equal(a.dof_state, c.dof_state)


def test_zero_actuation_stays_within_the_standing_yardstick(he_model, model, standing_case):
    n = 8
    a, b = _standing_arms(he_model, model), _standing_arms(he_model, model)
    a.set_dof_actuation_forces(torch.zeros(n, ND, device="cuda:0"))
    a.simulate(2)
    b.simulate(2)
    torch.cuda.synchronize()
    d = traj_err(model, a, b.dof_state.view(n, ND, 2).cpu().numpy().astype(np.float64),
                 b.rb_state.view(n, NB, 13).cpu().numpy())
    print(f"\nzero actuation against none: {d:.3e}  (standing yardstick {standing_case['eB']:.3e})")
    assert d <= standing_case["eB"]  # expected 0 (the same bits)


def _env_step_run(he_model, model, golden, fused, steps=4, legs=None):
    """he_env_step on 24 standing bodies under tracking-free random actions, the arms in EFFORT mode with
    an actuation set once (it persists) and replaced at step 2."""
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
    eng.set_dof_drive_modes(ARM_MODES)
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
    for k in range(steps):
        a = cu(rng.uniform(-0.3, 0.3, (n, 69)).astype(np.float32))
        if k in (0, 2):
            eng.set_dof_actuation_forces(_arm_tau(n, 10 + k))
        eng.env_step(_abi.imitation_params(), em, a, *bufs, seed=7, step_index=k)
    return snap(eng) + tuple(b.clone() for b in bufs)


def test_env_step_with_an_actuation_fused_equals_two_launches(he_model, model, golden):
    one, two = _env_step_run(he_model, model, golden, 1), _env_step_run(he_model, model, golden, 0)
    assert same_bits(one, two)
    assert float(one[4].view(24, ND)[:, ARM0:].abs().max()) > 1.0  # dof_force carries the arms' actuation


def test_leg_class_with_an_actuation_leaves_the_step_unchanged(he_model, model, golden):
    assert same_bits(_env_step_run(he_model, model, golden, 1, legs="0"), _env_step_run(he_model, model, golden, 1, legs="1"))


def test_cleared_actuation_leaves_the_untouched_kernels(he_model, model):
    """After a clear the engine steps as a fresh engine does that is loaded with its state and contact
    cache (and has the same drive modes)."""
    a = _standing_arms(he_model, model)
    a.set_dof_actuation_forces(_arm_tau(8, 1))
    a.simulate(2)
    a.clear_dof_actuation_forces()
    s = snap(a)
    b = _standing_arms(he_model, model)
    b.root_states.copy_(s[0])
    b.dof_state.copy_(s[1])
    b.contact_cache.copy_(s[5])
    for _ in range(3):
        a.simulate(2)
        b.simulate(2)
    assert not torch.equal(s[0], a.root_states)
    assert same_bits(snap(a), snap(b))


# ------------------------------------------------------------------ G5: drive modes
def test_effort_arms_equal_a_model_without_arm_gains(he_model, model):
    """Arms EFFORT, the rest POS, no actuation: the bits of an engine whose model blob has zero arm gains."""
    n = 8
    zero = _abi.HeModel.from_buffer_copy(he_model)
    for d in range(ARM0, ND):
        zero.stiffness[d] = zero.damping[d] = 0.0
    root, dof = cases.standing_state(model, n, np.random.default_rng(4), xy_jitter=1.0)
    tgt = np.random.default_rng(6).uniform(-0.3, 0.3, (n, ND)).astype(np.float32)
    a, b, plain = (make_engine(m, n, _abi.default_sim_params()) for m in (he_model, zero, he_model))
    a.set_dof_drive_modes(ARM_MODES)
    for eng in (a, b, plain):
        load(eng, root, dof, tgt)
        for _ in range(3):
            eng.simulate(2)
    assert same_bits(snap(a), snap(b))
    assert not torch.equal(a.dof_state, plain.dof_state)  # the arms' drives were acting
    # NONE takes the drive away as EFFORT does
    c = make_engine(he_model, n, _abi.default_sim_params())
    c.set_dof_drive_modes([POS] * ARM0 + [NONE] * (ND - ARM0))
    load(c, root, dof, tgt)
    for _ in range(3):
        c.simulate(2)
    assert same_bits(snap(c), snap(b))


def test_all_pos_set_explicitly_is_the_default(he_model, model):
    a, b = _standing(he_model, model), _standing(he_model, model)
    a.set_dof_drive_modes(ARM_MODES)
    a.set_dof_drive_modes([POS] * ND)
    for _ in range(3):
        a.simulate(2)
        b.simulate(2)
    assert same_bits(snap(a), snap(b))


def test_actuation_on_pos_dofs_is_a_zero_actuation(he_model, model):
    n = 8
    a, b, c = (_standing_arms(he_model, model) for _ in range(3))
    t = np.zeros((n, ND), np.float32)
    t[:, :ARM0] = np.random.default_rng(8).uniform(-50.0, 50.0, (n, ARM0)).astype(np.float32)
    a.set_dof_actuation_forces(cu(t))
    b.set_dof_actuation_forces(torch.zeros(n, ND, device="cuda:0"))
    for eng in (a, b, c):
        eng.simulate(2)
    assert same_bits(snap(a), snap(b))


def test_actuation_is_clamped_to_the_effort_limit(he_model, model):
    """2 x effort gives the bits of effort (on the shoulders, both signs)."""
    n = 8
    lim = _effort(he_model)
    t = np.zeros((n, ND), np.float32)
    for name, sign in (("L_Shoulder", 1.0), ("R_Shoulder", -1.0)):
        d = 3 * (BODY_NAMES.index(name) - 1)
        t[:, d:d + 3] = sign * lim[d:d + 3]
    a, b, c = (_standing_arms(he_model, model) for _ in range(3))
    a.set_dof_actuation_forces(cu(2.0 * t))
    b.set_dof_actuation_forces(cu(t))
    c.set_dof_actuation_forces(cu(0.5 * t))
    for eng in (a, b, c):
        eng.simulate(1)
    assert bool(torch.isfinite(a.dof_state).all())
    assert same_bits(snap(a), snap(b))
    assert not torch.equal(a.dof_state, c.dof_state)


# ------------------------------------------------------------------ G6: dof_force
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_dof_force_reports_the_clamped_actuation(he_model, solver):
    """In flight, every dof in EFFORT mode, no joint limits: the drive and limit parts of dof_force are
    zero, so it equals the clamped actuation exactly."""
    n = 8
    rng = np.random.default_rng(47)
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), vel=0.5, ang=0.5)
    tau = rng.uniform(-30.0, 30.0, (n, ND)).astype(np.float32)
    tau[:, ::7] *= 40.0  # some past the effort limit
    lim = _effort(he_model).astype(np.float32)
    eng = make_engine(he_model, n, SOLVERS[solver](joint_limits=0, self_collision=0))
    load(eng, root, dof, dof[..., 0].copy())
    eng.set_dof_drive_modes(ALL_EFFORT)
    eng.set_dof_actuation_forces(cu(tau))
    eng.simulate(2)
    torch.cuda.synchronize()
    assert int(eng.num_contacts.max()) == 0
    want = np.clip(tau, -lim[None, :], lim[None, :])
    assert (want != tau).any()
    got = eng.dof_force.view(n, ND).cpu().numpy()
    print(f"\ndof_force {solver}: largest |dof_force - clamped actuation| {np.abs(got - want).max():.3e}")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("solver", ["pgs_explicit", "pgs", "tgs4"])
def test_dof_force_of_pos_legs_is_the_drives(he_model, rest_case, solver):
    """Legs POS, arms EFFORT, an actuation written on every dof: the leg rows of dof_force are the
    drives', those of the run without actuation, within G1's allowance (2 x / 4 x the drive yardstick,
    relative to the largest leg force). G1's setting with the yardstick's gains (kp_scale 1e-6, target
    offsets U(-400, 400) rad: leg forces up to 0.32 N m), the arms' tau scaled to a predicted largest
    |du| of 0.2 rad/s. The arms' torques move the legs' velocities through the floating base, which the
    implicit drive answers by coef du with coef = dt kp <= 1.4e-5 N m s: at most 2.7e-6 N m, 8e-6
    of the largest leg force, under every allowance (asserted below from the test's own numbers).
    Measured on the MI355X (of the largest leg force, 0.393 N m): PGS without the midpoint bias 1.69e-6
    against an allowance of 6.65e-5; PGS 1.69e-6 against 1.77e-3; TGS 5.12e-7 against 9.00e-4."""
    c = rest_case
    n = c["n"]
    sp = SOLVERS3[solver](kp_scale=1e-6, **KW3)
    dt = sp.dt / sp.substeps
    rng = np.random.default_rng(53)
    q = c["dof"][..., 0]
    tgt = (q + rng.uniform(-400.0, 400.0, (n, ND))).astype(np.float32)
    tau = rng.normal(size=(n, ND))
    Q = np.concatenate([np.zeros((n, 6 + ARM0)), tau[:, ARM0:]], axis=1)
    tau *= (0.2 / np.abs(_predict(c, dt, Q)).max(axis=1))[:, None]
    tau32 = tau.astype(np.float32)
    assert (np.abs(tau32) < _effort(he_model)[None, :]).all()
    forces = []
    for t in (tau32, None):
        eng = make_engine(he_model, n, sp)
        load(eng, c["root"], c["dof"], tgt, rb=c["rb"])
        eng.set_dof_drive_modes(ARM_MODES)
        if t is not None:
            eng.set_dof_actuation_forces(cu(t))
        eng.simulate(1)
        torch.cuda.synchronize()
        forces.append(eng.dof_force.view(n, ND).cpu().numpy().astype(np.float64))
    with_act, without = forces
    scale = float(np.abs(without[:, :ARM0]).max())
    rel = float(np.abs(with_act[:, :ARM0] - without[:, :ARM0]).max() / scale)
    yard = _drive_yardstick(he_model, c, solver)
    coupling = dt * float(np.array(he_model.stiffness[:ARM0]).max()) * 1e-6 * 0.2 / scale
    print(f"\ndof_force of the POS legs {solver}: {rel:.3e} of the largest leg force {scale:.3f} N m  "
          f"(allowance {ALLOW_ACT[solver] * yard:.3e}, coupling bound {coupling:.3e})")
    assert coupling < ALLOW_ACT[solver] * yard
    assert rel <= ALLOW_ACT[solver] * yard
    # the arms' rows are the applied actuation (no drive there)
    assert np.array_equal(with_act[:, ARM0:].astype(np.float32), tau32[:, ARM0:])


# ------------------------------------------------------------------ G7: invalid calls
def test_invalid_calls_are_refused_with_a_reason(he_model, model):
    from humanoid_amd.engine import EngineError, load_library
    n = 8
    eng = _standing(he_model, model)
    good = torch.zeros(n, ND, device="cuda:0")
    ids = torch.tensor([0, 1], dtype=torch.int32, device="cuda:0")
    vel = [POS] * ND
    vel[7] = _abi.DOF_MODE_VEL
    for call, reason in (
            (lambda: eng.set_dof_drive_modes(vel), "DOF_MODE_VEL"),
            (lambda: eng.set_dof_drive_modes([POS] * 68 + [4]), "out of range"),
            (lambda: eng.set_dof_drive_modes([POS] * 68 + [-1]), "out of range"),
            (lambda: eng.set_dof_drive_modes([POS] * 68), "69 modes"),
            (lambda: eng.set_dof_actuation_forces(torch.zeros(n, ND + 1, device="cuda:0")), "elements"),
            (lambda: eng.set_dof_actuation_forces(torch.zeros(ND, n, device="cuda:0")), "[num_envs,69]"),
            (lambda: eng.set_dof_actuation_forces(torch.zeros(n, ND, device="cuda:0", dtype=torch.float64)), "float32"),
            (lambda: eng.set_dof_actuation_forces(torch.zeros(ND, n, device="cuda:0").t()), "contiguous"),
            (lambda: eng.set_dof_actuation_forces(torch.zeros(n, ND)), "cuda"),
            (lambda: eng.set_dof_actuation_forces_indexed(good[:4], ids), "elements"),
            (lambda: eng.set_dof_actuation_forces_indexed(good, ids.long()), "int32")):
        with pytest.raises(EngineError) as ei:
            call()
        assert reason in str(ei.value), str(ei.value)
    lib = load_library()
    modes = (C.c_int32 * ND)(*([POS] * ND))
    assert lib.he_set_dof_drive_modes(None, modes) != 0 and b"null handle" in lib.he_last_error()
    assert lib.he_set_dof_actuation_forces(None, C.c_void_p(good.data_ptr()), None) != 0
    assert b"null handle" in lib.he_last_error()
    assert lib.he_set_dof_actuation_forces_indexed(None, C.c_void_p(good.data_ptr()), C.c_void_p(ids.data_ptr()), 2, None) != 0
    assert b"null handle" in lib.he_last_error()
    h = C.c_void_p()
    sp = _abi.default_sim_params()
    assert lib.he_create(C.byref(sp), 0, C.byref(h)) == 0
    assert lib.he_set_dof_drive_modes(h, modes) != 0 and b"he_set_model first" in lib.he_last_error()
    assert lib.he_set_dof_actuation_forces(h, C.c_void_p(good.data_ptr()), None) != 0 and b"no envs" in lib.he_last_error()
    assert lib.he_set_model(h, C.byref(he_model)) == 0
    assert lib.he_set_dof_drive_modes(h, modes) == 0  # valid before he_create_envs
    assert lib.he_set_dof_actuation_forces_indexed(h, C.c_void_p(good.data_ptr()), C.c_void_p(ids.data_ptr()), 2, None) != 0
    assert b"no envs" in lib.he_last_error()
    lib.he_destroy(h)
    # nothing was changed and the engine still steps: the bits of an engine that was never called
    ref = _standing(he_model, model)
    eng.simulate(2)
    ref.simulate(2)
    assert same_bits(snap(eng), snap(ref))
    assert bool(torch.isfinite(eng.root_states).all())


# ------------------------------------------------------------------ G8: the gym facade
def _facade_sim_effort_arms(n):
    """tests/test_facade_env.py's _facade_sim with DOF_MODE_EFFORT on the arms."""
    from humanoid_amd.isaacgym import gymapi
    from humanoid_amd.model import DEFAULT_MODEL_JSON
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    opts = gymapi.AssetOptions()
    opts.angular_damping, opts.max_angular_velocity = 0.01, 100.0
    opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
    asset = gym.load_asset(sim, "/", DEFAULT_MODEL_JSON, opts)
    gym.add_ground(sim, gymapi.PlaneParams())
    dof_prop = gym.get_asset_dof_properties(asset)
    dof_prop["driveMode"] = gymapi.DOF_MODE_POS
    dof_prop["driveMode"][ARM0:] = gymapi.DOF_MODE_EFFORT
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-5, -5, 0), gymapi.Vec3(5, 5, 5), 4)
        gym.begin_aggregate(env, 160, 160, True)
        pose = gymapi.Transform(gymapi.Vec3(0.1 * i, 0.0, 0.89), gymapi.Quat(0, 0, 0, 1))
        h = gym.create_actor(env, asset, pose, f"humanoid_{i}", i, 0, 0)
        gym.enable_actor_dof_force_sensors(env, h)
        gym.set_actor_dof_properties(env, h, dof_prop)
        gym.set_actor_rigid_shape_properties(env, h, gym.get_actor_rigid_shape_properties(env, h))
        gym.end_aggregate(env)
    gym.prepare_sim(sim)
    return gym, sim


def test_facade_sets_the_engines_actuation(he_model):
    from humanoid_amd.engine import Engine
    from humanoid_amd.isaacgym import gymtorch
    n = 8
    gym, sim = _facade_sim_effort_arms(n)
    rng = np.random.default_rng(9)
    r0, d0 = cases.random_state(n, rng, height=(0.9, 1.1))
    src_r, src_d = cu(r0), cu(d0.reshape(n * ND, 2))
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_r), gymtorch.unwrap_tensor(ids), n)
    gym.set_dof_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_d), gymtorch.unwrap_tensor(ids), n)

    def direct():
        e = Engine(he_model, n, device=0, sim_params=_abi.default_sim_params())
        e.set_dof_drive_modes(ARM_MODES)
        e.root_states.copy_(src_r)
        e.dof_state.copy_(src_d)
        return e

    eng, plain = direct(), direct()
    taus = [cu(rng.uniform(-20.0, 20.0, (n * ND,)).astype(np.float32)) for _ in range(4)]
    for step in range(3):
        assert gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(taus[step]))
        eng.set_dof_actuation_forces(taus[step])
        gym.simulate(sim)
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        eng.simulate(2)
        plain.simulate(2)
    torch.cuda.synchronize()
    assert same_bits(snap(sim.engine), snap(eng))
    assert not torch.equal(plain.dof_state, eng.dof_state)
    # the indexed form replaces the listed envs' rows only
    some = torch.tensor([2, 5, 7], dtype=torch.int32, device="cuda:0")
    assert gym.set_dof_actuation_force_tensor_indexed(sim, gymtorch.unwrap_tensor(taus[3]), gymtorch.unwrap_tensor(some), 3)
    merged = taus[2].clone().view(n, ND)
    merged[some.long()] = taus[3].view(n, ND)[some.long()]
    eng.set_dof_actuation_forces(merged)
    keep = direct()  # the last full write goes on
    for src, dst in zip(snap(eng), (keep.root_states, keep.dof_state)):
        dst.copy_(src)
    keep.contact_cache.copy_(eng.contact_cache)
    keep.set_dof_actuation_forces(taus[2])
    gym.simulate(sim)
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    eng.simulate(2)
    keep.simulate(2)
    torch.cuda.synchronize()
    assert same_bits(snap(sim.engine), snap(eng))
    got, kept = sim.engine.dof_state.view(n, ND, 2), keep.dof_state.view(n, ND, 2)
    rest = [e for e in range(n) if e not in (2, 5, 7)]
    assert torch.equal(got[rest], kept[rest])
    assert all(not torch.equal(got[e], kept[e]) for e in (2, 5, 7))
