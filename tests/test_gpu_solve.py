"""GPU checks of the joint-space solves (include/humanoid_solve.h) against the float64 numpy reference of
tests/solve_reference.py, which tests/test_solve.py pins (residual, sparse L^T D L, free fall, round
trip, the fp64 oracle's explicit step). The five states are those of tests/test_gpu_dynamics.py's
`ctx`: env 0 as created, 1-3 random tumbling, 4 all-zero dof angles with nonzero rates.

Tolerance per figure: 8 x that figure's own float32 floor (MARGIN of tests/test_gpu_dynamics.py). The
floor is solve_reference evaluated in float32 against float64 on the same states and right-hand sides,
the largest over the five envs; it is computed and printed here and never taken from the kernel. Two
figures per output, each the largest over the envs: the forward error max|x - x64| / max|x64| and the
componentwise residual max_i |M64 x - b|_i / (|M64||x| + |b|)_i.

Floors and the kernels' measured figures on the five states (MI355X; forward error, then residual):

    case                                         forward floor  kernel      residual floor  kernel
    forward dynamics, no force, armature on      1.39e-05       2.23e-05    3.88e-07        4.62e-07
      the same without gravity                   7.46e-06       1.37e-05    4.44e-07        1.18e-06
    forward dynamics, no force, armature off     4.31e-05       5.89e-05    5.85e-07        3.24e-07
      the same without gravity                   3.67e-05       5.63e-05    6.34e-07        7.98e-07
    forward dynamics, forced, armature on        5.90e-06       9.62e-06    2.19e-07        2.86e-07
      the same without gravity                   5.95e-06       9.77e-06    2.14e-07        2.92e-07
    forward dynamics, forced, armature off       1.13e-06       1.10e-06    4.04e-07        6.49e-07
      the same without gravity                   1.13e-06       1.09e-06    4.41e-07        6.24e-07
    computed torque, tau (no force / forced)     9.02e-07       8.53e-07    7.94e-07        4.57e-07
                                                 2.68e-07       2.63e-07    1.27e-07        9.98e-08
    computed torque, base acceleration           5.90e-07       3.04e-07
    computed torque, round trip (no f / forced)  1.50e-05       3.34e-05    /  1.12e-05     3.48e-05
    solve k = 6, J of R_Hand                     4.26e-07       5.93e-07    4.63e-06        1.16e-06
    solve k = 32, normal vectors                 1.20e-05       8.89e-06    5.08e-07        7.68e-07

J M^-1 J^T asymmetry 5.79e-08 (floor 1.39e-08); kernel tau against the torch recipe 1.76e-06 of max|tau|
(the two floors sum to 1.80e-06), base acceleration 9.4e-07 (1.18e-06); engine step against forward
dynamics 1.30e-05 of max|a| with the kernel, 1.47e-05 with the float64 reference in its place (forward
floor 1.04e-05). With the subtree inertias referred to the root origin instead of each joint's own, as the
dynamics library's tensors are, the residuals were 6e-06 ... 8e-05 and the armature-off forward error
1.3e-04: a row of a solve is read at its own scale, not at the scale of M's largest entry.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
import dynamics_reference as DR  # noqa: E402
import solve_reference as SR  # noqa: E402
from test_gpu_dynamics import MARGIN, N, ctx  # noqa: E402,F401  (the five states, one engine, one Dynamics)

from humanoid_amd import _abi  # noqa: E402
from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
NB, ND, NG = DR.NB, DR.ND, DR.NG
SENTINEL = 12345.0
R_HAND = BODY_NAMES.index("R_Hand")


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _report(name, fig, floor):
    print(f"{name}: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")


def _held(name, fig, floor):
    _report(name, fig, floor)
    assert np.isfinite(fig) and fig <= MARGIN * floor, (name, fig, MARGIN * floor)


@pytest.fixture(scope="module")
def sol(ctx, he_model):  # noqa: F811
    """A Solver on ctx's engine, the module's inputs, and a cache of (M, c) per setting in both dtypes
    (computed once per setting, left unchanged)."""
    from humanoid_amd import solve

    class S:
        pass

    s = S()
    s.solve = solve
    s.solver = solve.Solver(ctx.eng)
    rng = np.random.default_rng(17)
    s.f = np.concatenate([np.zeros((N, 6)), rng.uniform(-100.0, 100.0, (N, ND))], axis=1).astype(np.float32)
    s.qdd_des = rng.uniform(-20.0, 20.0, (N, ND)).astype(np.float32)
    s.rhs32 = rng.normal(size=(N, 32, NG)).astype(np.float32)
    cache = {}

    def terms(armature=True, gravity=True):
        key = (armature, gravity)
        if key not in cache:
            cache[key] = tuple(SR.terms(he_model, ctx.root, ctx.dof, ctx.g, dt, armature=armature, no_gravity=not gravity)
                               for dt in (np.float64, np.float32))
        return cache[key]

    s.terms = terms
    # env 0 is at rest: without a generalised force it is in exact free fall (qdd = (g, 0)), the state of
    # exact equilibrium for which solve_reference.residual has the normwise figure
    s.rest = np.array([not ctx.root[e, 7:].any() and not ctx.dof[e].any() for e in range(N)])
    assert s.rest.tolist() == [True] + [False] * (N - 1)
    yield s
    del s.solver


# ------------------------------------------------------------------ S1: forward dynamics
@pytest.mark.parametrize("gravity", [True, False], ids=["gravity", "nogravity"])
@pytest.mark.parametrize("armature", [True, False], ids=["armature", "noarmature"])
@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
def test_forward_dynamics(ctx, sol, forced, armature, gravity):  # noqa: F811
    """qdd = M^-1 (gen_force - c), gen_force NULL or (0_6, U(-100, 100)), each armature / gravity setting
    against the floor of that setting (armature off: cond(M) 1.9e6 against 3.8e3, a floor of its own).
    Without a force env 0 is in exact free fall: every entry of the exact qdd but g is zero, the
    componentwise residual in the rows those entries feed is one rounding over another (measured: 1.0 for
    a 1e-6 perturbation of the exact answer, 1.8e-2 for the float32 sparse L^T D L on the CPU, 0.86 for the
    kernel, 2.8e-6 for the float32 Cholesky, whose zeros come out exact), and that env takes the normwise
    residual instead (solve_reference.residual); without gravity too its exact answer is 0 and the kernel's
    must be."""
    (M64, c64), (M32, c32) = sol.terms(armature, gravity)
    f = sol.f if forced else None
    x64 = SR.forward_dynamics(M64, c64, f)
    x32 = SR.forward_dynamics(M32, c32, f)
    b64 = (0.0 if f is None else f.astype(np.float64)) - c64
    sol.solver.armature, sol.solver.gravity = armature, gravity
    try:
        x = host(sol.solver.forward_dynamics(None if f is None else cu(f)))
    finally:
        sol.solver.armature, sol.solver.gravity = True, True
    assert x.shape == (N, NG) and x.dtype == np.float32
    tag = f"forward dynamics {'forced' if forced else 'free'} armature={armature} gravity={gravity}"
    print(f"cond(M) {np.linalg.cond(M64[1]):.2e}")
    _held(tag + ", forward error", SR.forward_error(x, x64).max(), SR.forward_error(x32, x64).max())
    rest = None if forced else sol.rest
    _held(tag + ", residual", SR.residual(M64, x, b64, rest).max(), SR.residual(M64, x32, b64, rest).max())


# ------------------------------------------------------------------ S2: computed torque
def test_computed_torque(ctx, sol):  # noqa: F811
    """tau and the base acceleration against the reference, with and without a generalised force; the
    residual of the defining equation; the round trip through the forward-dynamics kernel gives qdd_des
    back."""
    (M64, c64), (M32, c32) = sol.terms()
    for f in (None, sol.f):
        tau64, ab64 = SR.computed_torque(M64, c64, sol.qdd_des, f)
        tau32, ab32 = SR.computed_torque(M32, c32, sol.qdd_des, f)
        tau_t, ab_t = sol.solver.computed_torque(cu(sol.qdd_des), None if f is None else cu(f))
        tau, ab = host(tau_t), host(ab_t)
        assert tau.shape == (N, ND) and ab.shape == (N, 6)
        tag = f"computed torque {'forced' if f is not None else 'free'}"
        _held(tag + ", tau forward error", SR.forward_error(tau, tau64).max(), SR.forward_error(tau32, tau64).max())
        _held(tag + ", base_acc forward error", SR.forward_error(ab, ab64).max(), SR.forward_error(ab32, ab64).max())
        _held(tag + ", residual", SR.torque_residual(M64, c64, sol.qdd_des, tau, ab, f).max(),
              SR.torque_residual(M64, c64, sol.qdd_des, tau32, ab32, f).max())
        # round trip: the float32 reference's own round trip is the floor
        g = np.zeros((N, NG), np.float32) if f is None else f.copy()
        g[:, 6:] += tau
        want = np.concatenate([ab64, sol.qdd_des.astype(np.float64)], axis=1)
        back = host(sol.solver.forward_dynamics(cu(g)))
        g32 = np.zeros((N, NG), np.float32) if f is None else f.copy()
        g32[:, 6:] += tau32
        back32 = SR.forward_dynamics(M32, c32, g32)
        _held(tag + ", round trip", SR.forward_error(back, want).max(), SR.forward_error(back32, want).max())


def test_computed_torque_equals_the_torch_recipe(ctx, sol):  # noqa: F811
    """The INTEGRATION.md recipe in torch on Dynamics' refreshed M and c (the path the kernel replaces).
    Both are float32 computations of the same tau, each held to 8 x its floor against float64 (the recipe's
    floor is the float32 reference's: it is that reference's arithmetic), so they differ by no more than
    the sum of the two tolerances. Measured: 1.76e-06 of max|tau|, within the plain sum of the two floors
    too (1.80e-06); base acceleration 9.4e-07 (1.18e-06)."""
    (M64, c64), (M32, c32) = sol.terms()
    tau64, ab64 = SR.computed_torque(M64, c64, sol.qdd_des)
    tau32, ab32 = SR.computed_torque(M32, c32, sol.qdd_des)
    ctx.dyn.refresh(jacobian=False)
    M, c = ctx.dyn.mass_matrix, ctx.dyn.bias
    qdd_des = cu(sol.qdd_des)
    qdd_base = torch.linalg.solve(M[:, :6, :6], -(c[:, :6] + (M[:, :6, 6:] @ qdd_des.unsqueeze(-1)).squeeze(-1)))
    qdd = torch.cat([qdd_base, qdd_des], dim=1)
    recipe = host(((M @ qdd.unsqueeze(-1)).squeeze(-1) + c)[:, 6:].contiguous())
    tau_t, ab_t = ctx.dyn.computed_torque(qdd_des)
    tau, ab = host(tau_t), host(ab_t)
    floor = SR.forward_error(tau32, tau64).max()
    d_tau = (np.abs(tau.astype(np.float64) - recipe).max(axis=1) / np.abs(tau64).max(axis=1)).max()
    floor_b = SR.forward_error(ab32, ab64).max()
    d_ab = (np.abs(ab.astype(np.float64) - host(qdd_base)).max(axis=1) / np.abs(ab64).max(axis=1)).max()
    print(f"kernel against torch recipe: tau {d_tau:.3e} (floor {floor:.3e}), base_acc {d_ab:.3e} (floor {floor_b:.3e}); "
          f"recipe against float64: {SR.forward_error(recipe, tau64).max():.3e}")
    assert d_tau <= MARGIN * (floor + floor)
    assert d_ab <= MARGIN * (floor_b + floor_b)


# ------------------------------------------------------------------ S3: solve
def _solve_case(ctx, sol, rhs, tag):  # noqa: F811
    (M64, _), (M32, _) = sol.terms()
    x64 = SR.solve(M64, rhs.astype(np.float64))
    x32 = SR.solve(M32, rhs)
    x = host(sol.solver.solve(cu(rhs)))
    assert x.shape == rhs.shape
    _held(tag + ", forward error", SR.forward_error(x, x64).max(), SR.forward_error(x32, x64).max())
    _held(tag + ", residual", SR.residual(M64, x, rhs).max(), SR.residual(M64, x32, rhs).max())
    return x, x32


def test_solve_with_a_jacobian_block(ctx, sol):  # noqa: F811
    """k = 6, rhs = jacobian[:, R_Hand]: J M^-1 against the reference, and J M^-1 J^T (the inverse
    operational-space inertia of the hand) symmetric to the float32 reference's own asymmetry."""
    J = ctx.J[:, R_HAND].copy()  # [N,6,75] f32, the dynamics kernel's
    assert np.abs(J[:, :, 6:]).max() > 0.1
    x, x32 = _solve_case(ctx, sol, J, "solve k=6 (J of R_Hand)")

    def asym(X):
        A = np.einsum("eik,ejk->eij", X.astype(np.float64), J.astype(np.float64))
        return (np.abs(A - A.transpose(0, 2, 1)).max(axis=(1, 2)) / np.abs(A).max(axis=(1, 2))).max(), A

    fig, A = asym(x)
    floor, _ = asym(x32)
    _held("J M^-1 J^T asymmetry", fig, floor)
    assert (np.linalg.eigvalsh(0.5 * (A + A.transpose(0, 2, 1))) > 0).all()


def test_solve_with_the_most_rows(ctx, sol):  # noqa: F811
    _solve_case(ctx, sol, sol.rhs32, "solve k=32")


def test_solve_rows_are_independent(ctx, sol):  # noqa: F811
    """Row j of a k = 3 call has the bits of the k = 1 call on that row."""
    rhs = sol.rhs32[:, :3].copy()
    x3 = host(sol.solver.solve(cu(rhs)))
    for j in range(3):
        x1 = host(sol.solver.solve(cu(rhs[:, j:j + 1])))
        assert np.array_equal(x1[:, 0], x3[:, j]), j
    assert not np.array_equal(x3[:, 0], x3[:, 1])
    # the no-gravity flag has nothing to act on here: accepted, same bits
    both = sol.solve.FLAG_ARMATURE | sol.solve.FLAG_NO_GRAVITY
    assert np.array_equal(host(sol.solver.solve(cu(rhs), flags=both)), x3)


# ------------------------------------------------------------------ S4: closure with the engine
def test_engine_step_acceleration_is_forward_dynamics(he_model):
    """The setup of test_gpu_dof_actuation.test_step_acceleration_closes_inverse_dynamics: 8 tumbling
    bodies in flight, every dof EFFORT, tau in +-200, one explicit PGS step, clamps out of reach. The
    engine's a = (u1 - u0) / dt against forward_dynamics((0, tau)) at the state before the step, as
    max|a - qdd| / max|a|; the yardstick is the same figure with the float64 reference's qdd in the
    kernel's place (the engine's own float32 step and the rounding of u1), to which the kernel may add 8 x
    its forward floor."""
    from humanoid_amd.solve import Solver
    from test_gpu_body_forces import load, make_engine
    n = 8
    rng = np.random.default_rng(43)
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), vel=0.5, ang=0.5)
    tau = rng.uniform(-200.0, 200.0, (n, ND)).astype(np.float32)
    sp = _abi.pgs_sim_params(bias_midpoint=0, substeps=1, angular_damping=0.0, joint_limits=0, self_collision=0,
                             max_joint_velocity=1e6, max_angular_velocity=1e6)
    eng = make_engine(he_model, n, sp)
    load(eng, root, dof, dof[..., 0].copy())
    eng.set_dof_drive_modes([_abi.DOF_MODE_EFFORT] * ND)
    assert (np.abs(tau) < np.array(he_model.effort[:ND])[None, :]).all()  # the effort clamp is out of reach too
    eng.set_dof_actuation_forces(cu(tau))
    f = np.concatenate([np.zeros((n, 6), np.float32), tau], axis=1)
    solver = Solver(eng)
    qdd = host(solver.forward_dynamics(cu(f))).astype(np.float64)

    def qd():
        return np.concatenate([host(eng.root_states)[:, 7:13], host(eng.dof_state).reshape(n, ND, 2)[:, :, 1]],
                              axis=1).astype(np.float64)

    u0 = qd()
    eng.simulate(1)
    torch.cuda.synchronize()
    assert int(eng.num_contacts.max()) == 0
    a = (qd() - u0) / float(sp.dt)
    g = tuple(sp.gravity)
    M64, c64 = SR.terms(he_model, root, dof, g, np.float64)
    M32, c32 = SR.terms(he_model, root, dof, g, np.float32)
    q64 = SR.forward_dynamics(M64, c64, f)
    floor = SR.forward_error(SR.forward_dynamics(M32, c32, f), q64).max()
    fig = (np.abs(a - qdd).max(axis=1) / np.abs(a).max(axis=1)).max()
    yard = (np.abs(a - q64).max(axis=1) / np.abs(a).max(axis=1)).max()
    print(f"engine step against forward dynamics: kernel {fig:.3e}  float64 reference (yardstick) {yard:.3e}  "
          f"forward floor {floor:.3e}  (max|a| {np.abs(a).max():.1f})")
    assert np.abs(a).max() > 100.0
    assert fig <= yard + MARGIN * floor


# ------------------------------------------------------------------ S5: mechanics
def test_second_call_is_bit_identical(ctx, sol):  # noqa: F811
    """Unchanged state, same bits: uninitialised LDS or a stray lane would show here."""
    s = sol.solver
    f, q, J = cu(sol.f), cu(sol.qdd_des), cu(ctx.J[:, R_HAND])
    first = (host(s.forward_dynamics(f)), *[host(t) for t in s.computed_torque(q, f)], host(s.solve(J)))
    outs = (torch.full((N, NG), float("nan"), device="cuda:0"), torch.full((N, ND), float("nan"), device="cuda:0"),
            torch.full((N, 6), float("nan"), device="cuda:0"), torch.full((N, 6, NG), float("nan"), device="cuda:0"))
    s.forward_dynamics(f, outs[0])
    s.computed_torque(q, f, outs[1], outs[2])
    s.solve(J, outs[3])
    for a, b in zip(first, outs):
        assert np.isfinite(a).all() and np.array_equal(a, host(b))


def test_null_outputs_and_sentinels(ctx, sol):  # noqa: F811
    """A NULL optional output of computed_torque leaves the other's bits as in the joint call and writes
    nothing else; nothing is written past the last env of any output."""
    s = sol.solver
    f, q, J = cu(sol.f), cu(sol.qdd_des), cu(ctx.J[:, R_HAND])
    tau0, ab0 = [host(t) for t in s.computed_torque(q, f)]

    def buf(numel):
        return torch.full((numel + NG,), SENTINEL, dtype=torch.float32, device="cuda:0")

    b_tau, b_ab = buf(N * ND), buf(N * 6)
    tau, none = s.computed_torque(q, f, b_tau[:N * ND].view(N, ND), want_base_acc=False)
    assert none is None and np.array_equal(host(tau), tau0)
    assert (host(b_tau)[N * ND:] == SENTINEL).all()
    none, ab = s.computed_torque(q, f, base_acc=b_ab[:N * 6].view(N, 6), want_tau=False)
    assert none is None and np.array_equal(host(ab), ab0)
    assert (host(b_ab)[N * 6:] == SENTINEL).all()
    assert np.array_equal(host(b_tau)[:N * ND].reshape(N, ND), tau0)  # untouched by the second call
    b_q, b_x, b_x1 = buf(N * NG), buf(N * 6 * NG), buf(N * NG)
    s.forward_dynamics(f, b_q[:N * NG].view(N, NG))
    s.solve(J, b_x[:N * 6 * NG].view(N, 6, NG))
    s.solve(J[:, :1].contiguous(), b_x1[:N * NG].view(N, 1, NG))
    for b, numel in ((b_q, N * NG), (b_x, N * 6 * NG), (b_x1, N * NG)):
        h = host(b)
        assert (h[numel:] == SENTINEL).all() and np.isfinite(h[:numel]).all() and not (h[:numel] == SENTINEL).any()
    # a NULL gen_force is the zero force
    assert np.array_equal(host(s.forward_dynamics(None)), host(s.forward_dynamics(torch.zeros(N, NG, device="cuda:0"))))


def test_launch_on_a_side_stream(ctx, sol):  # noqa: F811
    s = sol.solver
    f = cu(sol.f)
    want = host(s.forward_dynamics(f))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert s.engine.stream.value == side.cuda_stream
        out = s.forward_dynamics(f)
    side.synchronize()
    assert np.array_equal(host(out), want)


# ------------------------------------------------------------------ S6: refusals on the device
def test_refusals_leave_the_outputs_unchanged(ctx, sol):  # noqa: F811
    s, E = sol.solver, sol.solve.SolveError
    dev = ctx.eng.device
    out = torch.full((N, NG), SENTINEL, device=dev)
    x = torch.full((N, 6, NG), SENTINEL, device=dev)
    tau = torch.full((N, ND), SENTINEL, device=dev)
    J, q = cu(ctx.J[:, R_HAND]), cu(sol.qdd_des)
    with pytest.raises(E, match="gen_force"):
        s.forward_dynamics(torch.zeros(N, NG - 1, device=dev), out)  # shape
    with pytest.raises(E, match="gen_force"):
        s.forward_dynamics(torch.zeros(N, NG, dtype=torch.float64, device=dev), out)  # dtype
    with pytest.raises(E, match="gen_force"):
        s.forward_dynamics(torch.zeros(N, NG), out)  # device
    with pytest.raises(E, match="gen_force"):
        s.forward_dynamics(torch.zeros(NG, N, device=dev).t(), out)  # contiguity
    with pytest.raises(E, match="out"):
        s.forward_dynamics(None, torch.zeros(N, NG))
    with pytest.raises(E, match="unknown flag"):
        s.forward_dynamics(None, out, flags=4)
    with pytest.raises(E, match="qdd_des"):
        s.computed_torque(torch.zeros(N, NG, device=dev), None, tau)
    with pytest.raises(E, match="base_acc"):
        s.computed_torque(q, None, tau, torch.zeros(N, 3, device=dev))
    with pytest.raises(E, match="unknown flag"):
        s.computed_torque(q, None, tau, flags=8)
    with pytest.raises(E, match="same tensor"):
        s.solve(J, J)
    ptrs = (ctx.eng.root_states.data_ptr(), ctx.eng.dof_state.data_ptr(), J.data_ptr())
    rc = s.lib.hs_solve(s.h, *ptrs, J.data_ptr(), 6, 1, None)  # the library's own check, below the binding's
    assert rc != 0 and "same buffer" in s.lib.hs_last_error().decode()
    for k in (0, 33):
        rc = s.lib.hs_solve(s.h, *ptrs, x.data_ptr(), k, 1, None)
        assert rc != 0 and "outside 1..32" in s.lib.hs_last_error().decode()
        with pytest.raises(E, match="outside 1..32"):
            s.solve(torch.zeros(N, k, NG, device=dev), x)
    with pytest.raises(E, match="out"):
        s.solve(J, torch.zeros(N, 5, NG, device=dev))
    with pytest.raises(E, match="rhs"):
        s.solve(torch.zeros(N, NG, 6, device=dev).transpose(1, 2), x)
    with pytest.raises(E, match="root_state"):
        s.solve(J, x, root_state=torch.zeros(N, 12, device=dev))
    torch.cuda.synchronize()
    for t in (out, x, tau):
        assert (t == SENTINEL).all().item()
    assert np.array_equal(host(J), ctx.J[:, R_HAND])


# ------------------------------------------------------------------ S7: the gym facade
def test_facade_solves_see_the_pending_simulate_calls():
    """Two gym.simulate calls and no fetch_results: solve_forward_dynamics first issues them, so it sees
    the state after the steps, and equals bit for bit a direct Solver on a second sim's engine stepped
    the same way. The other two entries run on the same state."""
    from humanoid_amd.isaacgym import gymtorch
    from humanoid_amd.solve import Solver
    from test_facade_env import _facade_sim
    n = 4
    gym, sim = _facade_sim(n)
    gym2, sim2 = _facade_sim(n)
    dev = sim.engine.device
    out = torch.zeros(n, NG, device=dev)
    assert sim.dynamics is None
    gym.solve_forward_dynamics(sim, None, gymtorch.unwrap_tensor(out))
    assert sim.dynamics is not None and sim.dynamics.engine is sim.engine
    before = host(out)
    for g, s in ((gym, sim), (gym2, sim2)):
        g.simulate(s)
        g.simulate(s)
    assert sim.pending_substeps == 2
    gym.solve_forward_dynamics(sim, None, gymtorch.unwrap_tensor(out))
    assert sim.pending_substeps == 0
    after = host(out)
    gym2.fetch_results(sim2, True)
    assert sim2.pending_substeps == 0
    direct = Solver(sim2.engine)
    assert torch.equal(sim.engine.dof_state, sim2.engine.dof_state)
    want = host(direct.forward_dynamics())
    assert np.array_equal(after, want)
    assert not np.array_equal(after, before)
    # computed torque and the block solve through the facade, against the direct solver
    qdd_des = torch.full((n, ND), 5.0, device=dev)
    tau, acc = torch.zeros(n, ND, device=dev), torch.zeros(n, 6, device=dev)
    gym.solve_computed_torque(sim, gymtorch.unwrap_tensor(qdd_des), gymtorch.unwrap_tensor(tau), gymtorch.unwrap_tensor(acc))
    tau_d, acc_d = direct.computed_torque(qdd_des)
    assert torch.equal(tau, tau_d) and torch.equal(acc, acc_d) and tau.abs().max().item() > 1.0
    tau2 = torch.zeros(n, ND, device=dev)
    gym.solve_computed_torque(sim, gymtorch.unwrap_tensor(qdd_des), gymtorch.unwrap_tensor(tau2))
    assert torch.equal(tau2, tau)
    rhs = torch.eye(NG, device=dev)[:4].repeat(n, 1, 1).contiguous()
    x = torch.zeros(n, 4, NG, device=dev)
    gym.solve_mass_matrix(sim, gymtorch.unwrap_tensor(rhs), gymtorch.unwrap_tensor(x))
    assert torch.equal(x, direct.solve(rhs))
    torch.cuda.synchronize()
