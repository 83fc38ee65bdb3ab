"""GPU checks of the inverse kinematics (include/humanoid_ik.h) against the float64 numpy reference of
tests/ik_reference.py, which tests/test_ik.py pins. Six envs: env 0 as the engine creates it (standing at
the origin, every dof zero: the series branches of the rotations), 1-5 the convergence inputs of
ik_reference (cases.random_state(ang=0.4) starts within the limits, targets read from poses up to 0.05 m
and 0.15 rad per dof away). At most 8 iterations a launch.

Tolerance per figure: 8 x that figure's own float32 floor (MARGIN of tests/test_gpu_dynamics.py). The floor
is ik_reference evaluated in float32 against float64 on the same inputs; it is computed and printed here
and never taken from the kernel. Figures are absolute: metres, radians, quaternion components.

Floors and the kernel's measured figures (MI355X; floor / kernel; every test prints them, `pytest -s`):

    one iteration      root position m    root quaternion    dof angles rad
    k = 1              1.5e-8 / 3.3e-11   6.0e-8 / 6.0e-8    2.4e-7 / 2.4e-7
    k = 6              3.0e-8 / 1.5e-8    2.3e-7 / 3.5e-7    1.8e-6 / 4.6e-6
    k = 12             3.0e-8 / 1.2e-7    1.5e-7 / 6.1e-7    2.1e-6 / 5.5e-6
    k = 32             6.0e-8 / 3.0e-8    7.2e-7 / 1.9e-6    5.8e-6 / 7.8e-6
    control path, 6    3.0e-8 / 2.8e-8    2.3e-7 / 1.2e-7    1.8e-6 / 8.4e-7
    control path, 32   6.0e-8 / 4.6e-8    7.2e-7 / 4.1e-7    5.8e-6 / 2.0e-6

    eight iterations   residual_out - e64(pose)   worst residual (m or rad)
    k = 6              3.2e-7 / 1.4e-7            2.0e-7 / 2.0e-7
    k = 9              1.8e-7 / 1.3e-7            2.3e-7 / 1.6e-7
    k = 12             2.3e-7 / 1.8e-7            1.7e-7 / 1.8e-7
    k = 15             2.6e-7 / 1.2e-7            2.4e-7 / 2.5e-7

The kernel's worst is 0.51 of its tolerance (k = 12, one iteration, the root quaternion). Through the facade
the written state's points sit 7.6e-8 m from their targets (floor 1.3e-7). The module runs in 7 s.

The facade test reads the points from the float64 kinematics of the sim's root and dof tensors after the
two indexed writes: the rigid-body tensor is filled by the step kernels, not by an indexed write.
"""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import ik_reference as IK  # noqa: E402
import task_reference as TR  # noqa: E402
from test_gpu_dynamics import MARGIN  # noqa: E402

from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
NB, ND, NG = DR.NB, DR.ND, DR.NG
N = 6
DAMPING, CLIP = 1e-4, 0.1
FIGURES = ("root_pos", "root_quat", "dof")


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _held(name, fig, floor):
    print(f"{name}: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    assert np.isfinite(fig) and fig <= MARGIN * floor, (name, fig, MARGIN * floor)


def _pose_figures(root, dof, root64, dof64):
    """The three figures of a pose against another: largest differences of the root position, the root
    quaternion and the dof angles."""
    root, dof = np.asarray(root, np.float64), np.asarray(dof, np.float64).reshape(-1, ND, 2)
    return dict(root_pos=np.abs(root[:, :3] - root64[:, :3]).max(), root_quat=np.abs(root[:, 3:7] - root64[:, 3:7]).max(),
                dof=np.abs(dof[..., 0] - dof64[..., 0]).max())


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ik(model, he_model):
    """One engine of six envs in the module's states, one InverseKinematics, the row sets with their
    targets, and a cache of the reference's results (computed once, left unchanged)."""
    from humanoid_amd import ik as ikmod
    from humanoid_amd.engine import Engine
    c = _Ctx()
    c.mod, c.he_model = ikmod, he_model
    c.eng = Engine(model, N, device=0)
    dev = c.eng.device
    root, dof, g_root, g_dof = IK.convergence_inputs(he_model, N, 17, rest_first=True)
    ids = torch.arange(1, N, dtype=torch.int32, device=dev)
    c.eng.set_root_state_indexed(cu(root), ids)
    c.eng.set_dof_state_indexed(cu(dof.reshape(N * ND, 2)), ids)
    torch.cuda.synchronize()
    c.root = host(c.eng.root_states)
    c.dof = host(c.eng.dof_state).reshape(N, ND, 2)
    assert np.array_equal(c.root[1:], root[1:]) and np.array_equal(c.dof[1:], dof[1:])
    assert c.root[0, 6] == 1.0 and abs(c.root[0, 2] - 0.89) < 1e-6 and not c.dof[0].any() and not c.root[0, :2].any()
    assert np.abs(c.root[1:, 7:]).max() > 0.5 and np.abs(c.dof[1:, :, 1]).max() > 0.5  # the velocities must not matter
    names = list(BODY_NAMES)
    c.sets = dict(TR.row_sets(names))
    c.sets.update({("conv", k): rows for k, rows in IK.convergence_rows(names).items()})
    c.targets = {k: IK.targets_of(he_model, g_root, g_dof, rows) for k, rows in c.sets.items()}
    c.ik = ikmod.InverseKinematics(c.eng)
    cache = {}

    def ref(key, iterations, dtype, limits=True):
        k = (key, iterations, dtype, limits)
        if k not in cache:
            tgt, trot = c.targets[key]
            cache[k] = IK.solve(he_model, c.root, c.dof, c.sets[key], tgt, trot, iterations, DAMPING, CLIP, dtype,
                                limits=limits)
        return cache[k]

    def run(key, iterations=1, **kw):
        tgt, trot = c.targets[key]
        c.ik.set_rows(c.sets[key])
        return c.ik.solve(cu(tgt), cu(trot), iterations, DAMPING, CLIP, **kw)

    c.ref, c.run = ref, run
    yield c
    del c.ik, c.eng


# ------------------------------------------------------------------ T1: one iteration against the reference
@pytest.mark.parametrize("k", [1, 6, 12, 32])
def test_one_iteration_matches_the_reference(ik, k):
    r64, d64, _ = ik.ref(k, 1, np.float64)
    r32, d32, _ = ik.ref(k, 1, np.float32)
    floor = _pose_figures(r32, d32, r64.astype(np.float64), d64.astype(np.float64))
    root, dof, res = (host(t) for t in ik.run(k))
    assert root.shape == (N, 13) and dof.shape == (N * ND, 2) and res.shape == (N, k)
    fig = _pose_figures(root, dof, r64.astype(np.float64), d64.astype(np.float64))
    for name in FIGURES:
        _held(f"k={k} one iteration {name}", fig[name], floor[name])
    assert not root[:, 7:].any() and not dof[:, 1].any()  # exactly zero
    assert np.abs(np.linalg.norm(root[:, 3:7].astype(np.float64), axis=1) - 1).max() <= 1e-6
    moved = np.abs(dof.reshape(N, ND, 2)[..., 0] - ik.dof[..., 0])
    if k != 1:  # (a row at the hand's origin does not see the hand's own joint)
        assert moved[:, 66:69].max() > 1e-4  # R_Hand's own dofs: the step's register tail
    assert np.abs(res).max() < np.abs(IK.row_errors(ik.he_model, ik.root, ik.dof, ik.sets[k], *ik.targets[k])).max()


# ------------------------------------------------------------------ T2: against the kernel's own control path
@pytest.mark.parametrize("k", [6, 32])
def test_one_iteration_is_the_control_path_integrated(ik, k):
    """ht_task_control in force mode with xdd_des = the clamped errors at the zero-velocity copy of the state,
    without gravity; its qdd through the reference's float64 integration; within T1's tolerance of hk_solve."""
    from humanoid_amd import task
    rows = ik.sets[k]
    tgt, trot = ik.targets[k]
    e = IK.row_errors(ik.he_model, ik.root, ik.dof, rows, tgt, trot)
    ebar = np.clip(e, -CLIP, CLIP).astype(np.float32)
    root0, dof0 = ik.root.copy(), ik.dof.copy()
    root0[:, 7:] = 0
    dof0[..., 1] = 0
    ts = task.TaskSpace(ik.eng)
    ts.set_rows(rows)
    _, _, qdd = ts.control(cu(ebar), None, "force", DAMPING, flags=task.FLAG_ARMATURE | task.FLAG_NO_GRAVITY,
                           root_state=cu(root0), dof_state=cu(dof0.reshape(N * ND, 2)), want_gen_force=False,
                           want_task_force=False)
    qdd = host(qdd).astype(np.float64)
    lim = IK.limits_of(ik.he_model)
    want_r, want_d = np.zeros((N, 13)), np.zeros((N, ND, 2))
    for i in range(N):
        want_r[i], want_d[i] = IK.integrate(root0[i], dof0[i], qdd[i], np.float64, lim)
    r64, d64, _ = ik.ref(k, 1, np.float64)
    r32, d32, _ = ik.ref(k, 1, np.float32)
    floor = _pose_figures(r32, d32, r64.astype(np.float64), d64.astype(np.float64))
    root, dof = (host(t) for t in ik.run(k, want_residual=False)[:2])
    fig = _pose_figures(root, dof, want_r, want_d)
    for name in FIGURES:
        _held(f"k={k} control path integrated {name}", fig[name], floor[name])
    del ts


# ------------------------------------------------------------------ T3: eight iterations
@pytest.mark.parametrize("k", [6, 9, 12, 15])
def test_eight_iterations_converge(ik, k):
    key = ("conv", k)
    rows = ik.sets[key]
    tgt, trot = ik.targets[key]
    root, dof, res = (host(t) for t in ik.run(key, 8))
    dof3 = dof.reshape(N, ND, 2)
    # residual_out is the error at the returned pose: the reference in both dtypes at that pose
    e64 = IK.row_errors(ik.he_model, root, dof3, rows, tgt, trot, np.float64)
    e32 = IK.row_errors(ik.he_model, root, dof3, rows, tgt, trot, np.float32)
    _held(f"k={k} residual_out against the float64 residual of the returned pose", np.abs(res - e64).max(),
          np.abs(e32 - e64).max())
    # the worst residual against the float32 reference's own after 8 iterations
    r32, d32, _ = ik.ref(key, 8, np.float32)
    floor = np.abs(IK.row_errors(ik.he_model, r32, d32, rows, tgt, trot, np.float64)).max()
    _held(f"k={k} worst residual after 8 iterations", np.abs(e64).max(), floor)
    r64, d64, res64 = ik.ref(key, 8, np.float64)
    assert np.abs(res64).max() <= 1e-6
    assert not root[:, 7:].any() and not dof[:, 1].any()
    lo, up = IK.limits_of(ik.he_model, np.float32)
    assert (dof3[..., 0] >= lo).all() and (dof3[..., 0] <= up).all()


# ------------------------------------------------------------------ T4: fed-back launches, bit for bit
def test_iterations_in_one_launch_are_launches_fed_back(ik, model):
    from humanoid_amd.engine import Engine
    for key in (6, ("conv", 15), 32):
        root4, dof4, res4 = ik.run(key, 4)
        r, d = None, None
        for _ in range(4):
            r, d, res = ik.run(key, 1, root_state=r, dof_state=d)
        assert torch.equal(r, root4) and torch.equal(d, dof4) and torch.equal(res, res4), key
        # in place: the outputs are the given starting pose
        r, d = ik.eng.root_states.clone(), ik.eng.dof_state.clone()
        r2, d2, res2 = ik.run(key, 4, root_state=r, dof_state=d, root_out=r, dof_out=d)
        assert r2 is r and d2 is d and torch.equal(r, root4) and torch.equal(d, dof4) and torch.equal(res2, res4), key
        # without the residual the pose has the same bits
        r3, d3, none = ik.run(key, 4, want_residual=False)
        assert none is None and torch.equal(r3, root4) and torch.equal(d3, dof4)
    # one env alone: env 0 of the six
    eng1 = Engine(model, 1, device=0)
    one = ik.mod.InverseKinematics(eng1)
    assert torch.equal(eng1.root_states, ik.eng.root_states[:1]) and torch.equal(eng1.dof_state, ik.eng.dof_state[:ND])
    for key in (6, 32):
        tgt, trot = ik.targets[key]
        one.set_rows(ik.sets[key])
        r1, d1, res1 = one.solve(cu(tgt[:1]), cu(trot[:1]), 4, DAMPING, CLIP)
        root4, dof4, res4 = ik.run(key, 4)
        assert torch.equal(r1, root4[:1]) and torch.equal(d1, dof4[:ND]) and torch.equal(res1, res4[:1]), key
    del one, eng1


# ------------------------------------------------------------------ T5: limits
def test_a_binding_limit_is_met_exactly(ik):
    """The engine's model with one dof boxed to 5 mrad about the starts: the reference's unconstrained
    iteration leaves the box (asserted), the kernel ends exactly on the box with the limits on, outside
    with them off."""
    from humanoid_amd.engine import Engine
    key = ("conv", 9)
    free = ik.ref(key, 2, np.float64, limits=False)
    moved = np.abs(free[1][1:, :, 0] - ik.dof[1:, :, 0]).max(axis=0)
    d = int(np.argmax(moved))
    assert moved[d] > 0.02
    m = copy.deepcopy(ik.he_model)
    start = ik.dof[:, d, 0]
    m.dof_lower[d], m.dof_upper[d] = float(start.min() - 0.005), float(start.max() + 0.005)
    lo, up = IK.limits_of(m, np.float32)
    eng = Engine(m, N, device=0)
    boxed = ik.mod.InverseKinematics(eng)
    boxed.set_rows(ik.sets[key])
    tgt, trot = ik.targets[key]
    state = dict(root_state=cu(ik.root), dof_state=cu(ik.dof.reshape(N * ND, 2)))
    held = host(boxed.solve(cu(tgt), cu(trot), 2, DAMPING, CLIP, **state)[1]).reshape(N, ND, 2)[..., 0]
    loose = host(boxed.solve(cu(tgt), cu(trot), 2, DAMPING, CLIP, limits=False, **state)[1]).reshape(N, ND, 2)[..., 0]
    assert (held >= lo).all() and (held <= up).all()
    assert ((held[:, d] == lo[d]) | (held[:, d] == up[d])).any()
    out = (loose[:, d] > up[d]) | (loose[:, d] < lo[d])
    assert out.any() and ((held[out, d] == lo[d]) | (held[out, d] == up[d])).all()
    # the engine's own limits are wide: the unboxed handle gives the loose pose
    assert np.array_equal(host(ik.run(key, 2)[1]).reshape(N, ND, 2)[..., 0], loose)
    del boxed, eng


# ------------------------------------------------------------------ T6: the engine's state and the facade
def test_the_engine_state_is_not_touched_and_the_facade_reaches_the_targets(ik):
    from humanoid_amd.isaacgym import gymtorch
    from test_facade_env import _facade_sim
    E = ik.mod.IKError
    before = [t.clone() for t in (ik.eng.root_states, ik.eng.dof_state, ik.eng.rb_state)]
    ik.run(("conv", 15), 8)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (ik.eng.root_states, ik.eng.dof_state, ik.eng.rb_state)))
    with pytest.raises(E, match="root_out aliases the engine's state"):
        ik.run(6, root_out=ik.eng.root_states)
    with pytest.raises(E, match="dof_out aliases the engine's state"):
        ik.run(6, dof_out=ik.eng.dof_state)
    with pytest.raises(E, match="target_rot is None"):
        ik.ik.solve(cu(ik.targets[6][0]))
    with pytest.raises(E, match="iterations"):
        ik.run(6, 65)
    assert all(torch.equal(a, b) for a, b in zip(before, (ik.eng.root_states, ik.eng.dof_state, ik.eng.rb_state)))

    # the facade: solve, write the pose with the two indexed writes, read the points of the written state
    n = 4
    gym, sim = _facade_sim(n)
    dev = sim.engine.device
    root_t = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    dof_t = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    hand = BODY_NAMES.index("R_Hand")
    rows = [("R_Hand", a) for a in range(3)] + [("Head", a) for a in range(3)]
    gym.simulate(sim)  # the rigid-body tensor is filled by a step
    gym.fetch_results(sim, True)
    gym.refresh_rigid_body_state_tensor(sim)
    rb0 = host(rb).reshape(n, NB, 13)
    head = BODY_NAMES.index("Head")
    assert np.abs(rb0[:, head, 2] - rb0[:, 0, 2]).min() > 0.3  # filled: the head is above the pelvis
    shift = np.array([[0.04, -0.03, 0.05], [-0.02, 0.03, -0.04]], np.float32)
    tgt = np.concatenate([rb0[:, hand, :3] + shift[0], rb0[:, head, :3] + shift[1]], axis=1).astype(np.float32)
    target = cu(tgt)
    root_out, dof_out = torch.zeros(n, 13, device=dev), torch.zeros(n * ND, 2, device=dev)
    res = torch.zeros(n, 6, device=dev)
    with pytest.raises(E, match="no rows set"):
        gym.solve_inverse_kinematics(sim, gymtorch.unwrap_tensor(target), gymtorch.unwrap_tensor(root_out),
                                     gymtorch.unwrap_tensor(dof_out))
    assert gym.set_ik_rows(sim, rows)
    gym.simulate(sim)
    assert sim.pending_substeps == 1
    with pytest.raises(E, match="aliases the engine's state"):
        gym.solve_inverse_kinematics(sim, gymtorch.unwrap_tensor(target), gymtorch.unwrap_tensor(root_t),
                                     gymtorch.unwrap_tensor(dof_out))
    assert sim.pending_substeps == 0  # flushed first
    live = [root_t.clone(), dof_t.clone()]
    assert gym.solve_inverse_kinematics(sim, gymtorch.unwrap_tensor(target), gymtorch.unwrap_tensor(root_out),
                                        gymtorch.unwrap_tensor(dof_out), residual_desc=gymtorch.unwrap_tensor(res))
    assert torch.equal(root_t, live[0]) and torch.equal(dof_t, live[1])
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(root_out), gymtorch.unwrap_tensor(ids), n)
    gym.set_dof_state_tensor_indexed(sim, gymtorch.unwrap_tensor(dof_out), gymtorch.unwrap_tensor(ids), n)
    assert torch.equal(root_t, root_out) and torch.equal(dof_t, dof_out)
    # The points of the sim's state after the writes, by the float64 kinematics of its root and dof tensors: the
    # rigid-body tensor is filled by the step kernels, not by an indexed write, and a step would move the
    # bodies off the pose.
    Mo = DR.Model(ik.he_model, np.float64)
    r1, d1 = host(root_t), host(dof_t).reshape(n, ND, 2)
    got = np.zeros((n, 6))
    for i in range(n):
        _, p = DR.fk(Mo, r1[i], d1[i])
        got[i] = np.concatenate([p[hand], p[head]])
    # T3's tolerance: 8 x the float32 reference's worst residual after the same 8 iterations from the same state
    r0, d0 = host(live[0]), host(live[1]).reshape(n, ND, 2)
    rows_i = [(BODY_NAMES.index(b), a, (0.0, 0.0, 0.0)) for b, a in rows]
    r32, d32, _ = IK.solve(ik.he_model, r0, d0, rows_i, tgt, None, 8, DAMPING, CLIP, np.float32)
    floor = np.abs(IK.row_errors(ik.he_model, r32, d32, rows_i, tgt, None, np.float64)).max()
    assert floor < 1e-6  # the reference has converged: the bound below is a bound
    _held("facade: the points' distance from their targets", np.abs(got - tgt).max(), floor)
    assert np.abs(host(res)).max() <= MARGIN * floor
    assert np.abs(got[:, :3] - rb0[:, hand, :3]).max() > 0.03  # the hand did move
