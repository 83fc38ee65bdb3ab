"""The physics step's body-lane phases on their rare paths and on the root / non-body lanes (DESIGN §4.1
"Control skeleton"): the integration tests its rare cases once per wave (the joint-rate and world
angular-velocity clamps, ocml's sincosf behind the half-angle series, the limit backstop) and the
rotation exponential / logarithm select their small-angle forms, so a wave in which one lane takes such a
path beside lanes that do not, or none does, has to give what the oracle gives. A handful of envs, one
policy step, TGS and PGS, each against oracle.physics_step through the parity tests' own comparison
(test_gpu_parity._physics_compare: its arrays, its one-step tolerances and its sensitivity probes).
States are given as the state tensors' arrays, which _physics_compare writes into the engine's zero-copy
root_states / dof_state views."""
import numpy as np
import pytest

import cases
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

N = 12
SOLVERS = [pytest.param(dict(solver_type=1), id="tgs"), pytest.param(dict(solver_type=0, solver_iterations=8), id="pgs")]


def _airborne(rng, n=N, **kw):
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), **kw)
    targets = rng.uniform(-0.5, 0.5, (n, 69)).astype(np.float32)
    return root, dof, targets


@pytest.mark.parametrize("solver", SOLVERS)
def test_both_velocity_clamps_beside_unclamped_envs(he_model, solver):
    """Joint rates above max_joint_velocity and chains whose summed rates pass max_angular_velocity in the
    even envs, slow bodies that reach neither in the odd ones: the wave tests decide per env."""
    rng = np.random.default_rng(61)
    root, dof, targets = _airborne(rng, vel=0.0)
    root[0::2, 10:13] = rng.normal(0, 20.0, (N // 2, 3)).astype(np.float32)
    dof[0::2, :, 1] = rng.normal(0, 25.0, (N // 2, 69)).astype(np.float32)
    dof[1::2, :, 1] = rng.normal(0, 0.5, (N // 2, 69)).astype(np.float32)
    # env 0: one joint alone over the joint cap, every chain under the world cap
    root[0, 10:13] = 0.0
    dof[0, :, 1] = 0.0
    dof[0, 3 * 7:3 * 7 + 3, 1] = (35.0, 0.0, 0.0)
    eng, _ = P._physics_compare(he_model, root, dof, targets, self_collision=0, max_angular_velocity=40.0,
                                max_joint_velocity=30.0, max_skip=0.0, max_widened=0.0, **solver)
    w = np.linalg.norm(eng.rb_state.view(N, 24, 13).cpu().numpy()[..., 10:13].astype(np.float64), axis=-1)
    assert w.max() < 40.0 * 1.5, w.max()


@pytest.mark.parametrize("solver", SOLVERS)
def test_joint_turned_past_two_radians_in_one_iteration(he_model, solver):
    """A free distal joint at 150 rad/s under one substep of 1/60 s (TGS: one position iteration) turns
    2.5 rad per integration: the half angle leaves the series' range, and that lane takes sincosf while the
    other 22 joints and the root keep the series. Caps lifted, drives and limits off. (The rate is the
    least that reaches the path: the position tolerance is absolute, and a rate's fp32 rounding times the
    step grows with the rate.)"""
    rng = np.random.default_rng(62)
    root, dof, targets = _airborne(rng)
    joints = np.where(np.arange(N) % 3 == 0, 22, np.where(np.arange(N) % 3 == 1, 17, -1))  # -1: no fast joint
    for e, j in enumerate(joints):
        if j >= 0:
            axis = rng.standard_normal(3)
            dof[e, 3 * j:3 * j + 3, 1] = (150.0 * axis / np.linalg.norm(axis)).astype(np.float32)
    sim = dict(solver, substeps=1)
    if sim["solver_type"] == 1:
        sim["solver_iterations"] = 1
    P._physics_compare(he_model, root, dof, targets, self_collision=0, joint_limits=0, kp_scale=0.0, kd_scale=0.0,
                       max_joint_velocity=1000.0, max_angular_velocity=5000.0, max_skip=0.0, **sim)


@pytest.mark.parametrize("solver", SOLVERS)
def test_limit_backstop_acts_with_limit_rows_present(he_model, model, solver):
    """Joints 5 mrad from pi (inside kLimitGuard, past the backstop's cap at pi - kLimitGuard / 2) moving
    outward at 60 rad/s in the even envs: their limit rows are present (the gap is negative) and cannot
    bring the angle under the cap within the step, so limit_clamp acts; the odd envs hang at rest."""
    rng = np.random.default_rng(63)
    root, dof = cases.standing_state(model, N, rng, xy_jitter=0.5)
    root[:, 2] += 1.5
    joints = rng.integers(0, 23, N)
    for e in range(0, N, 2):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        j = joints[e]
        dof[e, 3 * j:3 * j + 3, 0] = (axis * (np.pi - 0.005)).astype(np.float32)
        dof[e, 3 * j:3 * j + 3, 1] = (axis * 60.0).astype(np.float32)
    eng, _ = P._physics_compare(he_model, root, dof, np.zeros((N, 69), np.float32), max_skip=0.0, self_collision=0,
                                kp_scale=0.0, kd_scale=0.0, **solver)
    q = eng.dof_state.view(N, 69, 2).cpu().numpy()[..., 0].reshape(N, 23, 3)
    t = np.linalg.norm(q[np.arange(N), joints].astype(np.float64), axis=1)[0::2]
    assert (t <= np.pi - 0.01 + 2e-6).all() and (t > np.pi - 0.1).all(), t


@pytest.mark.parametrize("solver", SOLVERS)
def test_env_without_rows_beside_env_with_rows(he_model, model, solver):
    """Airborne envs with no contact and no limit row (TGS: tgs_free_iterations) and standing envs with
    their foot contacts in the same launch."""
    rng = np.random.default_rng(64)
    root, dof = cases.standing_state(model, N, rng, xy_jitter=1.0)
    ra, da = cases.random_state(N // 2, rng, height=(3.0, 4.0), ang=0.3)
    root[1::2], dof[1::2] = ra, da
    targets = np.zeros((N, 69), np.float32)
    targets[1::2] = da[..., 0]
    _, out = P._physics_compare(he_model, root, dof, targets, self_collision=0, max_skip=0.0, **solver)
    assert (out["num_contacts"][1::2] == 0).all() and (out["num_contacts"][0::2] > 0).all()


@pytest.mark.parametrize("solver", SOLVERS)
def test_negative_zero_root_velocity_and_zero_rate_joints(he_model, solver):
    """Root velocity components of -0.0 and +0.0 and joints at zero rate (of either sign): the root's and the rate-less joints' terms enter the chain sums as zeros."""
    rng = np.random.default_rng(65)
    root, dof, targets = _airborne(rng)
    root[0::2, 7] = -0.0
    root[0::3, 9] = -0.0
    root[1::2, 11] = -0.0
    root[2, 7:13] = -0.0
    root[3, 7:13] = 0.0
    for e in range(N):
        j = rng.choice(23, 6, replace=False)
        for k in j[:3]:
            dof[e, 3 * k:3 * k + 3, 1] = 0.0
        for k in j[3:]:
            dof[e, 3 * k:3 * k + 3, 1] = -0.0
    dof[2, :, 1] = -0.0
    dof[3, :, 1] = 0.0
    targets[2:4] = dof[2:4, :, 0]
    P._physics_compare(he_model, root, dof, targets, self_collision=0, max_skip=0.0, max_widened=0.0, **solver)
