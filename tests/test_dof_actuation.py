"""Torque control without a GPU (he_set_dof_drive_modes, he_set_dof_actuation_forces): the
C ABI's new symbols, the premise of the GPU test that equates a joint torque with a pair of body
torques (tests/test_gpu_dof_actuation.py), in float64, and the gym facade's checks that run before
prepare_sim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from humanoid_amd.body_sets import BODY_NAMES

from test_independent_dynamics import Body, _fk, _flow, _jacobians

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, ND, NG = 24, 69, 75
SYMBOLS = ("he_set_dof_drive_modes", "he_set_dof_actuation_forces", "he_set_dof_actuation_forces_indexed")


# ------------------------------------------------------------------ C1: the ABI
def test_header_compiles_and_library_exports_the_symbols(tmp_path):
    from humanoid_amd import _abi, engine
    src = tmp_path / "act.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_engine.h"\n'
                   "#define SAME(f, t) _Static_assert(__builtin_types_compatible_p(__typeof__(&f), t), #f)\n"
                   "SAME(he_set_dof_drive_modes, int (*)(he_engine*, const int32_t*));\n"
                   "SAME(he_set_dof_actuation_forces, int (*)(he_engine*, const float*, void*));\n"
                   "SAME(he_set_dof_actuation_forces_indexed, int (*)(he_engine*, const float*, const int32_t*, int, void*));\n"
                   'int main(){printf("%d %d %d %d %d\\n", HE_DOF_MODE_NONE, HE_DOF_MODE_POS, HE_DOF_MODE_VEL,'
                   " HE_DOF_MODE_EFFORT, (int)HE_BUF_COUNT); return 0;}\n")
    exe = tmp_path / "act"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [_abi.DOF_MODE_NONE, _abi.DOF_MODE_POS, _abi.DOF_MODE_VEL, _abi.DOF_MODE_EFFORT, 12]
    assert (_abi.DOF_MODE_NONE, _abi.DOF_MODE_POS, _abi.DOF_MODE_VEL, _abi.DOF_MODE_EFFORT) == (0, 1, 2, 3)
    lib = C.CDLL(engine.LIB_PATH)  # loads without a GPU
    assert all(hasattr(lib, s) for s in SYMBOLS)
    V, I = C.c_void_p, C.c_int
    assert _abi.ACTUATION_PROTOTYPES == {SYMBOLS[0]: [V, V], SYMBOLS[1]: [V, V, V], SYMBOLS[2]: [V, V, V, I, V]}
    assert all(engine.HE_PROTOTYPES[s] == _abi.ACTUATION_PROTOTYPES[s] for s in SYMBOLS)
    # refused without a handle, with a reason, on a machine without a GPU too
    bound = engine.load_library()
    modes = (C.c_int32 * ND)(*([1] * ND))
    assert bound.he_set_dof_drive_modes(None, modes) != 0 and b"null handle" in bound.he_last_error()
    assert bound.he_set_dof_actuation_forces(None, None, None) != 0 and b"null handle" in bound.he_last_error()
    assert bound.he_set_dof_actuation_forces_indexed(None, None, None, 0, None) != 0
    assert b"null handle" in bound.he_last_error()


# ------------------------------------------------------------------ C2: a joint torque is a torque pair
JOINTS = ("L_Hip", "Spine", "L_Shoulder", "R_Hand")


def test_torque_pair_on_child_and_parent_is_the_joint_torque(he_model):
    """The world torque +t R_child e_k on a joint's child body and -t R_child e_k on its parent has
    the generalized force t on that joint's dof k and 0 on the other 74 (by virtual power with the
    finite-difference angular Jacobians of the numpy kinematics): the joint's relative rate is in the
    child's frame, and every other dof turns child and parent alike or neither. 5 random poses, a
    hip, a spine joint, a shoulder and a hand, each axis.
    The tolerance is the Jacobians' own error: every body turns rigidly with the root, so the root's
    angular columns of every Jo_b are the identity and its linear columns zero; eps is the largest
    entry of that residual over the pose's bodies. An entry of Q is tau . (Jo_child - Jo_parent)[:, i]
    with |tau| = t, so it is off by at most 2 sqrt(3) t eps.
    Measured: largest |Q - t e| 8.8e-11 against a bound of 3.4e-10 at that pose (t = 1.4)."""
    import cases
    B = Body(he_model)
    root, dof = cases.random_state(5, np.random.default_rng(3), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
    worst = bound_at_worst = 0.0
    t = 1.4
    for e in range(5):
        _, Jo, _ = _jacobians(B, root[e], dof[e])
        R, _p = _fk(B, _flow(root[e], dof[e], np.zeros(NG), 0.0))
        eps = max(float(np.abs(Jo[:, :, 0:3] - np.eye(3)[None]).max()), float(np.abs(Jo[:, :, 3:6]).max()))
        tol = 2.0 * np.sqrt(3.0) * t * eps
        for name in JOINTS:
            b = BODY_NAMES.index(name)
            a = int(B.parents[b])
            for k in range(3):
                tau = t * R[b][:, k]
                Q = Jo[b].T @ tau - Jo[a].T @ tau
                want = np.zeros(NG)
                want[6 + 3 * (b - 1) + k] = t
                err = float(np.abs(Q - want).max())
                if err > worst:
                    worst, bound_at_worst = err, tol
                assert err <= tol, (e, name, k, err, tol)
    print(f"\ntorque pair: largest |Q - t e| {worst:.3e} (bound there {bound_at_worst:.3e})")
    assert worst > 0.0  # the Jacobians are numerical: an exact zero would mean nothing was compared


# ------------------------------------------------------------------ C3: the facade before prepare_sim
def _sim_with_env():
    from humanoid_amd.isaacgym import gymapi
    from humanoid_amd.model import DEFAULT_MODEL_JSON
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    asset = gym.load_asset(sim, "/", DEFAULT_MODEL_JSON, gymapi.AssetOptions())
    envs = [gym.create_env(sim, gymapi.Vec3(-5, -5, 0), gymapi.Vec3(5, 5, 5), 4) for _ in range(2)]
    for i, env in enumerate(envs):
        gym.create_actor(env, asset, gymapi.Transform(), f"humanoid_{i}", i, 0, 0)
    return gymapi, gym, sim, asset, envs


def test_facade_accepts_effort_and_none_and_refuses_the_rest():
    gymapi, gym, sim, asset, envs = _sim_with_env()
    props = gym.get_asset_dof_properties(asset)
    assert np.all(props["driveMode"] == gymapi.DOF_MODE_NONE)  # get_asset_dof_properties is unchanged
    props["driveMode"] = gymapi.DOF_MODE_POS
    props["driveMode"][42:] = gymapi.DOF_MODE_EFFORT
    props["driveMode"][:3] = gymapi.DOF_MODE_NONE
    assert gym.set_actor_dof_properties(envs[0], 0, props) is True
    assert sim.dof_modes.tolist() == [0] * 3 + [1] * 39 + [3] * 27
    # the same modes on the next env pass; other modes there do not
    assert gym.set_actor_dof_properties(envs[1], 0, props) is True
    other = props.copy()
    other["driveMode"][10] = gymapi.DOF_MODE_EFFORT
    with pytest.raises(NotImplementedError, match="drive modes differ"):
        gym.set_actor_dof_properties(envs[1], 0, other)
    vel = props.copy()
    vel["driveMode"][5] = gymapi.DOF_MODE_VEL
    with pytest.raises(NotImplementedError, match="velocity target"):
        gym.set_actor_dof_properties(envs[1], 0, vel)
    # a refused call left the sim's modes as they were
    assert sim.dof_modes.tolist() == [0] * 3 + [1] * 39 + [3] * 27
    assert hasattr(gym, "set_dof_actuation_force_tensor") and hasattr(gym, "set_dof_actuation_force_tensor_indexed")


def test_facade_vel_mode_raises_on_the_first_env_too():
    gymapi, gym, sim, asset, envs = _sim_with_env()
    props = gym.get_asset_dof_properties(asset)
    props["driveMode"] = gymapi.DOF_MODE_VEL
    with pytest.raises(NotImplementedError, match="DOF_MODE_VEL"):
        gym.set_actor_dof_properties(envs[0], 0, props)
    assert sim.dof_modes is None
