"""GPU checks of the force sensors behind the gym facade (gym.create_asset_force_sensor /
acquire_force_sensor_tensor / refresh_force_sensor_tensor; humanoid_amd/sensors.py defines the reading)
against tests/reaction_reference.py's sensor_reading on the engine's own buffers. Five humanoids stand on the
plane under their PD drives; sensors on both ankles (the right one offset and rotated) and on one wrist in
world axes.

Tolerance: 8 x the reading's own float32 floor (MARGIN of tests/test_gpu_dynamics.py): the normwise error
per env, max|x - x64| / max|x64| over the env's readings, the largest over the envs; the floor is the same
figure of the reference evaluated in float32 on the same buffers, computed and printed here.

Measured (MI355X): through the facade after four launches of two simulate calls, floor 5.82e-08, tolerance
4.66e-07, readings 4.06e-08; on an engine directly after three simulate calls, floor 4.31e-07, readings
1.78e-07. Standing, the two ankles' vertical forces sum to -686.6 N per env (on the ankles, by the shins) with
687.5 N of weight above the ankles and 726.1 N of contact force under the feet.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import reaction_reference as RR  # noqa: E402
from test_gpu_dynamics import MARGIN  # noqa: E402

from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
N = 5
NB, ND, NG = DR.NB, DR.ND, DR.NG
L_ANKLE, R_ANKLE, L_WRIST = (BODY_NAMES.index(b) for b in ("L_Ankle", "R_Ankle", "L_Wrist"))
Q = np.array([0.1, -0.3, 0.2, 0.9]) / np.linalg.norm([0.1, -0.3, 0.2, 0.9])
POSES = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.03, -0.02, -0.05] + Q.tolist(), [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]
BODIES, WORLD = [L_ANKLE, R_ANKLE, L_WRIST], [False, False, True]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _facade_sim(n, sensors=True):
    """tests/test_facade_env.py's sim: n humanoids on the plane under DOF_MODE_POS drives, here with sensors."""
    from humanoid_amd.isaacgym import gymapi
    from humanoid_amd.model import DEFAULT_MODEL_JSON
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    opts = gymapi.AssetOptions()
    opts.angular_damping, opts.max_angular_velocity = 0.01, 100.0
    opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
    asset = gym.load_asset(sim, "/", DEFAULT_MODEL_JSON, opts)
    if sensors:
        for b, pose, world in zip(BODIES, POSES, WORLD):
            props = gymapi.ForceSensorProperties()
            props.use_world_frame = world
            t = gymapi.Transform(gymapi.Vec3(*pose[:3]), gymapi.Quat(*pose[3:]))
            assert gym.create_asset_force_sensor(asset, gym.find_asset_rigid_body_index(asset, BODY_NAMES[b]), t, props) == \
                len(asset.force_sensors) - 1
    gym.add_ground(sim, gymapi.PlaneParams())
    dof_prop = gym.get_asset_dof_properties(asset)
    dof_prop["driveMode"] = gymapi.DOF_MODE_POS
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


def test_refresh_without_an_acquire_is_the_flush_alone():
    """The reference calls refresh_force_sensor_tensor every step with no sensor: it flushes the pending
    simulate calls as every refresh does, and makes neither a Dynamics nor a ForceSensors."""
    gym, sim = _facade_sim(2, sensors=False)
    before = host(sim.engine.dof_state)
    gym.simulate(sim)
    assert sim.pending_substeps == 1
    assert gym.refresh_force_sensor_tensor(sim) is True
    assert sim.pending_substeps == 0 and sim.dynamics is None and sim.force_sensors is None
    assert not np.array_equal(host(sim.engine.dof_state), before)  # the step ran
    with pytest.raises(ValueError, match="create_asset_force_sensor"):
        gym.acquire_force_sensor_tensor(sim)
    assert sim.dynamics is None


def test_readings_match_the_reference_on_the_engines_buffers(he_model):
    from humanoid_amd.isaacgym import gymtorch
    gym, sim = _facade_sim(N)
    eng = sim.engine
    # sensors created but not acquired: still nothing but the flush
    gym.simulate(sim)
    gym.refresh_force_sensor_tensor(sim)
    assert sim.force_sensors is None and sim.dynamics is None
    t = gymtorch.wrap_tensor(gym.acquire_force_sensor_tensor(sim))
    assert tuple(t.shape) == (N * 3, 6) and t.dtype == torch.float32
    assert gymtorch.wrap_tensor(gym.acquire_force_sensor_tensor(sim)).data_ptr() == t.data_ptr()  # one tensor
    gym.refresh_force_sensor_tensor(sim)
    assert not host(t).any()  # before the first launch after the acquire: zero
    for _ in range(3):
        gym.simulate(sim)
        gym.simulate(sim)
        gym.fetch_results(sim, True)
    # the test's own copy of the generalised velocity before the last launch
    qd_before = np.concatenate([host(eng.root_states)[:, 7:13], host(eng.dof_state).reshape(N, ND, 2)[:, :, 1]], axis=1)
    gym.simulate(sim)
    gym.simulate(sim)
    assert sim.pending_substeps == 2
    gym.refresh_force_sensor_tensor(sim)
    assert sim.pending_substeps == 0
    got = host(t).reshape(N, 3, 6)
    dt_step = 2 * float(eng.params.dt)
    root, dof = host(eng.root_states), host(eng.dof_state).reshape(N, ND, 2)
    cf, df = host(eng.contact_forces).reshape(N, NB, 3), host(eng.dof_force).reshape(N, ND)
    g = tuple(eng.params.gravity)
    args = (he_model, root, dof, qd_before, dt_step, cf, df, BODIES, POSES, WORLD, g)
    x64, x32 = RR.sensor_reading(*args, dtype=np.float64), RR.sensor_reading(*args, dtype=np.float32)
    fig, floor = RR.error(got, x64).max(), RR.error(x32, x64).max()
    print(f"sensor readings: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    # a figure, not a check (settling is the solver's): the ankles carry the weight above them
    w = RR.sensor_reading(he_model, root, dof, qd_before, dt_step, cf, df, BODIES[:2], POSES[:2], [True, True], g)
    Mo = DR.Model(he_model, np.float64)
    above = (Mo.mass.sum() - Mo.sub[L_ANKLE] @ Mo.mass - Mo.sub[R_ANKLE] @ Mo.mass) * abs(g[2])
    print(f"summed vertical ankle force per env {w[:, :, 2].sum(axis=1)} N; the weight above the ankles {above:.1f} N; "
          f"contact force on the feet {cf[:, :, 2].sum(axis=1)} N")
    assert np.isfinite(fig) and fig <= MARGIN * floor, (fig, MARGIN * floor)
    assert np.abs(x64[:, :2, :3]).max() > 50.0  # the ankles are loaded: the check is not of zeros
    # a second refresh with nothing pending reports the same launch: the same reading
    gym.refresh_force_sensor_tensor(sim)
    assert np.array_equal(host(t).reshape(N, 3, 6), got)


def test_force_sensors_on_an_engine_directly(model, he_model):
    """ForceSensors without the facade: before_step / read around Engine.simulate, and its refusals."""
    from humanoid_amd.engine import Engine
    from humanoid_amd.sensors import ForceSensors
    eng = Engine(model, N, device=0)
    with pytest.raises(ValueError, match="body 0"):
        ForceSensors(eng, [0], [POSES[0]])
    with pytest.raises(ValueError, match="no sensor"):
        ForceSensors(eng, [], [])
    fs = ForceSensors(eng, BODIES, POSES, WORLD)
    out = torch.full((N * 3, 6), 7.0, device=eng.device)
    fs.read(1.0, out)
    assert not host(out).any()
    eng.simulate(2)
    qd_before = np.concatenate([host(eng.root_states)[:, 7:13], host(eng.dof_state).reshape(N, ND, 2)[:, :, 1]], axis=1)
    fs.before_step()
    eng.simulate(1)
    dt_step = float(eng.params.dt)
    got = host(fs.read(dt_step, out)).reshape(N, 3, 6)
    args = (he_model, host(eng.root_states), host(eng.dof_state).reshape(N, ND, 2), qd_before, dt_step,
            host(eng.contact_forces).reshape(N, NB, 3), host(eng.dof_force).reshape(N, ND), BODIES, POSES, WORLD,
            tuple(eng.params.gravity))
    x64, x32 = RR.sensor_reading(*args, dtype=np.float64), RR.sensor_reading(*args, dtype=np.float32)
    fig, floor = RR.error(got, x64).max(), RR.error(x32, x64).max()
    print(f"direct: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    assert np.isfinite(fig) and fig <= MARGIN * floor
    with pytest.raises(ValueError, match="out of shape"):
        fs.read(dt_step, torch.zeros(N, 6, device=eng.device))
