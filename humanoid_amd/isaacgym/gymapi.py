"""``isaacgym.gymapi`` facade over the HIP engine: the subset of the Isaac Gym Python
API that puffer-phc calls (``envs/isaacgym_env.py:6-99``, ``envs/humanoid_phc.py:74, 127-134,
185-383, 497-554, 747-789``), with the same names, argument meaning and tensor semantics, so that
the env changes only its imports::

    from humanoid_amd.isaacgym import gymapi, gymtorch

Semantics kept: one sim per process, envs created one by one with one actor each, dof/shape
properties set per actor, ``prepare_sim`` before tensors are acquired, engine-owned state
tensors aliased by torch views (``gymtorch.wrap_tensor``), indexed writes by int32 actor ids,
``simulate`` advancing one substep, ``fetch_results`` completing them.

Engine-specific behaviour (documented, not silent):
* consecutive ``simulate`` calls are fused into one kernel launch of N substeps, issued at the
  next ``fetch_results`` / tensor write / refresh -- the results are identical to N launches;
* all envs share one articulation, PD gains and filter table (what puffer-phc does): a
  ``set_actor_dof_properties`` / ``set_actor_rigid_shape_properties`` that differs between envs
  raises ``NotImplementedError``;
* torque control: ``set_actor_dof_properties`` takes ``DOF_MODE_POS``, ``DOF_MODE_EFFORT`` and
  ``DOF_MODE_NONE`` per dof (the same for every env; ``DOF_MODE_VEL`` raises: there is no velocity
  target tensor). A dof that is not POS has no PD drive; ``set_dof_actuation_force_tensor`` /
  ``..._indexed`` put joint torques on the EFFORT dofs, clamped to the dofs' effort limits (the
  engine's choice, as for the PD drive). The torques are in the coordinates of the dynamics tensors
  below (``M qdd + c = (0_6, tau)``), and they stay set until the next write: callers that write them
  before every ``simulate`` see Isaac Gym's behaviour whichever rule its binary follows;
* no viewer (headless only: ``create_viewer`` raises), CPU pipeline refused (the engine is GPU-only);
* camera SENSORS exist (``render_env.py:151-171, 218-227, 398-411``): ``create_camera_sensor``,
  ``set_camera_location`` / ``set_camera_transform`` / ``attach_camera_to_body``,
  ``render_all_camera_sensors``, ``get_camera_image`` (colour, depth, segmentation) and its GPU-tensor
  form, ``set_rigid_body_color`` / ``set_rigid_body_segmentation_id``. They are drawn by the HIP ray
  caster (``include/humanoid_render.h`` defines the image); all cameras of a sim share one size, a
  camera sees its own env only, optical flow is refused, and a camera transform keeps the view
  direction but not a roll about it (the image's up is the world's);
* the dynamics-query tensors exist: ``acquire_jacobian_tensor`` [N,24,6,75] and
  ``acquire_mass_matrix_tensor`` [N,75,75] with ``refresh_jacobian_tensors`` /
  ``refresh_mass_matrix_tensors``, formed by one HIP kernel from the root and dof state
  (``include/humanoid_dynamics.h`` has the definitions). Columns are Isaac Gym's floating-base order
  (root linear 3, root angular 3, the 69 dofs); the dof columns refer to the engine's child-frame
  relative rates of the exp-map ball joints, and the mass matrix carries the dof armature, as the
  engine's own solve does. ENGINE EXTENSION (not in Isaac Gym): ``acquire_bias_force_tensor`` [N,75]
  / ``refresh_bias_force_tensors``, the gravity + Coriolis force c of ``M qdd + c = tau``;
* ENGINE EXTENSION: the solves with that ``M``, each one HIP launch from the current state with ``M``
  kept in registers (``include/humanoid_solve.h``): ``solve_forward_dynamics`` (``qdd = M^-1 (f - c)``),
  ``solve_computed_torque`` (joint torques and base acceleration for desired joint accelerations) and
  ``solve_mass_matrix`` (``M^-1`` on up to 32 rows per env, e.g. a Jacobian block);
* ENGINE EXTENSION: the derivatives of those dynamics (``include/humanoid_derivatives.h``):
  ``solve_dynamics_derivatives`` gives d tau / d q and d tau / d qd of ``tau = M a + c`` in one launch, exact,
  and ``solve_forward_dynamics_derivatives`` the forward dynamics with d qdd / d q, d qdd / d qd and ``M^-1``;
* ENGINE EXTENSION: task-space control in one launch (``include/humanoid_task.h``): ``set_task_rows``
  names up to 32 task rows (velocity components of points on bodies, the same for every env), and
  ``solve_task_space`` gives the generalised force (``mode="force"``: ``J^T F``) or the joint torques
  (``mode="joint"``, for ``set_dof_actuation_force_tensor``) that give those rows a desired acceleration;
* ENGINE EXTENSION: the balance quantities in one launch (``include/humanoid_centroidal.h``):
  ``acquire_centroidal_tensor(sim, actor, which)`` for the centre of mass, its velocity, the momentum
  about the centre of mass, the centroidal momentum matrix [N,6,75], its rate term and the energies, and
  ``refresh_centroidal_tensors``, which refreshes every acquired one;
* ENGINE EXTENSION: inverse kinematics in one launch (``include/humanoid_ik.h``): ``set_ik_rows`` names up
  to 32 rows (position components of points on bodies, orientation components of bodies), and
  ``solve_inverse_kinematics`` gives the root and dof state, velocities zero, that puts them at their
  targets, in the shapes the indexed state writes take. The sim's state is not touched.
"""
from __future__ import annotations

import copy
import os
from typing import List

import numpy as np

from .. import _abi
from ..model import DEFAULT_MODEL_JSON, HumanoidModel, parse_mjcf

# ----------------------------------------------------------------------------------- constants
SIM_PHYSX = 1
SIM_FLEX = 2
UP_AXIS_Y = 0
UP_AXIS_Z = 1
DOF_MODE_NONE = 0
DOF_MODE_POS = 1
DOF_MODE_VEL = 2
DOF_MODE_EFFORT = 3
STATE_NONE, STATE_POS, STATE_VEL, STATE_ALL = 0, 1, 2, 3
# gymapi.CoordinateSpace (apply_rigid_body_force_tensors, render_env.py:105-126): the envs share one
# world frame here, so ENV_SPACE and GLOBAL_SPACE are the same frame
ENV_SPACE, LOCAL_SPACE, GLOBAL_SPACE = _abi.SPACE_ENV, _abi.SPACE_LOCAL, _abi.SPACE_GLOBAL

# camera sensors (render_env.py:151-171): image types, mesh kinds, camera follow modes
IMAGE_COLOR, IMAGE_DEPTH, IMAGE_SEGMENTATION, IMAGE_OPTICAL_FLOW = 0, 1, 2, 3
MESH_NONE, MESH_COLLISION, MESH_VISUAL, MESH_VISUAL_AND_COLLISION = 0, 1, 2, 3
FOLLOW_POSITION, FOLLOW_TRANSFORM = 0, 1  # include/humanoid_render.h HR_FOLLOW_*

DofPropertiesDtype = np.dtype([("hasLimits", "?"), ("lower", "<f4"), ("upper", "<f4"), ("driveMode", "<i4"),
                               ("velocity", "<f4"), ("effort", "<f4"), ("stiffness", "<f4"), ("damping", "<f4"),
                               ("friction", "<f4"), ("armature", "<f4")])


# ----------------------------------------------------------------------------------- value types
class Vec3:
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)

    def __iter__(self):
        return iter((self.x, self.y, self.z))


class Quat:
    def __init__(self, x=0.0, y=0.0, z=0.0, w=1.0):
        self.x, self.y, self.z, self.w = float(x), float(y), float(z), float(w)


class Transform:
    def __init__(self, p=None, r=None):
        self.p = p if p is not None else Vec3()
        self.r = r if r is not None else Quat()


class PhysXParams:
    def __init__(self):
        self.num_threads = 4
        self.solver_type = 1
        self.num_position_iterations = 4
        self.num_velocity_iterations = 0
        self.contact_offset = 0.02
        self.rest_offset = 0.0
        self.bounce_threshold_velocity = 0.2
        self.max_depenetration_velocity = 10.0
        self.default_buffer_size_multiplier = 10.0
        self.use_gpu = True
        self.max_gpu_contact_pairs = 8 * 1024 * 1024
        self.num_subscenes = 0


class SimParams:
    def __init__(self):
        self.dt = 1.0 / 60.0
        self.substeps = 2  # Isaac Gym's default; the reference leaves it (isaacgym_env.py:6-35)
        self.up_axis = UP_AXIS_Z
        self.gravity = Vec3(0.0, 0.0, -9.81)
        self.use_gpu_pipeline = True
        self.num_client_threads = 0
        self.physx = PhysXParams()


class AssetOptions:
    def __init__(self):
        self.angular_damping = 0.0
        self.linear_damping = 0.0
        self.max_angular_velocity = 64.0
        self.default_dof_drive_mode = DOF_MODE_NONE
        self.fix_base_link = False


class PlaneParams:
    def __init__(self):
        self.normal = Vec3(0.0, 0.0, 1.0)
        self.distance = 0.0
        self.static_friction = 1.0
        self.dynamic_friction = 1.0
        self.restitution = 0.0


class CameraProperties:
    def __init__(self):
        self.width = 1600
        self.height = 900
        self.horizontal_fov = 90.0
        self.near_plane = 0.001
        self.far_plane = 2.0e6
        self.enable_tensors = False


class _Camera:
    """One camera sensor of a sim: what hr_camera holds, filled by set_camera_location /
    set_camera_transform / attach_camera_to_body."""

    def __init__(self, env_index, props: CameraProperties):
        self.env = env_index
        self.props = copy.copy(props)
        self.pos = (0.0, -4.0, 2.0)
        self.target = (0.0, 0.0, 1.0)
        self.follow_body = -1
        self.follow_mode = FOLLOW_POSITION


class ForceSensorProperties:
    def __init__(self):
        self.enable_forward_dynamics_forces = True
        self.enable_constraint_solver_forces = True
        self.use_world_frame = False


class RigidBodyProperties:
    def __init__(self, mass, com, inertia):
        self.mass = float(mass)
        self.com = Vec3(*com)
        self.inertia = inertia


class RigidShapeProperties:
    def __init__(self, filter_=0, friction=1.0):
        self.filter = int(filter_)
        self.friction = float(friction)
        self.restitution = 0.0
        self.contact_offset = 0.02
        self.rest_offset = 0.0


class GymTensor:
    """Handle returned by ``acquire_*_tensor`` and ``gymtorch.unwrap_tensor``: a device pointer
    with shape/dtype (``GymTensor.h:20-28``: dtype 1 = f32, 2 = int32, ...)."""

    def __init__(self, data_ptr, shape, dtype, device, owner=None):
        self.data_ptr = int(data_ptr)
        self.shape = tuple(shape)
        self.dtype = dtype
        self.device = int(device)
        self.own_data = False
        self._owner = owner


# ----------------------------------------------------------------------------------- handles
class Asset:
    def __init__(self, model: HumanoidModel, options: AssetOptions):
        self.model = model
        self.options = options
        self.force_sensors = []


class _Env:
    def __init__(self, index):
        self.index = index
        self.actor = None
        self.cameras = []     # indices into sim.cameras; a camera handle is its position in this list
        self.body_rgb = None  # [24,3] once set_rigid_body_color has touched the env
        self.body_seg = None  # [24] from create_actor's segmentation_id / set_rigid_body_segmentation_id


class Sim:
    def __init__(self, device, params: SimParams):
        self.device = device
        self.params = params
        self.envs: List[_Env] = []
        self.asset: Asset | None = None
        self.plane: PlaneParams | None = None
        self.dof_props = None
        self.dof_modes = None  # [69] gymapi.DOF_MODE_* once set_actor_dof_properties has been called
        self.shape_filters = None
        self.self_collision = None
        self.start_poses = []
        self.engine = None
        self.pending_substeps = 0
        self.cameras: List[_Camera] = []
        self.renderer = None
        self.cameras_dirty = True
        self.appearance_dirty = True
        self.appearance = (None, None)  # the device tensors the renderer reads
        self.rendered = False
        self.dynamics = None          # humanoid_amd.dynamics.Dynamics, created by the first acquire
        self.dynamics_acquired = set()  # of "jacobian", "mass_matrix", "bias"
        self.task_stage = None        # [N,75] the (0_6; tau) solve_task_space's joint mode writes
        self.centroidal_acquired = set()  # of humanoid_amd.centroidal.OUTPUTS
        self.force_sensors = None     # humanoid_amd.sensors.ForceSensors, created by acquire_force_sensor_tensor
        self.force_sensor_tensor = None  # [N*S,6]
        self.force_sensor_dt = 0.0    # the simulated time of the last launch since the acquire


# ----------------------------------------------------------------------------------- the Gym object
class Gym:
    # -- sim ----------------------------------------------------------------------------------
    def create_sim(self, compute_device, graphics_device, physics_engine, params: SimParams):
        if compute_device < 0 or not params.use_gpu_pipeline:
            raise NotImplementedError("the HIP engine has no CPU pipeline (use device_type='cuda')")
        if physics_engine != SIM_PHYSX:
            raise NotImplementedError("only the rigid-body (SIM_PHYSX-equivalent) pipeline exists")
        if graphics_device >= 0:
            raise NotImplementedError("headless only: the engine has no viewer")
        return Sim(int(compute_device), copy.deepcopy(params))

    def destroy_sim(self, sim: Sim):
        sim.engine = None

    def add_ground(self, sim: Sim, plane: PlaneParams):
        sim.plane = copy.deepcopy(plane)

    # -- assets ---------------------------------------------------------------------------------
    def load_asset(self, sim: Sim, root: str, filename: str, options: AssetOptions = None) -> Asset:
        path = filename if os.path.isabs(filename) else os.path.join(root, filename)
        if path.endswith(".json"):
            with open(path) as f:
                model = HumanoidModel.from_json(f.read())
        elif os.path.basename(path) == "smpl_humanoid.xml" and not os.path.exists(path):
            raise FileNotFoundError(f"{path} (the baked model is at {DEFAULT_MODEL_JSON})")
        else:
            model = parse_mjcf(path)
        a = Asset(model, copy.deepcopy(options) if options is not None else AssetOptions())
        sim.asset = a
        return a

    def get_asset_rigid_body_count(self, asset: Asset) -> int:
        return asset.model.num_bodies

    def get_asset_dof_count(self, asset: Asset) -> int:
        return 3 * (asset.model.num_bodies - 1)  # one 3-dof ball joint per non-root body

    def find_asset_rigid_body_index(self, asset: Asset, name: str) -> int:
        try:
            return asset.model.body_names.index(name)
        except ValueError:
            return -1

    def create_asset_force_sensor(self, asset: Asset, body_idx: int, pose: Transform, props=None):
        """A force sensor on body ``body_idx`` of every actor made from the asset, at ``pose`` in the body's
        frame: it reads the wrench the body's parent joint transmits (``humanoid_amd/sensors.py`` defines the
        reading). ``props``: a :class:`ForceSensorProperties`; both of its force switches must be on."""
        props = ForceSensorProperties() if props is None else props
        if not (props.enable_forward_dynamics_forces and props.enable_constraint_solver_forces):
            raise NotImplementedError("force sensor: enable_forward_dynamics_forces and enable_constraint_solver_forces "
                                      "must both be True (the reading is the whole joint wrench)")
        body_idx = int(body_idx)
        if body_idx == 0:
            raise ValueError("force sensor on body 0: a sensor measures the body's parent joint, and the root has none")
        if not 0 < body_idx < asset.model.num_bodies:
            raise ValueError(f"force sensor: body {body_idx} outside 1..{asset.model.num_bodies - 1}")
        asset.force_sensors.append((body_idx, copy.deepcopy(pose), bool(props.use_world_frame)))
        return len(asset.force_sensors) - 1

    def get_asset_dof_properties(self, asset: Asset):
        m = asset.model
        p = np.zeros(3 * (m.num_bodies - 1), DofPropertiesDtype)
        p["hasLimits"] = True
        p["lower"], p["upper"] = m.dof_lower, m.dof_upper
        p["driveMode"] = asset.options.default_dof_drive_mode
        p["velocity"] = asset.options.max_angular_velocity
        p["effort"], p["stiffness"], p["damping"], p["armature"] = m.effort, m.stiffness, m.damping, m.armature
        return p

    # -- envs / actors ----------------------------------------------------------------------------
    def create_env(self, sim: Sim, lower: Vec3, upper: Vec3, num_per_row: int):
        e = _Env(len(sim.envs))
        e.sim = sim
        sim.envs.append(e)
        return e

    def begin_aggregate(self, env, max_bodies, max_shapes, self_collisions):
        return True

    def end_aggregate(self, env):
        return True

    def create_actor(self, env: _Env, asset: Asset, pose: Transform, name: str, group: int, filter_: int,
                     segmentation_id: int = 0):
        if env.actor is not None:
            raise NotImplementedError("one actor per env (the humanoid)")
        sim = env.sim
        if group != env.index:
            raise NotImplementedError("envs are independent collision groups (col_group = env_id)")
        sc = 0 if filter_ else 1  # filter 1 = self-collision off (humanoid_phc.py:337)
        if sim.self_collision is None:
            sim.self_collision = sc
        elif sim.self_collision != sc:
            raise NotImplementedError("self-collision must be the same for every env")
        env.actor = name
        env.body_seg = np.full(_abi.NB, int(segmentation_id), np.int32)  # the actor's default id
        sim.start_poses.append(((pose.p.x, pose.p.y, pose.p.z), (pose.r.x, pose.r.y, pose.r.z, pose.r.w)))
        return 0

    def enable_actor_dof_force_sensors(self, env, actor):
        return True  # dof forces are always produced

    def get_actor_rigid_body_properties(self, env: _Env, actor):
        m = env.sim.asset.model
        return [RigidBodyProperties(m.mass[b], m.com[b], m.inertia[b]) for b in range(m.num_bodies)]

    def set_actor_dof_properties(self, env: _Env, actor, props):
        sim = env.sim
        modes = np.asarray(props["driveMode"], np.int32)
        if np.any(modes == DOF_MODE_VEL):
            raise NotImplementedError("DOF_MODE_VEL: the engine has no velocity target tensor "
                                      "(DOF_MODE_POS, DOF_MODE_EFFORT and DOF_MODE_NONE exist)")
        if not np.all(np.isin(modes, (DOF_MODE_NONE, DOF_MODE_POS, DOF_MODE_EFFORT))):
            raise ValueError(f"driveMode outside gymapi.DOF_MODE_*: {sorted(set(modes.tolist()))}")
        if sim.dof_props is not None:
            if not all(np.array_equal(sim.dof_props[k], props[k]) for k in ("stiffness", "damping", "effort", "armature")):
                raise NotImplementedError("per-env PD gains differ: the engine shares one articulation")
            if not np.array_equal(sim.dof_modes, modes):
                raise NotImplementedError("per-env drive modes differ: the engine shares one articulation")
        else:
            sim.dof_props = np.array(props, copy=True)
            sim.dof_modes = modes.copy()
        return True

    def get_actor_rigid_shape_properties(self, env: _Env, actor):
        m = env.sim.asset.model
        fr = env.sim.plane.static_friction if env.sim.plane else 1.0
        return [RigidShapeProperties(int(m.filter_ints[b]), fr) for b in range(m.num_bodies)]

    def set_actor_rigid_shape_properties(self, env: _Env, actor, props):
        sim = env.sim
        f = np.array([p.filter for p in props], np.int32)
        if sim.shape_filters is None:
            sim.shape_filters = f
        elif not np.array_equal(sim.shape_filters, f):
            raise NotImplementedError("per-env filter tables differ")
        return True

    # -- prepare: build the engine ------------------------------------------------------------------
    def prepare_sim(self, sim: Sim):
        from ..engine import Engine
        if sim.asset is None or not sim.envs:
            raise RuntimeError("prepare_sim before load_asset/create_actor")
        m = copy.deepcopy(sim.asset.model)
        if sim.dof_props is not None:
            m.stiffness = np.asarray(sim.dof_props["stiffness"], np.float64)
            m.damping = np.asarray(sim.dof_props["damping"], np.float64)
            m.armature = np.asarray(sim.dof_props["armature"], np.float64)
            m.effort = np.asarray(sim.dof_props["effort"], np.float64)
        if sim.shape_filters is not None:
            m.filter_ints = sim.shape_filters
        sp, px, o = sim.params, sim.params.physx, sim.asset.options
        plane = sim.plane or PlaneParams()
        # physx.solver_type 1 (TGS, isaacgym_env.py:16) with num_position_iterations per physics step;
        # solver_type 0 maps onto the engine's velocity-level PGS step, num_position_iterations sweeps
        # (8 is the engine's tested count)
        if px.solver_type not in (0, 1):
            raise NotImplementedError(f"physx.solver_type {px.solver_type}: 0 (PGS) or 1 (TGS)")
        if px.solver_type == 1 and px.num_velocity_iterations != 0:
            raise NotImplementedError("TGS velocity iterations: the reference runs 0 (isaacgym_env.py:18)")
        if not 1 <= px.num_position_iterations <= 16:
            raise NotImplementedError("num_position_iterations must be in [1, 16]")
        solver = dict(solver_type=int(px.solver_type), solver_iterations=int(px.num_position_iterations))
        params = _abi.default_sim_params(
            dt=sp.dt, contact_offset=px.contact_offset, max_depenetration_velocity=px.max_depenetration_velocity,
            angular_damping=o.angular_damping, max_angular_velocity=o.max_angular_velocity,
            friction=plane.static_friction, self_collision=int(bool(sim.self_collision)), substeps=int(sp.substeps),
            **solver)
        params.gravity[:] = (sp.gravity.x, sp.gravity.y, sp.gravity.z)
        n = len(sim.envs)
        xy = np.array([p[0][:2] for p in sim.start_poses], np.float32)
        sim.engine = Engine(m, n, device=sim.device, sim_params=params, start_xy=xy)
        self._model = m
        if sim.dof_modes is not None and np.any(sim.dof_modes != DOF_MODE_POS):
            sim.engine.set_dof_drive_modes(sim.dof_modes)
        poses = np.array([list(p[0]) + list(p[1]) for p in sim.start_poses], np.float32)
        if not (np.allclose(poses[:, 2], 0.89) and np.allclose(poses[:, 3:7], [0, 0, 0, 1])):
            import torch
            rs = torch.zeros(n, 13, device=sim.engine.device)
            rs[:, :7] = torch.from_numpy(poses).to(rs.device)
            sim.engine.set_root_state_indexed(rs, torch.arange(n, dtype=torch.int32, device=rs.device))
            # _initial_humanoid_root_states (humanoid_phc.py:522-523) is the root state tensor read
            # right after prepare_sim with the velocities zeroed: the creation poses, which the
            # Default / Hybrid state init resets to (he_create_envs set it for the z=0.89 pose only)
            sim.engine.initial_root_states.copy_(rs)
        return True

    # -- tensors ----------------------------------------------------------------------------------
    def _acquire(self, sim: Sim, kind: int):
        if sim.engine is None:
            raise RuntimeError("acquire_*_tensor before prepare_sim")
        t = sim.engine.buffer(kind)
        return GymTensor(t.data_ptr(), t.shape, 1, sim.device, owner=t)

    def acquire_actor_root_state_tensor(self, sim):
        return self._acquire(sim, _abi.BUF_ROOT_STATE)

    def acquire_dof_state_tensor(self, sim):
        return self._acquire(sim, _abi.BUF_DOF_STATE)

    def acquire_rigid_body_state_tensor(self, sim):
        return self._acquire(sim, _abi.BUF_RB_STATE)

    def acquire_net_contact_force_tensor(self, sim):
        return self._acquire(sim, _abi.BUF_CONTACT_FORCE)

    def acquire_dof_force_tensor(self, sim):
        return self._acquire(sim, _abi.BUF_DOF_FORCE)

    def acquire_force_sensor_tensor(self, sim):
        """[N*S,6]: per env the S sensors of the asset in their creation order, force 3 then torque 3, on
        the body by its parent, in the sensor's frame (``use_world_frame``: world axes). Filled by
        ``refresh_force_sensor_tensor`` for the step the last launch ran; zero before any."""
        import torch
        if sim.engine is None:
            raise RuntimeError("acquire_force_sensor_tensor before prepare_sim")
        if not sim.asset.force_sensors:
            raise ValueError("acquire_force_sensor_tensor: the asset has no force sensor (create_asset_force_sensor)")
        if sim.force_sensors is None:
            from ..sensors import ForceSensors
            if sim.dynamics is None:
                from ..dynamics import Dynamics
                sim.dynamics = Dynamics(sim.engine)
            fs = sim.asset.force_sensors
            poses = [[p.p.x, p.p.y, p.p.z, p.r.x, p.r.y, p.r.z, p.r.w] for _, p, _ in fs]
            sim.force_sensors = ForceSensors(sim.engine, [b for b, _, _ in fs], poses, [w for _, _, w in fs],
                                             reaction=sim.dynamics.reaction)
            sim.force_sensor_tensor = torch.zeros(sim.engine.num_envs * len(fs), 6, dtype=torch.float32,
                                                  device=sim.engine.device)
        t = sim.force_sensor_tensor
        return GymTensor(t.data_ptr(), t.shape, 1, sim.device, owner=t)

    # -- dynamics-query tensors -------------------------------------------------------------------
    def _acquire_dynamics(self, sim: Sim, actor_name: str, which: str):
        if sim.engine is None:
            raise RuntimeError(f"acquire_{which}_tensor before prepare_sim")
        if not any(env.actor == actor_name for env in sim.envs):
            raise ValueError(f"no env has an actor named {actor_name!r}")
        if sim.dynamics is None:
            from ..dynamics import Dynamics
            sim.dynamics = Dynamics(sim.engine)
        sim.dynamics_acquired.add(which)
        t = getattr(sim.dynamics, which)
        return GymTensor(t.data_ptr(), t.shape, 1, sim.device, owner=t)

    def acquire_jacobian_tensor(self, sim: Sim, actor_name: str):
        """[N,24,6,75]: per body the rows (origin linear velocity 3, world angular velocity 3) over the
        columns (root linear 3, root angular 3, 69 dof rates). Filled by ``refresh_jacobian_tensors``."""
        return self._acquire_dynamics(sim, actor_name, "jacobian")

    def acquire_mass_matrix_tensor(self, sim: Sim, actor_name: str):
        """[N,75,75], the joint-space inertia with the dof armature. Filled by
        ``refresh_mass_matrix_tensors``."""
        return self._acquire_dynamics(sim, actor_name, "mass_matrix")

    def acquire_bias_force_tensor(self, sim: Sim, actor_name: str):
        """Engine extension: [N,75], the gravity + Coriolis force. Filled by ``refresh_bias_force_tensors``."""
        return self._acquire_dynamics(sim, actor_name, "bias")

    def _refresh_dynamics(self, sim: Sim, which: str):
        if which in sim.dynamics_acquired:  # before its acquire: a no-op, as in Isaac Gym
            self._flush(sim)
            sim.dynamics.refresh(jacobian=which == "jacobian", mass_matrix=which == "mass_matrix", bias=which == "bias")
        return True

    def refresh_jacobian_tensors(self, sim: Sim):
        return self._refresh_dynamics(sim, "jacobian")

    def refresh_mass_matrix_tensors(self, sim: Sim):
        return self._refresh_dynamics(sim, "mass_matrix")

    def refresh_bias_force_tensors(self, sim: Sim):
        return self._refresh_dynamics(sim, "bias")

    # -- the solves with M (engine extensions) ------------------------------------------------------
    def _solve_dynamics(self, sim: Sim, what: str):
        if sim.engine is None:
            raise RuntimeError(f"{what} before prepare_sim")
        self._flush(sim)  # the solve sees the state after every simulate call so far
        if sim.dynamics is None:
            from ..dynamics import Dynamics
            sim.dynamics = Dynamics(sim.engine)
        return sim.dynamics

    def solve_forward_dynamics(self, sim: Sim, gen_force_desc, out_desc):
        """Engine extension: out [N,75] = M^-1 (gen_force - c) at the current state; ``gen_force_desc``
        [N,75] or None for zero."""
        dyn = self._solve_dynamics(sim, "solve_forward_dynamics")
        dyn.forward_dynamics(None if gen_force_desc is None else self._tensor(gen_force_desc), self._tensor(out_desc))
        return True

    def solve_computed_torque(self, sim: Sim, qdd_des_desc, tau_out_desc, base_acc_desc=None):
        """Engine extension: tau [N,69] (and the base acceleration [N,6] when asked) for the desired joint
        accelerations qdd_des [N,69]: M (a_b; qdd_des) + c = (0_6; tau). The torques are not clamped;
        ``set_dof_actuation_force_tensor`` clamps to the effort limits when they are applied."""
        dyn = self._solve_dynamics(sim, "solve_computed_torque")
        dyn.solver.computed_torque(self._tensor(qdd_des_desc), None, self._tensor(tau_out_desc),
                                   None if base_acc_desc is None else self._tensor(base_acc_desc),
                                   want_base_acc=base_acc_desc is not None)
        return True

    def solve_reaction_wrenches(self, sim: Sim, qdd_desc, wrench_out_desc, base_acc_desc=None, force_desc=None,
                                torque_desc=None, frame="world"):
        """Engine extension: wrench_out [N,24,6], the wrench every joint transmits (force 3, torque 3 about
        the joint's own origin, on the body by its parent; row 0: what something outside must exert on the
        root) for the joint accelerations qdd [N,69] (None: zero) at the current state
        (``include/humanoid_wrench.h``). ``base_acc_desc`` [N,6] prescribes the base acceleration, None
        leaves the base free; ``force_desc`` / ``torque_desc`` [N*24,3] are external forces at the bodies'
        centres of mass and torques in world axes; ``frame`` "world" or "body"."""
        dyn = self._solve_dynamics(sim, "solve_reaction_wrenches")

        def opt(desc):
            return None if desc is None else self._tensor(desc)

        dyn.reaction.compute(opt(qdd_desc), opt(base_acc_desc), opt(force_desc), opt(torque_desc), frame, wrench=False,
                             out={"wrench": self._tensor(wrench_out_desc)})
        return True

    def solve_mass_matrix(self, sim: Sim, rhs_desc, out_desc):
        """Engine extension: out [N,k,75] = M^-1 on each of the k <= 32 rows of rhs [N,k,75]."""
        dyn = self._solve_dynamics(sim, "solve_mass_matrix")
        dyn.solve(self._tensor(rhs_desc), self._tensor(out_desc))
        return True

    def solve_dynamics_derivatives(self, sim: Sim, acc_desc, dtau_dq_out_desc=None, dtau_dv_out_desc=None,
                                   tau_out_desc=None, by_direction=False):
        """Engine extension: the derivatives of the inverse dynamics tau = M a + c at the current state and
        the generalised acceleration acc [N,75] (None: zero), in one launch
        (``include/humanoid_derivatives.h``): dtau_dq [N,75,75] along the pose directions, dtau_dv [N,75,75]
        with respect to the generalised velocity, both indexed [i, j] (``by_direction``: [j, i]), and tau
        [N,75] itself. An output whose descriptor is None is not computed; at least one must be given."""
        dyn = self._solve_dynamics(sim, "solve_dynamics_derivatives")
        out = {name: self._tensor(d) for name, d in (("dtau_dq", dtau_dq_out_desc), ("dtau_dv", dtau_dv_out_desc),
                                                     ("tau", tau_out_desc)) if d is not None}
        dyn.derivatives.inverse_dynamics(None if acc_desc is None else self._tensor(acc_desc), dtau_dq=False,
                                         dtau_dv=False, by_direction=by_direction, out=out)
        return True

    def solve_forward_dynamics_derivatives(self, sim: Sim, gen_force_desc, qdd_out_desc, dqdd_dq_out_desc,
                                           dqdd_dv_out_desc, dqdd_dtau_out_desc=None):
        """Engine extension: the forward dynamics qdd [N,75] = M^-1 (gen_force - c) at the current state
        (``gen_force_desc`` [N,75] or None for zero) with its derivatives along the pose directions and with
        respect to the generalised velocity, [N,75,75] each indexed [i, j], and M^-1 [N,75,75] when
        ``dqdd_dtau_out_desc`` is given: what a linearisation x' = A x + B u of the continuous dynamics
        is assembled from."""
        dyn = self._solve_dynamics(sim, "solve_forward_dynamics_derivatives")
        r = dyn.derivatives.forward_dynamics(None if gen_force_desc is None else self._tensor(gen_force_desc),
                                             dqdd_dtau=dqdd_dtau_out_desc is not None)
        for name, d in (("qdd", qdd_out_desc), ("dqdd_dq", dqdd_dq_out_desc), ("dqdd_dv", dqdd_dv_out_desc),
                        ("dqdd_dtau", dqdd_dtau_out_desc)):
            if d is not None:
                self._tensor(d).copy_(r[name])
        return True

    # -- task-space control (engine extensions) -----------------------------------------------------
    def set_task_rows(self, sim: Sim, rows):
        """Engine extension: the task rows of ``solve_task_space``, ``(body index or name, axis, point=(0, 0,
        0))`` each: axis 0..2 is the world linear velocity component x / y / z of the point given in the body's
        frame, 3..5 the body's world angular velocity component. 1 to 32 rows, the same for every env; they
        replace the rows set before."""
        dyn = self._solve_dynamics(sim, "set_task_rows")
        dyn.task.set_rows(rows)
        return True

    def solve_task_space(self, sim: Sim, xdd_des_desc, tau_or_force_out_desc, mode="joint", damping=0.0,
                         gen_force_desc=None, qdd_out_desc=None):
        """Engine extension: what gives the task rows the accelerations xdd_des [N,k] at the current state.
        ``mode="joint"``: the joint torques tau [N,69] of minimum norm (base unactuated), as
        ``set_dof_actuation_force_tensor`` takes them; ``mode="force"``: the operational-space generalised
        force J^T F [N,75]. ``gen_force_desc`` [N,75] is a generalised force already acting (a posture
        torque there is projected into the task's null space); ``qdd_out_desc`` [N,75] takes the resulting
        acceleration. The torques are not clamped to the effort limits."""
        import torch
        from ..task import MODES, TaskError
        dyn = self._solve_dynamics(sim, "solve_task_space")
        if mode not in MODES:
            raise TaskError(f"solve_task_space: unknown mode {mode!r} (one of {sorted(MODES)})")
        out = self._tensor(tau_or_force_out_desc)
        joint = mode == "joint"
        n = sim.engine.num_envs
        if joint:  # the kernel writes (0_6; tau): through a [N,75] staging tensor into the caller's [N,69]
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, _abi.ND):
                raise TaskError(f"tau_out: expected a tensor of shape ({n}, {_abi.ND}) in joint mode")
            if sim.task_stage is None:
                sim.task_stage = torch.empty(n, _abi.NG, dtype=torch.float32, device=sim.engine.device)
        u, _, _ = dyn.task.control(self._tensor(xdd_des_desc),
                                   None if gen_force_desc is None else self._tensor(gen_force_desc), mode, damping,
                                   out=sim.task_stage if joint else out, want_task_force=False,
                                   qdd=None if qdd_out_desc is None else self._tensor(qdd_out_desc),
                                   want_qdd=qdd_out_desc is not None)
        if joint:
            out.copy_(u[:, 6:])
        return True

    # -- inverse kinematics (engine extensions) -----------------------------------------------------
    def set_ik_rows(self, sim: Sim, rows):
        """Engine extension: the rows of ``solve_inverse_kinematics``, ``(body index or name, axis, point=(0, 0,
        0))`` each: axis 0..2 is the world position component x / y / z of the point given in the body's frame,
        3..5 a component of the body's orientation error. 1 to 32 rows, the same for every env; they replace
        the rows set before (and are apart from ``set_task_rows``')."""
        dyn = self._solve_dynamics(sim, "set_ik_rows")
        dyn.ik.set_rows(rows)
        return True

    def solve_inverse_kinematics(self, sim: Sim, target_desc, root_out_desc, dof_out_desc, target_rot_desc=None,
                                 iterations=8, damping=1e-4, step_clip=0.1, residual_desc=None):
        """Engine extension: the pose that puts the ik rows at ``target`` [N,k] (and, for angular rows, the
        bodies at the orientations ``target_rot`` [N,24,4], xyzw), from the current state in ``iterations``
        steps of one launch (``include/humanoid_ik.h``). ``root_out`` [N,13] and ``dof_out`` [N*69,2] take the
        pose with every velocity zero, as ``set_actor_root_state_tensor_indexed`` and
        ``set_dof_state_tensor_indexed`` take them (the sim's own state tensors are refused: the state is
        not touched); ``residual_desc`` [N,k] the rows' remaining errors. The dof angles stay within the
        model's limits."""
        dyn = self._solve_dynamics(sim, "solve_inverse_kinematics")
        dyn.ik.solve(self._tensor(target_desc), None if target_rot_desc is None else self._tensor(target_rot_desc),
                     iterations, damping, step_clip, root_out=self._tensor(root_out_desc),
                     dof_out=self._tensor(dof_out_desc), want_residual=residual_desc is not None,
                     residual=None if residual_desc is None else self._tensor(residual_desc))
        return True

    # -- balance quantities (engine extensions) -----------------------------------------------------
    def acquire_centroidal_tensor(self, sim: Sim, actor_name: str, which: str):
        """Engine extension: one of the centroidal tensors (``include/humanoid_centroidal.h``), ``which`` in
        "com" [N,3], "com_vel" [N,3], "momentum" [N,6] (linear, angular about the centre of mass), "cmm"
        [N,6,75] (the centroidal momentum matrix), "cmm_bias" [N,6], "energy" [N,2] (kinetic, potential).
        Filled by ``refresh_centroidal_tensors``."""
        from ..centroidal import OUTPUTS
        if sim.engine is None:
            raise RuntimeError("acquire_centroidal_tensor before prepare_sim")
        if not any(env.actor == actor_name for env in sim.envs):
            raise ValueError(f"no env has an actor named {actor_name!r}")
        if which not in OUTPUTS:
            raise ValueError(f"acquire_centroidal_tensor: unknown tensor {which!r} (one of {OUTPUTS})")
        if sim.dynamics is None:
            from ..dynamics import Dynamics
            sim.dynamics = Dynamics(sim.engine)
        sim.centroidal_acquired.add(which)
        t = getattr(sim.dynamics.centroidal, which)
        return GymTensor(t.data_ptr(), t.shape, 1, sim.device, owner=t)

    def refresh_centroidal_tensors(self, sim: Sim):
        """Engine extension: every acquired centroidal tensor, in one launch, at the state after every
        ``simulate`` call so far. Before any acquire: a no-op that reports success."""
        if sim.centroidal_acquired:
            from ..centroidal import OUTPUTS
            self._flush(sim)
            sim.dynamics.centroidal.refresh(**{name: name in sim.centroidal_acquired for name in OUTPUTS})
        return True

    def _flush(self, sim: Sim):
        if sim.pending_substeps:
            k, sim.pending_substeps = sim.pending_substeps, 0
            if sim.force_sensors is not None:  # acquired force sensors read this launch's mean acceleration
                sim.force_sensors.before_step()
                sim.force_sensor_dt = k * float(sim.engine.params.dt)
            sim.engine.simulate(k)

    def refresh_dof_state_tensor(self, sim):
        self._flush(sim)

    def refresh_force_sensor_tensor(self, sim):
        """Flush, then fill the acquired force-sensor tensor for the launch that last ran. Before any
        acquire: the flush alone."""
        self._flush(sim)
        if sim.force_sensors is not None:
            sim.force_sensors.read(sim.force_sensor_dt, sim.force_sensor_tensor)
        return True

    refresh_actor_root_state_tensor = refresh_dof_state_tensor
    refresh_rigid_body_state_tensor = refresh_dof_state_tensor
    refresh_dof_force_tensor = refresh_dof_state_tensor
    refresh_net_contact_force_tensor = refresh_dof_state_tensor

    @staticmethod
    def _tensor(desc):
        from . import gymtorch
        return gymtorch.wrap_tensor(desc)

    def set_dof_position_target_tensor(self, sim: Sim, desc):
        self._flush(sim)
        sim.engine.set_dof_targets(self._tensor(desc))
        return True

    def set_actor_root_state_tensor_indexed(self, sim: Sim, desc, ids_desc, n: int):
        self._flush(sim)
        sim.engine.set_root_state_indexed(self._tensor(desc), self._tensor(ids_desc)[:n])
        return True

    def set_dof_state_tensor_indexed(self, sim: Sim, desc, ids_desc, n: int):
        self._flush(sim)
        sim.engine.set_dof_state_indexed(self._tensor(desc), self._tensor(ids_desc)[:n])
        return True

    def set_dof_position_target_tensor_indexed(self, sim: Sim, desc, ids_desc, n: int):
        self._flush(sim)
        sim.engine.set_dof_targets_indexed(self._tensor(desc), self._tensor(ids_desc)[:n])
        return True

    # -- torque control -------------------------------------------------------------------------------
    def set_dof_actuation_force_tensor(self, sim: Sim, desc):
        """Joint torques [N*69] (or [N,69]) on the DOF_MODE_EFFORT dofs, clamped to the dofs' effort
        limits. The engine keeps them until the next write (``include/humanoid_engine.h``); written
        before every ``simulate``, as every known caller does, that is Isaac Gym's behaviour."""
        self._flush(sim)
        sim.engine.set_dof_actuation_forces(self._tensor(desc))
        return True

    def set_dof_actuation_force_tensor_indexed(self, sim: Sim, desc, ids_desc, n: int):
        self._flush(sim)
        sim.engine.set_dof_actuation_forces_indexed(self._tensor(desc), self._tensor(ids_desc)[:n])
        return True

    # -- external forces (render_env.py:105-126) ------------------------------------------------------
    def apply_rigid_body_force_tensors(self, sim: Sim, force_desc=None, torque_desc=None, space: int = ENV_SPACE):
        """Forces at the bodies' centres of mass and torques, [N*24,3] each (a None descriptor: absent),
        acting during the next ``simulate`` only, as Isaac Gym clears them after each simulation step."""
        self._flush(sim)
        f = None if force_desc is None else self._tensor(force_desc)
        t = None if torque_desc is None else self._tensor(torque_desc)
        if f is None and t is None:
            return False  # Isaac Gym: nothing to apply (the engine's clear is Engine.clear_body_forces)
        sim.engine.apply_body_forces(f, t, int(space), hold=1)
        return True

    def apply_rigid_body_force_at_pos_tensors(self, sim: Sim, force_desc, pos_desc, space: int = ENV_SPACE):
        """Forces applied at the points ``pos`` ([N*24,3] each), acting during the next ``simulate``."""
        self._flush(sim)
        sim.engine.apply_body_forces_at_pos(self._tensor(force_desc), self._tensor(pos_desc), int(space), hold=1)
        return True

    # -- env state: save, restore, clone (engine extensions; INTEGRATION.md "Snapshots and branching") --
    # Each flushes the batched simulate() calls first, like a tensor write. An acquired force-sensor or
    # dynamics tensor is stale until its next refresh.
    def save_env_states(self, sim: Sim, ids_desc=None):
        """The packed states int32 [k, W] of envs ``ids`` (an int32 descriptor; None: every env in order) as
        a descriptor of a fresh tensor (``gymtorch.wrap_tensor`` gives the tensor itself)."""
        from . import gymtorch
        self._flush(sim)
        return gymtorch.unwrap_tensor(sim.engine.save_envs(None if ids_desc is None else self._tensor(ids_desc)))

    def load_env_states(self, sim: Sim, state_desc, ids_desc=None):
        """Rows of packed states (``save_env_states``) into envs ``ids`` (None: every env in order)."""
        self._flush(sim)
        sim.engine.load_envs(self._tensor(state_desc), None if ids_desc is None else self._tensor(ids_desc))
        return True

    def clone_env_states(self, sim: Sim, src_ids_desc, dst_ids_desc):
        """Env ``src_ids[i]`` copied to env ``dst_ids[i]`` (int32 descriptors), the whole state, root x and y
        included. A dst that is also a src of the call is undefined."""
        self._flush(sim)
        sim.engine.clone_envs(self._tensor(src_ids_desc), self._tensor(dst_ids_desc))
        return True

    # -- stepping -----------------------------------------------------------------------------------
    def simulate(self, sim: Sim):
        sim.pending_substeps += 1

    def fetch_results(self, sim: Sim, wait: bool = True):
        self._flush(sim)
        return True

    # -- camera sensors (render_env.py:151-171, 218-227, 398-411) -------------------------------------
    def create_camera_sensor(self, env: _Env, props: CameraProperties):
        """A camera on ``env`` (before or after prepare_sim); the handle counts the env's cameras."""
        sim = env.sim
        if props.width < 1 or props.height < 1:
            raise ValueError(f"camera size {props.width} x {props.height}")
        if sim.cameras and (sim.cameras[0].props.width, sim.cameras[0].props.height) != (props.width, props.height):
            raise NotImplementedError(
                f"camera of {props.width} x {props.height} in a sim whose cameras are {sim.cameras[0].props.width} x "
                f"{sim.cameras[0].props.height}: the cameras of one sim share one size (one launch draws them all)")
        sim.cameras.append(_Camera(env.index, props))
        env.cameras.append(len(sim.cameras) - 1)
        sim.cameras_dirty = True
        return len(env.cameras) - 1

    @staticmethod
    def _camera(env: _Env, handle) -> _Camera:
        if not 0 <= int(handle) < len(env.cameras):
            raise ValueError(f"env {env.index} has no camera {handle}")
        return env.sim.cameras[env.cameras[int(handle)]]

    @staticmethod
    def _forward(t: Transform):
        """A transform's position and the point one metre along its +X axis (the view direction of an
        Isaac Gym camera transform)."""
        q = np.array([t.r.x, t.r.y, t.r.z], np.float64)
        v = np.array([1.0, 0.0, 0.0])
        c = 2.0 * np.cross(q, v)
        fwd = v + t.r.w * c + np.cross(q, c)
        p = np.array([t.p.x, t.p.y, t.p.z], np.float64)
        return tuple(p), tuple(p + fwd)

    def set_camera_location(self, handle, env: _Env, pos: Vec3, target: Vec3):
        c = self._camera(env, handle)
        c.pos, c.target = tuple(pos), tuple(target)
        c.follow_body = -1
        env.sim.cameras_dirty = True

    def set_camera_transform(self, handle, env: _Env, transform: Transform):
        c = self._camera(env, handle)
        c.pos, c.target = self._forward(transform)
        c.follow_body = -1
        env.sim.cameras_dirty = True

    def attach_camera_to_body(self, handle, env: _Env, body: int, local_transform: Transform, mode: int):
        """The camera follows ``body`` of the env's actor, resolved on the device at render time:
        FOLLOW_POSITION keeps the world orientation of the offset, FOLLOW_TRANSFORM rotates with the body."""
        if mode not in (FOLLOW_POSITION, FOLLOW_TRANSFORM):
            raise ValueError(f"camera follow mode {mode}")
        if not 0 <= int(body) < _abi.NB:
            raise ValueError(f"body {body} outside [0, {_abi.NB})")
        c = self._camera(env, handle)
        c.pos, c.target = self._forward(local_transform)
        c.follow_body, c.follow_mode = int(body), int(mode)
        env.sim.cameras_dirty = True

    def set_rigid_body_color(self, env: _Env, actor, body: int, mesh_type: int, color: Vec3):
        if mesh_type not in (MESH_VISUAL, MESH_VISUAL_AND_COLLISION):
            return  # only the visual colour is drawn
        if not 0 <= int(body) < _abi.NB:
            raise ValueError(f"body {body} outside [0, {_abi.NB})")
        if env.body_rgb is None:
            from ..render import BODY_RGB
            env.body_rgb = np.tile(np.asarray(BODY_RGB, np.float32), (_abi.NB, 1))
        env.body_rgb[int(body)] = tuple(color)
        env.sim.appearance_dirty = True

    def set_rigid_body_segmentation_id(self, env: _Env, actor, body: int, seg_id: int):
        if not 0 <= int(body) < _abi.NB:
            raise ValueError(f"body {body} outside [0, {_abi.NB})")
        if env.body_seg is None:
            env.body_seg = np.zeros(_abi.NB, np.int32)
        env.body_seg[int(body)] = int(seg_id)
        env.sim.appearance_dirty = True

    def _sync_renderer(self, sim: Sim):
        import torch
        from .. import render as R
        if sim.engine is None:
            raise RuntimeError("render_all_camera_sensors before prepare_sim")
        if not sim.cameras:
            raise RuntimeError("render_all_camera_sensors without a camera sensor")
        if sim.renderer is None:
            sim.renderer = R.Renderer(sim.engine)
        sim.renderer.set_terrain_from_engine()  # host values only: the engine's terrain as it is now
        if sim.cameras_dirty:
            sim.renderer.set_cameras([
                R.camera(c.env, c.props.width, c.props.height, c.pos, c.target, hfov_deg=c.props.horizontal_fov,
                         near=c.props.near_plane, far=c.props.far_plane, follow_body=c.follow_body,
                         follow_mode=c.follow_mode) for c in sim.cameras])
            sim.cameras_dirty = False
        if sim.appearance_dirty:
            dev = sim.engine.device
            rgb = seg = None
            if any(e.body_rgb is not None for e in sim.envs):
                host = np.stack([e.body_rgb if e.body_rgb is not None
                                 else np.tile(np.asarray(R.BODY_RGB, np.float32), (_abi.NB, 1)) for e in sim.envs])
                rgb = torch.from_numpy(np.ascontiguousarray(host, np.float32)).to(dev)
            if any(e.body_seg is not None and e.body_seg.any() for e in sim.envs):
                host = np.stack([e.body_seg if e.body_seg is not None else np.zeros(_abi.NB, np.int32)
                                 for e in sim.envs])
                seg = torch.from_numpy(np.ascontiguousarray(host, np.int32)).to(dev)
            sim.renderer.set_appearance(rgb, seg)
            sim.appearance = (rgb, seg)
            sim.appearance_dirty = False

    def render_all_camera_sensors(self, sim: Sim):
        self._flush(sim)
        self._sync_renderer(sim)
        sim.renderer.render()
        sim.rendered = True
        return True

    # -- ray-cast sensor (engine extensions) ------------------------------------------------------------
    def _ray_renderer(self, sim: Sim, what: str):
        from .. import render as R
        if sim.engine is None:
            raise RuntimeError(f"{what} before prepare_sim")
        self._flush(sim)  # the sensor sees the state after every simulate call so far
        if sim.renderer is None:
            sim.renderer = R.Renderer(sim.engine)
        sim.renderer.set_terrain_from_engine()
        return sim.renderer

    def set_ray_sensor(self, sim: Sim, rays, body="Pelvis", frame="heading"):
        """Engine extension: the rays of ``cast_ray_sensor``, [R,6] host values (origin 3, direction 3), the
        same for every env, in a frame attached to ``body`` (an index or a name): "position", "heading" (about
        z by the body's heading) or "transform". 1 to 1024 rays; they replace the rays set before.
        ``humanoid_amd.render.height_scan_rays`` gives a grid of straight-down rays."""
        self._ray_renderer(sim, "set_ray_sensor").set_rays(rays, body, frame)
        return True

    def cast_ray_sensor(self, sim: Sim, dist_desc, hit_desc, max_range, skip_bodies=True):
        """Engine extension: one launch casts every env's rays at the current state against the env's terrain
        and, unless ``skip_bodies``, its 24 body geoms. dist [N,R] f32: the distance along the ray, +inf where
        nothing is hit within ``max_range``; hit [N,R] i32: -2 nothing, -1 terrain, else the body index. Either
        descriptor may be None, not both."""
        ren = self._ray_renderer(sim, "cast_ray_sensor")
        if dist_desc is None and hit_desc is None:
            from ..render import RenderError
            raise RenderError("cast_ray_sensor: no output tensor")
        ren.cast_rays(max_range, skip_bodies, None if dist_desc is None else self._tensor(dist_desc),
                      None if hit_desc is None else self._tensor(hit_desc))
        return True

    def _image(self, sim: Sim, env: _Env, handle, image_type):
        if image_type == IMAGE_OPTICAL_FLOW:
            raise NotImplementedError("IMAGE_OPTICAL_FLOW: the ray caster draws single frames and keeps no "
                                      "previous-frame geometry to difference against")
        if image_type not in (IMAGE_COLOR, IMAGE_DEPTH, IMAGE_SEGMENTATION):
            raise ValueError(f"image type {image_type}")
        idx = env.cameras[int(handle)] if 0 <= int(handle) < len(env.cameras) else None
        if idx is None:
            raise ValueError(f"env {env.index} has no camera {handle}")
        if not sim.rendered or sim.renderer is None or idx >= sim.renderer.num_cameras:
            raise RuntimeError("get_camera_image before render_all_camera_sensors: nothing has been drawn for "
                               "this camera yet")
        r = sim.renderer
        return (r.color, r.depth, r.seg)[image_type][idx]

    def get_camera_image(self, sim: Sim, env: _Env, handle, image_type):
        """numpy copy of the last render: colour uint8 [H, W*4] (Isaac Gym's flattened RGBA rows, reshaped
        by the caller, render_env.py:160), depth float32 [H,W], segmentation int32 [H,W]."""
        t = self._image(sim, env, handle, image_type)
        a = t.cpu().numpy()
        return a.reshape(a.shape[0], -1) if image_type == IMAGE_COLOR else a

    def get_camera_image_gpu_tensor(self, sim: Sim, env: _Env, handle, image_type):
        """The renderer's own image memory ([H,W,4] u8, [H,W] f32 / i32) as a GymTensor: wrap_tensor
        aliases it, and every later render_all_camera_sensors refreshes it in place."""
        from . import gymtorch
        if not sim.rendered:  # Isaac Gym hands the tensor out before the first render: draw once
            self.render_all_camera_sensors(sim)
        return gymtorch.unwrap_tensor(self._image(sim, env, handle, image_type))

    def start_access_image_tensors(self, sim: Sim):
        self._flush(sim)
        return True

    end_access_image_tensors = start_access_image_tensors
    step_graphics = start_access_image_tensors

    # -- viewer (absent) -----------------------------------------------------------------------------
    def create_viewer(self, sim, props):
        raise NotImplementedError("headless only: the engine has no viewer")


_GYM = None


def acquire_gym() -> Gym:
    global _GYM
    if _GYM is None:
        _GYM = Gym()
    return _GYM
