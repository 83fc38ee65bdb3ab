"""Force sensors: the wrench a body's parent joint transmits, read at a sensor pose on the body, from
the step the engine last ran (``gym.acquire_force_sensor_tensor``; usable with an
:class:`humanoid_amd.engine.Engine` directly).

The reading, defined. ``before_step()`` is called immediately before a launch and copies the generalised
velocity ``qd`` ``[N,75]`` (root linear 3, root angular 3, the 69 dof rates). ``read(dt, out)`` after the
launch, with ``dt`` the simulated time it advanced, forms the step's mean acceleration
``qdd = (qd_now - qd_before) / dt`` (``include/humanoid_solve.h``'s convention: the time derivative of those
velocities) and, for sensor ``s`` on body ``b`` with pose ``(p_s, q_s)`` in b's frame:

* ``F_b``: the force part of ``hw_compute``'s ``wrench[b]`` in world axes (``include/humanoid_wrench.h``),
  prescribed base with ``base_acc = qdd[0:6]``, ``qdd_des = qdd[6:]``, ``body_force`` the engine's net
  contact forces and no torque. Only the contacts' forces enter the force sum, so it is exact;
* ``N_b = sum_i (tau_{b,i} - armature_{b,i} qdd_{b,i}) R_b e_i`` with ``tau`` the engine's dof forces (drive,
  limit and actuation): every joint is a ball joint, which transmits about its centre exactly its three
  dof torques. (The kernel's own torque would need the contacts' moments, which the engine does not export);
* reading ``= (Q^T F_b, Q^T (N_b - (R_b p_s) x F_b))`` with ``Q = R_b R(q_s)``, or ``Q = 1`` for a sensor
  with ``world_frame`` set.

It is the wrench on the body by its parent. Before the first launch after construction the reading is
zero. An env whose state was written since the last launch (a reset) reads rows that mean nothing until
the next launch: the velocity difference then spans the write.
"""
from __future__ import annotations

from . import _abi
from ._abi import NB, ND, NG


def _quat_matrix(q):
    """[S,3,3] of xyzw quaternions [S,4] (normalised here)."""
    import torch
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


class ForceSensors:
    """``S`` sensors, the same on every env of ``engine``: ``bodies`` [S] body indices (1..23: a sensor
    measures a parent joint, which the root has none of), ``poses`` [S,7] (position 3, quaternion xyzw)
    in the body's frame, ``world_frame`` [S] bools (the reading in world axes instead of the sensor's).
    ``reaction`` is the :class:`humanoid_amd.reaction.Reaction` to launch with (made here when None)."""

    def __init__(self, engine, bodies, poses, world_frame=None, reaction=None):
        import torch
        bodies = [int(b) for b in bodies]
        if not bodies:
            raise ValueError("ForceSensors: no sensor")
        for b in bodies:
            if not 1 <= b < NB:
                raise ValueError(f"ForceSensors: body {b} outside 1..{NB - 1} (a sensor measures a parent joint)")
        dev, f32 = engine.device, torch.float32
        poses = torch.as_tensor(poses, dtype=f32).reshape(len(bodies), 7).to(dev)
        world = [False] * len(bodies) if world_frame is None else [bool(w) for w in world_frame]
        if len(world) != len(bodies):
            raise ValueError("ForceSensors: world_frame and bodies differ in length")
        if reaction is None:
            from .reaction import Reaction
            reaction = Reaction(engine)
        self.engine, self.reaction, self.num_sensors = engine, reaction, len(bodies)
        n = engine.num_envs
        self.bodies = torch.tensor(bodies, dtype=torch.long, device=dev)
        self.offset = poses[:, :3].contiguous()                       # p_s, body frame
        self.rot = _quat_matrix(poses[:, 3:7])                        # R(q_s)
        self.world = torch.tensor(world, dtype=torch.bool, device=dev)
        self.armature = torch.tensor([float(a) for a in engine.he_model.armature], dtype=f32, device=dev)
        self.qd_before = torch.zeros(n, NG, dtype=f32, device=dev)
        self.qdd = torch.zeros(n, NG, dtype=f32, device=dev)
        self.qdd_des = torch.zeros(n, ND, dtype=f32, device=dev)
        self.base_acc = torch.zeros(n, 6, dtype=f32, device=dev)
        self.stepped = False

    def _velocity(self, out):
        e, n = self.engine, self.engine.num_envs
        out[:, :6] = e.root_states[:, 7:13]
        out[:, 6:] = e.dof_state.view(n, ND, 2)[:, :, 1]

    def before_step(self):
        """Copy the generalised velocity: call immediately before the launch ``read`` is to report."""
        self._velocity(self.qd_before)
        self.stepped = True

    def read(self, dt: float, out):
        """The readings [N*S,6] (force 3, torque 3 per sensor) into ``out`` for the launch that followed
        ``before_step`` and advanced ``dt`` of simulated time; zeros before any."""
        import torch
        e, n, s = self.engine, self.engine.num_envs, self.num_sensors
        if tuple(out.shape) != (n * s, 6):
            raise ValueError(f"ForceSensors.read: out of shape {tuple(out.shape)}, expected {(n * s, 6)}")
        if not self.stepped:
            out.zero_()
            return out
        self._velocity(self.qdd)
        self.qdd.sub_(self.qd_before).div_(float(dt))
        self.qdd_des.copy_(self.qdd[:, 6:])
        self.base_acc.copy_(self.qdd[:, :6])
        wrench = self.reaction.compute(self.qdd_des, self.base_acc, body_force=e.contact_forces, frame="world",
                                       flags=_abi.FLAG_ARMATURE)["wrench"]
        F = wrench[:, self.bodies, :3]                                                   # [N,S,3]
        rb = e.rb_state.view(n, NB, 13)[:, self.bodies, 3:7].reshape(n * s, 4)
        Rb = _quat_matrix(rb).view(n, s, 3, 3)
        d0 = (3 * (self.bodies - 1))[:, None] + torch.arange(3, device=self.bodies.device)[None, :]  # [S,3] dofs
        tau = e.dof_force.view(n, ND)[:, d0] - self.armature[d0] * self.qdd_des[:, d0]  # [N,S,3], joint axes
        N = torch.einsum("nsij,nsj->nsi", Rb, tau)
        lever = torch.einsum("nsij,sj->nsi", Rb, self.offset)
        N = N - torch.cross(lever, F, dim=-1)
        Q = torch.einsum("nsij,sjk->nsik", Rb, self.rot)
        eye = torch.eye(3, dtype=Q.dtype, device=Q.device).expand_as(Q)
        Q = torch.where(self.world[None, :, None, None], eye, Q)
        o = out.view(n, s, 6)
        o[:, :, :3] = torch.einsum("nsji,nsj->nsi", Q, F)
        o[:, :, 3:] = torch.einsum("nsji,nsj->nsi", Q, N)
        return out
