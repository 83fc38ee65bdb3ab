"""Dynamics-query tensors: ctypes shim over ``libhumanoid_dynamics.so`` (``include/humanoid_dynamics.h``).

One HIP kernel forms, for the state the engine is in, the body Jacobians ``[N,24,6,75]``, the
joint-space inertia ``[N,75,75]`` and the gravity / Coriolis force ``[N,75]`` of every env from the
engine's root-state and dof-state buffers alone (its own forward kinematics, so it is right
immediately after an indexed state write); the library only reads the engine's memory.
:class:`Dynamics` owns the three output tensors and launches on the engine's current stream. There is
no CPU path: without the library or a GPU the constructor raises.

Columns follow Isaac Gym's floating-base order: root linear velocity 3, root angular velocity 3, the
69 dof velocities. The dof velocities are the engine's child-frame relative rates of the exp-map ball
joints, not derivatives of the exp-map coordinates (the header has the definitions).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _abi

from ._abi import FLAG_ARMATURE, FLAG_NO_GRAVITY, FLAGS_DEFAULT, NG  # noqa: F401  (include/humanoid_dynamics.h)
from .build import LIBRARIES

LIB_PATH = LIBRARIES["dynamics"].path
JAC_ROWS = 6

_V, _I = C.c_void_p, C.c_int
# every exported symbol with its prototype (_abi.bind_library)
HD_PROTOTYPES = {
    "hd_last_error": (C.c_char_p, []), "hd_version": [], "hd_validate_model": [_V], "hd_create": [_I, _V, _V, _I, _V],
    "hd_destroy": [_V], "hd_compute": [_V, _V, _V, _V, _V, _V, C.c_uint32, _V],
}
HD_SYMBOLS = tuple(HD_PROTOTYPES)


class DynamicsError(RuntimeError):
    pass


# load (never build) the library, a return code, hd_validate_model and _abi.check_tensor, raising DynamicsError
_LIBRARY = _abi.Library(LIB_PATH, HD_PROTOTYPES, "hd", DynamicsError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


def output_shapes(num_envs: int):
    n = int(num_envs)
    return {"jacobian": (n, _abi.NB, JAC_ROWS, NG), "mass_matrix": (n, NG, NG), "bias": (n, NG)}


class Dynamics(_abi.QueryBinding):
    """The dynamics-query tensors of one :class:`humanoid_amd.engine.Engine`.

    ``jacobian`` f32 [N,24,6,75] (rows: body-origin linear velocity, world angular velocity),
    ``mass_matrix`` f32 [N,75,75] and ``bias`` f32 [N,75] are allocated once and refreshed in place
    (views stay valid). ``armature`` (default on: the inertia the engine's own solve uses) puts the
    model's dof armature on the mass matrix's diagonal; ``gravity`` (default on) keeps gravity in the
    bias force. Gravity is the engine's ``sim_params.gravity``."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the dynamics kernel has no CPU path"

    def __init__(self, engine, armature: bool = True):
        import torch
        super().__init__(engine, armature)
        shapes = output_shapes(self.num_envs)
        self.jacobian = torch.zeros(shapes["jacobian"], dtype=torch.float32, device=self.device)
        self.mass_matrix = torch.zeros(shapes["mass_matrix"], dtype=torch.float32, device=self.device)
        self.bias = torch.zeros(shapes["bias"], dtype=torch.float32, device=self.device)
        self._solver = None  # humanoid_amd.solve.Solver, created by the first solve
        self._task = None  # humanoid_amd.task.TaskSpace, created by the first use

    def refresh_into(self, jacobian=None, mass_matrix=None, bias=None, flags: Optional[int] = None, root_state=None,
                     dof_state=None):
        """hd_compute into caller tensors (``None``: that output is not computed). The states default to
        the engine's live root-state / dof-state buffers. Every tensor is checked (shape, dtype, device,
        contiguity) before any pointer is passed."""
        import torch
        shapes = output_shapes(self.num_envs)
        if jacobian is None and mass_matrix is None and bias is None:
            raise DynamicsError("refresh: no output asked for")
        f32 = torch.float32
        p_jac = None if jacobian is None else check_tensor(jacobian, f32, shapes["jacobian"], self.device, "jacobian")
        p_mass = None if mass_matrix is None else check_tensor(mass_matrix, f32, shapes["mass_matrix"], self.device,
                                                               "mass_matrix")
        p_bias = None if bias is None else check_tensor(bias, f32, shapes["bias"], self.device, "bias")
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hd_compute(self.h, p_root, p_dof, p_jac, p_mass, p_bias, self._flags(flags), self.engine.stream))

    def refresh(self, jacobian: bool = True, mass_matrix: bool = True, bias: bool = True):
        """Recompute what is asked from the engine's current state: one launch on the current stream, no
        host synchronisation, in place."""
        self.refresh_into(self.jacobian if jacobian else None, self.mass_matrix if mass_matrix else None,
                          self.bias if bias else None)

    def generalized_velocity(self):
        """qd [N,75] of the engine's current state: root linear velocity, root angular velocity, the 69
        dof velocities (a torch gather; defining property: ``jacobian @ qd == rb_state[..., 7:13]``)."""
        import torch
        e = self.engine
        return torch.cat([e.root_states[:, 7:13], e.dof_state.view(self.num_envs, _abi.ND, 2)[:, :, 1]], dim=1)

    def inverse_dynamics(self, qdd):
        """tau = mass_matrix @ qdd + bias for qdd [N,75], from the tensors as last refreshed (a torch
        one-liner, no kernel of its own)."""
        return (self.mass_matrix @ qdd.unsqueeze(-1)).squeeze(-1) + self.bias

    # -- the solves with M (include/humanoid_solve.h): kernels of their own, from the engine's current
    # state, not from the tensors as last refreshed
    @property
    def solver(self):
        """The :class:`humanoid_amd.solve.Solver` of this engine (created on first use), with this
        object's ``armature`` and ``gravity`` settings."""
        if getattr(self, "_solver", None) is None:
            from .solve import Solver
            self._solver = Solver(self.engine, armature=self.armature)
        self._solver.armature, self._solver.gravity = self.armature, self.gravity
        return self._solver

    @property
    def task(self):
        """The :class:`humanoid_amd.task.TaskSpace` of this engine (created on first use; its rows stay
        set), with this object's ``armature`` and ``gravity`` settings."""
        if getattr(self, "_task", None) is None:
            from .task import TaskSpace
            self._task = TaskSpace(self.engine, armature=self.armature)
        self._task.armature, self._task.gravity = self.armature, self.gravity
        return self._task

    @property
    def ik(self):
        """The :class:`humanoid_amd.ik.InverseKinematics` of this engine (created on first use; its rows
        stay set), with this object's ``armature`` setting; gravity does not enter it."""
        if getattr(self, "_ik", None) is None:
            from .ik import InverseKinematics
            self._ik = InverseKinematics(self.engine, armature=self.armature)
        self._ik.armature = self.armature
        return self._ik

    @property
    def centroidal(self):
        """The :class:`humanoid_amd.centroidal.Centroidal` of this engine (created on first use): centre of
        mass, momentum, the centroidal momentum matrix and the energies. It has no settings to hand over:
        armature and gravity do not enter its momentum rows."""
        if getattr(self, "_centroidal", None) is None:
            from .centroidal import Centroidal
            self._centroidal = Centroidal(self.engine)
        return self._centroidal

    @property
    def reaction(self):
        """The :class:`humanoid_amd.reaction.Reaction` of this engine (created on first use): the wrench
        every joint transmits and the bodies' accelerations, with this object's ``armature`` and ``gravity``
        settings."""
        if getattr(self, "_reaction", None) is None:
            from .reaction import Reaction
            self._reaction = Reaction(self.engine, armature=self.armature)
        self._reaction.armature, self._reaction.gravity = self.armature, self.gravity
        return self._reaction

    @property
    def derivatives(self):
        """The :class:`humanoid_amd.derivatives.Derivatives` of this engine (created on first use): the
        derivatives of the inverse and forward dynamics with respect to the pose and the generalised
        velocity, with this object's ``armature`` and ``gravity`` settings."""
        if getattr(self, "_derivatives", None) is None:
            from .derivatives import Derivatives
            self._derivatives = Derivatives(self.engine, armature=self.armature)
        self._derivatives.armature, self._derivatives.gravity = self.armature, self.gravity
        return self._derivatives

    def forward_dynamics(self, gen_force=None, out=None):
        """qdd [N,75] = M^-1 (gen_force - c) at the engine's current state: one launch, M never written."""
        return self.solver.forward_dynamics(gen_force, out)

    def computed_torque(self, qdd_des, gen_force=None, out=None, base_acc=None):
        """(tau [N,69], base_acc [N,6]) with M (base_acc; qdd_des) + c - gen_force = (0; tau)."""
        return self.solver.computed_torque(qdd_des, gen_force, out, base_acc)

    def solve(self, rhs, out=None):
        """M^-1 on each of the k <= 32 rows of rhs [N,k,75]."""
        return self.solver.solve(rhs, out)
