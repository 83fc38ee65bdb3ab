"""Centroidal dynamics: ctypes shim over the ``hc_`` entry points of ``libhumanoid_dynamics.so``
(``include/humanoid_centroidal.h``).

One HIP kernel forms, for the state the engine is in, the centre of mass ``com`` ``[N,3]``, its velocity
``com_vel`` ``[N,3]``, the momentum ``[N,6]`` (linear, then angular about the centre of mass), the
centroidal momentum matrix ``cmm`` ``[N,6,75]`` (``momentum = cmm @ qd``), its rate term ``cmm_bias``
``[N,6]`` (``d/dt momentum = cmm @ qdd + cmm_bias``) and the ``energy`` ``[N,2]`` (kinetic, potential) of
every env from the engine's root-state and dof-state buffers alone, so it is right immediately after an
indexed state write. :class:`Centroidal` owns the six tensors and launches on the engine's current
stream. The columns are those of :mod:`humanoid_amd.dynamics`. There is no CPU path: without the library
or a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes as C

from . import _abi
from .dynamics import LIB_PATH

from ._abi import NG  # noqa: F401

OUTPUTS = ("com", "com_vel", "momentum", "cmm", "cmm_bias", "energy")  # hc_outputs' members, in order
MOMENTUM_ROWS = 6


class HcOutputs(C.Structure):
    """hc_outputs: the six device pointers, in the header's order."""
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


_V, _I = C.c_void_p, C.c_int
# every exported hc_ symbol with its prototype (_abi.bind_library)
HC_PROTOTYPES = {
    "hc_last_error": (C.c_char_p, []), "hc_version": [], "hc_validate_model": [_V], "hc_create": [_I, _V, _V, _I, _V],
    "hc_destroy": [_V], "hc_compute": [_V, _V, _V, _V, _V],
}
HC_SYMBOLS = tuple(HC_PROTOTYPES)


class CentroidalError(RuntimeError):
    pass


# load (never build) the library, a return code, hc_validate_model and _abi.check_tensor, raising CentroidalError
_LIBRARY = _abi.Library(LIB_PATH, HC_PROTOTYPES, "hc", CentroidalError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


def output_shapes(num_envs: int):
    n = int(num_envs)
    return {"com": (n, 3), "com_vel": (n, 3), "momentum": (n, MOMENTUM_ROWS), "cmm": (n, MOMENTUM_ROWS, NG),
            "cmm_bias": (n, MOMENTUM_ROWS), "energy": (n, 2)}


class Centroidal(_abi.QueryBinding):
    """The centroidal tensors of one :class:`humanoid_amd.engine.Engine`: ``com``, ``com_vel``,
    ``momentum``, ``cmm``, ``cmm_bias`` and ``energy`` are allocated once and refreshed in place (views
    stay valid). Gravity (the potential energy's) is the engine's ``sim_params.gravity``; there are no
    flags: armature never reaches the base rows of the mass matrix."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the centroidal kernel has no CPU path"

    def __init__(self, engine):
        import torch
        super().__init__(engine)
        self.gravity_vector = tuple(float(x) for x in engine.params.gravity)
        for name, shape in output_shapes(self.num_envs).items():
            setattr(self, name, torch.zeros(shape, dtype=torch.float32, device=self.device))

    def refresh_into(self, com=None, com_vel=None, momentum=None, cmm=None, cmm_bias=None, energy=None,
                     root_state=None, dof_state=None):
        """hc_compute into caller tensors (``None``: that output is neither computed nor written). The
        states default to the engine's live root-state / dof-state buffers. Every tensor is checked
        (shape, dtype, device, contiguity) before any pointer is passed."""
        import torch
        given = dict(com=com, com_vel=com_vel, momentum=momentum, cmm=cmm, cmm_bias=cmm_bias, energy=energy)
        if all(t is None for t in given.values()):
            raise CentroidalError("refresh: no output asked for")
        shapes = output_shapes(self.num_envs)
        out = HcOutputs()
        for name, t in given.items():
            if t is not None:
                setattr(out, name, check_tensor(t, torch.float32, shapes[name], self.device, name))
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hc_compute(self.h, p_root, p_dof, C.byref(out), self.engine.stream))

    def refresh(self, com: bool = True, com_vel: bool = True, momentum: bool = True, cmm: bool = True,
                cmm_bias: bool = True, energy: bool = True):
        """Recompute what is asked from the engine's current state: one launch on the current stream, no
        host synchronisation, in place."""
        want = dict(com=com, com_vel=com_vel, momentum=momentum, cmm=cmm, cmm_bias=cmm_bias, energy=energy)
        self.refresh_into(**{name: getattr(self, name) if on else None for name, on in want.items()})

    def average_angular_velocity(self):
        """[N,3]: the locked inertia's angular velocity, ``cmm[:, 3:6, 3:6]^-1 momentum[:, 3:6]``, from the
        tensors as last refreshed (a torch one-liner, no kernel of its own)."""
        import torch
        return torch.linalg.solve(self.cmm[:, 3:6, 3:6], self.momentum[:, 3:6])

    def capture_point(self, ground_z: float = 0.0):
        """[N,2]: the instantaneous capture point of the linear inverted pendulum,
        ``com_xy + com_vel_xy * sqrt((com_z - ground_z) / |g_z|)``, from the tensors as last refreshed."""
        import torch
        t = torch.sqrt((self.com[:, 2:3] - ground_z) / abs(self.gravity_vector[2]))
        return self.com[:, :2] + self.com_vel[:, :2] * t
