"""Joint-space solves: ctypes shim over ``libhumanoid_solve.so`` (``include/humanoid_solve.h``).

The solves with the mass matrix ``M`` that a controller calls each step, each one launch that forms
``M`` (and the bias force ``c`` where the entry needs it) from the engine's root-state and dof-state
buffers, factors it in registers and writes only the answer:

* ``forward_dynamics``: ``qdd = M^-1 (gen_force - c)`` ``[N,75]``;
* ``computed_torque``: the joint torques ``[N,69]`` and the base acceleration ``[N,6]`` with
  ``M (a_b; qdd_des) + c - gen_force = (0_6; tau)`` (floating-base inverse dynamics);
* ``solve``: ``M^-1`` on ``k <= 32`` rows per env ``[N,k,75]`` (a Jacobian block gives ``J M^-1``).

``M``, ``c`` and the column order (root linear 3, root angular 3, 69 child-frame dof rates) are those
of :mod:`humanoid_amd.dynamics`. There is no CPU path: without the library or a GPU the constructor
raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _abi

from ._abi import FLAG_ARMATURE, FLAG_NO_GRAVITY, FLAGS_DEFAULT, NG  # noqa: F401  (include/humanoid_solve.h)
from .build import LIBRARIES

LIB_PATH = LIBRARIES["solve"].path
MAX_RHS = 32

_V, _I, _U = C.c_void_p, C.c_int, C.c_uint32
# every exported symbol with its prototype (_abi.bind_library)
HS_PROTOTYPES = {
    "hs_last_error": (C.c_char_p, []), "hs_version": [], "hs_validate_model": [_V], "hs_create": [_I, _V, _V, _I, _V],
    "hs_destroy": [_V], "hs_forward_dynamics": [_V, _V, _V, _V, _V, _U, _V],
    "hs_computed_torque": [_V, _V, _V, _V, _V, _V, _V, _U, _V], "hs_solve": [_V, _V, _V, _V, _V, _I, _U, _V],
}
HS_SYMBOLS = tuple(HS_PROTOTYPES)


class SolveError(RuntimeError):
    pass


# load (never build) the library, a return code, hs_validate_model and _abi.check_tensor, raising SolveError
_LIBRARY = _abi.Library(LIB_PATH, HS_PROTOTYPES, "hs", SolveError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


class Solver(_abi.QueryBinding):
    """The joint-space solves of one :class:`humanoid_amd.engine.Engine`.

    ``armature`` (default on: the inertia the engine's own solve uses) puts the model's dof armature on
    ``M``'s diagonal; ``gravity`` (default on) keeps gravity in ``c``. Gravity is the engine's
    ``sim_params.gravity``. The states default to the engine's live buffers, every launch goes on the
    engine's stream without synchronising the host, and an ``out`` tensor is allocated when not given."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the solve kernels have no CPU path"

    def forward_dynamics(self, gen_force=None, out=None, flags: Optional[int] = None, root_state=None, dof_state=None):
        """qdd [N,75] = M^-1 (gen_force - c); ``gen_force`` [N,75] or None for zero."""
        import torch
        n = self.num_envs
        p_f = None if gen_force is None else check_tensor(gen_force, torch.float32, (n, NG), self.device, "gen_force")
        out, p_out = self._out(out, (n, NG), "out")
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hs_forward_dynamics(self.h, p_root, p_dof, p_f, p_out, self._flags(flags), self.engine.stream))
        return out

    def computed_torque(self, qdd_des, gen_force=None, out=None, base_acc=None, flags: Optional[int] = None,
                        root_state=None, dof_state=None, want_tau: bool = True, want_base_acc: bool = True):
        """(tau [N,69], base_acc [N,6]) with M (base_acc; qdd_des) + c - gen_force = (0; tau). ``out`` and
        ``base_acc`` are filled when given and allocated otherwise; ``want_tau`` / ``want_base_acc`` False
        leaves that output out of the launch (None is returned in its place)."""
        import torch
        n = self.num_envs
        f32 = torch.float32
        if not (want_tau or want_base_acc):
            raise SolveError("computed_torque: no output asked for")
        p_q = check_tensor(qdd_des, f32, (n, _abi.ND), self.device, "qdd_des")
        p_f = None if gen_force is None else check_tensor(gen_force, f32, (n, NG), self.device, "gen_force")
        p_tau = p_acc = None
        if want_tau:
            out, p_tau = self._out(out, (n, _abi.ND), "out")
        if want_base_acc:
            base_acc, p_acc = self._out(base_acc, (n, 6), "base_acc")
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hs_computed_torque(self.h, p_root, p_dof, p_q, p_f, p_tau, p_acc, self._flags(flags),
                                           self.engine.stream))
        return (out if want_tau else None), (base_acc if want_base_acc else None)

    def solve(self, rhs, out=None, flags: Optional[int] = None, root_state=None, dof_state=None):
        """out [N,k,75] = M^-1 on each of the k rows of ``rhs`` [N,k,75], 1 <= k <= 32; not in place."""
        import torch
        n = self.num_envs
        if not isinstance(rhs, torch.Tensor) or rhs.dim() != 3:
            raise SolveError(f"rhs: expected a torch tensor of shape ({n}, k, {NG})")
        k = int(rhs.shape[1])
        if not 1 <= k <= MAX_RHS:
            raise SolveError(f"rhs: k = {k} outside 1..{MAX_RHS}")
        p_rhs = check_tensor(rhs, torch.float32, (n, k, NG), self.device, "rhs")
        if out is rhs:
            raise SolveError("out: rhs and out are the same tensor (the solve is not in place)")
        out, p_out = self._out(out, (n, k, NG), "out")
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hs_solve(self.h, p_root, p_dof, p_rhs, p_out, k, self._flags(flags), self.engine.stream))
        return out
