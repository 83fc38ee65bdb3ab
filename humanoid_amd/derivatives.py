"""Dynamics derivatives: ctypes shim over the ``hg_`` entry points of ``libhumanoid_solve.so``
(``include/humanoid_derivatives.h``).

One launch of the computed-torque kernel gives, for the state the engine is in and a generalised
acceleration ``acc`` ``[N,75]``, how the inverse dynamics ``tau = M(q) a + c(q, qd)`` changes with the pose,
``dtau_dq`` ``[N,75,75]``, and with the generalised velocity, ``dtau_dv`` ``[N,75,75]``, and ``tau``
``[N,75]`` itself (base rows included). The derivatives are exact (tangents propagated along the tree, no
differencing); a pose direction is the header's ``q (+) delta``, the map of the inverse kinematics' step.
:meth:`Derivatives.forward_dynamics` turns them into the derivatives of ``qdd = M^-1 (gen_force - c)`` with
the solves of :mod:`humanoid_amd.solve`. The columns are those of :mod:`humanoid_amd.dynamics`. There is no
CPU path: without the library or a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _abi
from .solve import LIB_PATH, MAX_RHS

from ._abi import FLAG_ARMATURE, FLAG_NO_GRAVITY, FLAGS_DEFAULT, NG  # noqa: F401  (include/humanoid_derivatives.h)

FLAG_BY_DIRECTION = 4  # HG_FLAG_BY_DIRECTION: the matrices as [e, j, i]
OUTPUTS = ("dtau_dq", "dtau_dv", "tau")  # hg_outputs' members, in order


class HgOutputs(C.Structure):
    """hg_outputs: the three device pointers, in the header's order."""
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


_V, _I, _U = C.c_void_p, C.c_int, C.c_uint32
# every exported hg_ symbol with its prototype (_abi.bind_library)
HG_PROTOTYPES = {
    "hg_last_error": (C.c_char_p, []), "hg_version": [], "hg_validate_model": [_V], "hg_create": [_I, _V, _V, _I, _V],
    "hg_destroy": [_V], "hg_compute": [_V, _V, _V, _V, _V, _U, _V],
}
HG_SYMBOLS = tuple(HG_PROTOTYPES)


class DerivativesError(RuntimeError):
    pass


# load (never build) the library, a return code, hg_validate_model and _abi.check_tensor, raising DerivativesError
_LIBRARY = _abi.Library(LIB_PATH, HG_PROTOTYPES, "hg", DerivativesError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


def output_shapes(num_envs: int):
    n = int(num_envs)
    return {"dtau_dq": (n, NG, NG), "dtau_dv": (n, NG, NG), "tau": (n, NG)}


class Derivatives(_abi.QueryBinding):
    """The dynamics derivatives of one :class:`humanoid_amd.engine.Engine`.

    ``armature`` (default on) adds ``armature * a`` to ``tau`` and puts the armature on the ``M`` of the
    forward form; ``gravity`` (default on) keeps gravity in ``c``. Gravity is the engine's
    ``sim_params.gravity``. The output tensors are allocated on first use and refreshed in place after that
    (views stay valid); every launch goes on the engine's stream without synchronising the host."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the derivative kernel has no CPU path"

    def inverse_dynamics(self, acc=None, dtau_dq: bool = True, dtau_dv: bool = True, tau: bool = False,
                         by_direction: bool = False, out=None, flags: Optional[int] = None, root_state=None,
                         dof_state=None):
        """hg_compute: a dict of the tensors asked for, by ``OUTPUTS``' names.

        ``acc`` [N,75] is the generalised acceleration (None: zero). ``dtau_dq[e, i, j]`` is the derivative
        of row ``i`` along pose direction ``j``, ``dtau_dv[e, i, j]`` that with respect to ``qd_j``;
        ``by_direction`` writes both as ``[e, j, i]`` (row ``j`` a right-hand side of ``Solver.solve``).
        ``out`` may map an output's name to a caller tensor, which is then filled in place of this object's
        own. The states default to the engine's live buffers."""
        import torch
        n, f32 = self.num_envs, torch.float32
        want = dict(dtau_dq=dtau_dq, dtau_dv=dtau_dv, tau=tau)
        given = dict(out or {})
        if set(given) - set(OUTPUTS):
            raise DerivativesError(f"inverse_dynamics: out names {sorted(set(given) - set(OUTPUTS))} (outputs: {OUTPUTS})")
        if not (any(want.values()) or given):
            raise DerivativesError("inverse_dynamics: no output asked for")
        p_acc = None if acc is None else check_tensor(acc, f32, (n, NG), self.device, "acc")
        shapes = output_shapes(n)
        o, result = HgOutputs(), {}
        for name in OUTPUTS:
            t = given.get(name)
            if t is None and want[name]:
                t = getattr(self, "_" + name, None)
                if t is None:  # this object's own storage, made once
                    t = torch.zeros(shapes[name], dtype=f32, device=self.device)
                    setattr(self, "_" + name, t)
            if t is not None:
                setattr(o, name, check_tensor(t, f32, shapes[name], self.device, name))
                if t is acc or any(t is r for r in result.values()):
                    raise DerivativesError(f"{name}: an output is also an input or another output")
                result[name] = t
        p_root, p_dof = self._states(root_state, dof_state)
        f = self._flags(flags) | (FLAG_BY_DIRECTION if by_direction else 0)
        _check(self.lib.hg_compute(self.h, p_root, p_dof, p_acc, C.byref(o), f, self.engine.stream))
        return result

    @property
    def solver(self):
        """The :class:`humanoid_amd.solve.Solver` of this engine (created on first use), with this object's
        ``armature`` and ``gravity`` settings."""
        if getattr(self, "_solver", None) is None:
            from .solve import Solver
            self._solver = Solver(self.engine, armature=self.armature)
        self._solver.armature, self._solver.gravity = self.armature, self.gravity
        return self._solver

    def forward_dynamics(self, gen_force=None, dqdd_dtau: bool = False, root_state=None, dof_state=None):
        """The forward dynamics ``qdd = M^-1 (gen_force - c)`` and its derivatives at fixed ``gen_force``
        [N,75] (None: zero): a dict of ``qdd`` [N,75], ``dqdd_dq`` and ``dqdd_dv`` [N,75,75] indexed
        ``[i, j]`` and, when asked, ``dqdd_dtau = M^-1``. Eight launches for the first three (the solve, the
        derivatives by direction at ``a = qdd``, ``M^-1`` on each matrix in three chunks of at most 32 rows) and torch
        copies between them, all on the engine's stream with no host synchronisation."""
        import torch
        n = self.num_envs
        sol = self.solver
        states = dict(root_state=root_state, dof_state=dof_state)
        qdd = sol.forward_dynamics(gen_force, **states)
        d = self.inverse_dynamics(qdd, by_direction=True, **states)

        def minv(rows):  # [N,75,75] rows -> M^-1 on every row, back as columns
            x = torch.cat([sol.solve(rows[:, c:c + MAX_RHS].contiguous(), **states) for c in range(0, NG, MAX_RHS)], dim=1)
            return x.transpose(1, 2).contiguous()

        result = dict(qdd=qdd, dqdd_dq=minv(d["dtau_dq"]).neg_(), dqdd_dv=minv(d["dtau_dv"]).neg_())
        if dqdd_dtau:
            eye = torch.eye(NG, dtype=torch.float32, device=self.device).expand(n, NG, NG)
            result["dqdd_dtau"] = minv(eye)
        return result
