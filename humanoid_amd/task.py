"""Task-space control: ctypes shim over ``libhumanoid_task.so`` (``include/humanoid_task.h``).

For a set of task rows (velocity components of points on bodies: hands, feet, head), one launch forms
from the engine's root-state and dof-state buffers the rows' Jacobian ``J``, factors the mass matrix
``M`` in registers and writes only what is asked for:

* ``terms``: ``J`` ``[N,k,75]``, ``J M^-1`` ``[N,k,75]``, the inverse operational-space inertia
  ``J M^-1 J^T`` ``[N,k,k]``, the velocity-product acceleration ``Jdot qd`` ``[N,k]`` and the free task
  acceleration ``J M^-1 (gen_force - c) + Jdot qd`` ``[N,k]``;
* ``control``: the generalised force ``u`` ``[N,75]`` that gives the task the acceleration ``xdd_des``
  (``mode="force"``: the operational-space force ``J^T F``; ``mode="joint"``: the joint torque of
  minimum norm with the floating base unactuated, base entries exactly zero), the task force ``F``
  ``[N,k]`` and the resulting ``qdd = M^-1 (gen_force + u - c)`` ``[N,75]``.

``M``, ``c`` and the column order (root linear 3, root angular 3, 69 child-frame dof rates) are those
of :mod:`humanoid_amd.dynamics`. There is no CPU path: without the library or a GPU the constructor
raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

from . import _abi

from ._abi import FLAG_ARMATURE, FLAG_NO_GRAVITY, FLAGS_DEFAULT, NG  # noqa: F401  (include/humanoid_task.h)
from .build import LIBRARIES

LIB_PATH = LIBRARIES["task"].path
MODE_FORCE, MODE_JOINT = 0, 1
MODES = {"force": MODE_FORCE, "joint": MODE_JOINT}
MAX_ROWS = 32


class HtRow(C.Structure):
    """ht_row: a body, an axis (0..2 linear x y z of the point, 3..5 angular) and a body-frame point."""
    _fields_ = [("body", C.c_int32), ("axis", C.c_int32), ("point", C.c_float * 3)]


_V, _I, _U, _F = C.c_void_p, C.c_int, C.c_uint32, C.c_float
# every exported symbol with its prototype (_abi.bind_library)
HT_PROTOTYPES = {
    "ht_last_error": (C.c_char_p, []), "ht_version": [], "ht_validate_model": [_V], "ht_create": [_I, _V, _V, _I, _V],
    "ht_destroy": [_V], "ht_set_rows": [_V, _V, _I],
    "ht_task_terms": [_V, _V, _V, _V, _V, _V, _V, _V, _V, _U, _V],
    "ht_task_control": [_V, _V, _V, _V, _V, _I, _F, _V, _V, _V, _U, _V],
}
HT_SYMBOLS = tuple(HT_PROTOTYPES)
TERMS = ("jac", "jminv", "lambda_inv", "bias_acc", "free_acc")  # ht_task_terms' outputs, in argument order


class TaskError(RuntimeError):
    pass


# load (never build) the library, a return code, ht_validate_model and _abi.check_tensor, raising TaskError
_LIBRARY = _abi.Library(LIB_PATH, HT_PROTOTYPES, "ht", TaskError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


def make_rows(rows):
    """(HtRow array, k) from ``(body index or name, axis, point=(0, 0, 0))`` tuples. Names are resolved
    here; the ranges are the library's to check."""
    from .body_sets import BODY_NAMES
    rows = list(rows)
    arr = (HtRow * max(len(rows), 1))()
    for r, row in enumerate(rows):
        if not isinstance(row, (tuple, list)) or not 2 <= len(row) <= 3:
            raise TaskError(f"rows[{r}]: expected (body, axis) or (body, axis, point), got {row!r}")
        body, axis = row[0], row[1]
        point = row[2] if len(row) == 3 else (0.0, 0.0, 0.0)
        if isinstance(body, str):
            if body not in BODY_NAMES:
                raise TaskError(f"rows[{r}]: no body named {body!r}")
            body = BODY_NAMES.index(body)
        if len(point) != 3:
            raise TaskError(f"rows[{r}]: the point has {len(point)} components, not 3")
        arr[r].body, arr[r].axis = int(body), int(axis)
        arr[r].point[:] = [float(x) for x in point]
    return arr, len(rows)


class TaskSpace(_abi.QueryBinding):
    """Task-space control on one :class:`humanoid_amd.engine.Engine`.

    ``armature`` (default on: the inertia the engine's own solve uses) puts the model's dof armature on
    ``M``'s diagonal; ``gravity`` (default on) keeps gravity in ``c``. Gravity is the engine's
    ``sim_params.gravity``. The rows are shared by every env and set by :meth:`set_rows`. The states
    default to the engine's live buffers, every launch goes on the engine's stream without synchronising
    the host, and an output tensor is allocated when not given."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the task kernel has no CPU path"

    def __init__(self, engine, armature: bool = True):
        self.num_rows = 0
        super().__init__(engine, armature)

    def set_rows(self, rows):
        """The task rows, ``(body index or name, axis, point=(0, 0, 0))`` each, 1 to 32 of them; they
        replace the rows set before. A refused call leaves those in place."""
        arr, k = make_rows(rows)
        _check(self.lib.ht_set_rows(self.h, arr, k))
        self.num_rows = k
        return k

    def _rows(self, what):
        if self.num_rows < 1:
            raise TaskError(f"{what}: no rows set (set_rows)")
        return self.num_rows

    def terms(self, gen_force=None, want=TERMS, out=None, flags: Optional[int] = None, root_state=None, dof_state=None):
        """The task terms named in ``want`` (any of "jac" [N,k,75], "jminv" [N,k,75], "lambda_inv"
        [N,k,k], "bias_acc" [N,k], "free_acc" [N,k]) as a dict; what is not named is left out of the
        launch. ``out`` may hold caller tensors by the same names (they are asked for too);
        ``gen_force`` [N,75] or None for zero enters free_acc."""
        import torch
        n, k = self.num_envs, self._rows("terms")
        out = dict(out or {})
        names = [t for t in TERMS if t in tuple(want) or t in out]
        unknown = [t for t in list(want) + list(out) if t not in TERMS]
        if unknown:
            raise TaskError(f"terms: unknown output {unknown[0]!r} (one of {TERMS})")
        if not names:
            raise TaskError("terms: no output asked for")
        shapes = {"jac": (n, k, NG), "jminv": (n, k, NG), "lambda_inv": (n, k, k), "bias_acc": (n, k), "free_acc": (n, k)}
        p_f = None if gen_force is None else check_tensor(gen_force, torch.float32, (n, NG), self.device, "gen_force")
        res, ptrs = {}, []
        for t in TERMS:
            if t in names:
                res[t], p = self._out(out.get(t), shapes[t], t)
                ptrs.append(p)
            else:
                ptrs.append(None)
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.ht_task_terms(self.h, p_root, p_dof, p_f, *ptrs, self._flags(flags),
                                      self.engine.stream))
        return res

    def control(self, xdd_des, gen_force=None, mode="force", damping: float = 0.0, out=None, task_force=None,
                qdd=None, flags: Optional[int] = None, root_state=None, dof_state=None, want_gen_force: bool = True,
                want_task_force: bool = True, want_qdd: bool = True):
        """(u [N,75], F [N,k], qdd [N,75]) that give the task the acceleration ``xdd_des`` [N,k]:
        ``mode`` "force" (u = J^T F) or "joint" (u = (0_6; tau) of minimum norm); ``damping`` >= 0 is added
        to the k x k system's diagonal. ``out``, ``task_force`` and ``qdd`` are filled when given and
        allocated otherwise; a ``want_*`` False leaves that output out of the launch (None in its place)."""
        import torch
        n, k = self.num_envs, self._rows("control")
        f32 = torch.float32
        if not (want_gen_force or want_task_force or want_qdd):
            raise TaskError("control: no output asked for")
        if isinstance(mode, str):
            if mode not in MODES:
                raise TaskError(f"control: unknown mode {mode!r} (one of {sorted(MODES)})")
            mode = MODES[mode]
        damping = float(damping)
        if not (damping >= 0.0 and math.isfinite(damping)):
            raise TaskError(f"control: damping {damping} is negative or not finite")
        p_x = check_tensor(xdd_des, f32, (n, k), self.device, "xdd_des")
        p_f = None if gen_force is None else check_tensor(gen_force, f32, (n, NG), self.device, "gen_force")
        p_u = p_tf = p_q = None
        if want_gen_force:
            out, p_u = self._out(out, (n, NG), "out")
        if want_task_force:
            task_force, p_tf = self._out(task_force, (n, k), "task_force")
        if want_qdd:
            qdd, p_q = self._out(qdd, (n, NG), "qdd")
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.ht_task_control(self.h, p_root, p_dof, p_x, p_f, int(mode), damping, p_u, p_tf, p_q,
                                        self._flags(flags), self.engine.stream))
        return (out if want_gen_force else None), (task_force if want_task_force else None), (qdd if want_qdd else None)
