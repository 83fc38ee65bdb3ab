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
import os
from typing import Optional

from . import _abi

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhumanoid_task.so")
_lib = None

# include/humanoid_task.h
FLAG_ARMATURE, FLAG_NO_GRAVITY = 1, 2
FLAGS_DEFAULT = FLAG_ARMATURE
MODE_FORCE, MODE_JOINT = 0, 1
MODES = {"force": MODE_FORCE, "joint": MODE_JOINT}
MAX_ROWS = 32
NG = 75  # HE_NUM_GEN: 6 root + 69 dof generalised velocities


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


def load_library(path: Optional[str] = None):
    """Load (never build) the task library; it loads without a GPU."""
    global _lib
    if _lib is None:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise TaskError(f"{p} not found: build it with `python -m humanoid_amd.build` (hipcc, gfx950)")
        _lib = _abi.bind_library(p, HT_PROTOTYPES)
    return _lib


def _check(rc):
    if rc != 0:
        raise TaskError(_lib.ht_last_error().decode())


def validate_model(he_model: _abi.HeModel):
    """The host-side model check of ht_create (ht_validate_model); raises :class:`TaskError`."""
    lib = load_library()
    _check(lib.ht_validate_model(C.byref(he_model)))


def check_tensor(t, dtype, shape, device, what):
    """_abi.check_tensor raising :class:`TaskError`."""
    return _abi.check_tensor(t, dtype, shape, device, what, TaskError)


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


class TaskSpace:
    """Task-space control on one :class:`humanoid_amd.engine.Engine`.

    ``armature`` (default on: the inertia the engine's own solve uses) puts the model's dof armature on
    ``M``'s diagonal; ``gravity`` (default on) keeps gravity in ``c``. Gravity is the engine's
    ``sim_params.gravity``. The rows are shared by every env and set by :meth:`set_rows`. The states
    default to the engine's live buffers, every launch goes on the engine's stream without synchronising
    the host, and an output tensor is allocated when not given."""

    def __init__(self, engine, armature: bool = True):
        import torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise TaskError("no HIP device visible: the task kernel has no CPU path")
        self.engine = engine  # keeps the engine (and the buffers the kernel reads) alive
        self.device = engine.device
        self.num_envs = engine.num_envs
        self.armature = bool(armature)
        self.gravity = True
        self.num_rows = 0
        g = (C.c_float * 3)(*[float(x) for x in engine.params.gravity])
        h = C.c_void_p()
        _check(self.lib.ht_create(engine.device_index, C.byref(engine.he_model), g, self.num_envs, C.byref(h)))
        self.h = h

    def __del__(self):
        _abi.destroy_handle(self, "ht_destroy")

    @property
    def flags(self) -> int:
        return (FLAG_ARMATURE if self.armature else 0) | (0 if self.gravity else FLAG_NO_GRAVITY)

    def set_rows(self, rows):
        """The task rows, ``(body index or name, axis, point=(0, 0, 0))`` each, 1 to 32 of them; they
        replace the rows set before. A refused call leaves those in place."""
        arr, k = make_rows(rows)
        _check(self.lib.ht_set_rows(self.h, arr, k))
        self.num_rows = k
        return k

    def _states(self, root_state, dof_state):
        import torch
        n = self.num_envs
        root = self.engine.root_states if root_state is None else root_state
        dof = self.engine.dof_state if dof_state is None else dof_state
        return (check_tensor(root, torch.float32, (n, 13), self.device, "root_state"),
                check_tensor(dof, torch.float32, (n * _abi.ND, 2), self.device, "dof_state"))

    def _out(self, t, shape, what):
        """The pointer of a checked caller tensor, or of a fresh one: (tensor, pointer)."""
        import torch
        if t is None:
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
        return t, check_tensor(t, torch.float32, shape, self.device, what)

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
        _check(self.lib.ht_task_terms(self.h, p_root, p_dof, p_f, *ptrs, int(self.flags if flags is None else flags),
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
                                        int(self.flags if flags is None else flags), self.engine.stream))
        return (out if want_gen_force else None), (task_force if want_task_force else None), (qdd if want_qdd else None)
