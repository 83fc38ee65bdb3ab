"""Joint reaction wrenches: ctypes shim over the ``hw_`` entry points of ``libhumanoid_solve.so``
(``include/humanoid_wrench.h``).

One launch of the computed-torque kernel gives, for a motion (desired joint accelerations ``qdd_des``
``[N,69]``, a prescribed base acceleration ``base_acc`` ``[N,6]`` or a free base) and external wrenches on
the bodies (``body_force`` at the centres of mass and ``body_torque``, ``[N*24,3]`` each, world axes), the
wrench every joint transmits ``wrench`` ``[N,24,6]`` (force, then torque about the joint's own origin; row
0 is what something outside must exert on the root), the joint torques ``tau`` ``[N,69]``, the base
acceleration used ``[N,6]`` and the bodies' accelerations ``body_acc`` ``[N,24,6]`` (origin, then angular),
from the engine's root-state and dof-state buffers alone. :class:`Reaction` owns the four tensors and
launches on the engine's current stream. The columns are those of :mod:`humanoid_amd.dynamics`. There is no
CPU path: without the library or a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _abi
from .solve import LIB_PATH

from ._abi import FLAG_ARMATURE, FLAG_NO_GRAVITY, FLAGS_DEFAULT, NB, ND, NG  # noqa: F401  (include/humanoid_wrench.h)

OUTPUTS = ("wrench", "tau", "base_acc", "body_acc")  # hw_outputs' members, in order
WRENCH_ROWS = 6
FRAMES = {"world": 0, "body": 1}  # HW_FRAME_*


class HwOutputs(C.Structure):
    """hw_outputs: the four device pointers, in the header's order."""
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


_V, _I, _U = C.c_void_p, C.c_int, C.c_uint32
# every exported hw_ symbol with its prototype (_abi.bind_library)
HW_PROTOTYPES = {
    "hw_last_error": (C.c_char_p, []), "hw_version": [], "hw_validate_model": [_V], "hw_create": [_I, _V, _V, _I, _V],
    "hw_destroy": [_V], "hw_compute": [_V, _V, _V, _V, _V, _V, _V, _V, _I, _U, _V],
}
HW_SYMBOLS = tuple(HW_PROTOTYPES)


class ReactionError(RuntimeError):
    pass


# load (never build) the library, a return code, hw_validate_model and _abi.check_tensor, raising ReactionError
_LIBRARY = _abi.Library(LIB_PATH, HW_PROTOTYPES, "hw", ReactionError)
load_library, _check, validate_model, check_tensor = (_LIBRARY.load, _LIBRARY.check, _LIBRARY.validate_model,
                                                      _LIBRARY.check_tensor)


def output_shapes(num_envs: int):
    n = int(num_envs)
    return {"wrench": (n, NB, WRENCH_ROWS), "tau": (n, ND), "base_acc": (n, 6), "body_acc": (n, NB, WRENCH_ROWS)}


class Reaction(_abi.QueryBinding):
    """The joint reaction wrenches of one :class:`humanoid_amd.engine.Engine`.

    ``armature`` (default on) adds ``armature * qdd`` to ``tau``; ``gravity`` (default on) keeps gravity in
    the wrenches. Gravity is the engine's ``sim_params.gravity``. The output tensors are allocated on first
    use and refreshed in place after that (views stay valid); every launch goes on the engine's stream
    without synchronising the host."""

    LIBRARY, NO_CPU_PATH = _LIBRARY, "the reaction kernel has no CPU path"

    def compute(self, qdd_des=None, base_acc=None, body_force=None, body_torque=None, frame="world",
                wrench: bool = True, tau: bool = False, base_acc_out: bool = False, body_acc: bool = False, out=None,
                flags: Optional[int] = None, root_state=None, dof_state=None):
        """hw_compute: a dict of the tensors asked for, by ``OUTPUTS``' names.

        ``qdd_des`` [N,69] (None: zero); ``base_acc`` [N,6] prescribes the base acceleration, None leaves the
        base free (nothing acts on the root); ``body_force`` / ``body_torque`` [N*24,3] are forces at the
        bodies' centres of mass and torques in world axes (None: zero). ``frame`` "world" or "body" is the
        axes of ``wrench``. ``out`` may map an output's name to a caller tensor, which is then filled in
        place of this object's own. The states default to the engine's live buffers."""
        import torch
        n, f32 = self.num_envs, torch.float32
        if frame not in FRAMES:
            raise ReactionError(f"compute: unknown frame {frame!r} (one of {sorted(FRAMES)})")
        want = dict(wrench=wrench, tau=tau, base_acc=base_acc_out, body_acc=body_acc)
        given = dict(out or {})
        if set(given) - set(OUTPUTS):
            raise ReactionError(f"compute: out names {sorted(set(given) - set(OUTPUTS))} (outputs: {OUTPUTS})")
        if not (any(want.values()) or given):
            raise ReactionError("compute: no output asked for")

        def optional(t, shape, what):
            return None if t is None else check_tensor(t, f32, shape, self.device, what)

        p_q = optional(qdd_des, (n, ND), "qdd_des")
        p_a = optional(base_acc, (n, 6), "base_acc")
        p_f = optional(body_force, (n * NB, 3), "body_force")
        p_t = optional(body_torque, (n * NB, 3), "body_torque")
        shapes = output_shapes(n)
        o, result = HwOutputs(), {}
        for name in OUTPUTS:
            t = given.get(name)
            if t is None and want[name]:
                t = getattr(self, "_" + name, None)
                if t is None:  # this object's own storage, made once
                    t = torch.zeros(shapes[name], dtype=f32, device=self.device)
                    setattr(self, "_" + name, t)
            if t is not None:
                setattr(o, name, check_tensor(t, f32, shapes[name], self.device, name))
                result[name] = t
        p_root, p_dof = self._states(root_state, dof_state)
        _check(self.lib.hw_compute(self.h, p_root, p_dof, p_q, p_a, p_f, p_t, C.byref(o), FRAMES[frame],
                                   self._flags(flags), self.engine.stream))
        return result
