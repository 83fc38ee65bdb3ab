"""ctypes shim over ``libhumanoid_engine.so`` (``include/humanoid_engine.h``).

This replaces ``gymtorch`` (``packages/gymtorch/gymtorch/gymtorch.cpp:33-158``, ``wrapper.py:11-56``)
and the Isaac Gym tensor API: engine-owned device buffers are exposed as zero-copy, non-owning
torch tensors (``__cuda_array_interface__``, DLPack fallback) and every compute call is enqueued on
torch's current stream. Errors raise :class:`EngineError` (gymtorch printed and returned an empty
tensor, ``gymtorch.cpp:40-51``). There is no CPU fallback: without the HIP library or a GPU the
constructor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi
from .build import LIBRARIES

LIB_PATH = LIBRARIES["engine"].path


class EngineError(RuntimeError):
    pass


_V, _I, _F, _I32, _I64, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_int32, C.c_int64, C.c_uint64
# every exported symbol with its prototype (_abi.bind_library)
HE_PROTOTYPES = {
    "he_last_error": (C.c_char_p, []), "he_version": [], "he_device_count": [_V],
    "he_hash_uniform": (_F, [_U64, _U64, C.c_uint32]),
    "he_create": [_V, _I, _V], "he_set_model": [_V, _V], "he_create_envs": [_V, _I, _V], "he_destroy": [_V],
    "he_get_buffer": [_V, _I, _V, _V, _V, _V], "he_set_dof_targets": [_V, _V, _V],
    "he_set_root_state_indexed": [_V, _V, _V, _I, _V], "he_set_dof_state_indexed": [_V, _V, _V, _I, _V],
    "he_set_dof_targets_indexed": [_V, _V, _V, _I, _V], "he_set_env_properties": [_V, _V, _V, _V],
    "he_simulate": [_V, _I, _V], "he_set_pd_params": [_V, _V, _V, _V, _I], "he_step_actions": [_V, _V, _I, _V],
    "he_refresh": [_V, _V],
    "he_load_motions": [_V, _I64, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V],
    "he_ingest_clips": [_V, _I, _V, _V, _V, _V, _I, _V, _V],
    "he_imitation_step": [_V, _V, _V, _V, _V, _V, _V, _V, _V],
    "he_motion_state": [_V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V],
    "he_reset_envs": [_V, _V, _V, _V, _I, _V, _V, _V, _V, _V],
    "he_env_step": [_V, _V, _V, _V, _I, _U64, _U64, _V, _V, _V, _V, _V, _V],
    "he_imitation_reset_step": [_V, _V, _V, _U64, _U64, _V, _V, _V, _V, _V, _V],
    "he_set_debug_stamps": [_V, _V], "he_set_eval": [_V, _V], "he_set_amp": [_V, _V], "he_set_fused_step": [_V, _I],
    "he_amp_observations": [_I, _V, _V, _V, _V, _V, _V, _V, _V, _V],
    **_abi.FORCE_PROTOTYPES, **_abi.ACTUATION_PROTOTYPES, **_abi.STATE_PROTOTYPES, **_abi.PROBE_PROTOTYPES,
    # include/humanoid_rollout.h
    "he_rollout_store": [_V, _V, _I, _I64, _V, _V, _I64, _I32, _V],
    "he_rollout_order": [_V, _I64, _V, _I, _V],
    "he_rollout_gather": [_V, _I, _V, _I64, _I32, _I32, _I32, _V],
    "he_gae": [_V, _V, _V, _I64, _F, _F, _V, _V],
    "he_gae_minibatch": [_V, _V, _V, _V, _V, _I64, _F, _F, _I32, _I32, _I32, _V, _V, _V],
    "he_episode_step": [_I32] + [_V] * 14,
}
HE_SYMBOLS = tuple(HE_PROTOTYPES)


# load (never build) the library and check a return code, raising EngineError. HE_ENGINE_LIB: diagnostics
# only (A/B timing of a variant build, tools/build_variant.py)
_LIBRARY = _abi.Library(LIB_PATH, HE_PROTOTYPES, "he", EngineError, env="HE_ENGINE_LIB")
load_library, _check = _LIBRARY.load, _LIBRARY.check


class _CudaArray:
    """Minimal ``__cuda_array_interface__`` holder for a non-owning device view."""

    def __init__(self, ptr, shape, typestr, owner):
        self._owner = owner  # keep the engine alive while the view exists
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": tuple(int(s) for s in shape),
                                         "typestr": typestr, "strides": None, "version": 3}


def wrap_device_pointer(ptr: int, shape, dtype, device_index: int, owner=None):
    """Zero-copy torch view of engine memory (gymtorch.wrap_tensor equivalent)."""
    import torch
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.int64: "<i8", torch.int16: "<i2", torch.uint8: "|u1"}[dtype]
    t = torch.as_tensor(_CudaArray(ptr, shape, typestr, owner), device=f"cuda:{device_index}")
    if t.data_ptr() != ptr:
        raise EngineError("zero-copy wrap produced a copy")
    return t


class Engine:
    """One engine instance = one simulation of ``num_envs`` humanoids on one GPU."""

    def __init__(self, model, num_envs: int, device: int = 0, sim_params: Optional[_abi.HeSimParams] = None,
                 start_xy: Optional[np.ndarray] = None):
        import torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible: the engine has no CPU path")
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self.params = sim_params if sim_params is not None else _abi.default_sim_params()
        self.he_model = model if isinstance(model, _abi.HeModel) else _abi.make_model(model)
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)  # make sure torch's context exists on this device
        h = C.c_void_p()
        _check(self.lib.he_create(C.byref(self.params), self.device_index, C.byref(h)))
        self.h = h
        _check(self.lib.he_set_model(self.h, C.byref(self.he_model)))
        xy = None
        if start_xy is not None:
            xy = np.ascontiguousarray(start_xy, np.float32).reshape(num_envs, 2)
        _check(self.lib.he_create_envs(self.h, int(num_envs), None if xy is None else xy.ctypes.data_as(C.c_void_p)))
        self.num_envs = int(num_envs)
        self._views = {}
        self.has_motions = False

    def __del__(self):
        _abi.destroy_handle(self, "he_destroy")

    @property
    def stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ buffers (acquire_*)
    def buffer(self, kind: int):
        import torch
        if kind in self._views:
            return self._views[kind]
        ptr = C.c_void_p()
        shape = (C.c_int64 * 8)()
        ndim = C.c_int()
        dtype = C.c_int()
        _check(self.lib.he_get_buffer(self.h, kind, C.byref(ptr), shape, C.byref(ndim), C.byref(dtype)))
        tdt = torch.float32 if dtype.value == _abi.DTYPE_F32 else torch.int32
        t = wrap_device_pointer(ptr.value, [shape[i] for i in range(ndim.value)], tdt, self.device_index, owner=self)
        self._views[kind] = t
        return t

    @property
    def root_states(self):
        return self.buffer(_abi.BUF_ROOT_STATE)

    @property
    def dof_state(self):
        return self.buffer(_abi.BUF_DOF_STATE)

    @property
    def rb_state(self):
        return self.buffer(_abi.BUF_RB_STATE)

    @property
    def contact_forces(self):
        return self.buffer(_abi.BUF_CONTACT_FORCE)

    @property
    def dof_force(self):
        return self.buffer(_abi.BUF_DOF_FORCE)

    @property
    def dof_targets(self):
        return self.buffer(_abi.BUF_DOF_TARGET)

    @property
    def num_contacts(self):
        """i32 [N]: contact slots (joint limits included) used by the last substep."""
        return self.buffer(_abi.BUF_NUM_CONTACTS)

    @property
    def dropped_contacts(self):
        """i32 [N]: contacts generated past the capacity in the last substep (the deepest kept)."""
        return self.buffer(_abi.BUF_DROPPED_CONTACTS)

    @property
    def contact_cache(self):
        """f32 [N, HE_CACHE_WORDS]: the solver's warm-start cache (signature, keys, impulses)."""
        return self.buffer(_abi.BUF_CONTACT_CACHE)

    @property
    def initial_root_states(self):
        """f32 [N,13]: _initial_humanoid_root_states (humanoid_phc.py:522-523), the root state the
        Default / Hybrid state init resets to; writable."""
        return self.buffer(_abi.BUF_INIT_ROOT_STATE)

    @property
    def physics_order(self):
        """i32 [N]: the physics launch's dispatch order (the env of each workgroup, expensive envs
        first; diagnostics, DESIGN §4.1 "Dispatch order"). A copy: the engine's own buffer is read
        by every physics launch and must not be written from outside."""
        return self.buffer(_abi.BUF_PHYS_ORDER).clone()

    @property
    def physics_cost(self):
        """i32 [N]: each env's wave cycles in the last physics launch (the order's input; a copy)."""
        return self.buffer(_abi.BUF_PHYS_COST).clone()

    # ------------------------------------------------------------------ state writes
    def _dev(self, t, dtype, what, shape=None):
        """The device pointer of a contiguous tensor of this dtype (and shape or element count) on the
        engine's device (_abi.check_tensor; gymtorch refused non-contiguous tensors, wrapper.py:47-49)."""
        return _LIBRARY.check_tensor(t, dtype, shape, self.device, what)

    def set_dof_targets(self, t):
        import torch
        _check(self.lib.he_set_dof_targets(self.h, self._dev(t, torch.float32, "dof targets", self.num_envs * _abi.ND),
                                           self.stream))

    def _indexed(self, fn, src, ids, row):
        import torch
        p_src = self._dev(src, torch.float32, "indexed write's full-size source", self.num_envs * row)
        p_ids = self._dev(ids, torch.int32, "indexed write's ids")
        _check(fn(self.h, p_src, p_ids, int(ids.numel()), self.stream))

    def set_root_state_indexed(self, src, ids):
        self._indexed(self.lib.he_set_root_state_indexed, src, ids, 13)

    def set_dof_state_indexed(self, src, ids):
        self._indexed(self.lib.he_set_dof_state_indexed, src, ids, 2 * _abi.ND)

    def set_dof_targets_indexed(self, src, ids):
        self._indexed(self.lib.he_set_dof_targets_indexed, src, ids, _abi.ND)

    def set_env_properties(self, mass_scale=None, friction=None, terrain_kind=None):
        import torch
        self._env_props = (mass_scale, friction, terrain_kind)  # keep alive
        vp = lambda t, dt, what: None if t is None else self._dev(t, dt, what)  # noqa: E731
        _check(self.lib.he_set_env_properties(self.h, vp(mass_scale, torch.float32, "mass_scale"),
                                              vp(friction, torch.float32, "friction"),
                                              vp(terrain_kind, torch.int32, "terrain_kind")))

    # ------------------------------------------------------------------ stepping
    def simulate(self, num_simulate: int = 2):
        """gym.simulate() x num_simulate (control_freq_inv), each he_sim_params.substeps physics steps."""
        _check(self.lib.he_simulate(self.h, int(num_simulate), self.stream))

    def set_pd_params(self, offset, scale, frozen_mask=None, clip_actions=True):
        off = np.ascontiguousarray(offset, np.float32)
        sc = np.ascontiguousarray(scale, np.float32)
        fz = None if frozen_mask is None else np.ascontiguousarray(frozen_mask, np.int32)
        _check(self.lib.he_set_pd_params(self.h, off.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                         None if fz is None else fz.ctypes.data_as(C.c_void_p), int(bool(clip_actions))))

    def step_actions(self, actions, num_simulate: int = 2):
        import torch
        _check(self.lib.he_step_actions(self.h, self._dev(actions, torch.float32, "actions"), int(num_simulate),
                                        self.stream))

    # ------------------------------------------------------------------ external wrenches
    def _body_rows(self, t, what):
        import torch
        if t is None:
            return None
        p = self._dev(t, torch.float32, what)
        if tuple(t.shape) not in ((self.num_envs, _abi.NB, 3), (self.num_envs * _abi.NB, 3)):
            raise EngineError(f"{what} must be [num_envs,24,3] or [num_envs*24,3], got {tuple(t.shape)}")
        return p

    def apply_body_forces(self, force=None, torque=None, space: int = _abi.SPACE_ENV, hold: int = 1):
        """gym.apply_rigid_body_force_tensors: forces (at the bodies' centres of mass) and torques,
        [N,24,3] or [N*24,3] in `space` (_abi.SPACE_*), acting during the next `hold` simulate() calls.
        Calls before the next physics launch accumulate; both None clears (clear_body_forces)."""
        _check(self.lib.he_apply_body_forces(self.h, self._body_rows(force, "force"), self._body_rows(torque, "torque"),
                                             int(space), int(hold), self.stream))

    def apply_body_forces_at_pos(self, force, pos, space: int = _abi.SPACE_ENV, hold: int = 1):
        """gym.apply_rigid_body_force_at_pos_tensors: forces applied at the points `pos` (adds
        (pos - com) x force to the torque, the body's CoM at the time of the call)."""
        _check(self.lib.he_apply_body_forces_at_pos(self.h, self._body_rows(force, "force"), self._body_rows(pos, "pos"),
                                                    int(space), int(hold), self.stream))

    def clear_body_forces(self):
        """Drop the pending wrench: the next launch runs without one."""
        _check(self.lib.he_apply_body_forces(self.h, None, None, _abi.SPACE_ENV, 1, self.stream))

    # ------------------------------------------------------------------ torque control
    def set_dof_drive_modes(self, modes):
        """he_set_dof_drive_modes: one gymapi.DOF_MODE_* per dof ([69]; all envs share the articulation):
        NONE 0, POS 1, EFFORT 3 (VEL 2 is refused). A dof that is not POS loses its PD drive; an EFFORT
        dof takes the actuation forces. Clears any actuation that is set."""
        m = np.ascontiguousarray(np.asarray(modes).reshape(-1), np.int32)
        if m.shape != (_abi.ND,):
            raise EngineError(f"dof drive modes: expected {_abi.ND} modes, got {m.shape[0]}")
        _check(self.lib.he_set_dof_drive_modes(self.h, m.ctypes.data_as(C.c_void_p)))

    def _actuation(self, t, what):
        import torch
        p = self._dev(t, torch.float32, what, self.num_envs * _abi.ND)
        if tuple(t.shape) not in ((self.num_envs, _abi.ND), (self.num_envs * _abi.ND,)):
            raise EngineError(f"{what} must be [num_envs,69] or [num_envs*69], got {tuple(t.shape)}")
        return p

    def set_dof_actuation_forces(self, t):
        """gym.set_dof_actuation_force_tensor: joint torques [N,69] or [N*69] (N m, the engine's
        child-frame joint coordinates). Applied on EFFORT dofs, clamped to the model's effort limits, in
        every physics step until replaced or cleared (include/humanoid_engine.h)."""
        _check(self.lib.he_set_dof_actuation_forces(self.h, self._actuation(t, "dof actuation forces"), self.stream))

    def set_dof_actuation_forces_indexed(self, src, ids):
        """Rows ``ids`` (int32 env ids) of the full-size ``src`` replace the actuation of those envs."""
        import torch
        p_src = self._actuation(src, "indexed actuation's full-size source")
        p_ids = self._dev(ids, torch.int32, "indexed actuation's ids")
        _check(self.lib.he_set_dof_actuation_forces_indexed(self.h, p_src, p_ids, int(ids.numel()), self.stream))

    def clear_dof_actuation_forces(self):
        """Drop the actuation: the next launch runs the kernels without it."""
        _check(self.lib.he_set_dof_actuation_forces(self.h, None, self.stream))

    # ------------------------------------------------------------------ env state: save, restore, clone
    @property
    def state_layout(self):
        """he_state_layout_get, cached: ``(words, {name: (offset, words, dtype)})`` of an env's packed state
        (include/humanoid_engine.h "env state"): the public buffers by their short names, then ``wrench``
        and ``dof_act``, offsets and sizes in 4-byte words, dtype an ``_abi.DTYPE_*``."""
        if getattr(self, "_state_layout", None) is None:
            layout = _abi.HeStateLayout()
            _check(self.lib.he_state_layout_get(self.h, C.byref(layout)))
            self._state_layout = _abi.state_fields(layout)
        return self._state_layout

    def _env_ids(self, ids, what):
        """(pointer, count) of int32 env ids [k], k <= num_envs; None: every env in order."""
        import torch
        if ids is None:
            return None, self.num_envs
        p = self._dev(ids, torch.int32, what)
        if ids.dim() != 1 or ids.numel() > self.num_envs:
            raise EngineError(f"{what}: expected int32 [k] with k <= {self.num_envs}, got {tuple(ids.shape)}")
        return p, int(ids.numel())

    def save_envs(self, ids=None, out=None):
        """he_save_envs: the packed states int32 [k, W] of envs ``ids`` (int32 [k] on the device; None: all
        envs in order), row i that of ``ids[i]``, into ``out`` or a fresh tensor. One launch, no sync."""
        import torch
        p_ids, k = self._env_ids(ids, "save_envs ids")
        words = self.state_layout[0]
        if out is None:
            out = torch.empty((k, words), dtype=torch.int32, device=self.device)
        p_out = self._dev(out, torch.int32, "save_envs out", (k, words))
        _check(self.lib.he_save_envs(self.h, p_ids, k, p_out, self.stream))
        return out

    def load_envs(self, state, ids=None):
        """he_load_envs: rows of a packed ``state`` int32 [k, W] into envs ``ids`` (None: all, in order)."""
        import torch
        p_ids, k = self._env_ids(ids, "load_envs ids")
        p_state = self._dev(state, torch.int32, "load_envs state", (k, self.state_layout[0]))
        _check(self.lib.he_load_envs(self.h, p_ids, k, p_state, self.stream))

    def clone_envs(self, src_ids, dst_ids):
        """he_clone_envs: env ``src_ids[i]`` copied to env ``dst_ids[i]`` (int32 [k] each). A dst that is also
        a src of the same call is undefined; ``src == dst`` entries are no-ops."""
        if src_ids is None or dst_ids is None:
            raise EngineError("clone_envs: src_ids and dst_ids are both required")
        p_src, k = self._env_ids(src_ids, "clone_envs src_ids")
        p_dst, k_dst = self._env_ids(dst_ids, "clone_envs dst_ids")
        if k != k_dst:
            raise EngineError(f"clone_envs: {k} sources for {k_dst} destinations")
        _check(self.lib.he_clone_envs(self.h, p_src, p_dst, k, self.stream))

    def state_field(self, state, name):
        """A typed view of field ``name`` of packed states int32 [k, W]: [k, words] float32 or int32,
        sharing the tensor's memory (``state_field(s, "root")`` is the saved batch's root states [k, 13])."""
        import torch
        words, fields = self.state_layout
        if name not in fields:
            raise EngineError(f"state_field: no field {name!r}; the state has {', '.join(fields)}")
        if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.dim() != 2 \
                or state.shape[1] != words:
            raise EngineError(f"state_field: expected int32 [k, {words}] packed states")
        off, n, dtype = fields[name]
        v = state[:, off:off + n]
        return v.view(torch.float32) if dtype == _abi.DTYPE_F32 else v

    def sim_state(self) -> _abi.HeSimState:
        """he_get_sim_state: the sim-global scalars behind the per-env rows (pending wrench's hold, whether
        an actuation is set, physics launches so far)."""
        s = _abi.HeSimState()
        _check(self.lib.he_get_sim_state(self.h, C.byref(s)))
        return s

    def set_sim_state(self, s):
        """he_set_sim_state from an ``_abi.HeSimState`` or a dict of its fields (``sim_state_dict``)."""
        if not isinstance(s, _abi.HeSimState):
            s = _abi.HeSimState(**{k: int(v) for k, v in dict(s).items()})
        _check(self.lib.he_set_sim_state(self.h, C.byref(s)))

    def sim_state_dict(self) -> dict:
        """``sim_state()`` as plain ints, for a checkpoint."""
        s = self.sim_state()
        return {name: int(getattr(s, name)) for name, _ in _abi.HeSimState._fields_}

    # ------------------------------------------------------------------ motion library
    def load_motions(self, tables):
        t = tables
        arrs = [np.ascontiguousarray(x, np.float32) for x in (t.gts, t.grs, t.lrs, t.gvs, t.gavs, t.dvs)]
        starts = np.ascontiguousarray(t.length_starts, np.int64)
        nf = np.ascontiguousarray(t.num_frames, np.int64)
        lens = np.ascontiguousarray(t.lengths, np.float32)
        dts = np.ascontiguousarray(t.dt, np.float32)
        F = arrs[0].shape[0]
        _check(self.lib.he_load_motions(self.h, int(F), int(nf.shape[0]), *[a.ctypes.data_as(C.c_void_p) for a in arrs],
                                        starts.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p),
                                        lens.ctypes.data_as(C.c_void_p), dts.ctypes.data_as(C.c_void_p)))
        self.has_motions = True

    def ingest_clips(self, clips, motion_clip=None):
        """Device-side motion ingestion (he_ingest_clips): ``clips`` are dicts with the .pkl
        schema's ``pose_quat_global`` [T,24,4] and ``root_trans_offset`` [T,3] (+ ``fps``);
        library motion i uses clip ``motion_clip[i]`` (default: one motion per clip)."""
        import torch
        nf = np.array([len(c["pose_quat_global"]) for c in clips], np.int64)
        # float64: dt and length are 1 / fps in Python floats, rounded to float32 afterwards (the reference)
        fps = np.array([float(c.get("fps", 30)) for c in clips], np.float64)
        for i, c in enumerate(clips):  # per clip: two mismatches can cancel in the concatenation
            if len(c["root_trans_offset"]) != nf[i]:
                raise EngineError(f"clip {i} has {nf[i]} pose frames and {len(c['root_trans_offset'])} translations")
        pose = torch.as_tensor(np.concatenate([np.asarray(c["pose_quat_global"], np.float32) for c in clips], 0))
        trans = torch.as_tensor(np.concatenate([np.asarray(c["root_trans_offset"], np.float32).reshape(-1, 3)
                                                for c in clips], 0))
        pose = pose.to(self.device).contiguous()
        trans = trans.to(self.device).contiguous()
        if pose.shape[1:] != (24, 4) or trans.shape[0] != pose.shape[0]:
            raise EngineError(f"clip arrays have shapes {tuple(pose.shape)} / {tuple(trans.shape)}")
        mc = None
        m = len(clips)
        if motion_clip is not None:
            mc = np.ascontiguousarray(motion_clip, np.int32)
            m = int(mc.shape[0])
        _check(self.lib.he_ingest_clips(self.h, len(clips), nf.ctypes.data_as(C.c_void_p), fps.ctypes.data_as(C.c_void_p),
                                        C.c_void_p(pose.data_ptr()), C.c_void_p(trans.data_ptr()), m,
                                        None if mc is None else mc.ctypes.data_as(C.c_void_p), self.stream))
        self.has_motions = True

    def motion_state(self, ids, times, offset=None, want_dof=True):
        import torch
        k = int(ids.numel())
        p_ids = self._dev(ids, torch.int64, "motion ids")
        p_times = self._dev(times, torch.float32, "motion times")
        p_offset = None if offset is None else self._dev(offset, torch.float32, "offset")
        dev = self.device
        out = dict(rg_pos=torch.empty(k, 24, 3, device=dev), rb_rot=torch.empty(k, 24, 4, device=dev),
                   body_vel=torch.empty(k, 24, 3, device=dev), body_ang_vel=torch.empty(k, 24, 3, device=dev))
        if want_dof:
            out["dof_pos"] = torch.empty(k, 69, device=dev)
            out["dof_vel"] = torch.empty(k, 69, device=dev)
        vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        _check(self.lib.he_motion_state(self.h, k, p_ids, p_times, p_offset, vp(out["rg_pos"]), vp(out["rb_rot"]),
                                        vp(out["body_vel"]), vp(out["body_ang_vel"]), vp(out.get("dof_pos")),
                                        vp(out.get("dof_vel")), self.stream))
        return out

    def env_motion(self, motion_ids, start_times, start_offsets, global_offset, progress) -> _abi.HeEnvMotion:
        """Per-env motion bookkeeping block; the returned struct keeps the tensors alive."""
        import torch
        n = self.num_envs
        checks = (("motion_ids", motion_ids, torch.int64, (n,)), ("start_times", start_times, torch.float32, (n,)),
                  ("start_offsets", start_offsets, torch.float32, (n,)),
                  ("global_offset", global_offset, torch.float32, (n, 3)), ("progress", progress, torch.int16, (n,)))
        em = _abi.HeEnvMotion(*[self._dev(t, dt, f"env motion buffer {what}", shape).value
                                for what, t, dt, shape in checks])
        em.keep_alive = (motion_ids, start_times, start_offsets, global_offset, progress)
        return em

    def imitation_step(self, params: _abi.HeImitationParams, em: _abi.HeEnvMotion, obs, rew, reward_raw, reset,
                       terminate):
        _check(self.lib.he_imitation_step(self.h, C.byref(params), C.byref(em), C.c_void_p(obs.data_ptr()),
                                          C.c_void_p(rew.data_ptr()), C.c_void_p(reward_raw.data_ptr()),
                                          C.c_void_p(reset.data_ptr()), C.c_void_p(terminate.data_ptr()), self.stream))

    def reset_envs(self, params, em, env_ids, phases, obs, reset, terminate):
        import torch
        p_ids = self._dev(env_ids, torch.int32, "env_ids")
        p_phases = self._dev(phases, torch.float32, "phases")
        _check(self.lib.he_reset_envs(self.h, C.byref(params), C.byref(em), p_ids,
                                      int(env_ids.numel()), p_phases, C.c_void_p(obs.data_ptr()),
                                      C.c_void_p(reset.data_ptr()), C.c_void_p(terminate.data_ptr()), self.stream))

    def env_step(self, params, em, actions, obs, rew, reward_raw, reset, terminate, seed: int, step_index: int,
                 num_simulate: int = 2):
        import torch
        a = self._dev(actions, torch.float32, "actions")
        _check(self.lib.he_env_step(self.h, C.byref(params), C.byref(em), a, int(num_simulate),
                                    C.c_uint64(seed), C.c_uint64(step_index), C.c_void_p(obs.data_ptr()),
                                    C.c_void_p(rew.data_ptr()), C.c_void_p(reward_raw.data_ptr()),
                                    C.c_void_p(reset.data_ptr()), C.c_void_p(terminate.data_ptr()), self.stream))

    def set_fused_step(self, enable):
        """he_set_fused_step: env_step as one launch (True / 1), as step_actions + imitation_reset_step
        (False / 0), or None / -1 = auto (the engine default: one launch up to 2048 envs)."""
        mode = -1 if enable is None or (not isinstance(enable, bool) and int(enable) < 0) else int(bool(enable))
        _check(self.lib.he_set_fused_step(self.h, mode))

    def imitation_reset_step(self, params, em, obs, rew, reward_raw, reset, terminate, seed: int, step_index: int):
        _check(self.lib.he_imitation_reset_step(self.h, C.byref(params), C.byref(em), C.c_uint64(seed),
                                                C.c_uint64(step_index), C.c_void_p(obs.data_ptr()),
                                                C.c_void_p(rew.data_ptr()), C.c_void_p(reward_raw.data_ptr()),
                                                C.c_void_p(reset.data_ptr()), C.c_void_p(terminate.data_ptr()),
                                                self.stream))

    def set_eval(self, buffers: Optional[_abi.HeEvalBuffers]):
        """Attach eval recording (he_set_eval; the struct is copied, call again per frame) or detach."""
        _check(self.lib.he_set_eval(self.h, None if buffers is None else C.byref(buffers)))

    def set_amp(self, amp_obs, amp_obs_demo=None):
        """Attach the AMP buffers (he_set_amp): ``amp_obs`` / ``amp_obs_demo`` f32 [N, S, 196]
        device tensors (humanoid_phc.py:600-611), updated by every following imitation launch;
        ``None`` detaches."""
        import torch
        if amp_obs is None:
            self._amp = None
            _check(self.lib.he_set_amp(self.h, None))
            return
        for t in (amp_obs, amp_obs_demo):
            if t is None:
                continue
            self._dev(t, torch.float32, "AMP buffer")
            if t.dim() != 3 or t.shape[0] != self.num_envs or t.shape[2] != _abi.AMP_OBS_STEP:
                raise EngineError(f"AMP buffer has shape {tuple(t.shape)}, expected [{self.num_envs}, S, 196]")
        if amp_obs_demo is not None and amp_obs_demo.shape != amp_obs.shape:
            raise EngineError("amp_obs_demo must have the shape of amp_obs")
        b = _abi.HeAmpBuffers(amp_obs.data_ptr(), None if amp_obs_demo is None else amp_obs_demo.data_ptr(),
                              int(amp_obs.shape[1]), 0)
        self._amp = (amp_obs, amp_obs_demo)  # keep alive while attached
        _check(self.lib.he_set_amp(self.h, C.byref(b)))

    def set_debug_stamps(self, buf=None):
        """Diagnostics: int64 [num_envs, 32] (HE_STAMP_SLOTS) device tensor receiving per-phase cycles, or None."""
        import torch
        if buf is not None:
            self._dev(buf, torch.int64, "debug stamps")
        self._stamps = buf
        _check(self.lib.he_set_debug_stamps(self.h, None if buf is None else C.c_void_p(buf.data_ptr())))

    def hash_uniform(self, seed, step, env):
        return self.lib.he_hash_uniform(seed, step, env)


def amp_observations(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos):
    """build_amp_observations_smpl (envs/common.py:191-267) with the reference's constant flags on
    device tensors (he_amp_observations): key_body_pos [K,4,3] in KEY_BODIES order -> [K,196]."""
    import torch
    lib = load_library()
    k = int(root_pos.shape[0])
    ins = (root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos)
    shapes = ((k, 3), (k, 4), (k, 3), (k, 3), (k, 69), (k, 69), (k, 4, 3))
    dev = root_pos.device
    ptrs = [_LIBRARY.check_tensor(t, torch.float32, sh, dev, "he_amp_observations")
            for t, sh in zip(ins, shapes)]
    out = torch.empty(k, _abi.AMP_OBS_STEP, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _check(lib.he_amp_observations(k, *ptrs, C.c_void_p(out.data_ptr()), stream))
    return out
