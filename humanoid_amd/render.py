"""Headless camera sensors: ctypes shim over ``libhumanoid_render.so`` (``include/humanoid_render.h``).

One HIP ray-casting kernel draws the engine's analytic scene (24 sphere / capsule / box geoms per
env, marker spheres, the env's terrain: plane, slope or steps) straight from the engine's rigid-body
state buffer; the library only reads the engine's memory. :class:`Renderer` owns the output images and
launches on the engine's current stream. The same scene answers a ray-cast sensor (``set_rays`` /
``cast_rays``: height scans, range fans), one launch for all envs. There is no CPU path and no window: without the library or a GPU
the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import Sequence

import numpy as np

from . import _abi
from .build import LIBRARIES

LIB_PATH = LIBRARIES["render"].path

# include/humanoid_render.h
FLAG_SHADOWS, FLAG_CHECKER, FLAG_NO_CULL = 1, 2, 4
FLAGS_DEFAULT = FLAG_SHADOWS | FLAG_CHECKER
SEG_MARKER = 1000
MAX_MARKERS = 24
FOLLOW_POSITION, FOLLOW_TRANSFORM, FOLLOW_POSITION_XY = 0, 1, 2
BODY_RGB = (0.80, 0.68, 0.52)
MAX_STEP_CELLS = 512
MAX_RAYS = 1024
RAY_FRAME_POSITION, RAY_FRAME_HEADING, RAY_FRAME_TRANSFORM = 0, 1, 2
RAY_FRAMES = {"position": RAY_FRAME_POSITION, "heading": RAY_FRAME_HEADING, "transform": RAY_FRAME_TRANSFORM}
RAYS_SKIP_BODIES = 1
HIT_NOTHING, HIT_TERRAIN = -2, -1

_V, _I = C.c_void_p, C.c_int
# every exported symbol with its prototype (_abi.bind_library)
HR_PROTOTYPES = {
    "hr_last_error": (C.c_char_p, []), "hr_version": [], "hr_create": [_I, _V, _I, _V], "hr_destroy": [_V],
    "hr_validate_cameras": [_V, _I, _I], "hr_set_cameras": [_V, _V, _I], "hr_set_appearance": [_V, _V, _V],
    "hr_set_markers": [_V, _V, _I, _V, C.c_float], "hr_render": [_V, _V, _V, _V, _V, C.c_uint32, _V],
    "hr_set_terrain": [_V, _V, C.c_float, C.c_float, C.c_float], "hr_set_rays": [_V, _V, _I, _I, _I],
    "hr_cast_rays": [_V, _V, C.c_float, _V, _V, C.c_uint32, _V],
}
HR_SYMBOLS = tuple(HR_PROTOTYPES)


class RenderError(RuntimeError):
    pass


class HrCamera(C.Structure):
    """include/humanoid_render.h hr_camera."""
    _fields_ = [("env", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("hfov_deg", C.c_float),
                ("near", C.c_float), ("far", C.c_float), ("follow_body", C.c_int32), ("follow_mode", C.c_int32),
                ("pos", C.c_float * 3), ("target", C.c_float * 3)]


class HrRay(C.Structure):
    """include/humanoid_render.h hr_ray."""
    _fields_ = [("origin", C.c_float * 3), ("dir", C.c_float * 3)]


def height_scan_rays(nx: int, ny: int, spacing: float, height: float, offset=(0.0, 0.0)) -> np.ndarray:
    """[nx*ny, 6] (origin, direction) of a grid of straight-down rays, ``spacing`` apart and centred on
    ``offset`` in x and y, starting ``height`` above the body origin: with ``cast_rays`` the ground's height
    under ray i is (body z + height) - dist[i]."""
    x = (np.arange(int(nx)) - (int(nx) - 1) / 2) * float(spacing) + float(offset[0])
    y = (np.arange(int(ny)) - (int(ny) - 1) / 2) * float(spacing) + float(offset[1])
    rays = np.zeros((len(x), len(y), 6))
    rays[..., 0], rays[..., 1], rays[..., 2] = x[:, None], y[None, :], float(height)
    rays[..., 5] = -1.0
    return rays.reshape(-1, 6)


def camera(env: int, width: int, height: int, pos, target, hfov_deg: float = 90.0, near: float = 0.001,
           far: float = 2.0e6, follow_body: int = -1, follow_mode: int = FOLLOW_POSITION) -> HrCamera:
    """One camera sensor. Fixed (``follow_body`` -1): ``pos`` / ``target`` are world points; following:
    offsets from the body origin, rotated by the body's rotation in ``FOLLOW_TRANSFORM`` mode; in
    ``FOLLOW_POSITION_XY`` mode only x and y follow and the heights are absolute."""
    c = HrCamera(int(env), int(width), int(height), float(hfov_deg), float(near), float(far), int(follow_body),
                 int(follow_mode))
    c.pos[:] = [float(x) for x in pos]
    c.target[:] = [float(x) for x in target]
    return c


# load (never build) the library and check a return code, raising RenderError
_LIBRARY = _abi.Library(LIB_PATH, HR_PROTOTYPES, "hr", RenderError)
load_library, _check = _LIBRARY.load, _LIBRARY.check


def validate_cameras(cams: Sequence[HrCamera], num_envs: int):
    """The host-side check of a camera set (hr_validate_cameras); raises :class:`RenderError`."""
    lib = load_library()
    arr = (HrCamera * max(len(cams), 1))(*cams)
    _check(lib.hr_validate_cameras(arr, len(cams), int(num_envs)))


class Renderer:
    """The camera sensors of one :class:`humanoid_amd.engine.Engine`.

    ``set_cameras`` (re)allocates the images: ``color`` u8 [K,H,W,4] RGBA, ``depth`` f32 [K,H,W]
    (negative view-space distance, -inf where nothing is hit), ``seg`` i32 [K,H,W]; ``render`` fills
    them from the engine's current rigid-body state, on the engine's current stream."""

    def __init__(self, engine):
        import torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RenderError("no HIP device visible: the renderer has no CPU path")
        self.engine = engine
        self.device = engine.device
        self.num_envs = engine.num_envs
        h = C.c_void_p()
        _check(self.lib.hr_create(engine.device_index, C.byref(engine.he_model), self.num_envs, C.byref(h)))
        self.h = h
        self.num_cameras = 0
        self.width = self.height = 0
        self.color = self.depth = self.seg = None
        self._appearance = (None, None)
        self._markers = None
        self._terrain = None
        self.num_rays = 0
        self.ray_dist = self.ray_hit = None

    def __del__(self):
        _abi.destroy_handle(self, "hr_destroy")

    def _dev(self, t, dtype, shape, what, at_least=None):
        return _LIBRARY.check_tensor(t, dtype, shape, self.device, what, at_least)

    def set_cameras(self, cams: Sequence[HrCamera]):
        """Replace the camera set (all of one size). A refused set raises and leaves the previous one."""
        import torch
        cams = list(cams)
        arr = (HrCamera * max(len(cams), 1))(*cams)
        _check(self.lib.hr_set_cameras(self.h, arr, len(cams)))
        k, w, h = len(cams), int(cams[0].width), int(cams[0].height)
        if (k, w, h) != (self.num_cameras, self.width, self.height):
            self.color = torch.zeros(k, h, w, 4, dtype=torch.uint8, device=self.device)
            self.depth = torch.zeros(k, h, w, dtype=torch.float32, device=self.device)
            self.seg = torch.zeros(k, h, w, dtype=torch.int32, device=self.device)
            self.num_cameras, self.width, self.height = k, w, h

    def set_appearance(self, body_rgb=None, body_seg=None):
        """Per-body colours f32 [N,24,3] and segmentation ids i32 [N,24] (device tensors, read at render
        time, so later in-place writes show); ``None``: the default colour / id 0."""
        import torch
        n = self.num_envs
        p_rgb = None if body_rgb is None else self._dev(body_rgb, torch.float32, (n, _abi.NB, 3), "body_rgb")
        p_seg = None if body_seg is None else self._dev(body_seg, torch.int32, (n, _abi.NB), "body_seg")
        _check(self.lib.hr_set_appearance(self.h, p_rgb, p_seg))
        self._appearance = (body_rgb, body_seg)  # keep alive while attached

    def set_markers(self, pos=None, rgb=None, radius: float = 0.05):
        """Marker spheres: ``pos`` f32 [N,m,3] world points (device tensor, read at render time), ``rgb``
        [m,3] host values; ``pos=None`` removes them. Markers cast no shadow and carry ``SEG_MARKER``."""
        import torch
        if pos is None:
            _check(self.lib.hr_set_markers(self.h, None, 0, None, 0.0))
            self._markers = None
            return
        if pos.dim() != 3:
            raise RenderError(f"marker positions must be [num_envs, m, 3], got {tuple(pos.shape)}")
        m = int(pos.shape[1])
        p = self._dev(pos, torch.float32, (self.num_envs, m, 3), "marker positions")
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(rgb, np.float32), (m, 3)))
        _check(self.lib.hr_set_markers(self.h, p, m, c.ctypes.data_as(C.c_void_p), float(radius)))
        self._markers = pos  # keep alive while attached

    def set_terrain(self, kind=None, slope: float = 0.0, step_height: float = 0.0, step_length: float = 1.0):
        """The ground of each env: ``kind`` i32 [N] (device tensor, read at render time: 1 the slope, 2 the
        steps, anything else the plane) or ``None`` for the plane everywhere; ``slope`` in radians, the steps'
        height and length in metres. A refused call raises and leaves the previous setting."""
        import torch
        p = None if kind is None else self._dev(kind, torch.int32, (self.num_envs,), "terrain kind")
        _check(self.lib.hr_set_terrain(self.h, p, float(slope), float(step_height), float(step_length)))
        self._terrain = kind  # keep alive while attached

    def set_terrain_from_engine(self):
        """The engine's own terrain: its sim params' slope and steps and the ``terrain_kind`` last given to
        ``Engine.set_env_properties`` (none given: the plane)."""
        par = self.engine.params
        kind = getattr(self.engine, "_env_props", (None, None, None))[2]
        self.set_terrain(kind, par.terrain_slope, par.step_height, par.step_length)

    def set_rays(self, rays, body="Pelvis", frame="heading"):
        """The ray-cast sensor's rays, [R,6] host values (origin 3, direction 3) in a frame attached to
        ``body`` (an index or a name) of every env; ``frame``: "position" (world axes), "heading" (rotated
        about z by the body's heading) or "transform" (the body's rotation). Directions are normalised in
        float64 before they are rounded. (Re)allocates ``ray_dist`` f32 [N,R] and ``ray_hit`` i32 [N,R]."""
        import torch
        a = np.array(rays, np.float64)
        if a.ndim != 2 or a.shape[1] != 6:
            raise RenderError(f"rays must be [R, 6] (origin, direction), got {a.shape}")
        with np.errstate(divide="ignore", invalid="ignore"):
            a[:, 3:] /= np.linalg.norm(a[:, 3:], axis=1, keepdims=True)
        if isinstance(body, str):
            from .body_sets import BODY_NAMES
            if body not in BODY_NAMES:
                raise RenderError(f"set_rays: no body named {body!r}")
            body = BODY_NAMES.index(body)
        if isinstance(frame, str):
            if frame not in RAY_FRAMES:
                raise RenderError(f"set_rays: unknown frame {frame!r} (one of {sorted(RAY_FRAMES)})")
            frame = RAY_FRAMES[frame]
        r = int(a.shape[0])
        arr = (HrRay * max(r, 1))()
        np.frombuffer(arr, np.float32)[:r * 6] = a.astype(np.float32).reshape(-1)
        _check(self.lib.hr_set_rays(self.h, arr, r, int(body), int(frame)))
        if r != self.num_rays:
            self.ray_dist = torch.zeros(self.num_envs, r, dtype=torch.float32, device=self.device)
            self.ray_hit = torch.zeros(self.num_envs, r, dtype=torch.int32, device=self.device)
            self.num_rays = r

    def cast_rays(self, max_range: float, skip_bodies: bool = True, dist=None, hit=None, rb_state=None):
        """hr_cast_rays: one launch for all envs, no host synchronisation. Returns (dist f32 [N,R]: t, +inf
        where nothing is hit within ``max_range``; hit i32 [N,R]: HIT_NOTHING, HIT_TERRAIN or the body
        index). With neither ``dist`` nor ``hit`` given the renderer's own ``ray_dist`` / ``ray_hit`` are
        filled; given one of them only that is written. ``skip_bodies``: the terrain only. Every tensor is
        checked to be on the device, contiguous, of its dtype and at least N*R long before a pointer is
        passed."""
        import torch
        if self.num_rays < 1:
            raise RenderError("cast_rays before set_rays")
        if dist is None and hit is None:
            dist, hit = self.ray_dist, self.ray_hit
        n = self.num_envs * self.num_rays
        p_dist = None if dist is None else self._dev(dist, torch.float32, None, "dist", n)
        p_hit = None if hit is None else self._dev(hit, torch.int32, None, "hit", n)
        p_rb = self._dev(self.engine.rb_state if rb_state is None else rb_state, torch.float32, None, "rb_state",
                         self.num_envs * _abi.NB * 13)
        _check(self.lib.hr_cast_rays(self.h, p_rb, float(max_range), p_dist, p_hit,
                                     RAYS_SKIP_BODIES if skip_bodies else 0, self.engine.stream))
        return dist, hit

    def render_into(self, color=None, depth=None, seg=None, flags: int = FLAGS_DEFAULT, rb_state=None):
        """hr_render into caller tensors (``None``: that output is not written). ``rb_state`` defaults to
        the engine's live buffer. The kernel writes K*H*W pixels into each output and reads every env's 24
        rigid-body rows: every tensor is checked to be on the device, contiguous, of its dtype (``color``
        uint8 x 4 per pixel, ``depth`` float32, ``seg`` int32) and at least that long before any pointer
        is passed; longer, or of another shape, is the caller's business."""
        import torch
        n = self.num_cameras * self.height * self.width
        p_color = None if color is None else self._dev(color, torch.uint8, None, "color", 4 * n)
        p_depth = None if depth is None else self._dev(depth, torch.float32, None, "depth", n)
        p_seg = None if seg is None else self._dev(seg, torch.int32, None, "seg", n)
        p_rb = self._dev(self.engine.rb_state if rb_state is None else rb_state, torch.float32, None, "rb_state",
                         self.num_envs * _abi.NB * 13)
        _check(self.lib.hr_render(self.h, p_rb, p_color, p_depth, p_seg, int(flags), self.engine.stream))

    def render(self, flags: int = FLAGS_DEFAULT):
        """Draw every camera into ``color`` / ``depth`` / ``seg`` (one launch, no host synchronisation)."""
        if self.color is None:
            raise RenderError("render before set_cameras")
        self.render_into(self.color, self.depth, self.seg, flags)
        return self.color


# ----------------------------------------------------------------------------------- files
def save_png(path, rgba):
    """Write an image [H,W,4] (or [H,W,3]) uint8 as a PNG (zlib + struct only)."""
    a = np.ascontiguousarray(np.asarray(rgba))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"save_png takes uint8 [H,W,3|4], got {a.dtype} {a.shape}")
    h, w, ch = a.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * ch)], axis=1).tobytes()  # filter 0 per row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, 6 if ch == 4 else 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_video(path, frames, fps: int = 30):
    """Write RGBA / RGB frames with ``imageio`` when it is installed (not a dependency of the engine)."""
    try:
        import imageio
    except ImportError as e:
        raise RenderError("write_video needs imageio; save_png writes single frames without it") from e
    with imageio.get_writer(path, fps=fps, macro_block_size=None) as w:
        for fr in frames:
            w.append_data(np.asarray(fr)[..., :3])
