"""Independent float64 motion ingestion: the checker for he_ingest_clips (csrc/he_ingest.hip) and for
its float32 host restatement (motion_lib.clip_to_motion).

Written from the definitions with rotation matrices (scipy Rotation), not from the kernel's
quaternion recipe; nothing here shares code with humanoid_amd.quat or motion_lib:

* positions by forward kinematics, ``p_child = p_parent + R_parent local_pos``, with the clip's own
  global rotations;
* local rotations ``R_parent^T R_child`` (the root's is its global one);
* linear velocity ``np.gradient(p) / dt``;
* raw angular velocity ``rotvec(R[f+1] R[f]^T) / dt``, zero on the clip's last frame;
* dof velocity ``rotvec(Rl[f]^T Rl[f+1]) / dt``, the last frame repeating the one before;
* linear and angular velocity through ``gaussian_filter1d(sigma=2, mode="nearest")`` within the clip;
* ``fps`` as given (a float): ``dt = 1 / fps``, ``length = 1 / fps * (frames - 1)``, both rounded to
  float32 only as the per-motion metadata the sampler reads.

``motion_state`` samples these float64 tables the way the engine's sampler is defined: which frame
pair and which blend weight is decided in float32 (``frame_select`` of csrc/he_imitation_env.h,
restated in NumPy float32), and so are the branches and the two weights of the reference's slerp
(the midpoint it returns for two rotations closer than ``sin(half angle) < 0.001``, the first
rotation it returns at ``cos >= 1``; see ``_slerp`` for why the weights): those are discontinuous
or ill-conditioned choices of the sampler, not of ingestion, and a float64 decision would compare
one side of a branch with the other. The tables, the blends and the exp map are float64.
"""
import numpy as np
from scipy.ndimage import gaussian_filter1d
from scipy.spatial.transform import Rotation

F32 = np.float32


def _rotvec(m):
    """Rotation matrices [...,3,3] -> rotation vectors [...,3] (angle in [0, pi])."""
    return Rotation.from_matrix(m.reshape(-1, 3, 3)).as_rotvec().reshape(m.shape[:-2] + (3,))


def ingest(model, clip):
    """One clip -> float64 per-frame tables. grs stays the input (the engine passes it through)."""
    q = np.asarray(clip["pose_quat_global"], np.float64)
    trans = np.asarray(clip["root_trans_offset"], np.float64).reshape(-1, 3)
    fps = float(clip.get("fps", 30))
    T, B = q.shape[:2]
    if T < 2:
        raise ValueError("a clip needs at least 2 frames")
    dt = 1.0 / fps
    parents = np.asarray(model.parents)
    local_pos = np.asarray(model.local_pos, np.float64)
    Rg = Rotation.from_quat(q.reshape(-1, 4)).as_matrix().reshape(T, B, 3, 3)
    Rl = np.empty_like(Rg)
    p = np.empty((T, B, 3))
    Rl[:, 0] = Rg[:, 0]
    p[:, 0] = trans
    for b in range(1, B):
        a = int(parents[b])
        assert 0 <= a < b
        p[:, b] = p[:, a] + Rg[:, a] @ local_pos[b]
        Rl[:, b] = np.swapaxes(Rg[:, a], -1, -2) @ Rg[:, b]
    gvs = gaussian_filter1d(np.gradient(p, axis=0) / dt, 2, axis=0, mode="nearest")
    raw = np.zeros((T, B, 3))
    raw[:-1] = _rotvec(Rg[1:] @ np.swapaxes(Rg[:-1], -1, -2)) / dt
    gavs = gaussian_filter1d(raw, 2, axis=0, mode="nearest")
    d = _rotvec(np.swapaxes(Rl[:-1], -1, -2) @ Rl[1:]) / dt
    dvs = np.concatenate([d, d[-1:]], axis=0)[:, 1:]
    lrs = Rotation.from_matrix(Rl.reshape(-1, 3, 3)).as_quat().reshape(T, B, 4)
    lrs = np.where(lrs[..., 3:] < 0, -lrs, lrs)
    return {"gts": p, "grs": q, "lrs": lrs, "gvs": gvs, "gavs": gavs, "dvs": dvs, "raw_gavs": raw,
            "fps": fps, "num_frames": T}


class Tables:
    """Concatenated float64 tables of a library + the per-motion float32 metadata."""

    def __init__(self, model, clips, motion_clip=None):
        ms = [ingest(model, c) for c in clips]
        nf = np.array([m["num_frames"] for m in ms], np.int64)
        starts = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int64)
        mc = np.arange(len(clips)) if motion_clip is None else np.asarray(motion_clip)
        for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs"):
            setattr(self, k, np.concatenate([m[k] for m in ms], axis=0))
        self.clips = ms
        self.motion_clip = mc
        self.num_frames = nf[mc]
        self.length_starts = starts[mc]
        self.fps = np.array([ms[c]["fps"] for c in mc], np.float64)
        self.lengths = np.array([1.0 / ms[c]["fps"] * (ms[c]["num_frames"] - 1) for c in mc], F32)
        self.dt = np.array([1.0 / ms[c]["fps"] for c in mc], F32)


def frame_select(tables, ids, times):
    """Frame pair and blend of each query, in float32 (csrc/he_imitation_env.h frame_select)."""
    ids = np.clip(np.asarray(ids, np.int64), 0, len(tables.num_frames) - 1)
    time = np.asarray(times, F32)
    length, dt, nf = tables.lengths[ids], tables.dt[ids], tables.num_frames[ids]
    phase = np.clip(time / length, F32(0), F32(1))
    time = np.maximum(time, F32(0))
    f0 = (phase * (nf - 1).astype(F32)).astype(np.int64)
    f1 = np.minimum(f0 + 1, nf - 1)
    blend = np.clip((time - f0.astype(F32) * dt) / dt, F32(0), F32(1))
    assert phase.dtype == F32 and blend.dtype == F32
    return tables.length_starts[ids] + f0, tables.length_starts[ids] + f1, blend


def _slerp(q0, q1, t):
    """Slerp of xyzw float64 quaternions [..., 4] at the float32 blend t [...]. The two weights and
    the branches (the nearer sign of q1, the midpoint for sin(half) < 0.001, q0 for cos >= 1) are the
    reference slerp's float32 ones (csrc/he_math.h slerp_ref), applied to the float64 quaternions:
    float32 rounds 1 - c*c to about 6e-8 / half^2 relative, so for rotations 0.02-0.04 rad apart the
    float32 slerp returns a quaternion whose NORM is off by 1e-4 to 1e-5 -- by the reference's
    design, far above the 2e-6 a rotation is compared at, and reproducible only from the same
    float32 cosine. The direction of the result and the exp map taken from it do not feel it."""
    a, b = q0.astype(F32), q1.astype(F32)
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = a[..., 0] * b[..., 0]
        for i in (1, 2, 3):
            c = c + a[..., i] * b[..., i]
        q1 = np.where((c < 0)[..., None], -q1, q1)
        c = np.abs(c)
        half = np.arccos(c)
        s = np.sqrt(F32(1) - c * c)
        ra, rb = np.sin((F32(1) - t) * half) / s, np.sin(t * half) / s
    assert ra.dtype == F32 and rb.dtype == F32
    o = ra.astype(np.float64)[..., None] * q0 + rb.astype(np.float64)[..., None] * q1
    o = np.where((np.abs(s) < F32(0.001))[..., None], 0.5 * q0 + 0.5 * q1, o)
    return np.where((c >= F32(1))[..., None], q0, o)


def motion_state(tables, ids, times, offset=None):
    """The six outputs of he_motion_state from the float64 tables."""
    g0, g1, blend = frame_select(tables, ids, times)
    bl = blend.astype(np.float64)[:, None, None]
    lerp = lambda x: (1.0 - bl) * x[g0] + bl * x[g1]  # noqa: E731
    pos = lerp(tables.gts)
    if offset is not None:
        pos = pos + np.asarray(offset, np.float64)[:, None, :]
    k = len(g0)
    rot = _slerp(tables.grs[g0], tables.grs[g1], bl[..., 0])
    lr = _slerp(tables.lrs[g0][:, 1:], tables.lrs[g1][:, 1:], bl[..., 0])
    dof_pos = Rotation.from_quat(lr.reshape(-1, 4)).as_rotvec().reshape(k, -1)
    return {"rg_pos": pos, "rb_rot": rot, "body_vel": lerp(tables.gvs), "body_ang_vel": lerp(tables.gavs),
            "dof_pos": dof_pos, "dof_vel": lerp(tables.dvs).reshape(k, -1)}
