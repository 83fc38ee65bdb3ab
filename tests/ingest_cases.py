"""Adversarial clip libraries for motion ingestion, and the bounds its tests hold the device to.

All seeded, under 1,000 frames in total. ``libraries(model)`` returns

* ``mixed``: clips of 2, 3, 8, 9, 16, 17, 37 and 150 frames (every Gaussian tap clamps for n <= 8;
  17 = 2 radius + 1), ordered so that the clip starts fall on every residue mod 8 (the kernels put
  8 frames into a block), with 24, 30, 60, 120 and 59.94 fps in one library and a total that is
  no multiple of 8; plus three copies of the 37-frame clip -- ``flip`` (each (frame, body)
  quaternion negated with probability 1/2: the same rotations), ``spin`` (a yaw of 2.5 rad per frame
  composed onto every body: large unaliased steps, where the angular velocity is well conditioned)
  -- and ``held`` (the middle 12 frames repeat one non-identity pose: zero raw velocities there);
* ``many``: 70 clips of 2-9 frames (the clip search and dense boundaries).
"""
import numpy as np
from scipy.spatial.transform import Rotation

SEED = 20241020
FPS = (24, 30, 60, 120, 59.94)
# (name, frames, fps) in library order; the starts 0, 2, 10, 47, 197, 200, 217, 246, 283, 292, 308
# are 0, 2, 2, 7, 5, 0, 1, 6, 3, 4, 4 mod 8; 345 frames in all
MIXED = (("n2", 2, 120), ("n8", 8, 24), ("n37", 37, 30), ("n150", 150, 59.94), ("n3", 3, 30), ("n17", 17, 59.94),
         ("held", 29, 24), ("flip", 37, 30), ("n9", 9, 60), ("n16", 16, 120), ("spin", 37, 30))
# 70 clips of 2-9 frames: every length nine times, less one 2 and one 3, shuffled: 391 frames, 7 mod 8
MANY_FRAMES = np.random.default_rng(SEED).permutation(np.tile(np.arange(2, 10), 9)[2:])
SPIN_STEP = 2.5
HELD = slice(8, 20)


def _clip(model, rng, frames, fps):
    from humanoid_amd import synthetic
    c = synthetic.make_clip(model, rng, num_frames=frames, fps=fps)
    c["fps"] = fps  # make_clip stores int(fps)
    return c


def _flipped(clip, rng):
    c = dict(clip)
    q = clip["pose_quat_global"].copy()
    q[rng.random(q.shape[:2]) < 0.5] *= -1
    c["pose_quat_global"] = q
    return c


def _spun(clip):
    c = dict(clip)
    q = np.asarray(clip["pose_quat_global"], np.float64)
    T, B = q.shape[:2]
    yaw = Rotation.from_rotvec(np.outer(SPIN_STEP * np.arange(T), [0.0, 0.0, 1.0]))
    out = np.stack([(yaw * Rotation.from_quat(q[:, b])).as_quat() for b in range(B)], axis=1)
    c["pose_quat_global"] = out.astype(np.float32)
    return c


def _held(clip):
    c = dict(clip)
    for k in ("pose_quat_global", "root_trans_offset"):
        x = clip[k].copy()
        x[HELD] = x[HELD.start]
        c[k] = x
    return c


def libraries(model):
    rng = np.random.default_rng(SEED)
    mixed = {}
    for name, frames, fps in MIXED:
        if name == "flip":
            mixed[name] = _flipped(mixed["n37"], rng)
        elif name == "spin":
            mixed[name] = _spun(mixed["n37"])
        elif name == "held":
            mixed[name] = _held(_clip(model, rng, frames, fps))
        else:
            mixed[name] = _clip(model, rng, frames, fps)
    many = [_clip(model, rng, int(n), FPS[i % len(FPS)]) for i, n in enumerate(MANY_FRAMES)]
    return {"mixed": list(mixed.values()), "many": many}


def mixed_index(name):
    return [m[0] for m in MIXED].index(name)


def starts(clips):
    nf = [len(c["pose_quat_global"]) for c in clips]
    return np.concatenate([[0], np.cumsum(nf)[:-1]]), int(np.sum(nf))


# ---------------------------------------------------------------- the reference project's fixture
# measured max |float64 reference - golden table| (tests/golden/motion_lib.npz, test_ingest_reference.py),
# and the bound: 3 times that
GOLDEN_MEASURED = {"gts": 5.7e-7, "gvs": 1.1e-5, "gavs": 3.4e-3, "dvs": 5.6e-5}
GOLDEN_BOUND = {k: 3.0 * v for k, v in GOLDEN_MEASURED.items()}


def golden_clips(g):
    """The reference project's raw clips stored in the motion_lib fixture."""
    return [dict(pose_quat_global=g[f"clip{i}_pose_quat_global"], root_trans_offset=g[f"clip{i}_root_trans_offset"],
                 fps=g[f"clip{i}_fps"].item()) for i in range(5)]


# ---------------------------------------------------------------- bounds
EPS = 2.0 ** -23
CHANNELS = ("gts", "gvs", "gavs", "dvs")  # positions, linear / angular / dof velocity
OUTPUT_OF = {"gts": "rg_pos", "gvs": "body_vel", "gavs": "body_ang_vel", "dvs": "dof_vel"}


def floors(ref):
    """Float32 rounding of one clip's channels (``ref``: ingest_reference.ingest of it): positions
    4 ulp of max(1, max |position|); a velocity is a position or rotation difference over dt, so the
    same value times fps."""
    pos = 4.0 * EPS * max(1.0, float(np.abs(ref["gts"]).max()))
    return {"gts": pos, "gvs": pos * ref["fps"], "gavs": pos * ref["fps"], "dvs": pos * ref["fps"]}


def host_errors(model, clip, ref):
    """e_host per channel: max |float32 host restatement - float64 reference| over the clip."""
    from humanoid_amd.motion_lib import clip_to_motion
    host = clip_to_motion(model, clip)
    return {k: float(np.abs(host[k].astype(np.float64) - ref[k]).max()) for k in CHANNELS}


def device_bounds(model, clip, ref):
    """What the device is held to, per channel: 3 max(e_host, floor). The device differs from the host
    restatement only in operation order, FMA contraction and the accuracy of acosf / sqrtf, each a
    few ulp at the same ill-conditioned points, so its error is another draw from the distribution
    e_host samples as a maximum over thousands of entries."""
    e, fl = host_errors(model, clip, ref), floors(ref)
    return {k: 3.0 * max(e[k], fl[k]) for k in CHANNELS}


def host_bounds(ref):
    """What the float32 host restatement is held to against the float64 reference, per channel, from
    the number format alone (nothing measured on the code under test):

    * positions: a chain of up to 9 links, each a normalised float32 quaternion product and a
      rotation of an offset below 0.5 m, a few ulp each: 16 ulp of max(1, max |position|);
    * linear velocity: a position difference over dt (the filter only averages): that times fps;
    * angular velocity: angle = acos(2 w^2 - 1) of a float32 quaternion product. The argument
      carries d = 8 ulp (the product's 4 terms, the square, the doubling), and acos turns an
      argument error d into min(sqrt(2 d), d / sin(angle)) of angle error -- the float32 acos
      near 1 that the reference project has by design. Over the clip's own frame-to-frame angles,
      times fps, plus the rounding of the velocity itself;
    * dof velocity: exp map = xyz (2 acos(w) / sqrt(1 - w^2)) of the product of two local rotations.
      The factor is well conditioned (its derivative in w is about -2/3: the acos and the sqrt see the
      same w), so the error is that of the vector parts: 4 ulp in each of the two local rotations
      and the product's 4 terms, doubled by the half angle -- 32 ulp of rotation; where
      sin(half) <= 2e-5 the reference's angle-axis may return 0, which costs the angle itself."""
    fps = ref["fps"]
    pos = 16.0 * EPS * max(1.0, float(np.abs(ref["gts"]).max()))
    d = 8.0 * EPS

    def acos_err(angle):
        with np.errstate(divide="ignore"):
            return np.minimum(np.sqrt(2.0 * d), d / np.abs(np.sin(angle)))

    th = np.linalg.norm(ref["raw_gavs"][:-1], axis=-1) / fps
    thd = np.linalg.norm(ref["dvs"], axis=-1) / fps
    ang = float(acos_err(th).max()) * fps + 16.0 * EPS * float(np.abs(ref["gavs"]).max())
    masked = float(np.where(np.sin(thd / 2.0) <= 2e-5, thd, 0.0).max())
    dof = (32.0 * EPS + masked) * fps + 16.0 * EPS * float(np.abs(ref["dvs"]).max())
    return {"gts": pos, "gvs": pos * fps, "gavs": ang, "dvs": dof}
