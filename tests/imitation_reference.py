"""Independent float64 imitation step: the checker for imitation_kernel (csrc/he_imitation.hip,
he_imitation_env.h, he_math.h) and for its C restatement (oracle/he_oracle.c).

Written from the reference project's definitions (envs/common.py:22-176 observations, :179-267 AMP
row, :298-317 reward, :325-364 termination; envs/humanoid_phc.py:138-152, 688-780, 848-860, 937-961,
1063-1067, 1297-1335) with rotation matrices and rotation vectors (scipy Rotation). No quaternion
product and no ``my_quat_rotate`` appear here, and nothing is shared with humanoid_amd/ or oracle/
(body_sets' name lists and the bit-defined ``oracle.hash_uniform`` draw excepted; the model's
``parents`` / ``local_pos`` are data). Motion samples come from ``ingest_reference.motion_state`` on
the float32 tables the engine is given, upcast to float64, so ingestion error does not enter.

Decisions taken in float32, and why (all are discontinuous choices of the step, where a float64
decision would compare one side of a branch with the other):

* ``env_time``: ``progress * control_dt + start + start_offset`` as three float32 operations (the
  reference project's float32 tensors, humanoid_phc.py:1236-1238). It picks the frame pair and the
  blend (``ingest_reference.frame_select``) and decides ``t >= len``;
* ``sample_time_interval``: the floor ``k = int((phase * len) / (1 / 30))`` in float32
  (motion_lib.py:526-535), and for Hybrid the draw's ``u < p`` and ``phase = u / p``. The product
  ``k * (1 / 30)`` is float64 (``time64``); the value the reference project *stores* as the env's
  start time is the one float32 multiply torch makes of ``long * float`` (``start_time``), and
  every later time of that env is built from the stored value, as there;
* the slerp's branches and its two float32 weights (``ingest_reference._slerp``). The float32
  weights leave a sample's quaternion with a norm of 1 + eps, eps up to 1e-4 for frames 0.02-0.04 rad
  apart. The reference project never renormalises it, and its formulas are not scale-free: a
  rotated vector is ``n2 R v + (n2 - 1) v`` (n2 the squared norm, R the rotation of the direction) and
  the angle of the reward is ``2 acos(n cos(theta / 2))``, theta the geodesic angle of
  ``R_ref R_sim^T`` -- equal to theta for unit quaternions. Both are written here in that matrix
  form, the norm taken from the float64 sample.

Everything else -- blends, rotations, norms, means, exponentials, the heading -- is float64.
"""
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np
from scipy.spatial.transform import Rotation

import ingest_reference as IR

F32 = np.float32
NB, ND = 24, 69
OBS_SELF, OBS_TASK = 358, 576
OBS_DIM = OBS_SELF + OBS_TASK
# observation blocks [a, b): common.py:91-94 (self) and :168-173 (task, after the 358 self floats)
OBS_BLOCKS = {"self_h": (0, 1), "self_pos": (1, 70), "self_rot": (70, 214), "self_vel": (214, 286),
              "self_ang": (286, 358), "task_dpos": (358, 430), "task_drot": (430, 574), "task_dvel": (574, 646),
              "task_dang": (646, 718), "task_rpos": (718, 790), "task_rrot": (790, 934)}
CURR = 1.0 / 30.0  # motion_lib.py:532


@dataclass
class Params:
    """config.py RewardConfig / EnvConfig defaults of the reference project."""
    k_pos: float = 100.0
    k_rot: float = 10.0
    k_vel: float = 0.1
    k_ang_vel: float = 0.1
    w_pos: float = 0.5
    w_rot: float = 0.3
    w_vel: float = 0.1
    w_ang_vel: float = 0.1
    power_coef: float = 0.0005
    use_power_reward: bool = True
    control_dt: float = 1.0 / 30.0
    enable_early_termination: bool = True
    eval_mode: bool = False
    termination_distance: Sequence[float] = field(default_factory=lambda: [0.25] * NB)
    reset_body_ids: Sequence[int] = field(default_factory=lambda: list(range(NB)))  # in list order
    state_init: str = "Random"
    hybrid_init_prob: float = 0.5
    test_mode: bool = False

    def distances(self):
        return np.broadcast_to(np.asarray(self.termination_distance, F32), (NB,)).astype(np.float64)


class Tables:
    """The float32 host tables the engine is given, upcast to float64 (metadata stays float32)."""

    def __init__(self, t):
        for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs"):
            x = np.asarray(getattr(t, k))
            assert x.dtype == F32, k
            setattr(self, k, x.astype(np.float64))
        self.num_frames = np.asarray(t.num_frames, np.int64)
        self.length_starts = np.asarray(t.length_starts, np.int64)
        self.lengths = np.asarray(t.lengths, F32)
        self.dt = np.asarray(t.dt, F32)


def env_time(progress, control_dt, start, start_offset):
    """he_imitation_env.h env_time: three float32 operations."""
    t = np.asarray(progress).astype(F32) * F32(control_dt)
    t = t + np.asarray(start, F32)
    t = t + np.asarray(start_offset, F32)
    assert t.dtype == F32
    return t


def exp_map(q):
    """torch_utils.py quat_to_exp_map of xyzw quaternions of any norm, as the reference project defines
    it: the angle 2 acos(w) wrapped into (-pi, pi], times xyz / sqrt(1 - w^2); zero where that root
    is below 1e-5 or undefined. For a unit quaternion this is its rotation vector; the float32 slerp
    leaves a norm of 1 + eps, which this formula reads as part of the angle (2 eps / tan(angle / 2))."""
    q = np.asarray(q, np.float64)
    w = q[..., 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(1.0 - w * w)
        a = 2.0 * np.arccos(w)
        a = np.arctan2(np.sin(a), np.cos(a))
        out = q[..., :3] * (a / s)[..., None]
    return np.where((np.abs(s) > 1e-5)[..., None], out, 0.0)


def sample(tables, ids, times, offset=None):
    """ingest_reference.motion_state, the dof positions by the reference project's exp map of the
    slerped local rotation as it stands (not renormalised)."""
    ids, times = np.asarray(ids, np.int64), np.asarray(times, F32)
    m = IR.motion_state(tables, ids, times, offset)
    g0, g1, blend = IR.frame_select(tables, ids, times)
    lr = IR._slerp(tables.lrs[g0][:, 1:], tables.lrs[g1][:, 1:], blend.astype(np.float64)[:, None])
    m["dof_pos"] = exp_map(lr).reshape(len(ids), -1)
    return m


# ------------------------------------------------------------------ rotations as (matrix, norm^2)
def _mat(q):
    """xyzw quaternions [...,4] of any norm -> (rotation matrices [...,3,3] of their directions,
    squared norms [...])."""
    q = np.asarray(q, np.float64)
    m = Rotation.from_quat(q.reshape(-1, 4)).as_matrix().reshape(q.shape[:-1] + (3, 3))
    return m, (q * q).sum(-1)


def _rotz(h):
    c, s, z, o = np.cos(h), np.sin(h), np.zeros_like(h), np.ones_like(h)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def _tan_norm(m, n2):
    """Tangent and normal of a rotation: columns 0 and 2 of its matrix; for a quaternion of squared
    norm n2 the reference project's rotate gives n2 R e + (n2 - 1) e."""
    n2 = n2[..., None]
    ex, ez = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    return np.concatenate([n2 * m[..., :, 0] + (n2 - 1.0) * ex, n2 * m[..., :, 2] + (n2 - 1.0) * ez], -1)


def heading(root_q):
    """Yaw of the root's rotated x axis (torch_utils.py calc_heading); also its horizontal length."""
    m, n2 = _mat(root_q)
    x = n2[..., None] * m[..., :, 0] + (n2[..., None] - 1.0) * np.array([1.0, 0.0, 0.0])
    return np.arctan2(x[..., 1], x[..., 0]), np.hypot(x[..., 0], x[..., 1])


def geodesic(ref_q, sim_q):
    """Angle of R_ref R_sim^T in [0, pi]."""
    a, _ = _mat(ref_q)
    b, _ = _mat(sim_q)
    d = a @ np.swapaxes(b, -1, -2)
    return np.linalg.norm(IR._rotvec(d), axis=-1)


def reward_angle(ref_q, sim_q):
    """common.py:304-305: 2 acos(w) of the product; with norms n_ref n_sim = n the product's w is
    n cos(theta / 2), and a w above 1 is the reference project's masked 0 (sqrt(1 - w^2) is NaN)."""
    th = geodesic(ref_q, sim_q)
    n = np.sqrt((np.asarray(ref_q, np.float64) ** 2).sum(-1) * (np.asarray(sim_q, np.float64) ** 2).sum(-1))
    w = n * np.cos(th / 2.0)
    return np.where(w >= 1.0, 0.0, 2.0 * np.arccos(np.minimum(w, 1.0)))


# ------------------------------------------------------------------ observation
def observation(pos, rot, vel, ang, ref):
    """[n, 934]: common.py:22-103 (self) then :106-176 (task, one time step) of body states
    [n,24,3|4] against the sample ``ref`` (rg_pos, rb_rot, body_vel, body_ang_vel)."""
    pos, vel, ang = (np.asarray(x, np.float64) for x in (pos, vel, ang))
    n = pos.shape[0]
    h, _ = heading(np.asarray(rot)[:, 0])
    hinv, hfwd = _rotz(-h)[:, None], _rotz(h)[:, None]  # [n,1,3,3]
    rs, n2s = _mat(rot)
    rr, n2r = _mat(ref["rb_rot"])
    rv = lambda v: np.einsum("nbij,nbj->nbi", np.broadcast_to(hinv, (n, NB, 3, 3)), v)  # noqa: E731
    root = pos[:, :1]
    o = np.zeros((n, OBS_DIM))
    o[:, 0] = pos[:, 0, 2]
    o[:, 1:70] = rv(pos - root)[:, 1:].reshape(n, -1)
    o[:, 70:214] = _tan_norm(hinv @ rs, n2s).reshape(n, -1)
    o[:, 214:286] = rv(vel).reshape(n, -1)
    o[:, 286:358] = rv(ang).reshape(n, -1)
    t = o[:, OBS_SELF:]
    t[:, 0:72] = rv(ref["rg_pos"] - pos).reshape(n, -1)
    t[:, 72:216] = _tan_norm(hinv @ rr @ np.swapaxes(rs, -1, -2) @ hfwd, n2r * n2s).reshape(n, -1)
    t[:, 216:288] = rv(ref["body_vel"] - vel).reshape(n, -1)
    t[:, 288:360] = rv(ref["body_ang_vel"] - ang).reshape(n, -1)
    t[:, 360:432] = rv(ref["rg_pos"] - root).reshape(n, -1)
    t[:, 432:576] = _tan_norm(hinv @ rr, n2r).reshape(n, -1)
    return o


def _split(rb):
    rb = np.asarray(rb, np.float64).reshape(-1, NB, 13)
    return rb[..., 0:3], rb[..., 3:7], rb[..., 7:10], rb[..., 10:13]


# ------------------------------------------------------------------ the step
def step(tables, p: Params, rb_state, dof_vel, dof_force, progress_in, motion_ids, start_times, start_offsets,
         global_offset):
    """The post-physics half of HumanoidPHC.step (humanoid_phc.py:138-152) for every env: progress + 1,
    reward, reset / terminate, and the observation against the t + dt sample."""
    pos, rot, vel, ang = _split(rb_state)
    n = pos.shape[0]
    mids = np.asarray(motion_ids, np.int64)
    prog = np.asarray(progress_in, np.int64) + 1
    t = env_time(prog, p.control_dt, start_times, start_offsets)
    ref = sample(tables, mids, t, global_offset)
    # reward, common.py:298-317
    msq = lambda a, b: ((a - b) ** 2).mean(-1).mean(-1)  # noqa: E731
    theta = reward_angle(ref["rb_rot"], rot)
    dist = {"pos": msq(ref["rg_pos"], pos), "rot": (theta ** 2).mean(-1), "vel": msq(ref["body_vel"], vel),
            "ang": msq(ref["body_ang_vel"], ang)}
    raw = np.zeros((n, 5))
    raw[:, 0] = np.exp(-p.k_pos * dist["pos"])
    raw[:, 1] = np.exp(-p.k_rot * dist["rot"])
    raw[:, 2] = np.exp(-p.k_vel * dist["vel"])
    raw[:, 3] = np.exp(-p.k_ang_vel * dist["ang"])
    rew = p.w_pos * raw[:, 0] + p.w_rot * raw[:, 1] + p.w_vel * raw[:, 2] + p.w_ang_vel * raw[:, 3]
    power = np.abs(np.asarray(dof_force, np.float64) * np.asarray(dof_vel, np.float64)).reshape(n, -1).sum(-1)
    if p.use_power_reward:  # humanoid_phc.py:1297-1305
        raw[:, 4] = np.where(prog <= 3, 0.0, -p.power_coef * power)
        rew = rew + raw[:, 4]
    # termination, common.py:325-364 + humanoid_phc.py:1313-1335
    pass_time = t >= tables.lengths[mids]
    ids = list(p.reset_body_ids)
    td = p.distances()[ids]  # self._termination_distances[..., self._reset_bodies_id]
    body_dist = np.linalg.norm(pos - ref["rg_pos"], axis=-1)
    fallen = np.zeros(n, bool)
    margin = np.full(n, np.inf)  # relative distance of the deciding quantity from its threshold
    if p.enable_early_termination and ids:
        d = body_dist[:, ids]
        if p.eval_mode:
            fallen = d.mean(-1) > td[0]
            margin = np.abs(d.mean(-1) / td[0] - 1.0)
        else:
            fallen = (d > td).any(-1)
            margin = np.abs(d / td - 1.0).min(-1)
        fallen = fallen & (prog > 1)
    reset = pass_time | fallen
    t2 = env_time(prog + 1, p.control_dt, start_times, start_offsets)  # humanoid_phc.py:1063-1067
    ref2 = sample(tables, mids, t2, global_offset)
    return {"rew": rew, "reward_raw": raw, "reset": reset, "terminate": fallen, "progress": prog,
            "obs": observation(pos, rot, vel, ang, ref2), "t": t, "t_obs": t2, "theta": geodesic(ref["rb_rot"], rot),
            "dist": dist, "power": power, "body_dist": body_dist, "term_margin": margin, "ref": ref, "ref_obs": ref2,
            "heading_len": heading(rot[:, 0])[1]}


# ------------------------------------------------------------------ resets
def resolve_init(p: Params, u):
    """(reference-state init?, phase) of each draw u (humanoid_phc.py:679-692, 733-745, 848-856)."""
    u = np.asarray(u, F32)
    ref = np.full(u.shape, p.state_init != "Default")
    ph = u.copy()
    if p.state_init == "Hybrid":
        ref = u < F32(p.hybrid_init_prob)
        ph = np.where(ref, u / F32(p.hybrid_init_prob), F32(0)).astype(F32)
    if p.state_init == "Start" or p.test_mode:
        ph = np.zeros_like(u)
    return ref, ph


def sample_time_interval(phase, length):
    """motion_lib.py:526-535 -> (k, k / 30 in float64, the float32 value the reference stores)."""
    x = (np.asarray(phase, F32) * np.asarray(length, F32)) / F32(CURR)
    assert x.dtype == F32
    k = x.astype(np.int64)
    return k, k * CURR, k.astype(F32) * F32(CURR)


def rest_positions(model):
    """Body origins of the zero pose in the root frame: the joint offsets summed along each chain."""
    lp = np.asarray(model.local_pos, np.float64)
    rest = np.zeros((NB, 3))
    for b in range(1, NB):
        rest[b] = rest[int(model.parents[b])] + lp[b]
    return rest


def reset(tables, p: Params, model, env_ids, draws, motion_ids, state):
    """The resets of ``env_ids`` with uniform draws ``draws`` (one per id) on a copy of ``state``
    (start_times, start_offsets, global_offset, progress, root_states, dof_state, dof_targets,
    rb_state, contact_forces, obs, reset, terminate, init_root): reference-state init
    (humanoid_phc.py:694-731, 848-860: the sample at the start time with the PRE-reset global offset,
    then offset, start offset and progress zeroed), default init (:688-692: the initial root state,
    zero dofs, body rows root + R rest_pos), _reset_env_tensors (:747-780) and the observation of the
    reset envs against the sample one control step after the start. Returns the new state and, per
    id, ref_init / k / time64."""
    s = {k: np.array(v, np.float64 if np.asarray(v).dtype.kind == "f" else None, copy=True) for k, v in state.items()}
    ids = np.asarray(env_ids, np.int64)
    mids = np.asarray(motion_ids, np.int64)[ids]
    ref_init, ph = resolve_init(p, draws)
    k, time64, stored = sample_time_interval(ph, tables.lengths[mids])
    k, time64, stored = np.where(ref_init, k, 0), np.where(ref_init, time64, 0.0), np.where(ref_init, stored, F32(0))
    r, d = ids[ref_init], ids[~ref_init]
    if len(r):
        m = sample(tables, mids[ref_init], stored[ref_init], s["global_offset"][r])
        rows = np.concatenate([m["rg_pos"], m["rb_rot"], m["body_vel"], m["body_ang_vel"]], -1)
        s["rb_state"][r] = rows
        s["root_states"][r] = rows[:, 0]
        s["dof_state"][r, :, 0] = m["dof_pos"]
        s["dof_state"][r, :, 1] = m["dof_vel"]
        s["dof_targets"][r] = m["dof_pos"]
        s["global_offset"][r] = 0.0
        s["start_times"][r] = stored[ref_init]
        s["start_offsets"][r] = 0.0
    if len(d):
        ir = np.asarray(s["init_root"], np.float64)[d]
        rm, _ = _mat(ir[:, 3:7])
        ro = np.einsum("nij,bj->nbi", rm, rest_positions(model))
        rows = np.zeros((len(d), NB, 13))
        rows[..., 0:3] = ir[:, None, 0:3] + ro
        rows[..., 3:7] = ir[:, None, 3:7]
        rows[..., 7:10] = ir[:, None, 7:10] + np.cross(ir[:, None, 10:13], ro)
        rows[..., 10:13] = ir[:, None, 10:13]
        s["rb_state"][d] = rows
        s["root_states"][d] = ir
        s["dof_state"][d] = 0.0
        s["dof_targets"][d] = 0.0
    s["contact_forces"][ids] = 0.0
    s["progress"][ids] = 0
    s["reset"][ids] = 0
    s["terminate"][ids] = 0
    pos, rot, vel, ang = _split(s["rb_state"][ids])
    t2 = env_time(np.ones(len(ids), np.int64), p.control_dt, s["start_times"][ids], s["start_offsets"][ids])
    ref2 = sample(tables, mids, t2, s["global_offset"][ids])
    s["obs"][ids] = observation(pos, rot, vel, ang, ref2)
    return s, {"ref_init": ref_init, "k": k, "time64": time64, "ref_obs": ref2}


# ------------------------------------------------------------------ AMP rows (common.py:179-267)
def amp_sets():
    """Joint indices of the AMP dof subset (humanoid_phc.py:186-194) and the key bodies."""
    from humanoid_amd import body_sets as BS
    joints = [i for i, name in enumerate(BS.DOF_NAMES) if name not in BS.REMOVE_NAMES]
    return np.array(joints), np.array(BS.body_ids(BS.KEY_BODIES))


def amp_row(root_pos, root_q, root_vel, root_ang, dof_pos, dof_vel, key_pos):
    """[n, 196]: root height, tangent / normal of the heading-free root rotation, heading-free root
    velocities, tangent / normal of every subset joint's rotation, their dof velocities, heading-free
    key-body offsets."""
    joints, _ = amp_sets()
    n = len(root_pos)
    h, _ = heading(root_q)
    hinv = _rotz(-h)
    rm, n2 = _mat(root_q)
    dp = np.asarray(dof_pos, np.float64).reshape(n, -1, 3)[:, joints]
    dv = np.asarray(dof_vel, np.float64).reshape(n, -1, 3)[:, joints]
    jm = Rotation.from_rotvec(dp.reshape(-1, 3)).as_matrix().reshape(n, len(joints), 3, 3)
    key = np.einsum("nij,nkj->nki", hinv, np.asarray(key_pos, np.float64) - np.asarray(root_pos, np.float64)[:, None])
    return np.concatenate([
        np.asarray(root_pos, np.float64)[:, 2:3], _tan_norm(hinv @ rm, n2),
        np.einsum("nij,nj->ni", hinv, root_vel), np.einsum("nij,nj->ni", hinv, root_ang),
        _tan_norm(jm, np.ones((n, len(joints)))).reshape(n, -1), dv.reshape(n, -1), key.reshape(n, -1)], -1)


def amp_from_sample(m):
    _, keys = amp_sets()
    return amp_row(m["rg_pos"][:, 0], m["rb_rot"][:, 0], m["body_vel"][:, 0], m["body_ang_vel"][:, 0], m["dof_pos"],
                   m["dof_vel"], m["rg_pos"][:, keys])


def amp_history(tables, p: Params, motion_ids, start_times, rb_state, dof_state, S):
    """[n, S, 196] of envs just reset to a reference state (humanoid_phc.py:791-819): row 0 from the
    reset state, row k from the motion at start - k dt (float32 times, no offset; a negative time
    samples time 0)."""
    _, keys = amp_sets()
    pos, rot, vel, ang = _split(rb_state)
    ds = np.asarray(dof_state, np.float64)
    n = len(pos)
    out = np.zeros((n, S, 196))
    out[:, 0] = amp_row(pos[:, 0], rot[:, 0], vel[:, 0], ang[:, 0], ds[..., 0], ds[..., 1], pos[:, keys])
    steps = F32(-p.control_dt) * (np.arange(S - 1).astype(F32) + F32(1))
    t = np.asarray(start_times, F32)[:, None] + steps[None, :]
    assert t.dtype == F32
    mids = np.repeat(np.asarray(motion_ids, np.int64), S - 1)
    m = sample(tables, mids, t.reshape(-1))
    out[:, 1:] = amp_from_sample(m).reshape(n, S - 1, 196)
    coord = np.concatenate([np.abs(pos).max((-1, -2))[:, None], np.abs(m["rg_pos"]).max((-1, -2)).reshape(n, S - 1)], 1)
    return out, t, coord
