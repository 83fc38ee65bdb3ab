"""The adversarial case set of the imitation step, and the bounds its tests hold the device to.

One library (``ingest_cases.libraries(model)["mixed"]``: 2-frame clips, a held pose, sign-flipped
frames, a 59.94 fps clip, starts on every residue mod 8) loaded as host tables, and K named cases,
each an env's simulated state plus its motion bookkeeping. Env i < 2K holds case i mod K; K is odd,
so every case sits at an even and an odd env index (both 32-lane halves of a wave), and one more copy
of case 0 makes the env count 2K + 1: odd, no multiple of 8 (a half-filled last wave and a partial
block). All seeded.

Every case is checked under every parameter set of ``PARAM_SETS`` (a parameter set is one launch);
``designed`` names the set a threshold case is built for. Flag margins (checked in float64 by
test_imitation_reference.py for every env under every set): a body or a mean that decides a
termination is at least a relative MARGIN = 1e-3 from its distance -- three orders above the float32
rounding of a distance of 0.1-0.5 m between coordinates of order 1 (derived, not measured); reset
phases are at least 1e-3 from an integer in ``phase len / (1 / 30)`` and Hybrid draws at least 1e-3
from the probability. Times are decided in float32 on both sides, so the ``t == len`` and ``one ulp
below`` cases need no margin.

Heading cases keep the horizontal length of the root's rotated x axis at cos(1.2) = 0.36 >= 0.3: below
that the heading (an atan2 of that axis) is ill-conditioned, which is the reference project's own
property and not the kernel's.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import imitation_reference as R
import ingest_cases as IC

F32 = np.float32
SEED = 20241103
MARGIN = 1e-3
NB, ND = 24, 69
CDT = 1.0 / 30.0
U = 2.0 ** -23  # one float32 rounding, as ingest_cases.EPS

ANGLES = (1e-6, 1e-4, 1e-2, 1.0, np.pi - 1e-3, np.pi - 1e-6)
YAWS = (("0", 0.0), ("+90", np.pi / 2), ("-90", -np.pi / 2), ("+pi", np.pi - 1e-4), ("-pi", -np.pi + 1e-4),
        ("rand", 2.2173))
TILTS = (0.0, 0.6, 1.2)


def _eval_bodies():
    from humanoid_amd.body_sets import EVAL_BODIES, body_ids
    return body_ids(EVAL_BODIES)


def _param_sets():
    ev = _eval_bodies()
    b = np.arange(NB)
    return {
        "train": R.Params(),
        "train_set": R.Params(reset_body_ids=ev, termination_distance=list(0.15 + 0.004 * b)),
        "eval": R.Params(eval_mode=True, reset_body_ids=ev, termination_distance=list(0.4 + 0.013 * b)),
        "eval_single": R.Params(eval_mode=True, reset_body_ids=[7], termination_distance=list(0.4 + 0.013 * b)),
        "eval_empty": R.Params(eval_mode=True, reset_body_ids=[], termination_distance=list(0.4 + 0.013 * b)),
        "nopower": R.Params(use_power_reward=False),
    }


PARAM_SETS = _param_sets()
STATE_INITS = ("Random", "Start", "Default", "Hybrid")


def abi_params(p: R.Params, **over):
    """The engine's parameter block of a reference parameter set."""
    from humanoid_amd import _abi
    kw = dict(reward={k: getattr(p, k) for k in ("k_pos", "k_rot", "k_vel", "k_ang_vel", "w_pos", "w_rot", "w_vel",
                                                   "w_ang_vel")},
              control_dt=p.control_dt, use_power_reward=p.use_power_reward, power_coef=p.power_coef,
              enable_early_termination=p.enable_early_termination, eval_mode=p.eval_mode,
              termination_distance=np.asarray(p.termination_distance, F32), reset_body_ids=list(p.reset_body_ids),
              state_init=p.state_init, hybrid_init_prob=p.hybrid_init_prob, test_mode=p.test_mode)
    kw.update(over)
    return _abi.imitation_params(**kw)


def with_init(p: R.Params, state_init):
    from dataclasses import replace
    return replace(p, state_init=state_init, hybrid_init_prob=0.5)


def _unit(rng, n=None):
    v = rng.normal(size=(3,) if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class CaseSet:
    def __init__(self, model):
        from humanoid_amd.motion_lib import build_tables
        self.model = model
        self.host_tables = build_tables(model, IC.libraries(model)["mixed"])
        self.tables = R.Tables(self.host_tables)
        self.rng = np.random.default_rng(SEED)
        self.cases = []
        self._build()
        K = len(self.cases)
        assert K % 2 == 1, K
        self.K = K
        self.order = np.concatenate([np.arange(K), np.arange(K), [0]])
        self.n = len(self.order)
        c = [self.cases[i] for i in self.order]
        self.names = [x["name"] for x in c]
        self.family = np.array([x["family"] for x in c])
        self.designed = [x["designed"] for x in c]
        self.rb_state = np.stack([x["rb"] for x in c]).astype(F32)
        self.dof_vel = np.stack([x["dof_vel"] for x in c]).astype(F32)
        self.dof_force = np.stack([x["dof_force"] for x in c]).astype(F32)
        self.progress_in = np.array([x["prog"] for x in c], np.int16)
        self.motion_ids = np.array([x["mid"] for x in c], np.int64)
        self.start_times = np.array([x["start"] for x in c], F32)
        self.start_offsets = np.array([x["soff"] for x in c], F32)
        self.global_offset = np.stack([x["goff"] for x in c]).astype(F32)
        rng = np.random.default_rng(SEED + 1)
        ir = np.zeros((self.n, 13), F32)  # the initial root states of the Default init: upright, any yaw
        ir[:, :2] = rng.uniform(-2, 2, (self.n, 2))
        ir[:, 2] = 0.9
        ir[:, 3:7] = Rotation.from_rotvec(np.outer(rng.uniform(-np.pi, np.pi, self.n), [0, 0, 1.0])).as_quat()
        self.init_root = ir

    # ------------------------------------------------------------ indexing
    def envs_of(self, name):
        return [i for i, x in enumerate(self.names) if x == name]

    def families(self):
        return sorted(set(self.family))

    def permutation(self):
        """perm[j] = the env whose case sits at position j after the move: the first 2K envs rotate
        by an odd shift of more than a block, so each changes parity and block; the last stays."""
        two_k, s = 2 * self.K, 37
        assert 8 <= s <= two_k - 8
        src = (np.arange(two_k) - s) % two_k
        return np.concatenate([src, [two_k]])

    def step_inputs(self, idx=None):
        idx = np.arange(self.n) if idx is None else np.asarray(idx)
        return dict(rb_state=self.rb_state[idx], dof_vel=self.dof_vel[idx], dof_force=self.dof_force[idx],
                    progress_in=self.progress_in[idx], motion_ids=self.motion_ids[idx],
                    start_times=self.start_times[idx], start_offsets=self.start_offsets[idx],
                    global_offset=self.global_offset[idx])

    def reference_step(self, pname, idx=None):
        return R.step(self.tables, PARAM_SETS[pname], **self.step_inputs(idx))

    # ------------------------------------------------------------ construction
    def _tracked(self, mid, prog, start=0.0, soff=0.0, goff=(0.0, 0.0, 0.0)):
        """The float32 sample at the time of the step: the simulated state of exact tracking."""
        t = R.env_time(np.array([prog + 1]), CDT, F32(start), F32(soff))
        m = R.sample(self.tables, [mid], t, np.asarray([goff], F32))
        return np.concatenate([m["rg_pos"], m["rb_rot"], m["body_vel"], m["body_ang_vel"]], -1)[0].astype(F32)

    def _margin(self, rb, prog, mid, start, soff, goff):
        """The smallest termination margin of one env over every parameter set (float64)."""
        one = dict(rb_state=np.asarray(rb, F32)[None], dof_vel=np.zeros((1, ND), F32), dof_force=np.zeros((1, ND), F32),
                   progress_in=np.array([prog]), motion_ids=np.array([mid]), start_times=np.array([start], F32),
                   start_offsets=np.array([soff], F32), global_offset=np.asarray([goff], F32))
        return min(float(R.step(self.tables, p, **one)["term_margin"][0]) for p in PARAM_SETS.values())

    def _add(self, name, family, rb, prog, mid, start=0.0, soff=0.0, goff=(0.0, 0.0, 0.0), designed=None,
             dof_vel=None, dof_force=None):
        """``rb``: the rows, or a function drawing them (drawn again while a body or a mean lies within
        the margin of a termination distance of some parameter set)."""
        rng = self.rng
        if callable(rb):
            for _ in range(50):
                rows = rb()
                if self._margin(rows, prog, mid, start, soff, goff) >= 2 * MARGIN:
                    break
            else:
                raise AssertionError(f"{name}: no draw keeps the margin")
            rb = rows
        self.cases.append(dict(
            name=name, family=family, rb=np.asarray(rb, F32), prog=int(prog), mid=int(mid), start=F32(start),
            soff=F32(soff), goff=np.asarray(goff, F32), designed=designed,
            dof_vel=rng.normal(0, 1.0, ND) if dof_vel is None else dof_vel,
            dof_force=rng.normal(0, 20.0, ND) if dof_force is None else dof_force))

    def _noisy(self, rb, pos=0.02, rot=0.05, vel=0.3):
        rng = self.rng
        rb = np.array(rb, np.float64)
        rb[:, 0:3] += rng.normal(0, pos, (NB, 3))
        rb[:, 3:7] = (Rotation.from_rotvec(rng.normal(0, rot, (NB, 3))) * Rotation.from_quat(rb[:, 3:7])).as_quat()
        rb[:, 7:13] += rng.normal(0, vel, (NB, 6))
        return rb.astype(F32)

    def _rotated(self, rb, angles):
        rb = np.array(rb, np.float64)
        err = Rotation.from_rotvec(_unit(self.rng, NB) * np.asarray(angles, np.float64)[:, None])
        rb[:, 3:7] = (err * Rotation.from_quat(rb[:, 3:7])).as_quat()
        return rb.astype(F32)

    def _displaced(self, rb, lengths):
        """Body b moved by a vector of length lengths[b] (0: left where it is)."""
        rb = np.array(rb, np.float64)
        rb[:, 0:3] += _unit(self.rng, NB) * np.asarray(lengths, np.float64)[:, None]
        return rb.astype(F32)

    def _posed(self, rb, yaw, tilt, axis):
        """The whole body turned rigidly about its root so that the root's rotation is
        Rz(yaw) R(axis, tilt): the rotated x axis has heading yaw for axis = y."""
        rb = np.array(rb, np.float64)
        want = Rotation.from_rotvec([0, 0, yaw]) * Rotation.from_rotvec(np.asarray(axis, np.float64) * tilt)
        g = want * Rotation.from_quat(rb[0, 3:7]).inv()
        rb[:, 0:3] = rb[0, 0:3] + g.apply(rb[:, 0:3] - rb[0, 0:3])
        rb[:, 3:7] = (g * Rotation.from_quat(rb[:, 3:7])).as_quat()
        rb[:, 7:10], rb[:, 10:13] = g.apply(rb[:, 7:10]), g.apply(rb[:, 10:13])
        return rb.astype(F32)

    def _frame_time_progress(self, mid):
        """A progress whose step time falls on a frame of the clip with a float32 blend of exactly 0."""
        for prog in range(3, 30):
            t = R.env_time(np.array([prog + 1]), CDT, F32(0), F32(0))
            _, _, bl = R.IR.frame_select(self.tables, [mid], t)
            if bl[0] == 0 and t[0] < self.tables.lengths[mid]:
                return prog
        raise AssertionError("no frame time with blend 0")

    def _start_for(self, mid, prog, target):
        """A float32 start time at which env_time(prog) is exactly the float32 ``target``."""
        s = F32(target) - F32(prog) * F32(CDT)
        for _ in range(64):
            for cand in (s, np.nextafter(s, F32(np.inf)), np.nextafter(s, F32(-np.inf))):
                if R.env_time(np.array([prog]), CDT, cand, F32(0))[0] == F32(target):
                    return cand
            s = np.nextafter(s, F32(np.inf))
        raise AssertionError("no start time reaches the target")

    def _build(self):
        rng, T = self.rng, self.tables
        mi = IC.mixed_index
        n37, n150, held, n2, flip, spin, n17 = (mi(k) for k in ("n37", "n150", "held", "n2", "flip", "spin", "n17"))
        sets = PARAM_SETS

        # ---- exact tracking, and the same with every simulated quaternion negated
        def exact(name, *a, **k):
            rb = self._tracked(*a, **k)
            fv, ff = rng.normal(0, 1.0, ND), rng.normal(0, 20.0, ND)
            neg = rb.copy()
            neg[:, 3:7] *= -1
            self._add(name, "exact", rb, a[1], a[0], dof_vel=fv, dof_force=ff, **k)
            self._add(name + "_neg", "exact", neg, a[1], a[0], dof_vel=fv, dof_force=ff, **k)
        exact("exact_frame", n37, self._frame_time_progress(n37))
        exact("exact_held", held, 14)
        _, _, st = R.sample_time_interval(F32(0.37), T.lengths[n150])
        exact("exact_after_reset", n150, 0, start=st)
        exact("exact_blend", flip, 7, start=0.0127)

        # ---- rotation error
        base = self._tracked(n150, 20)
        for a in ANGLES:
            self._add(f"rot_{a:.7g}", "rotation", self._rotated(base, np.full(NB, a)), 20, n150)
        self._add("rot_mixed", "rotation", self._rotated(base, np.resize(ANGLES, NB)), 20, n150)
        self._add("rot_spin", "rotation", self._rotated(self._tracked(spin, 9), np.resize(ANGLES[::-1], NB)), 9, spin)

        # ---- root heading and tilt
        posed = lambda yaw, tilt, axis: (  # noqa: E731
            lambda: self._posed(self._noisy(self._tracked(n37, 11)), yaw, tilt, axis))
        for yn, yaw in YAWS:
            for tilt in TILTS:
                self._add(f"head_{yn}_tilt{tilt:g}", "heading", posed(yaw, tilt, [0, 1.0, 0]), 11, n37)
        self._add("head_rand_axis", "heading", posed(-1.3, 0.6, [np.cos(0.7), np.sin(0.7), 0]), 11, n37)

        # ---- termination margins, train mode
        base = self._tracked(n150, 5)
        one = lambda b, length: np.where(np.arange(NB) == b, length, 0.0)  # noqa: E731
        td = sets["train_set"].distances()
        self._add("term_beyond", "termination", self._displaced(base, one(7, td[7] * (1 + MARGIN))), 5, n150,
                  designed="train_set")
        self._add("term_inside", "termination", self._displaced(base, one(7, td[7] * (1 - MARGIN))), 5, n150,
                  designed="train_set")
        self._add("term_outside_set", "termination", self._displaced(base, one(18, 10 * td[18])), 5, n150,
                  designed="train_set")
        self._add("term_perbody_inside", "termination", self._displaced(base, one(20, td[20] * (1 - MARGIN))), 5, n150,
                  designed="train_set")
        self._add("term_perbody_beyond", "termination", self._displaced(base, one(1, td[1] * (1 + MARGIN))), 5, n150,
                  designed="train_set")
        for prog in (0, 1):
            b0 = self._tracked(n150, prog)
            self._add(f"term_beyond_prog{prog}", "termination", self._displaced(b0, one(7, td[7] * (1 + MARGIN))),
                      prog, n150, designed="train_set")
        ts = sets["train"].distances()
        self._add("term_scalar_beyond", "termination", self._displaced(base, one(23, ts[23] * (1 + MARGIN))), 5, n150,
                  designed="train")
        self._add("term_scalar_inside", "termination", self._displaced(base, one(23, ts[23] * (1 - MARGIN))), 5, n150,
                  designed="train")

        # ---- eval mode: the mean over the reset set against the first listed body's distance
        ev = np.array(_eval_bodies())
        inset = np.isin(np.arange(NB), ev)
        te = sets["eval"].distances()
        self._add("eval_above", "eval", self._displaced(base, np.where(inset, te[ev[0]] * (1 + MARGIN), 0.0)), 5, n150,
                  designed="eval")
        self._add("eval_below", "eval", self._displaced(base, np.where(inset, te[ev[0]] * (1 - MARGIN), 0.0)), 5, n150,
                  designed="eval")
        rest = (0.9 * te[ev[0]] * len(ev) - 5.0) / (len(ev) - 1)
        far = np.where(inset, rest, 0.0)
        far[ev[5]] = 5.0
        self._add("eval_far_body", "eval", self._displaced(base, far), 5, n150, designed="eval")
        self._add("eval_single_above", "eval", self._displaced(base, one(7, te[7] * (1 + MARGIN))), 5, n150,
                  designed="eval_single")
        self._add("eval_single_below", "eval", self._displaced(base, one(7, te[7] * (1 - MARGIN))), 5, n150,
                  designed="eval_single")
        self._add("eval_prog1", "eval", self._displaced(self._tracked(n150, 0), np.where(inset, 2.0, 0.0)), 0, n150,
                  designed="eval")

        # ---- power term
        self._add("power_prog3", "power", lambda: self._noisy(self._tracked(n17, 2)), 2, n17)
        self._add("power_prog4", "power", lambda: self._noisy(self._tracked(n17, 3)), 3, n17)
        fv, ff = rng.normal(0, 1.0, ND), rng.normal(0, 20.0, ND)
        fv[30:33], ff[30:33] = [-20.0, 15.0, 8.0], [300.0, -40.0, 25.0]
        self._add("power_dominant", "power", lambda: self._noisy(self._tracked(n17, 6)), 6, n17, dof_vel=fv, dof_force=ff)
        fv, ff = rng.normal(0, 1.0, ND), np.zeros(ND)
        ff[66:69] = [55.0, -70.0, 31.0]
        self._add("power_last_joint", "power", lambda: self._noisy(self._tracked(n17, 6)), 6, n17, dof_vel=fv, dof_force=ff)

        # ---- time
        ln = T.lengths[n37]
        self._add("time_step_before_end", "time", lambda: self._noisy(self._tracked(n37, 34)), 34, n37)
        s = self._start_for(n37, 3, ln)
        self._add("time_eq_len", "time", lambda: self._noisy(self._tracked(n37, 2, start=s)), 2, n37, start=s)
        s = self._start_for(n37, 3, np.nextafter(ln, F32(0)))
        self._add("time_ulp_below_len", "time", lambda: self._noisy(self._tracked(n37, 2, start=s)), 2, n37, start=s)
        self._add("time_past_end", "time", lambda: self._noisy(self._tracked(n37, 107)), 107, n37)
        self._add("time_start_offset", "time", lambda: self._noisy(self._tracked(n37, 9, start=0.1, soff=0.217)), 9, n37,
                  start=0.1, soff=0.217)
        self._add("time_2frame_inside", "time", lambda: self._noisy(self._tracked(n2, 0, start=-0.03)), 0, n2, start=-0.03)
        self._add("time_2frame_past", "time", lambda: self._noisy(self._tracked(n2, 4)), 4, n2)
        self._add("time_held", "time", lambda: self._noisy(self._tracked(held, 12, start=0.011)), 12, held, start=0.011)

        # ---- offsets and magnitude
        for nm, go in (("offset_pp", (50.0, 50.0, 0.0)), ("offset_nn", (-50.0, -50.0, 0.0))):
            self._add(nm, "offset", self._tracked(n150, 15, goff=go), 15, n150, goff=go)
        go = (50.0, -50.0, 0.0)
        self._add("offset_error", "offset", self._displaced(self._tracked(n150, 15, goff=go), np.full(NB, 0.2)), 15,
                  n150, goff=go)
        go = (-50.0, 50.0, 0.25)
        self._add("offset_pass_time", "offset", lambda: self._noisy(self._tracked(n37, 50, goff=go)), 50, n37, goff=go)

        # ---- saturation: every exponential underflows
        rb = np.array(self._tracked(n150, 8, goff=(3.0, -2.0, 0.5)), np.float64)
        rb[:, 0:3] += _unit(rng, NB) * 30.0
        rb[:, 7:13] += np.where(rng.random((NB, 6)) < 0.5, -100.0, 100.0)
        self._add("saturated", "saturation", self._rotated(rb, np.full(NB, np.pi - 1e-3)), 8, n150,
                  goff=(3.0, -2.0, 0.5))

    # ------------------------------------------------------------ resets
    def reset_state(self, sentinel=True):
        """The engine-side state a reset writes into, sentinel-filled where a reset must write."""
        n = self.n
        fill = (lambda shape, v: np.full(shape, v, F32)) if sentinel else (lambda shape, v: np.zeros(shape, F32))
        dof = fill((n, ND, 2), -5.0)
        dof[..., 1] = self.dof_vel  # the step of mode 1 reads the dof velocities here
        return dict(start_times=self.start_times.copy(), start_offsets=self.start_offsets.copy(),
                    global_offset=self.global_offset.copy(), progress=(self.progress_in + 1).astype(np.int16),
                    root_states=fill((n, 13), -3.0), dof_state=dof, dof_targets=fill((n, ND), -6.0),
                    rb_state=self.rb_state.copy(), contact_forces=fill((n, NB, 3), 7.0), obs=fill((n, 934), -8.0),
                    reset=np.ones(n, np.uint8), terminate=np.ones(n, np.uint8), init_root=self.init_root.copy())

    def reset_ids_and_draws(self, state_init):
        """Mode 2: two of every three envs in a seeded order, draws with the margins of the module
        docstring (a draw that misses one is drawn again)."""
        rng = np.random.default_rng(SEED + 2 + STATE_INITS.index(state_init))
        ids = rng.permutation(np.flatnonzero(np.arange(self.n) % 3 != 1)).astype(np.int32)
        u = np.zeros(len(ids), F32)
        for j, e in enumerate(ids):
            while True:
                u[j] = F32(rng.uniform(0, 1))
                if j % 5 == 0:
                    u[j] = F32(u[j] * 0.08)  # early starts: the AMP history reaches before time 0
                if draw_margin(self.tables, self.motion_ids[e], u[j], state_init) >= MARGIN:
                    break
        return ids, u

    def device_reset_step(self, reset_flags, seed=1234):
        """Mode 1: the first step index at which the hashed draws of every env in ``reset_flags`` keep
        the margins under all four state inits."""
        from oracle import oracle as O
        envs = np.flatnonzero(reset_flags)
        for step in range(1000):
            u = np.array([O.hash_uniform(seed, step, int(e)) for e in envs], F32)
            if all(draw_margin(self.tables, self.motion_ids[e], x, si) >= MARGIN for e, x in zip(envs, u)
                   for si in STATE_INITS):
                return seed, step, u
        raise AssertionError("no step index keeps the margins")


def draw_margin(tables, mid, u, state_init):
    """Distance of a reset draw from its decisions, in float64: the Hybrid probability and the
    integer steps of phase len / (1 / 30)."""
    p = 0.5
    m = np.inf
    ph = float(u)
    if state_init == "Hybrid":
        m = abs(float(u) - p)
        if float(u) >= p:
            return m
        ph = float(u) / p
    if state_init in ("Default", "Start"):
        return np.inf
    x = ph * float(tables.lengths[mid]) / R.CURR
    return min(m, abs(x - np.rint(x)))


# ---------------------------------------------------------------- bounds
RAW = ("raw_pos", "raw_rot", "raw_vel", "raw_ang", "raw_power")
BLOCKS = ("rew",) + RAW + tuple(R.OBS_BLOCKS)
RESET_BLOCKS = ("row_pos", "row_rot", "row_vel", "dof_vel")


def _angle_err(a):
    """Float32 error of the reward's angle 2 acos(w): w carries d = 4 roundings (the product's terms),
    acos turns that into min(2 d / sin(a / 2), 2 sqrt(2 d)); the wrap through sin / cos / atan2 adds
    8 roundings of the angle."""
    d = 4.0 * U
    with np.errstate(divide="ignore"):
        return np.minimum(2.0 * d / np.abs(np.sin(a / 2.0)), 2.0 * np.sqrt(2.0 * d)) + 8.0 * U * a


def _exp_floor(k, dist, ddist):
    return np.exp(-k * dist) * (k * ddist + U * k * dist + 2.0 * U) + 1e-37


def _heading_err(hl):
    """Heading angle: the rotated x axis carries 4 roundings of order 1, atan2 divides by the axis'
    horizontal length, the half-angle sine and cosine add 2."""
    return (4.0 / hl + 2.0) * U


def obs_floors(pos, rot, vel, ang, ref):
    """Float32 rounding model of the 11 observation blocks of each env, from operand magnitudes
    (nothing measured): P the largest coordinate, D / V / W the largest position / velocity / angular
    velocity vector involved, e_h the heading error."""
    pos, vel, ang = (np.asarray(x, np.float64) for x in (pos, vel, ang))
    nrm = lambda x: np.linalg.norm(x, axis=-1).max(-1)  # noqa: E731
    P = np.maximum(1.0, np.maximum(np.abs(pos).max((-1, -2)), np.abs(ref["rg_pos"]).max((-1, -2))))
    eh = _heading_err(R.heading(np.asarray(rot)[:, 0])[1])
    root = pos[:, :1]
    D = np.maximum.reduce([nrm(pos - root), nrm(ref["rg_pos"] - pos), nrm(ref["rg_pos"] - root)])
    V = np.maximum.reduce([nrm(vel), nrm(ref["body_vel"]), nrm(ref["body_vel"] - vel)])
    W = np.maximum.reduce([nrm(ang), nrm(ref["body_ang_vel"]), nrm(ref["body_ang_vel"] - ang)])
    fpos = 4.0 * U * P + (6.0 * U + eh) * D  # the sample's blend + offset, the difference, the rotation
    return {"self_h": U * P, "self_pos": fpos, "task_dpos": fpos, "task_rpos": fpos,
            "self_vel": (9.0 * U + eh) * V, "task_dvel": (9.0 * U + eh) * V,
            "self_ang": (9.0 * U + eh) * W, "task_dang": (9.0 * U + eh) * W,
            # one quaternion product is 4 roundings; the tangent / normal another 4
            "self_rot": 8.0 * U + eh, "task_rrot": 12.0 * U + eh, "task_drot": 20.0 * U + 2.0 * eh}


def step_floors(cs: CaseSet, p: R.Params, ref_out, idx=None):
    """floor(block) of every env for one parameter set: dict block -> [n]."""
    inp = cs.step_inputs(idx)
    pos, rot, vel, ang = R._split(inp["rb_state"])
    o, r = ref_out, ref_out["ref"]
    P = np.maximum(1.0, np.maximum(np.abs(pos).max((-1, -2)), np.abs(r["rg_pos"]).max((-1, -2))))
    V = np.maximum(np.abs(vel).max((-1, -2)), np.abs(r["body_vel"]).max((-1, -2)))
    W = np.maximum(np.abs(ang).max((-1, -2)), np.abs(r["body_ang_vel"]).max((-1, -2)))
    d = o["dist"]
    sq = lambda mag, x: 8.0 * U * (mag * np.sqrt(x) + x)  # noqa: E731  a mean square of differences of size mag
    th = R.reward_angle(r["rb_rot"], rot)
    ea = _angle_err(th)
    f = {"raw_pos": _exp_floor(p.k_pos, d["pos"], sq(P, d["pos"])),
         "raw_rot": _exp_floor(p.k_rot, d["rot"], (2.0 * th * ea + ea * ea).mean(-1) + 4.0 * U * d["rot"]),
         "raw_vel": _exp_floor(p.k_vel, d["vel"], sq(V, d["vel"])),
         "raw_ang": _exp_floor(p.k_ang_vel, d["ang"], sq(W, d["ang"])),
         "raw_power": 8.0 * U * np.abs(o["reward_raw"][:, 4]) + 1e-37}
    f["rew"] = (p.w_pos * f["raw_pos"] + p.w_rot * f["raw_rot"] + p.w_vel * f["raw_vel"] + p.w_ang_vel * f["raw_ang"]
                + f["raw_power"] + 2.0 * U * np.abs(o["rew"]))
    f.update(obs_floors(pos, rot, vel, ang, o["ref_obs"]))
    return f


def step_errors(got, ref_out):
    """max |got - reference| of every env per block: dict block -> [n]."""
    e = {"rew": np.abs(np.asarray(got["rew"], np.float64) - ref_out["rew"])}
    raw = np.abs(np.asarray(got["reward_raw"], np.float64) - ref_out["reward_raw"])
    for i, k in enumerate(RAW):
        e[k] = raw[:, i]
    ob = np.abs(np.asarray(got["obs"], np.float64) - ref_out["obs"])
    for k, (a, b) in R.OBS_BLOCKS.items():
        e[k] = ob[:, a:b].max(-1)
    return e


def family_max(cs: CaseSet, per_env, idx=None):
    fam = cs.family if idx is None else cs.family[idx]
    return {f: float(per_env[fam == f].max()) for f in sorted(set(fam))}


def bound(e_host_family, floor_env, family):
    """What the device is held to, per env: 3 max(e_host of the env's family, floor of the env)."""
    eh = np.array([e_host_family[f] for f in family])
    return 3.0 * np.maximum(eh, floor_env)


def row_floors(rows):
    """Float32 rounding of reset rows [n,24,13] (a sample written out): positions 4 roundings of the
    largest coordinate, rotations 4 roundings, velocities 4 roundings of the largest velocity."""
    rows = np.asarray(rows, np.float64)
    P = np.maximum(1.0, np.abs(rows[..., 0:3]).max((-1, -2)))
    V = np.maximum(1.0, np.abs(rows[..., 7:13]).max((-1, -2)))
    return {"row_pos": 4.0 * U * P, "row_rot": 4.0 * U * np.ones_like(P), "row_vel": 4.0 * U * V}


def row_errors(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    q = np.minimum(np.abs(got[..., 3:7] - ref[..., 3:7]).max(-1), np.abs(got[..., 3:7] + ref[..., 3:7]).max(-1))
    return {"row_pos": d[..., 0:3].max((-1, -2)), "row_rot": q.max(-1), "row_vel": d[..., 7:13].max((-1, -2))}


AMP_BLOCKS = {"amp_h": (0, 1), "amp_root_rot": (1, 7), "amp_root_vel": (7, 13), "amp_dof_rot": (13, 127),
              "amp_dof_vel": (127, 184), "amp_key_pos": (184, 196)}


def amp_floors(rows, coord=1.0):
    """Float32 rounding of AMP rows [n,S,196] from their own magnitudes (``coord``: the largest
    coordinate the key-body offsets are differences of); the joint rotations come
    from an exp map, whose angle 2 acos(w) costs 2 * 4 U / sin(angle / 2) (at most 2 sqrt(8 U))
    before it is turned back into a rotation, so the bound of that block is the float32 acos' own."""
    rows = np.asarray(rows, np.float64)
    mag = lambda a, b: np.maximum(1.0, np.abs(rows[..., a:b]).max(-1))  # noqa: E731
    eh = _heading_err(0.3)
    one = np.ones(rows.shape[:-1])
    tn = rows[..., 13:127].reshape(rows.shape[:-1] + (-1, 6))
    trace = tn[..., 0] + np.cross(tn[..., 3:6], tn[..., 0:3])[..., 1] + tn[..., 5]
    a = np.arccos(np.clip((trace - 1.0) / 2.0, -1.0, 1.0))  # the joints' angles, from the rows themselves
    with np.errstate(divide="ignore"):
        ea = (np.minimum(8.0 * U / np.abs(np.sin(a / 2.0)), 2.0 * np.sqrt(8.0 * U)) + 8.0 * U).max(-1)
    return {"amp_h": U * mag(0, 1), "amp_root_rot": (8.0 * U + eh) * one, "amp_root_vel": (9.0 * U + eh) * mag(7, 13),
            "amp_dof_rot": ea, "amp_dof_vel": 4.0 * U * mag(127, 184),
            "amp_key_pos": 4.0 * U * np.maximum(1.0, coord) + (6.0 * U + eh) * mag(184, 196)}


# ---------------------------------------------------------------- reference / oracle runs shared by the tests
STATE_KEYS = ("start_times", "start_offsets", "global_offset", "progress", "root_states", "dof_state", "dof_targets",
              "rb_state", "contact_forces", "obs", "reset", "terminate")


def oracle_tables(cs: CaseSet):
    from oracle import oracle as O
    return O.MotionTables.from_tables(cs.host_tables)


def oracle_step(cs: CaseSet, p: R.Params, idx=None, lib=None):
    from oracle import oracle as O
    i = cs.step_inputs(idx)
    return O.imitation_step(abi_params(p), oracle_tables(cs), i["rb_state"], i["dof_vel"], i["dof_force"],
                            i["progress_in"], i["motion_ids"], i["start_times"], i["start_offsets"], i["global_offset"])


def reference_reset(cs: CaseSet, state_init, mode, pname="train"):
    """The expected state after a reset launch. mode 2: he_reset_envs on reset_ids_and_draws; mode 1:
    he_imitation_reset_step = the step, then the reset of the envs it flags with the hashed draws.
    Returns (state, ids, draws, info, step outputs or None, (seed, step index) or None)."""
    p = with_init(PARAM_SETS[pname], state_init)
    st = cs.reset_state()
    if mode == 2:
        ids, u = cs.reset_ids_and_draws(state_init)
        out, info = R.reset(cs.tables, p, cs.model, ids, u, cs.motion_ids, st)
        return out, ids, u, info, None, None
    step = R.step(cs.tables, p, **cs.step_inputs())
    seed, index, u = cs.device_reset_step(step["reset"])
    ids = np.flatnonzero(step["reset"]).astype(np.int32)
    st["progress"] = step["progress"].astype(np.int16)
    st["obs"] = step["obs"]
    st["reset"], st["terminate"] = step["reset"].astype(np.uint8), step["terminate"].astype(np.uint8)
    out, info = R.reset(cs.tables, p, cs.model, ids, u, cs.motion_ids, st)
    # the step's flags are its outputs: the device reset does not clear them (the learner reads them)
    out["reset"], out["terminate"] = st["reset"], st["terminate"]
    return out, ids, u, info, step, (seed, index)


def oracle_reset(cs: CaseSet, state_init, mode, ids, u, pname="train"):
    from oracle import oracle as O
    p = with_init(PARAM_SETS[pname], state_init)
    st = cs.reset_state()
    if mode == 1:
        o = oracle_step(cs, p)
        st["progress"], st["obs"] = o["progress"].copy(), o["obs"].copy()
        flags = o["reset"].copy(), o["terminate"].copy()
    O.reset_envs(abi_params(p), oracle_tables(cs), np.asarray(ids, np.int32), np.asarray(u, F32), cs.motion_ids, st,
                 rest_pos=O.rest_positions(cs.model))
    if mode == 1:
        st["reset"], st["terminate"] = flags
    return st


def reset_errors(cs: CaseSet, got, ref, ids, info):
    """Errors and floors of the rows a reset writes, per reset env: dict block -> ([k] error, [k] floor).
    Exp-map dof positions and targets are left to cases.assert_expmap_close."""
    ids = np.asarray(ids)
    e = row_errors(np.asarray(got["rb_state"])[ids], ref["rb_state"][ids])
    f = row_floors(ref["rb_state"][ids])
    out = {k: (e[k], f[k]) for k in e}
    root = np.abs(np.asarray(got["root_states"], np.float64)[ids] - ref["root_states"][ids])
    root[:, 3:7] = 0.0  # the root row's rotation is the body row's, compared sign-free there
    out["root_row"] = (root.max(-1), np.maximum(f["row_pos"], f["row_vel"]))
    dv = np.abs(np.asarray(got["dof_state"], np.float64)[ids, :, 1] - ref["dof_state"][ids, :, 1]).max(-1)
    out["dof_vel"] = (dv, 4.0 * U * np.maximum(1.0, np.abs(ref["dof_state"][ids, :, 1]).max(-1)))
    pos, rot, vel, ang = R._split(ref["rb_state"][ids])
    fo = obs_floors(pos, rot, vel, ang, info["ref_obs"])
    ob = np.abs(np.asarray(got["obs"], np.float64)[ids] - ref["obs"][ids])
    for k, (a, b) in R.OBS_BLOCKS.items():
        out[k] = (ob[:, a:b].max(-1), fo[k])
    return out


def amp_reference(cs: CaseSet, ref_state, ids, S):
    """AMP history rows [k,S,196] of reference-state resets, and their float32 sample times."""
    p = PARAM_SETS["train"]
    ids = np.asarray(ids)
    return R.amp_history(cs.tables, p, cs.motion_ids[ids], ref_state["start_times"][ids], ref_state["rb_state"][ids],
                         ref_state["dof_state"][ids], S)


def amp_errors(got, ref, coord=1.0):
    d = np.abs(np.asarray(got, np.float64) - ref)
    f = amp_floors(ref, coord)
    return {k: (d[..., a:b].max(-1), f[k]) for k, (a, b) in AMP_BLOCKS.items()}


# ---------------------------------------------------------------- verdicts shared by the CPU and GPU tests
def _e_host(e_host, key, families):
    return {f: 0.0 for f in families} if e_host is None else e_host[key]


def step_failures(cs: CaseSet, p: R.Params, got, ref, e_host=None, idx=None, blocks=BLOCKS, envs=None):
    """(named case, check) pairs an imitation step fails: a flag or the progress unequal, or a block
    beyond 3 max(e_host of the family, floor of the env). ``e_host``: block -> family -> value (None:
    the floor alone, what the oracle itself is held to). ``envs``: a mask of the envs to judge."""
    names = cs.names if idx is None else [cs.names[i] for i in idx]
    fam = cs.family if idx is None else cs.family[idx]
    on = np.ones(len(names), bool) if envs is None else np.asarray(envs, bool)
    bad = set()
    for k in ("reset", "terminate", "progress"):
        if k in got:
            ne = np.asarray(got[k]).astype(np.int64) != np.asarray(ref[k]).astype(np.int64)
            bad |= {(names[i], k) for i in np.flatnonzero(ne & on)}
    fl, er = step_floors(cs, p, ref, idx), step_errors(got, ref)
    ratio = {}
    for k in blocks:
        b = bound(_e_host(e_host, k, cs.families()), fl[k], fam)
        bad |= {(names[i], k) for i in np.flatnonzero((er[k] > b) & on)}
        r = np.where(on, er[k] / b, 0.0)
        ratio[k] = (float(r.max()), names[int(r.argmax())])
    return bad, er, fl, ratio


def reset_failures(cs: CaseSet, got, ref, ids, info, mode, e_host=None):
    """(named case, check) pairs a reset launch fails: bookkeeping, flags, zeroed contact forces and
    offsets unequal anywhere; a state row or (mode 2) an observation of an env outside ``ids``
    changed; a written row or the post-reset observation beyond 3 max(e_host, floor); exp-map dof
    positions and targets beyond cases.expmap_tol."""
    import cases
    bad = set()
    ids = np.asarray(ids)
    fam = cs.family[ids]
    for k in ("start_times", "start_offsets", "global_offset", "progress", "contact_forces", "reset", "terminate"):
        a = np.asarray(got[k])
        b = np.asarray(ref[k]).astype(a.dtype)
        bad |= {(cs.names[i], k) for i in np.flatnonzero((a != b).reshape(cs.n, -1).any(-1))}
    keep = np.setdiff1d(np.arange(cs.n), ids)
    for k in ("root_states", "dof_state", "dof_targets", "rb_state") + (("obs",) if mode == 2 else ()):
        a, b = np.asarray(got[k])[keep], np.asarray(ref[k])[keep].astype(F32)
        bad |= {(cs.names[i], "untouched " + k) for i in keep[(a != b).reshape(len(keep), -1).any(-1)]}
    er = reset_errors(cs, got, ref, ids, info)
    ratio = {}
    for k, (e, f) in er.items():
        b = bound(_e_host(e_host, k, cs.families()), f, fam)
        bad |= {(cs.names[i], k) for i in ids[e > b]}
        ratio[k] = (float((e / b).max()), cs.names[int(ids[(e / b).argmax()])])
    for k, a, b in (("dof_pos", np.asarray(got["dof_state"])[ids, :, 0], ref["dof_state"][ids, :, 0]),
                    ("dof_targets", np.asarray(got["dof_targets"])[ids], ref["dof_targets"][ids])):
        bad |= {(cs.names[i], k) for i in ids[(np.abs(a - b) > cases.expmap_tol(b)).any(-1)]}
    return bad, er, ratio


def host_errors_by_family(cs: CaseSet, er, envs=None):
    """block -> family -> max error, from per-env errors (of ``envs``, default all)."""
    fam = cs.family if envs is None else cs.family[np.asarray(envs)]
    out = {}
    for k, v in er.items():
        e = v[0] if isinstance(v, tuple) else v
        out[k] = {f: float(e[fam == f].max()) if (fam == f).any() else 0.0 for f in cs.families()}
    return out
