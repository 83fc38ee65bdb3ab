"""The imitation kernel (csrc/he_imitation.hip, he_imitation_env.h, he_math.h) against the independent
float64 reference (tests/imitation_reference.py) on the adversarial case set (tests/imitation_cases.py):
135 envs, every named case on both 32-lane halves of a wave, a half-filled last wave.

Flags, progress, start times, offsets and the Hybrid choice are equal on every env. Reward, raw terms,
observation blocks, reset rows and AMP rows are held, per block and env, to 3 max(e_host, floor):
e_host the C oracle's error against the same reference per case family, computed on the CPU in the
same run, floor the float32 rounding model of imitation_cases. No number of the kernel's own enters.

Measured on an MI355X, device error / bound of the worst case (the bound is 1): reward 0.033
(head_-90_tilt0.6; 0.048 rot_spin with the power term off), raw pos / rot / vel / ang / power 0.006 /
0.028 / 0.032 / 0.043 / 0.044, self pos / rot / vel / ang 0.052 / 0.13 (exact_frame) / 0.044 / 0.07, task
dpos / drot / dvel / dang / rpos / rrot 0.033 / 0.12 / 0.032 / 0.032 / 0.045 / 0.15 (rot_mixed); reset rows
pos / rot / vel 0.096 / 0.11 / 0.064, post-reset observation 0.19 (self_rot, head_-pi_tilt0); AMP rows
0.14 (amp_h, offset_pass_time row 0).
"""
import numpy as np
import pytest

from humanoid_amd import _abi

import imitation_cases as C
import imitation_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S_AMP = 10


def _cu(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def cs(model):
    return C.CaseSet(model)


@pytest.fixture(scope="module")
def host_steps(cs):
    """Per parameter set: the reference's outputs and e_host (block -> family -> the oracle's error)."""
    out = {}
    for pn, p in C.PARAM_SETS.items():
        ref = cs.reference_step(pn)
        out[pn] = (ref, C.host_errors_by_family(cs, C.step_errors(C.oracle_step(cs, p), ref)))
    return out


class Launch:
    """An engine over the case set's library with the envs ``idx`` of the set loaded."""

    def __init__(self, he_model, cs, idx=None, sentinel=False, amp=False):
        from humanoid_amd.engine import Engine
        if not torch.cuda.is_available():
            pytest.fail("GPU test run without a visible GPU")
        self.cs = cs
        self.idx = np.arange(cs.n) if idx is None else np.asarray(idx)
        self.n = n = len(self.idx)
        self.eng = eng = Engine(he_model, n, device=0, sim_params=_abi.default_sim_params())
        eng.load_motions(cs.host_tables)
        self.amp = None
        if amp:
            self.amp = (torch.full((n, S_AMP, 196), -9.0, device="cuda:0"), torch.full((n, S_AMP, 196), -9.0, device="cuda:0"))
            eng.set_amp(*self.amp)
        self.load(sentinel)

    def load(self, sentinel=False, motion_ids=None):
        cs, eng, n, i = self.cs, self.eng, self.n, self.idx
        st = cs.reset_state()
        eng.rb_state.copy_(_cu(cs.rb_state[i].reshape(n * 24, 13)))
        if sentinel:
            eng.root_states.copy_(_cu(st["root_states"][i]))
            eng.dof_targets.copy_(_cu(st["dof_targets"][i]).view(eng.dof_targets.shape))
            eng.contact_forces.copy_(_cu(st["contact_forces"][i].reshape(n * 24, 3)))
            eng.initial_root_states.copy_(_cu(st["init_root"][i]))
        eng.dof_state.copy_(_cu(st["dof_state"][i].reshape(n * 69, 2)))
        eng.dof_force.copy_(_cu(cs.dof_force[i].reshape(-1)))
        mids = cs.motion_ids[i] if motion_ids is None else motion_ids
        self.book = dict(motion_ids=_cu(mids, torch.int64), start_times=_cu(cs.start_times[i]),
                         start_offsets=_cu(cs.start_offsets[i]), global_offset=_cu(cs.global_offset[i]),
                         progress=_cu(cs.progress_in[i], torch.int16))
        self.em = eng.env_motion(*[self.book[k] for k in ("motion_ids", "start_times", "start_offsets", "global_offset",
                                                          "progress")])
        fill = -8.0 if sentinel else 0.0
        one = 1 if sentinel else 0
        self.out = dict(obs=torch.full((n, 934), fill, device="cuda:0"), rew=torch.zeros(n, device="cuda:0"),
                        reward_raw=torch.zeros(n, 5, device="cuda:0"),
                        reset=torch.full((n,), one, dtype=torch.uint8, device="cuda:0"),
                        terminate=torch.full((n,), one, dtype=torch.uint8, device="cuda:0"))

    def _outs(self):
        o = self.out
        return o["obs"], o["rew"], o["reward_raw"], o["reset"], o["terminate"]

    def step(self, p):
        self.eng.imitation_step(C.abi_params(p), self.em, *self._outs())
        return self.results()

    def reset_step(self, p, seed, index):
        self.eng.imitation_reset_step(C.abi_params(p), self.em, *self._outs(), seed=seed, step_index=index)
        return self.results()

    def reset_envs(self, p, ids, draws):
        self.book["progress"].copy_(_cu(self.cs.progress_in[self.idx] + 1, torch.int16))  # as after a step
        o = self.out
        self.eng.reset_envs(C.abi_params(p), self.em, _cu(ids, torch.int32), _cu(np.asarray(draws, np.float32)), o["obs"],
                            o["reset"], o["terminate"])
        return self.results()

    def results(self):
        torch.cuda.synchronize()
        eng, n = self.eng, self.n
        r = {k: v.cpu().numpy() for k, v in self.out.items()}
        r.update({k: v.cpu().numpy() for k, v in self.book.items()})
        r.update(root_states=eng.root_states.cpu().numpy().copy(), dof_state=eng.dof_state.view(n, 69, 2).cpu().numpy().copy(),
                 dof_targets=eng.dof_targets.view(n, 69).cpu().numpy().copy(),
                 rb_state=eng.rb_state.view(n, 24, 13).cpu().numpy().copy(),
                 contact_forces=eng.contact_forces.view(n, 24, 3).cpu().numpy().copy())
        if self.amp:
            r["amp"], r["amp_demo"] = self.amp[0].cpu().numpy(), self.amp[1].cpu().numpy()
        return r


def _report(what, ratio):
    print(f"{what}: device error / bound (the bound is 3 max(e_host, floor)), worst case: "
          + ", ".join(f"{k} {v:.2g} ({name})" for k, (v, name) in ratio.items()))


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_imitation_step_matches_reference(he_model, cs, host_steps, pname):
    p = C.PARAM_SETS[pname]
    ref, e_host = host_steps[pname]
    got = Launch(he_model, cs).step(p)
    bad, er, fl, ratio = C.step_failures(cs, p, got, ref, e_host)
    _report(pname, ratio)
    assert not bad, f"{pname}: {sorted(bad)}"
    # exact tracking: raw terms 1 minus their bound (the rotation term on the held clip, where the
    # sample's quaternion has unit norm; elsewhere the reference carries the float32 slerp's norm)
    for i in np.flatnonzero(cs.family == "exact"):
        for c, k in ((0, "raw_pos"), (2, "raw_vel"), (3, "raw_ang")) + (((1, "raw_rot"),) if "held" in cs.names[i] else ()):
            assert got["reward_raw"][i, c] >= 1.0 - C.bound(e_host[k], fl[k], cs.family)[i], (cs.names[i], k)
    # the negated twins: the same rotations
    for name in [x for x in set(cs.names) if x.endswith("_neg")]:
        for a, b in zip(cs.envs_of(name), cs.envs_of(name[:-4])):
            assert abs(float(got["rew"][a]) - float(got["rew"][b])) <= C.bound(e_host["rew"], fl["rew"], cs.family)[a]
            d = np.abs(got["obs"][a].astype(np.float64) - got["obs"][b])
            for k, (lo, hi) in R.OBS_BLOCKS.items():
                assert d[lo:hi].max() <= C.bound(e_host[k], fl[k], cs.family)[a], (name, k)
    # saturation: the flags stay defined, the reward is the power term alone
    for i in cs.envs_of("saturated"):
        assert np.isfinite(got["rew"][i]) and np.isfinite(got["obs"][i]).all() and got["reset"][i] in (0, 1)
        assert abs(float(got["rew"][i]) - float(got["reward_raw"][i, 4])) <= 3.0 * fl["rew"][i]
    if pname == "eval_empty":
        assert not got["terminate"].any()


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("state_init", C.STATE_INITS)
def test_resets_match_reference(he_model, cs, state_init, mode):
    ref, ids, u, info, step, key = C.reference_reset(cs, state_init, mode)
    host = C.oracle_reset(cs, state_init, mode, ids, u)
    e_host = C.host_errors_by_family(cs, C.reset_errors(cs, host, ref, ids, info), ids)
    p = C.with_init(C.PARAM_SETS["train"], state_init)
    lz = Launch(he_model, cs, sentinel=True)
    got = lz.reset_envs(p, ids, u) if mode == 2 else lz.reset_step(p, *key)
    bad, er, ratio = C.reset_failures(cs, got, ref, ids, info, mode, e_host)
    _report(f"mode {mode} {state_init}", ratio)
    assert not bad, sorted(bad)
    if mode == 1:  # the step's own outputs: reward and raw terms everywhere, observation where no reset followed
        e_step = C.host_errors_by_family(cs, C.step_errors(C.oracle_step(cs, p), step))
        raw = C.step_failures(cs, p, got, step, e_step, blocks=("rew",) + C.RAW)[0]
        obs = C.step_failures(cs, p, {k: got[k] for k in ("rew", "reward_raw", "obs")}, step, e_step,
                              blocks=tuple(R.OBS_BLOCKS), envs=~step["reset"])[0]
        raw = {b for b in raw if b[1] != "progress"}  # a reset env's progress is 0, checked above
        assert not raw and not obs, sorted(raw | obs)


@pytest.mark.parametrize("pname", ["train", "eval"])
def test_results_independent_of_wave_half_and_position(he_model, cs, pname):
    """The set moved so that every case changes parity (the other 32-lane half of its wave) and block:
    each case's outputs are the same bits."""
    p = C.PARAM_SETS[pname]
    perm = cs.permutation()
    a = Launch(he_model, cs).step(p)
    b = Launch(he_model, cs, idx=perm).step(p)
    for k in ("obs", "rew", "reward_raw", "reset", "terminate", "progress"):
        ne = (a[k][perm] != b[k]).reshape(cs.n, -1).any(-1)
        assert not ne.any(), f"{k}: {[cs.names[i] for i in perm[ne]]} differ after the move"


def test_metadata_cache_is_keyed_by_motion_id(he_model, cs):
    """A launch on a fresh engine, and the same launch on an engine whose per-env motion metadata was
    cached by a prior step with another motion id in every env: the same bits."""
    p = C.PARAM_SETS["train"]
    want = Launch(he_model, cs).step(p)
    lz = Launch(he_model, cs)
    m = len(cs.host_tables.num_frames)
    other = (cs.motion_ids + 1 + np.arange(cs.n) % (m - 1)) % m
    assert (other != cs.motion_ids).all()
    lz.load(motion_ids=other)
    lz.step(p)
    lz.load()
    got = lz.step(p)
    for k in ("obs", "rew", "reward_raw", "reset", "terminate", "progress"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_amp_history_before_time_zero(he_model, cs):
    """he_set_amp with S = 10, then a reset of envs whose start time is below (S - 1) dt: history
    rows sample t - k dt < 0 and clamp to time 0. All 196 floats of every row against the float64
    AMP row (common.py:179-267); envs outside env_ids keep their buffers."""
    from oracle import oracle as O
    ref, ids, u, info, _, _ = C.reference_reset(cs, "Random", 2)
    rows, t, coord = C.amp_reference(cs, ref, ids, S_AMP)
    assert (t < 0).sum() > 20
    host = C.oracle_reset(cs, "Random", 2, ids, u)
    zero = np.zeros((cs.n, S_AMP, 196), np.float32)
    hb, _ = O.amp_init(zero, zero, ids, host["rb_state"], host["dof_state"], C.oracle_tables(cs), cs.motion_ids,
                       host["start_times"], 1 / 30)
    e_host = {k: float(e.max()) for k, (e, f) in C.amp_errors(hb[ids], rows, coord).items()}
    lz = Launch(he_model, cs, sentinel=True, amp=True)
    got = lz.reset_envs(C.with_init(C.PARAM_SETS["train"], "Random"), ids, u)
    np.testing.assert_array_equal(got["start_times"], ref["start_times"].astype(np.float32))
    er = C.amp_errors(got["amp"][ids], rows, coord)
    ratio = {}
    for k, (e, f) in er.items():
        b = 3.0 * np.maximum(e_host[k], f)
        j = np.unravel_index((e / b).argmax(), e.shape)
        ratio[k] = (float((e / b).max()), f"{cs.names[int(ids[j[0]])]} row {j[1]}")
    _report("AMP history", ratio)
    for k, (v, where) in ratio.items():
        assert v <= 1.0, f"{k}: {v:.3g} of the bound at {where}"
    np.testing.assert_array_equal(got["amp_demo"][ids], got["amp"][ids])
    keep = np.setdiff1d(np.arange(cs.n), ids)
    assert (got["amp"][keep] == -9.0).all() and (got["amp_demo"][keep] == -9.0).all()
