"""The float64 imitation reference (tests/imitation_reference.py) pinned to the reference project's
own outputs, and the float32 C oracle (oracle/he_oracle.c) held to it on the adversarial case set
(tests/imitation_cases.py). CPU only.

Reference against the golden fixtures (written by the reference project itself), max |difference|
measured: GOLDEN_STEP and GOLDEN_RESET below; the bounds are 3 times these, the flags, progress and
start times are equal.

Oracle against the reference on the case set: per output block and case family e_host <= 3 floor,
floor the float32 rounding model of imitation_cases (nothing measured enters it). Measured worst
e_host / floor over all parameter sets: reward 0.06, raw terms 0.01-0.11, observation blocks
0.02-0.35 (task_rrot, power_prog4), reset rows 0.41 (row_rot), post-reset observation 0.46
(self_rot), AMP rows 0.41 (amp_h).

Discrimination (test_broken_oracle_fails_a_named_case): ten one-line breaks of a copy of
he_oracle.c outside the repository each fail a named case; the table is in the test.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import imitation_cases as C
import imitation_reference as R

# measured max |float64 reference - golden| per block (env_step.npz); bound = 3 x
GOLDEN_STEP = {"rew": 5.5e-7, "raw_pos": 3.2e-8, "raw_rot": 1.9e-6, "raw_vel": 2.9e-8, "raw_ang": 3.1e-8,
               "raw_power": 1.6e-7, "self_h": 1e-9, "self_pos": 2.4e-7, "self_rot": 6.2e-7, "self_vel": 7.3e-7,
               "self_ang": 4.8e-7, "task_dpos": 1.4e-7, "task_drot": 1.6e-6, "task_dvel": 4.6e-7, "task_dang": 3.6e-7,
               "task_rpos": 2.7e-7, "task_rrot": 8.9e-7}
# measured on env_reset.npz: rows (positions, sign-free rotations, velocities), dof velocity, observation
# (the resets land on frames of 30 fps clips, blend 0: velocities are the table's own, difference 0)
GOLDEN_RESET = {"row_pos": 5.6e-8, "row_rot": 1.3e-7, "row_vel": 0.0, "dof_vel": 0.0, "obs": 1.3e-6}


@pytest.fixture(scope="module")
def cs(model):
    return C.CaseSet(model)


def _golden_tables(g):
    from humanoid_amd.motion_lib import MotionTables
    return R.Tables(MotionTables(gts=g["gts"], grs=g["grs"], lrs=g["lrs"], gvs=g["gvs"], gavs=g["gavs"], dvs=g["dvs"],
                                 num_frames=g["num_frames"], length_starts=g["length_starts"],
                                 lengths=g["motion_lengths"], dt=g["motion_dt"], fps=1.0 / g["motion_dt"]))


# ------------------------------------------------------------ reference vs the reference project
def test_reference_step_matches_golden(golden):
    from humanoid_amd.body_sets import EVAL_BODIES, body_ids
    g = golden("env_step")
    t = _golden_tables(g)
    ins = (g["rb_state"], g["dof_vel"], g["dof_force"], g["progress_in"], g["motion_ids"], g["start_times"],
           g["start_offsets"], g["global_offset"])
    o = R.step(t, R.Params(), *ins)
    err = C.step_errors({"rew": g["rew"], "reward_raw": g["reward_raw"], "obs": g["obs"]}, o)
    print("golden step, measured: " + ", ".join(f"{k} {v.max():.2g}" for k, v in err.items()))
    for k, v in err.items():
        assert v.max() <= 3.0 * GOLDEN_STEP[k], f"{k}: {v.max():.3g} > 3 x {GOLDEN_STEP[k]:.3g}"
    np.testing.assert_array_equal(o["reset"], g["reset"])
    np.testing.assert_array_equal(o["terminate"], g["terminate"])
    np.testing.assert_array_equal(o["progress"], g["progress_out"])
    assert g["terminate"].any() and not g["terminate"].all()
    # the eval variant: the mean over EVAL_BODIES against 0.5 (humanoid_phc.py:1431-1437)
    pe = R.Params(eval_mode=True, termination_distance=[0.5] * 24, reset_body_ids=body_ids(EVAL_BODIES))
    oe = R.step(t, pe, *ins)
    np.testing.assert_array_equal(oe["reset"], g["reset_eval"])
    np.testing.assert_array_equal(oe["terminate"], g["terminate_eval"])


def test_reference_reset_matches_golden(golden, model):
    g, s = golden("env_reset"), golden("env_step")
    t = _golden_tables(s)
    n = g["root_states"].shape[0]
    state = dict(start_times=np.zeros(n, np.float32), start_offsets=np.zeros(n, np.float32),
                 global_offset=g["global_offset_in"], progress=np.full(n, 7, np.int16),
                 root_states=np.zeros((n, 13), np.float32), dof_state=np.zeros((n, 69, 2), np.float32),
                 dof_targets=np.zeros((n, 69), np.float32), rb_state=g["rb_state_in"],
                 contact_forces=np.ones((n, 24, 3), np.float32), obs=np.zeros((n, 934), np.float32),
                 reset=np.ones(n, np.uint8), terminate=np.ones(n, np.uint8))
    ids = g["env_ids"]
    out, info = R.reset(t, R.Params(), model, ids, g["phases"], np.arange(n), state)
    assert info["ref_init"].all()
    np.testing.assert_array_equal(out["start_times"][ids].astype(np.float32), g["start_times"][ids])
    np.testing.assert_allclose(out["start_times"][ids], info["time64"], rtol=2.0 ** -23, atol=0)
    np.testing.assert_array_equal(out["global_offset"], g["global_offset"])
    assert (out["progress"][ids] == 0).all() and (out["contact_forces"][ids] == 0).all()
    e = C.row_errors(g["rb_state"][ids], out["rb_state"][ids])
    e["dof_vel"] = np.abs(g["dof_vel"][ids] - out["dof_state"][ids, :, 1]).max(-1)
    e["obs"] = np.abs(g["obs"][ids] - out["obs"][ids]).max(-1)
    print("golden reset, measured: " + ", ".join(f"{k} {v.max():.2g}" for k, v in e.items()))
    for k, v in e.items():
        assert v.max() <= 3.0 * GOLDEN_RESET[k], f"{k}: {v.max():.3g} > 3 x {GOLDEN_RESET[k]:.3g}"
    np.testing.assert_allclose(out["root_states"][ids, :3], g["root_states"][ids, :3], atol=3 * GOLDEN_RESET["row_pos"])
    np.testing.assert_allclose(out["root_states"][ids, 7:], g["root_states"][ids, 7:], atol=3 * GOLDEN_RESET["row_vel"])
    cases.assert_expmap_close(out["dof_state"][ids, :, 0], g["dof_pos"][ids])
    cases.assert_expmap_close(out["dof_targets"][ids], g["dof_pos"][ids])


# ------------------------------------------------------------ the case set itself
def test_case_layout(cs):
    assert cs.n % 2 == 1 and cs.n % 8 != 0 and 100 <= cs.n <= 150
    assert len(set(cs.names[:cs.K])) == cs.K, "case names are unique"
    for name in set(cs.names):
        par = {i % 2 for i in cs.envs_of(name)}
        assert par == {0, 1}, f"{name} sits on one wave half only"
    perm = cs.permutation()
    assert sorted(perm) == list(range(cs.n))
    moved = np.arange(cs.n)[:-1]
    assert ((perm[moved] % 2) != (moved % 2)).all() and ((perm[moved] // 8) != (moved // 8)).all()
    assert set(cs.families()) == {"exact", "rotation", "heading", "termination", "eval", "power", "time", "offset",
                                  "saturation"}
    refs = {pn: cs.reference_step(pn) for pn in C.PARAM_SETS}
    # every margin holds in float64, under every parameter set
    for pn, r in refs.items():
        bad = np.flatnonzero(r["term_margin"] < C.MARGIN * (1 - 1e-3))
        assert bad.size == 0, f"{pn}: {[cs.names[i] for i in bad]} within the margin of a termination distance"
        assert (r["heading_len"] >= 0.3).all()
    for si in C.STATE_INITS:
        ids, u = cs.reset_ids_and_draws(si)
        assert {int(i) % 2 for i in ids} == {0, 1} and len(ids) < cs.n
        assert all(C.draw_margin(cs.tables, cs.motion_ids[e], x, si) >= C.MARGIN for e, x in zip(ids, u))
    # what each named case is for
    flag = lambda pn, name, key: {bool(refs[pn][key][i]) for i in cs.envs_of(name)}  # noqa: E731
    want = {("train_set", "term_beyond"): True, ("train_set", "term_inside"): False,
            ("train_set", "term_outside_set"): False, ("train_set", "term_perbody_inside"): False,
            ("train_set", "term_perbody_beyond"): True, ("train_set", "term_beyond_prog0"): False,
            ("train_set", "term_beyond_prog1"): True, ("train", "term_scalar_beyond"): True,
            ("train", "term_scalar_inside"): False, ("train", "term_outside_set"): True,
            ("eval", "eval_above"): True, ("eval", "eval_below"): False, ("eval", "eval_far_body"): False,
            ("eval", "eval_prog1"): False, ("eval_single", "eval_single_above"): True,
            ("eval_single", "eval_single_below"): False, ("train", "saturated"): True}
    for (pn, name), v in want.items():
        assert flag(pn, name, "terminate") == {v}, (pn, name)
    assert not refs["eval_empty"]["terminate"].any()
    tr = refs["train"]
    for name, v in (("time_step_before_end", False), ("time_eq_len", True), ("time_ulp_below_len", False),
                    ("time_past_end", True), ("time_2frame_inside", False), ("time_2frame_past", True),
                    ("offset_pass_time", True)):
        assert flag("train", name, "reset") == {v} and flag("train", name, "terminate") == {False}, name
    i = cs.envs_of("time_eq_len")[0]
    ln = cs.tables.lengths[cs.motion_ids[i]]
    assert tr["t"][i] == ln and tr["t"][cs.envs_of("time_ulp_below_len")[0]] == np.nextafter(ln, np.float32(0))
    i = cs.envs_of("time_step_before_end")[0]
    assert tr["t"][i] < ln <= tr["t_obs"][i]  # the t + dt sample clamps to the last frame
    i = cs.envs_of("exact_frame")[0]
    assert R.IR.frame_select(cs.tables, cs.motion_ids[[i]], tr["t"][[i]])[2][0] == 0
    # exact tracking: no geodesic error, raw terms 1 minus their bound. The rotation term is 1 only
    # where the sample's quaternion has unit norm (the held clip): elsewhere the float32 slerp's norm
    # defect is an angle to the reference project's 2 acos(w), and the reference carries it.
    fl = C.step_floors(cs, C.PARAM_SETS["train"], tr)
    for i in np.flatnonzero(cs.family == "exact"):
        assert tr["theta"][i].max() < 1e-6, cs.names[i]
        for c, k in ((0, "raw_pos"), (2, "raw_vel"), (3, "raw_ang")):
            assert tr["reward_raw"][i, c] >= 1.0 - 3.0 * fl[k][i], (cs.names[i], k)
        if cs.names[i].startswith("exact_held"):
            assert tr["reward_raw"][i, 1] >= 1.0 - 3.0 * fl["raw_rot"][i]
    # power gate, saturation
    assert flag("train", "power_prog3", "progress") == {True} and tr["progress"][cs.envs_of("power_prog3")[0]] == 3
    assert tr["reward_raw"][cs.envs_of("power_prog3")[0], 4] == 0 and tr["reward_raw"][cs.envs_of("power_prog4")[0], 4] < 0
    assert (refs["nopower"]["reward_raw"][:, 4] == 0).all()
    i = cs.envs_of("power_last_joint")[0]
    assert np.abs(cs.dof_force[i, :66]).max() == 0 and tr["reward_raw"][i, 4] < -0.01
    i = cs.envs_of("saturated")[0]
    assert (tr["reward_raw"][i, :4] < 1e-38).all() and abs(tr["rew"][i] - tr["reward_raw"][i, 4]) < 1e-38


# ------------------------------------------------------------ oracle vs reference
@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_oracle_step_matches_reference(cs, pname):
    p = C.PARAM_SETS[pname]
    ref, got = cs.reference_step(pname), C.oracle_step(cs, p)
    bad, er, fl, _ = C.step_failures(cs, p, got, ref)
    worst = {k: max(C.family_max(cs, er[k] / fl[k]).items(), key=lambda kv: kv[1]) for k in C.BLOCKS}
    print(f"{pname}: e_host / floor, worst family: " + ", ".join(f"{k} {v:.2g} ({f})" for k, (f, v) in worst.items()))
    print(f"{pname}: e_host: " + ", ".join(f"{k} {er[k].max():.2g}" for k in C.BLOCKS))
    print(f"{pname}: floor (smallest, largest env): " + ", ".join(f"{k} {fl[k].min():.2g}..{fl[k].max():.2g}" for k in C.BLOCKS))
    assert not bad, f"{pname}: {sorted(bad)}"
    # the negated twins: the same rotations, so the same outputs within the same bound
    for name in [x for x in set(cs.names) if x.endswith("_neg")]:
        a, b = cs.envs_of(name)[0], cs.envs_of(name[:-4])[0]
        assert abs(float(got["rew"][a]) - float(got["rew"][b])) <= 3.0 * fl["rew"][a]
        d = np.abs(got["obs"][a].astype(np.float64) - got["obs"][b])
        for k, (lo, hi) in R.OBS_BLOCKS.items():
            assert d[lo:hi].max() <= 3.0 * fl[k][a], (name, k)


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("state_init", C.STATE_INITS)
def test_oracle_reset_matches_reference(cs, state_init, mode):
    ref, ids, u, info, step, _ = C.reference_reset(cs, state_init, mode)
    got = C.oracle_reset(cs, state_init, mode, ids, u)
    bad, er, _ = C.reset_failures(cs, got, ref, ids, info, mode)
    print(f"mode {mode} {state_init}: e_host / floor: " + ", ".join(f"{k} {(e / f).max():.2g}" for k, (e, f) in er.items()))
    assert not bad, sorted(bad)
    k = info["ref_init"]
    np.testing.assert_allclose(ref["start_times"][ids][k], info["time64"][k], rtol=2.0 ** -23, atol=0)
    if state_init == "Hybrid":
        assert 0 < k.sum() < len(ids), "both kinds of init occur"
    if mode == 1:  # resets by pass-time and by falling, and one that reads a non-zero offset
        assert (step["reset"] & ~step["terminate"]).any() and step["terminate"].any()
        assert np.abs(cs.global_offset[ids]).max() == 50.0


def test_oracle_amp_history_matches_reference(cs):
    from oracle import oracle as O
    S = 10
    ref, ids, u, info, _, _ = C.reference_reset(cs, "Random", 2)
    got = C.oracle_reset(cs, "Random", 2, ids, u)
    rows, t, coord = C.amp_reference(cs, ref, ids, S)
    assert (t < 0).sum() > 20 and (ref["start_times"][ids] < (S - 1) / 30.0).sum() >= 6
    buf = np.zeros((cs.n, S, 196), np.float32)
    b, _ = O.amp_init(buf, buf, ids, got["rb_state"], got["dof_state"], C.oracle_tables(cs), cs.motion_ids,
                      got["start_times"], 1 / 30)
    er = C.amp_errors(b[ids], rows, coord)
    print("AMP: e_host / floor: " + ", ".join(f"{k} {(e / f).max():.2g}" for k, (e, f) in er.items()))
    for k, (e, f) in er.items():
        assert (e <= 3.0 * f).all(), k


# ------------------------------------------------------------ discrimination
# (break, old text, new text, a named case it must fail). Every break failed these, measured:
#   prog_ge_1        term_beyond_prog0 (terminate, reset), eval_prog1
#   power_lt_3       power_prog3 (raw_power, rew)
#   pass_time_gt     time_eq_len (reset)
#   no_reset_mask    term_outside_set (terminate)
#   eval_dist_0      eval_single_below (terminate)
#   eval_div_24      eval_above (terminate)
#   slerp_no_flip    exact_blend (raw terms, observation)
#   obs_sample_t     every moving case (task blocks), e.g. time_start_offset
#   hq_negated       head_+90_tilt0 (task_drot)
#   offset_after_zero offset_pass_time (row_pos of the reset)
BREAKS = [
    ("prog_ge_1", "fallen = fallen && prog > 1;", "fallen = fallen && prog >= 1;", "term_beyond_prog0"),
    ("power_lt_3", "if (prog <= 3) pr = 0;", "if (prog < 3) pr = 0;", "power_prog3"),
    ("pass_time_gt", "int pass_time = t >= M->lengths[mid];", "int pass_time = t > M->lengths[mid];", "time_eq_len"),
    ("no_reset_mask", "for (int j = 0; j < NB; ++j) if (p->reset_body_mask >> j & 1) {\n"
     "                R d[3]; v3_sub(s.pos[j], m.pos[j], d);\n                if (v3_norm(d)",
     "for (int j = 0; j < NB; ++j) if (1) {\n"
     "                R d[3]; v3_sub(s.pos[j], m.pos[j], d);\n                if (v3_norm(d)", "term_outside_set"),
    ("eval_dist_0", "if (td < 0) td = p->term_dist[j];", "td = p->term_dist[0];", "eval_single_below"),
    ("eval_div_24", "fallen = cnt > 0 && (sum / cnt) > td;", "fallen = cnt > 0 && (sum / 24) > td;", "eval_above"),
    ("slerp_no_flip", "q1[i] = cf < 0.0f ? -q1f[i] : q1f[i];", "q1[i] = q1f[i];", "exact_blend"),
    ("obs_sample_t", "float t2 = env_time(prog + 1, p->control_dt, start_times[i], start_offsets[i]);",
     "float t2 = env_time(prog, p->control_dt, start_times[i], start_offsets[i]);", "time_start_offset"),
    ("hq_negated", "heading_quat(h, hq);", "heading_quat(-h, hq);", "head_+90_tilt0"),
    ("offset_after_zero", "motion_eval(M, mid, t, global_offset + 3 * e, 1, &m);",
     "global_offset[3 * e] = global_offset[3 * e + 1] = global_offset[3 * e + 2] = 0.0f; "
     "motion_eval(M, mid, t, global_offset + 3 * e, 1, &m);", "offset_pass_time"),
]


def _build_variant(tmp, name, old, new):
    """A broken copy of he_oracle.c compiled outside the repository."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "oracle", "he_oracle.c")).read()
    assert old in src, f"{name}: the oracle's text moved"
    d = os.path.join(tmp, name, "oracle")
    os.makedirs(d)
    shutil.copytree(os.path.join(root, "include"), os.path.join(tmp, name, "include"))
    with open(os.path.join(d, "he_oracle.c"), "w") as f:
        f.write(src.replace(old, new))
    so = os.path.join(d, "libvariant.so")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-fPIC", "-fopenmp", "-ffp-contract=off", "-std=gnu11", "-shared",
                    "-o", so, os.path.join(d, "he_oracle.c"), "-lm"], check=True, capture_output=True)
    lib = ctypes.CDLL(so)
    lib.ho_hash_uniform.restype = ctypes.c_float
    lib.ho_hash_uniform.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.ho_sample_time_interval.restype = ctypes.c_float
    lib.ho_sample_time_interval.argtypes = [ctypes.c_float, ctypes.c_float]
    return lib


@pytest.fixture(scope="module")
def expected(cs):
    """What the sound oracle is compared with: the reference's outputs of every launch."""
    steps = {pn: cs.reference_step(pn) for pn in C.PARAM_SETS}
    resets = {(si, m): C.reference_reset(cs, si, m) for si in ("Random", "Hybrid") for m in (2, 1)}
    return steps, resets


@pytest.mark.parametrize("name,old,new,must_fail", BREAKS, ids=[b[0] for b in BREAKS])
def test_broken_oracle_fails_a_named_case(cs, expected, tmp_path, monkeypatch, name, old, new, must_fail):
    from oracle import oracle as O
    O.lib()
    monkeypatch.setattr(O, "_lib", _build_variant(str(tmp_path), name, old, new))
    steps, resets = expected
    failed = set()
    for pn, ref in steps.items():
        bad = C.step_failures(cs, C.PARAM_SETS[pn], C.oracle_step(cs, C.PARAM_SETS[pn]), ref)[0]
        failed |= {(pn,) + b for b in bad}
    for (si, mode), (ref, ids, u, info, _, _) in resets.items():
        bad = C.reset_failures(cs, C.oracle_reset(cs, si, mode, ids, u), ref, ids, info, mode)[0]
        failed |= {(f"reset{mode}_{si}",) + b for b in bad}
    names = {f[1] for f in failed}
    print(f"{name}: fails {len(failed)} checks on {len(names)} cases, e.g. {sorted(failed)[:6]}")
    assert must_fail in names, f"{name} passes {must_fail}: a case is missing"
