"""The float64 ingestion reference (tests/ingest_reference.py) pinned to the reference project's own
tables, and the float32 host restatement (motion_lib.clip_to_motion, MotionLibSMPL metadata) held
to it on the adversarial clip set (tests/ingest_cases.py). CPU only.

Reference against the golden tables (tests/golden/motion_lib.npz, written by the reference project
from the raw clips stored beside them), max |difference| measured over the 7 motions:
gts 5.7e-7, gvs 1.1e-5, gavs 3.4e-3, dvs 5.6e-5 (the float32 torch path's rounding; gavs is its
float32 acos near 1). The bounds are 3 times these.

Host restatement against the reference: bounds from the number format (ingest_cases.host_bounds),
measured at most 0.11 of the bound on positions, 0.13 on linear velocity, 0.27 on angular velocity
and 0.41 on dof velocity. With fps truncated to an integer (59.94 read as 59) the 150-frame clip is
off by 0.075 m/s, 0.12 rad/s and 0.061 rad/s against bounds of 3.1e-4, 7.7e-2 and 2.4e-4.
"""
import numpy as np
import pytest

import ingest_cases as IC
import ingest_reference as IR

GOLDEN_BOUND = IC.GOLDEN_BOUND
golden_clips = IC.golden_clips


@pytest.fixture(scope="module")
def libs(model):
    return IC.libraries(model)


@pytest.fixture(scope="module")
def refs(model, libs):
    return {name: [IR.ingest(model, c) for c in clips] for name, clips in libs.items()}


def test_reference_matches_golden_tables(golden, model):
    g = golden("motion_lib")
    t = IR.Tables(model, golden_clips(g), g["sample_idxes"])
    np.testing.assert_array_equal(t.num_frames, g["num_frames"])
    np.testing.assert_array_equal(t.length_starts[:5], g["length_starts"][:5])
    np.testing.assert_array_equal(t.lengths, g["motion_lengths"])
    np.testing.assert_array_equal(t.dt, g["motion_dt"])
    for m, (s, n, c) in enumerate(zip(g["length_starts"], g["num_frames"], g["sample_idxes"])):
        r = t.clips[c]
        for k, bound in GOLDEN_BOUND.items():
            err = np.abs(r[k] - g[k][s:s + n]).max()
            assert err <= bound, f"motion {m} (clip {c}) {k}: {err:.3g} > {bound:.3g}"
        np.testing.assert_array_equal(r["grs"], g["grs"][s:s + n])
        lr = g["lrs"][s:s + n]
        assert np.minimum(np.abs(r["lrs"] - lr), np.abs(r["lrs"] + lr)).max() <= 1e-6


def test_reference_sampling_matches_golden(golden, model):
    """The sampler half: the reference's motion_state of its own tables against the reference
    project's get_motion_state, at the golden tests' sampling tolerances on top of the table bounds."""
    import cases
    g = golden("motion_lib")
    t = IR.Tables(model, golden_clips(g), g["sample_idxes"])
    r = IR.motion_state(t, g["q_ids"], g["q_times"], g["q_offset"])
    for k, tab, tol in (("rg_pos", "gts", 2e-6), ("body_vel", "gvs", 1e-5), ("body_ang_vel", "gavs", 1e-5),
                        ("dof_vel", "dvs", 1e-5)):
        np.testing.assert_allclose(r[k], g["ms_" + k], rtol=0, atol=GOLDEN_BOUND[tab] + tol, err_msg=k)
    x, y = r["rb_rot"], g["ms_rb_rot"]
    assert np.minimum(np.abs(x - y).max(-1), np.abs(x + y).max(-1)).max() <= 5e-6
    cases.assert_expmap_close(r["dof_pos"], g["ms_dof_pos"])


def test_case_set_layout(libs, refs):
    """The properties the adversarial set is built for."""
    total = 0
    for name, clips in libs.items():
        st, n = IC.starts(clips)
        total += n
        assert n % 8 != 0, name
        assert set(int(s) % 8 for s in st) == set(range(8)), name
        assert {float(c["fps"]) for c in clips} == {float(f) for f in IC.FPS}, name
    assert total < 1000
    assert sorted(len(c["pose_quat_global"]) for c in libs["mixed"])[:2] == [2, 3]
    assert {2, 3, 8, 9, 16, 17, 37, 150} <= {len(c["pose_quat_global"]) for c in libs["mixed"]}
    assert len(libs["many"]) == 70 and {len(c["pose_quat_global"]) for c in libs["many"]} == set(range(2, 10))
    i = {n: IC.mixed_index(n) for n in ("n37", "flip", "spin", "held")}
    q, qf = libs["mixed"][i["n37"]]["pose_quat_global"], libs["mixed"][i["flip"]]["pose_quat_global"]
    flipped = (q != qf).any(-1)
    assert 0.3 < flipped.mean() < 0.7 and np.array_equal(np.where(flipped[..., None], -qf, qf), q)
    # the held pose: not the identity, and exactly no raw angular or dof velocity inside it
    held = refs["mixed"][i["held"]]
    inside = slice(IC.HELD.start, IC.HELD.stop - 1)
    assert np.abs(held["raw_gavs"][inside]).max() < 1e-12 and np.abs(held["dvs"][inside]).max() < 1e-12
    assert np.abs(held["raw_gavs"][IC.HELD.stop - 1]).max() > 0.1
    assert np.abs(held["lrs"][IC.HELD.start, 1:, :3]).max() > 0.05
    # the spin: 2.5 rad per frame about z on top of the clip's own motion
    spin = refs["mixed"][i["spin"]]
    np.testing.assert_allclose(spin["raw_gavs"][:-1, 0, 2], IC.SPIN_STEP * 30.0, rtol=0.02)
    np.testing.assert_allclose(spin["dvs"], refs["mixed"][i["n37"]]["dvs"], atol=1e-3)


@pytest.mark.parametrize("lib", ["mixed", "many"])
def test_host_restatement_matches_reference(model, libs, refs, lib):
    worst = {k: 0.0 for k in IC.CHANNELS}
    for i, (clip, ref) in enumerate(zip(libs[lib], refs[lib])):
        err, bound = IC.host_errors(model, clip, ref), IC.host_bounds(ref)
        for k in IC.CHANNELS:
            worst[k] = max(worst[k], err[k] / bound[k])
            assert err[k] <= bound[k], (f"{lib} clip {i} ({ref['num_frames']} frames at {ref['fps']} fps) {k}: "
                                        f"{err[k]:.3g} > {bound[k]:.3g}")
        # what the device's bound is built from stays meaningful: the reference inside it by itself
        assert all(np.isfinite(v) and v > 0 for v in IC.device_bounds(model, clip, ref).values())
    print(f"{lib}: host error / bound, worst clip: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_host_restatement_sign_invariance(model, libs):
    """q and -q are one rotation: the host tables of the sign-flipped copy equal the original's bit
    for bit (IEEE arithmetic is symmetric in sign, and every product passes through quat_pos)."""
    from humanoid_amd.motion_lib import clip_to_motion
    a = clip_to_motion(model, libs["mixed"][IC.mixed_index("n37")])
    b = clip_to_motion(model, libs["mixed"][IC.mixed_index("flip")])
    for k in ("gts", "gvs", "gavs", "dvs"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["lrs"][:, 1:], b["lrs"][:, 1:])


def test_host_metadata_fractional_fps(model, libs):
    """MotionLibSMPL's per-motion metadata by the reference's formulas (its load_motions and
    get_motion_num_steps) with fps as given: 59.94 is not 59."""
    import torch
    from humanoid_amd.motion_lib import MotionLibSMPL
    clips = libs["mixed"]
    lib = MotionLibSMPL({f"c{i:02d}": c for i, c in enumerate(clips)}, model, device="cpu", is_deterministic=True)
    ids = [3, 5, 0, 3, 10]  # the two 59.94 fps clips, one of them twice
    picked, inv = lib.select_motions(len(ids), sample_idxes=ids)
    fps = [float(clips[i]["fps"]) for i in ids]
    nf = [len(clips[i]["pose_quat_global"]) for i in ids]
    assert fps[0] == 59.94 and fps[1] == 59.94
    lengths = torch.tensor([1.0 / f * (n - 1) for f, n in zip(fps, nf)], dtype=torch.float32)
    dt = torch.tensor([1.0 / f for f in fps], dtype=torch.float32)
    fps_t = torch.tensor(fps, dtype=torch.float32)
    assert torch.equal(lib.get_motion_length(), lengths)
    assert torch.equal(lib._motion_dt, dt)
    assert torch.equal(lib._motion_fps, fps_t)
    assert torch.equal(lib.get_motion_num_steps(), (torch.tensor(nf) * 30.0 / fps_t).ceil().int())
    assert lib.get_motion_num_steps()[0].item() == 76  # 150 frames at 59.94 fps; at 59 it is 77
    # and the tables built from the same selection carry the same metadata
    t = lib.load_motions(len(ids), sample_idxes=ids)
    np.testing.assert_array_equal(t.lengths, lengths.numpy())
    np.testing.assert_array_equal(t.dt, dt.numpy())
    np.testing.assert_array_equal(t.fps, fps_t.numpy())
    ref = IR.Tables(model, picked, inv)
    np.testing.assert_array_equal(t.lengths, ref.lengths)
    np.testing.assert_array_equal(t.dt, ref.dt)
    np.testing.assert_array_equal(t.length_starts, ref.length_starts)
