"""Device-side motion ingestion (he_ingest_clips) against

* the host restatement (``motion_lib.build_tables``, itself pinned to the reference's motion_lib golden
  vectors in test_oracle_golden.py): both engines sample the same motion states at the same times.
  Tolerances: positions / rotations 2e-5 (fp32 FK in a different operation order); linear velocity
  1e-3 abs + 1e-4 rel (the Gaussian filter accumulates in fp32 here, fp64 in scipy); angular and dof
  velocities 3e-3 abs + 1e-3 rel (arccos of a near-identity rotation difference in fp32, as for the
  reference loader's own fp32 path, test_oracle_golden.py);
* the reference project's own output for its own raw clips (tests/golden/motion_lib.npz), with no host
  restatement in between: 3 x the float64 reference's measured distance from those tables
  (ingest_cases.GOLDEN_MEASURED) plus test_motion_state_matches_golden's sampling tolerances;
* the independent float64 reference (tests/ingest_reference.py) on the adversarial libraries of
  tests/ingest_cases.py, at every frame of every motion and at seeded random times. Per clip and
  channel the device is held to 3 max(e_host, floor), e_host = max |float32 host restatement -
  float64 reference| computed on the CPU (ingest_cases.device_bounds: why 3, and the floor);
  rotations are a pass-through of the input, compared sign-free at 2e-6; dof positions as exp maps
  (cases.assert_expmap_close).
  Measured on an MI355X, device error / max(e_host, floor) of the worst clip (the bound is 3):
  positions 0.48 (mixed) / 0.52 (many), linear velocity 0.31 / 0.36, angular velocity 1.00 / 1.64,
  dof velocity 1.01 / 1.09; rotations 2.4e-7 / 2.9e-7. Golden clips: 7.2e-7 m, 1.1e-5 m/s,
  1.2e-3 rad/s and 2.3e-5 rad/s against bounds of 3.7e-6, 4.3e-5, 1.0e-2 and 1.8e-4;
* itself: a clip's tables do not depend on its neighbours or its offset in the library, nor on the
  signs of its quaternions, bit for bit; a refused library leaves the loaded one in place.

Tried on an MI355X with he_ingest.hip broken on purpose (in-bounds changes only), these fail:
``a.dt[0]`` for ``a.dt[c]`` -- every_frame (both), clip_isolation; the filter's upper clamp moved from
the clip's end to the table's -- every_frame, clip_isolation, sign_invariance, golden_clips and the
two host-table tests; RADIUS 9 -- every_frame[mixed] (the spin clip); RADIUS 7 -- every_frame (both),
golden_clips; qmul_norm without quat_pos -- every_frame[mixed], sign_invariance.
"""
import numpy as np
import pytest

import cases
import ingest_cases as IC
import ingest_reference as IR

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OUTPUTS = ("rg_pos", "rb_rot", "body_vel", "body_ang_vel", "dof_pos", "dof_vel")


def _clips(model):
    from humanoid_amd import synthetic
    rng = np.random.default_rng(7)
    out = [synthetic.make_clip(model, rng, num_frames=t) for t in (150, 37, 5, 2, 90)]
    out.append(synthetic.make_standstill_clip(model, num_frames=20))
    return out


@pytest.fixture(scope="module")
def libs(model):
    return IC.libraries(model)


def _engine(he_model, n=4):
    from humanoid_amd.engine import Engine
    assert torch.cuda.is_available(), "GPU test run without a visible GPU"
    return Engine(he_model, n, device=0)


def _query(eng, ids, times, offset=None):
    cu = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dt), device="cuda:0")  # noqa: E731
    r = eng.motion_state(cu(ids, np.int64), cu(times, np.float32), None if offset is None else cu(offset, np.float32))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _frame_times(tables, motions=None):
    """(ids, times) of every frame of the given motions: t = f * dt as the float32 product."""
    motions = range(len(tables.num_frames)) if motions is None else motions
    ids = np.concatenate([np.full(tables.num_frames[m], m, np.int64) for m in motions])
    f = np.concatenate([np.arange(tables.num_frames[m]) for m in motions]).astype(np.float32)
    return ids, f * tables.dt[ids]


def _quat_dist(a, b):
    return np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1))


def test_ingest_matches_host_tables(model, he_model):
    from humanoid_amd.engine import Engine
    from humanoid_amd.motion_lib import build_tables
    clips = _clips(model)
    n = 8
    host = Engine(he_model, n, device=0)
    host.load_motions(build_tables(model, clips))
    dev = Engine(he_model, n, device=0)
    dev.ingest_clips(clips)
    rng = np.random.default_rng(1)
    k = 4096
    ids = torch.as_tensor(rng.integers(0, len(clips), k), device="cuda:0")
    lens = torch.as_tensor([(len(c["pose_quat_global"]) - 1) / 30.0 for c in clips], device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    times = torch.rand(k, device="cuda:0", generator=gen) * lens[ids] * 1.02  # includes the clamp past the end
    a = host.motion_state(ids, times)
    b = dev.motion_state(ids, times)
    torch.cuda.synchronize()
    tol = {"rg_pos": (2e-5, 0), "rb_rot": (2e-5, 0), "dof_pos": (2e-4, 0), "body_vel": (1e-3, 1e-4),
           "body_ang_vel": (3e-3, 1e-3), "dof_vel": (3e-3, 1e-3)}
    for key, (atol, rtol) in tol.items():
        x, y = b[key].cpu().numpy(), a[key].cpu().numpy()
        if key == "rb_rot":  # sign-free
            x = np.where((x * y).sum(-1, keepdims=True) < 0, -x, x)
        np.testing.assert_allclose(x, y, atol=atol, rtol=rtol, err_msg=key)


def test_ingest_motion_clip_mapping(model, he_model):
    """Per-env motion entries sharing clips (motion i -> clip map) equal per-env copies."""
    from humanoid_amd.engine import Engine
    clips = _clips(model)
    n = 8
    mapping = np.array([3, 0, 0, 5, 1, 1, 1, 4], np.int32)
    shared = Engine(he_model, n, device=0)
    shared.ingest_clips(clips, mapping)
    copies = Engine(he_model, n, device=0)
    copies.ingest_clips([clips[i] for i in mapping])
    ids = torch.arange(n, device="cuda:0").repeat(64)
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    times = torch.rand(ids.numel(), device="cuda:0", generator=gen) * 0.5
    a = shared.motion_state(ids, times)
    b = copies.motion_state(ids, times)
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_ingest_rejects_bad_input(he_model):
    from humanoid_amd.engine import Engine, EngineError
    eng = Engine(he_model, 4, device=0)
    with pytest.raises(EngineError):
        eng.ingest_clips([{"pose_quat_global": np.zeros((3, 24, 4), np.float32),
                           "root_trans_offset": np.zeros((3, 3), np.float32), "fps": 30}], np.array([0, 2], np.int32))


def test_ingest_golden_clips(he_model, golden):
    """The reference project's raw clips through device ingestion, sampled where the reference project
    sampled its own tables: device ingestion against reference output, nothing in between."""
    g = golden("motion_lib")
    eng = _engine(he_model)
    eng.ingest_clips(IC.golden_clips(g), g["sample_idxes"].astype(np.int32))
    r = _query(eng, g["q_ids"], g["q_times"], g["q_offset"])
    for k, tab, tol in (("rg_pos", "gts", 2e-6), ("body_vel", "gvs", 1e-5), ("body_ang_vel", "gavs", 1e-5),
                        ("dof_vel", "dvs", 1e-5)):
        err = np.abs(r[k] - g["ms_" + k]).max()
        print(f"golden {k}: {err:.3g} (bound {IC.GOLDEN_BOUND[tab] + tol:.3g})")
        np.testing.assert_allclose(r[k], g["ms_" + k], rtol=0, atol=IC.GOLDEN_BOUND[tab] + tol, err_msg=k)
    assert _quat_dist(r["rb_rot"], g["ms_rb_rot"]).max() <= 5e-6
    cases.assert_expmap_close(r["dof_pos"], g["ms_dof_pos"])


@pytest.mark.parametrize("lib", ["mixed", "many"])
def test_ingest_every_frame(model, he_model, libs, lib):
    """Every frame of every motion at t = f dt, and 2048 seeded random times up to 1.02 x the length
    (the clamp past the end included), against the float64 reference's motion_state."""
    clips = libs[lib]
    eng = _engine(he_model)
    eng.ingest_clips(clips)
    t = IR.Tables(model, clips)
    ids, times = _frame_times(t)
    rng = np.random.default_rng(11)
    rid = rng.integers(0, len(clips), 2048)
    ids = np.concatenate([ids, rid])
    times = np.concatenate([times, rng.random(2048, np.float32) * t.lengths[rid] * np.float32(1.02)])
    got, ref = _query(eng, ids, times), IR.motion_state(t, ids, times)
    scale = {k: np.array([max(IC.host_errors(model, c, r)[k], IC.floors(r)[k]) for c, r in zip(clips, t.clips)])
             for k in IC.CHANNELS}
    ratio = {}
    for k in IC.CHANNELS:
        out = IC.OUTPUT_OF[k]
        err = np.abs(got[out] - ref[out]).reshape(len(ids), -1).max(-1)
        per_clip = np.zeros(len(clips))
        np.maximum.at(per_clip, ids, err / scale[k][ids])
        ratio[k] = per_clip
        print(f"{lib} {out}: device error / max(e_host, floor), worst clip {per_clip.argmax()}: {per_clip.max():.3g}")
    rot = _quat_dist(got["rb_rot"], ref["rb_rot"]).max()
    print(f"{lib} rb_rot: {rot:.3g}")
    for k in IC.CHANNELS:
        bad = np.flatnonzero(ratio[k] > 3.0)
        assert bad.size == 0, (f"{lib} {IC.OUTPUT_OF[k]}: clips {bad.tolist()} at {ratio[k][bad].round(2).tolist()} "
                               f"x max(e_host, floor), the bound is 3")
    assert rot <= 2e-6
    cases.assert_expmap_close(got["dof_pos"], ref["dof_pos"])


def test_ingest_clip_isolation(model, he_model, libs):
    """A clip's tables are its own: the 17-frame 59.94 fps clip (every filter tap range reaches both
    of its ends) between two different pairs of neighbours, starting at frame 3 and at frame 18 (3
    and 2 mod 8, other blocks, other clip indices, other first-clip fps), gives the same bits."""
    m = {name: libs["mixed"][IC.mixed_index(name)] for name in ("n2", "n3", "n9", "n16", "n17", "spin")}
    lib_a, at_a = [m["n3"], m["n17"], m["n9"]], 1
    lib_b, at_b = [m["n16"], m["n2"], m["n17"], m["spin"]], 2
    assert IC.starts(lib_a)[0][at_a] == 3 and IC.starts(lib_b)[0][at_b] == 18
    out = []
    for lib, at in ((lib_a, at_a), (lib_b, at_b)):
        eng = _engine(he_model)
        eng.ingest_clips(lib)
        ids, times = _frame_times(IR.Tables(model, lib), [at])
        rng = np.random.default_rng(5)
        times = np.concatenate([times, rng.random(64, np.float32) * np.float32(16 / 59.94)])
        out.append(_query(eng, np.full(len(times), at), times))
    for k in OUTPUTS:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)


def test_ingest_sign_invariance(model, he_model, libs):
    """q and -q are one rotation. The copy of the 37-frame clip with half of its quaternions negated
    gives the original's positions, velocities and dof states bit for bit (IEEE arithmetic is
    symmetric in sign and every rotation product passes through quat_pos), and its rotations up to
    sign (they are the input, passed through)."""
    clips = libs["mixed"]
    eng = _engine(he_model)
    eng.ingest_clips(clips)
    t = IR.Tables(model, clips)
    a, b = IC.mixed_index("n37"), IC.mixed_index("flip")
    ids, times = _frame_times(t, [a])
    rng = np.random.default_rng(6)
    times = np.concatenate([times, rng.random(256, np.float32) * t.lengths[a] * np.float32(1.02)])
    x, y = _query(eng, np.full(len(times), a), times), _query(eng, np.full(len(times), b), times)
    for k in OUTPUTS:
        if k != "rb_rot":
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)
    assert _quat_dist(x["rb_rot"], y["rb_rot"]).max() == 0.0
    assert (x["rb_rot"] != y["rb_rot"]).any()  # and the signs did differ


def test_ingest_refusals_leave_library(model, he_model, libs):
    """Each bad library raises EngineError and leaves the loaded one in place: the same query returns
    the same bits after it. No refused library reaches a kernel (a one-frame motion is never sampled)."""
    from humanoid_amd.engine import EngineError
    from humanoid_amd.motion_lib import build_tables
    m = {name: libs["mixed"][IC.mixed_index(name)] for name in ("n3", "n8", "n9")}
    good = [m["n8"], m["n3"]]
    eng = _engine(he_model)
    eng.ingest_clips(good)
    ids, times = _frame_times(IR.Tables(model, good))
    before = _query(eng, ids, times)

    def one_frame(c):
        return dict(c, pose_quat_global=c["pose_quat_global"][:1], root_trans_offset=c["root_trans_offset"][:1])

    short = dict(m["n9"], root_trans_offset=m["n9"]["root_trans_offset"][:-1])
    long = dict(m["n8"], root_trans_offset=np.concatenate([m["n8"]["root_trans_offset"]] * 2)[:9])
    bad = {"one frame": ([m["n9"], one_frame(m["n3"])], None, "at least 2"),
           "one frame alone": ([one_frame(m["n3"])], None, "at least 2"),
           "fps 0": ([dict(m["n9"], fps=0)], None, "fps"),
           "fps negative": ([m["n8"], dict(m["n9"], fps=-30.0)], None, "fps"),
           "fps nan": ([dict(m["n9"], fps=float("nan"))], None, "fps"),
           "fps inf": ([dict(m["n9"], fps=float("inf"))], None, "fps"),
           "clip index too large": ([m["n9"], m["n3"]], [0, 2], "maps to clip"),
           "clip index negative": ([m["n9"], m["n3"]], [-1, 0], "maps to clip"),
           "translation frames": ([short], None, "translations"),
           "translation frames that cancel": ([short, long], None, "translations")}
    for what, (clips, mapping, text) in bad.items():
        with pytest.raises(EngineError, match=text):
            eng.ingest_clips(clips, None if mapping is None else np.array(mapping, np.int32))
        after = _query(eng, ids, times)
        for k in OUTPUTS:
            np.testing.assert_array_equal(before[k], after[k], err_msg=f"{what}: {k}")
    # he_load_motions: a table with a one-frame motion
    tab = build_tables(model, [m["n9"], m["n3"]])
    tab.num_frames = np.array([9, 1], np.int64)
    with pytest.raises(EngineError, match="at least 2"):
        eng.load_motions(tab)
    after = _query(eng, ids, times)
    for k in OUTPUTS:
        np.testing.assert_array_equal(before[k], after[k], err_msg=f"one-frame table: {k}")
