"""GPU checks of the engine's host-side ownership (he_engine.cpp over he_host.h): a refused motion reload
leaves the loaded library as it was, and creating and destroying engines returns their device memory."""
import dataclasses
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _engine(he_model, n):
    from humanoid_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(he_model, n, device=0)


def _tables(g):
    from humanoid_amd.motion_lib import MotionTables
    return MotionTables(gts=g["gts"], grs=g["grs"], lrs=g["lrs"], gvs=g["gvs"], gavs=g["gavs"], dvs=g["dvs"],
                        num_frames=g["num_frames"], length_starts=g["length_starts"], lengths=g["motion_lengths"],
                        dt=g["motion_dt"], fps=1.0 / g["motion_dt"])


def _reversed(t):
    """The same motions in the opposite order: other frames behind every motion id."""
    rev = np.arange(len(t.num_frames))[::-1]
    lens, starts = np.asarray(t.num_frames), np.asarray(t.length_starts)
    order = np.concatenate([np.arange(starts[m], starts[m] + lens[m]) for m in rev])
    frames = {f: np.asarray(getattr(t, f))[order] for f in ("gts", "grs", "lrs", "gvs", "gavs", "dvs")}
    return dataclasses.replace(t, **frames, num_frames=lens[rev],
                               length_starts=np.concatenate([[0], np.cumsum(lens[rev])[:-1]]),
                               lengths=np.asarray(t.lengths)[rev], dt=np.asarray(t.dt)[rev], fps=np.asarray(t.fps)[rev])


def test_refused_reload_keeps_the_loaded_library(he_model, golden):
    """ingest_clips and load_motions refused by their argument checks change nothing: the motion states read
    back afterwards are the bits read before. A valid reload then equals a fresh engine's load."""
    from humanoid_amd.engine import EngineError
    t = _tables(golden("motion_lib"))
    m = len(t.num_frames)
    assert m >= 2
    rng = np.random.default_rng(11)
    ids_np = rng.integers(0, m, 256)
    ids = torch.as_tensor(ids_np, dtype=torch.int64, device="cuda:0")
    times = torch.as_tensor((rng.random(256) * np.asarray(t.lengths)[ids_np]).astype(np.float32), device="cuda:0")

    def states(eng):
        out = eng.motion_state(ids, times)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    eng = _engine(he_model, 4)
    eng.load_motions(t)
    before = states(eng)
    assert all(np.isfinite(v).all() for v in before.values()) and np.abs(before["rg_pos"]).max() > 0.1
    with pytest.raises(EngineError, match="maps to clip 2 of 1"):
        eng.ingest_clips([{"pose_quat_global": np.zeros((3, 24, 4), np.float32),
                           "root_trans_offset": np.zeros((3, 3), np.float32), "fps": 30}], np.array([0, 2], np.int32))
    long = np.asarray(t.num_frames).copy()
    long[-1] += 1  # one frame past the table's end
    with pytest.raises(EngineError, match="outside the"):
        eng.load_motions(dataclasses.replace(t, num_frames=long))
    after = states(eng)
    for key in before:
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key

    t2 = _reversed(t)
    eng.load_motions(t2)
    got = states(eng)
    fresh = _engine(he_model, 4)
    fresh.load_motions(t2)
    want = states(fresh)
    for key in want:
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    assert any(not np.array_equal(got[key], before[key]) for key in got)  # the reload took effect


def test_create_destroy_returns_the_device_memory(he_model):
    """Five engines of 4096 envs created and destroyed in turn leave the device's free memory where the first
    left it, to within one engine's buffers: an engine that kept its buffers would take about four."""
    from humanoid_amd import _abi
    n = 4096

    eng = _engine(he_model, n)  # warm-up: the kernels' first dispatch, torch's context, and the footprint
    footprint = 0
    for kind in range(12):
        b = eng.buffer(kind)
        footprint += b.numel() * b.element_size()
    assert footprint == n * 4 * (13 + 2 * _abi.ND + 13 * _abi.NB + 3 * _abi.NB + 2 * _abi.ND + 2 + _abi.CACHE_WORDS + 13 + 2)
    assert footprint > 12 << 20  # well above the allocator's granularity
    del eng, b
    gc.collect()  # the views point back at their engine
    torch.cuda.synchronize()

    free = []
    for _ in range(5):
        eng = _engine(he_model, n)
        del eng
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print(f"engine footprint {footprint} bytes; free after each cycle: {free}")
    assert free[-1] >= free[0] - footprint, (free, footprint)
