"""CPU checks of the terrain in the camera sensors and of the ray-cast sensor: the two definitions'
place in the render library's ABI, every refusal (sent, past the null check, with a stand-in handle: a
zeroed block of memory, which is a renderer without terrain and without rays), the numpy reference
(tests/terrain_reference.py) against hits computed by hand, and the reference's own rounding, float32
against float64, which gives the GPU tests (test_gpu_terrain_render.py) their tolerances."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_reference as RR  # noqa: E402
import terrain_reference as TR  # noqa: E402


def _lib():
    from humanoid_amd import build, render
    if not os.path.exists(render.LIB_PATH):
        build.build()
    return render.load_library()


def _reason(lib, rc):
    assert rc != 0
    return lib.hr_last_error().decode()


def test_header_is_c99_and_constants_match(tmp_path):
    from humanoid_amd import render
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "humanoid_render.h"\n'
                   'int main(void){printf("%zu %zu %d %d %d %d %d %u\\n", sizeof(hr_ray), offsetof(hr_ray, dir), '
                   "HR_MAX_STEP_CELLS, HR_MAX_RAYS, HR_RAY_FRAME_POSITION, HR_RAY_FRAME_HEADING, HR_RAY_FRAME_TRANSFORM, "
                   "HR_RAYS_SKIP_BODIES); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(render.HrRay), render.HrRay.dir.offset, render.MAX_STEP_CELLS, render.MAX_RAYS,
                   render.RAY_FRAME_POSITION, render.RAY_FRAME_HEADING, render.RAY_FRAME_TRANSFORM, render.RAYS_SKIP_BODIES]
    assert got == [24, 12, 512, 1024, 0, 1, 2, 1]
    # the reference restates them too
    assert (TR.MAX_STEP_CELLS, TR.MAX_RAYS, TR.FRAME_POSITION, TR.FRAME_HEADING, TR.FRAME_TRANSFORM) == tuple(got[2:7])
    assert render.RAY_FRAMES == {"position": 0, "heading": 1, "transform": 2}
    assert (render.HIT_NOTHING, render.HIT_TERRAIN) == (TR.HIT_NOTHING, TR.HIT_TERRAIN) == (-2, -1)


def test_library_exports_the_terrain_and_ray_symbols():
    from humanoid_amd import render
    lib = _lib()
    for sym in ("hr_set_terrain", "hr_set_rays", "hr_cast_rays"):
        assert hasattr(lib, sym) and sym in render.HR_SYMBOLS
    assert lib.hr_version() == 1 and C.sizeof(render.HrCamera) == 56  # neither moved


def _rays(*rows):
    from humanoid_amd import render
    arr = (render.HrRay * max(len(rows), 1))()
    for i, r in enumerate(rows):
        arr[i].origin[:] = r[:3]
        arr[i].dir[:] = r[3:]
    return arr


def test_every_refusal_without_a_device():
    lib = _lib()
    one, two = C.c_void_p(4096), C.c_void_p(8192)  # never dereferenced: every call below is refused first
    down = (0.0, 0.0, 1.0, 0.0, 0.0, -1.0)
    assert "hr_set_terrain: null handle" in _reason(lib, lib.hr_set_terrain(None, None, 0.1, 0.05, 0.4))
    assert "hr_set_rays: null handle" in _reason(lib, lib.hr_set_rays(None, _rays(down), 1, 0, 0))
    assert "hr_cast_rays: null handle" in _reason(lib, lib.hr_cast_rays(None, one, 1.0, one, None, 0, None))

    block = C.create_string_buffer(4096)  # the stand-in handle
    fake = C.cast(block, C.c_void_p)
    zero = block.raw

    def terrain_refusals():
        for bad in (math.nan, math.inf, -math.inf):
            assert "slope" in _reason(lib, lib.hr_set_terrain(fake, one, bad, 0.05, 0.4))
        for bad in (math.nan, math.inf, -1e-3):
            assert "step_height" in _reason(lib, lib.hr_set_terrain(fake, one, 0.1, bad, 0.4))
        for bad in (math.nan, math.inf, 0.0, -0.4):
            assert "step_length" in _reason(lib, lib.hr_set_terrain(fake, one, 0.1, 0.05, bad))

    def ray_refusals():
        assert "null ray array" in _reason(lib, lib.hr_set_rays(fake, None, 1, 0, 0))
        for r in (0, -1, 1025):
            assert f"{r} rays" in _reason(lib, lib.hr_set_rays(fake, _rays(*[down] * 4), r, 0, 0))
        for b in (-1, 24):
            assert f"body {b}" in _reason(lib, lib.hr_set_rays(fake, _rays(down), 1, b, 0))
        for m in (-1, 3):
            assert f"frame_mode {m}" in _reason(lib, lib.hr_set_rays(fake, _rays(down), 1, 0, m))
        for i in range(6):
            for bad in (math.nan, math.inf):
                row = list(down)
                row[i] = bad
                assert "ray 1 has a component that is not finite" in _reason(lib, lib.hr_set_rays(fake, _rays(down, row), 2, 0, 1))
        for row in ((0, 0, 1, 0, 0, -1.002), (0, 0, 1, 0, 0, -0.998), (0, 0, 1, 0, 0, 0), (0, 0, 1, 0.6, 0.6, 0.6)):
            assert "unit length" in _reason(lib, lib.hr_set_rays(fake, _rays(down, down, row), 3, 0, 2))

    terrain_refusals()
    ray_refusals()
    assert block.raw == zero  # a refused call leaves the handle as it was
    # hr_cast_rays, in the order the header lists its refusals; the zeroed handle has no rays
    cast = lambda *a: lib.hr_cast_rays(fake, *a)  # noqa: E731
    assert "null rb_state" in _reason(lib, cast(None, 1.0, one, two, 0, None))
    assert "no output" in _reason(lib, cast(one, 1.0, None, None, 0, None))
    for bits in (2, 4, 0x80000000, 3):
        assert "unknown flag bits" in _reason(lib, cast(one, 1.0, one, two, bits, None))
    for bad in (math.nan, math.inf, 0.0, -1.0):
        assert "max_range" in _reason(lib, cast(one, bad, one, two, 1, None))
    assert "no rays set" in _reason(lib, cast(one, 1.0, one, None, 1, None))
    assert "no rays set" in _reason(lib, cast(one, 1.0, None, two, 0, None))
    assert block.raw == zero
    # hr_set_terrain needs no device: an accepted call changes the handle, refusals after it change nothing,
    # the same call again gives the same bytes, and values within the limits' edges are accepted
    assert lib.hr_set_terrain(fake, one, 0.17, 0.05, 0.4) == 0
    good = block.raw
    assert good != zero
    terrain_refusals()
    ray_refusals()
    assert block.raw == good
    assert lib.hr_set_terrain(fake, None, -0.3, 0.0, 1e-3) == 0 and block.raw != good
    assert lib.hr_set_terrain(fake, one, 0.17, 0.05, 0.4) == 0 and block.raw == good


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def test_python_layer_checks_before_any_library_call():
    import torch
    from humanoid_amd import render
    r = object.__new__(render.Renderer)
    r.lib, r.h, r.engine = _NoCalls(), None, None
    r.num_envs, r.num_rays, r.device = 3, 5, torch.device("cpu")
    r.ray_dist = r.ray_hit = None
    for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32)[:, 0], np.zeros(3, np.int32)):
        with pytest.raises(render.RenderError, match="terrain kind"):
            r.set_terrain(bad)
    with pytest.raises(AssertionError, match="library call hr_set_terrain"):
        r.set_terrain(torch.zeros(3, dtype=torch.int32), 0.1, 0.05, 0.4)
    n = 15
    good = {"dist": torch.zeros(n), "hit": torch.zeros(n, dtype=torch.int32), "rb_state": torch.zeros(3 * 24, 13)}
    wrong = {"dist": torch.float64, "hit": torch.int64, "rb_state": torch.float64}
    for name, ok in good.items():
        for t in (ok.to(wrong[name]), torch.stack([ok, ok], -1)[..., 0], ok.numpy(), ok.reshape(-1)[:-1]):
            with pytest.raises(render.RenderError, match=name):
                r.cast_rays(5.0, **{**({"dist": good["dist"]} if name == "rb_state" else {}), name: t})
    with pytest.raises(AssertionError, match="library call hr_cast_rays"):
        r.cast_rays(5.0, dist=good["dist"], hit=good["hit"], rb_state=good["rb_state"])
    r.num_rays = 0
    with pytest.raises(render.RenderError, match="before set_rays"):
        r.cast_rays(5.0, dist=good["dist"], rb_state=good["rb_state"])
    for bad in (np.zeros((3, 5)), np.zeros(6)):
        with pytest.raises(render.RenderError, match=r"\[R, 6\]"):
            r.set_rays(bad)
    with pytest.raises(render.RenderError, match="no body named"):
        r.set_rays(np.zeros((1, 6)), body="Tail")
    with pytest.raises(render.RenderError, match="unknown frame"):
        r.set_rays(np.zeros((1, 6)), frame="world")
    # the grid of a height scan: straight down, centred, x-major
    g = render.height_scan_rays(3, 2, 0.5, 1.25, offset=(0.1, 0.0))
    assert g.shape == (6, 6) and (g[:, 3:] == (0, 0, -1)).all() and (g[:, 2] == 1.25).all()
    np.testing.assert_allclose(g[:, 0], [-0.4, -0.4, 0.1, 0.1, 0.6, 0.6], atol=1e-15)
    np.testing.assert_allclose(g[:, 1], [-0.25, 0.25] * 3, atol=1e-15)


def test_facade_ray_sensor_needs_a_prepared_sim():
    from test_render import _facade_sim
    gymapi, gym, sim, envs = _facade_sim()
    with pytest.raises(RuntimeError, match="set_ray_sensor before prepare_sim"):
        gym.set_ray_sensor(sim, np.zeros((1, 6)))
    with pytest.raises(RuntimeError, match="cast_ray_sensor before prepare_sim"):
        gym.cast_ray_sensor(sim, None, None, 5.0)


def test_reference_matches_hand_computed_hits():
    """Steps of 0.05 m x 0.4 m (tread c spans [0.4 c, 0.4 (c+1)) at height 0.05 c) and the 10 degree slope."""
    ter = TR.terrain(None, np.deg2rad(10.0), 0.05, 0.4)
    L, S = float(ter["step_length"]), float(ter["step_height"])  # the float32 values, as the device holds them
    # straight down onto tread 3 (x = 1.37 lies in [1.2, 1.6)): from z = 1 to z = 3 S
    hit, t, n, ckx = TR.one_ray(ter, 2, (1.37, 0.2, 1.0), (0, 0, -1))
    assert hit and abs(t - (1.0 - 3 * S)) < 1e-12 and n == (0, 0, 1) and abs(ckx - 1.37) < 1e-12
    # horizontal at z = 0.07 from x = 0.1: over riser 1 (top at S = 0.05), into riser 2 (top 0.1) at x = 2 L
    hit, t, n, ckx = TR.one_ray(ter, 2, (0.1, 0.0, 0.07), (1, 0, 0))
    assert hit and abs(t - (2 * L - 0.1)) < 1e-12 and n == (-1, 0, 0)
    assert abs(ckx - 1.5 * L) < 1e-12  # the checker takes the middle of tread 1, the cell the ray left
    # the same ray with far short of the riser: the walk ends at the boundary it cannot reach
    assert not TR.one_ray(ter, 2, (0.1, 0.0, 0.07), (1, 0, 0), far=0.6)[0]
    # starting inside the solid (tread 3 is at 0.15): no hit, whatever the direction
    for d in ((0, 0, -1), (0, 0, 1), (1, 0, 0.2), (-1, 0, -0.2)):
        assert not TR.one_ray(ter, 2, (1.37, 0.0, 0.1), d)[0]
    # descending from over tread 5 (0.25) towards -x at slope 1:5: z = 0.5 - s / 5 at x = 2.1 - s stays above
    # treads 4..1 over their spans (0.4 > 0.2 at x = 1.6, ..., 0.16 > 0.05 at x = 0.4) and meets z = 0 at
    # s = 2.5, x = -0.4: cell 0, which is all of x < L
    hit, t, n, ckx = TR.one_ray(ter, 2, (2.1, 0.0, 0.5), (-1, 0, -0.2))
    assert hit and abs(t - 2.5 * math.sqrt(1.04)) < 1e-9 and n == (0, 0, 1) and abs(ckx + 0.4) < 1e-9
    # rising, or level and not moving up the stairs: nothing to enter
    assert not TR.one_ray(ter, 2, (2.1, 0.0, 0.5), (-1, 0, 0.0), far=20.0)[0]
    assert not TR.one_ray(ter, 2, (2.1, 0.0, 0.5), (0, 1, 0.0))[0]
    # the slope z = x tan(10 deg) straight under (1, 0, 2)
    sn, cs = float(np.sin(np.float32(np.deg2rad(10.0)))), float(np.cos(np.float32(np.deg2rad(10.0))))
    hit, t, n, _ = TR.one_ray(ter, 1, (1.0, 0.0, 2.0), (0, 0, -1))
    assert hit and abs(t - (2.0 - sn / cs)) < 1e-12 and np.allclose(n, (-sn, 0, cs), atol=0, rtol=0)
    assert abs(sn - math.sin(math.radians(10))) < 1e-7
    assert not TR.one_ray(ter, 1, (1.0, 0.0, 0.1), (0, 0, -1))[0]  # under the slope
    assert not TR.one_ray(ter, 1, (1.0, 0.0, 2.0), (1, 0, 0.2))[0]  # climbing faster than the slope
    # the plane, and the kinds that mean it
    assert TR.one_ray(ter, 0, (1.0, 0.0, 2.0), (0, 0, -1))[:2] == (True, 2.0)
    assert [TR.kind_of(TR.terrain((7, -1, 1, 2, 0)), e) for e in range(5)] == [0, 0, 1, 2, 0]
    assert TR.kind_of(ter, 3) == 0 and TR.kind_of(None, 0) == 0
    # the 512-cell bound: from (0.2, 0, z0) along (1, 0, -0.01) the ray is at z0 + 0.002 - 0.004 c over the
    # boundary x = 0.4 c, where riser c tops out at 0.05 c: it clears the risers up to c = (z0 + 0.002) / 0.054.
    # z0 = 24: 444.5, so it leaves cell 444 into riser 445; z0 = 30: 555.6, past the 512 cells, no hit
    hit, t, n, ckx = TR.one_ray(ter, 2, (0.2, 0.0, 24.0), (1, 0, -0.01), far=1e6)
    assert hit and n == (-1, 0, 0) and abs(ckx / L - 444.5) < 1e-9 and abs(t - (445 * L - 0.2) * math.sqrt(1.0001)) < 1e-9
    assert not TR.one_ray(ter, 2, (0.2, 0.0, 30.0), (1, 0, -0.01), far=1e6)[0]
    # float32 gives the same answers on all of these
    assert TR.one_ray(ter, 2, (0.1, 0.0, 0.07), (1, 0, 0), dtype=np.float32)[2] == (-1, 0, 0)
    assert not TR.one_ray(ter, 2, (0.2, 0.0, 30.0), (1, 0, -0.01), far=1e6, dtype=np.float32)[0]


def test_reference_self_check(model):
    """The reference against itself, float32 against float64, on RR.scene() with the kinds (2, 1, 2, 0):
    its own rounding leaves no pixel without an agreeing neighbour and edge pixels within the cap, and the depth floor it measures is the constant the GPU tolerance is 8 x of. The views are the
    six of the issue; with the scattered bodies in the scene none of them needed moving (the view
    (1,-2,1) -> (1,0,0.2), which holds the checker line and the riser plane x = 1 in its image plane, is not
    among them: it fails on its own)."""
    rb = RR.scene()
    segs, rgbs = RR.distinct_seg(), RR.distinct_rgb()
    cams = TR.cameras()
    floor, worst = 0.0, 0
    both = RR.FLAG_SHADOWS | RR.FLAG_CHECKER
    plane = RR.render(model.geom_type, model.geom_params, rb, cams, rgbs, segs, None, both, np.float64)
    for ter in TR.settings():
        r64 = TR.render(model.geom_type, model.geom_params, rb, cams, ter, rgbs, segs, None, both, np.float64)
        r32 = TR.render(model.geom_type, model.geom_params, rb, cams, ter, rgbs, segs, None, both, np.float32)
        for k in range(len(cams)):
            a, b = tuple(x[k] for x in r32), tuple(x[k] for x in r64)
            worst = max(worst, RR.check(a, b, np.inf))
            agree, _ = RR.compare(a, b, np.inf)
            fin = agree & np.isfinite(b[1])
            with np.errstate(invalid="ignore"):
                floor = max(floor, float(np.abs(a[1] - b[1])[fin].max()))
            # worth testing on: the ground fills a good part of every view
            assert ((b[2] == 0) & np.isfinite(b[1])).mean() > 0.4
        # risers are in view (their normal shades them darker than any tread: n.l < 0, ambient only) and so
        # are bodies and their shadows
        assert (r64[1][:6] != plane[1][:6]).mean() > 0.3 and len(np.unique(r64[2])) > 40
    print(f"terrain reference float32 vs float64: at most {worst} edge pixels per image (the cap: "
          f"{RR.CAP * RR.W * RR.H:.1f}), depth floor {floor:.3e} m, GPU depth tolerance {TR.TERRAIN_DEPTH_TOL:.3e} m")
    assert 0.5 * TR.TERRAIN_DEPTH_FLOOR <= floor <= TR.TERRAIN_DEPTH_FLOOR, floor
    assert TR.TERRAIN_DEPTH_TOL == 8 * TR.TERRAIN_DEPTH_FLOOR and TR.TERRAIN_DEPTH_TOL <= 1e-3
    # a terrain of plane kinds, and none, is the image render_reference draws
    for ter in (TR.terrain((0, 7, -1, 0)), None):
        flat = TR.render(model.geom_type, model.geom_params, rb, cams[:8], ter, rgbs, segs, None, both, np.float64)
        assert all(np.array_equal(x, y[:8]) for x, y in zip(flat, plane))


def test_reference_ray_self_check(model):
    """The sensor's reference, float32 against float64: 185 rays per env, each kind in turn on all four envs
    and the mixed kinds, both step settings, the three frames, with and without bodies. No ray changes its
    hit id; the largest distance difference per env is the floor the GPU tolerance is 8 x of (env 3 sits at
    x = 1000 m, so its bodies' floor is that of the image's far scenes)."""
    rb = RR.scene()
    rays = TR.sensor_rays()
    assert rays.shape == (185, 6) and np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6
    floors = {True: np.zeros(4), False: np.zeros(4)}
    seen = set()
    for mode in (TR.FRAME_POSITION, TR.FRAME_HEADING, TR.FRAME_TRANSFORM):
        for kinds in ((0,) * 4, (1,) * 4, (2,) * 4, TR.KINDS):
            for s, l in TR.STEP_SETTINGS:
                ter = TR.terrain(kinds, TR.SLOPE, s, l)
                for skip in (True, False):
                    d64, h64 = TR.cast(model.geom_type, model.geom_params, rb, rays, TR.RAY_BODY, mode, ter, TR.MAX_RANGE, skip, np.float64)
                    d32, h32 = TR.cast(model.geom_type, model.geom_params, rb, rays, TR.RAY_BODY, mode, ter, TR.MAX_RANGE, skip, np.float32)
                    assert (h64 == h32).all()
                    assert (np.isfinite(d64) == (h64 > TR.HIT_NOTHING)).all() and (d64[np.isfinite(d64)] <= TR.MAX_RANGE).all()
                    assert skip == (not (h64 >= 0).any())
                    fin = np.isfinite(d64)
                    diff = np.abs(np.where(fin, d32, 0.0) - np.where(fin, d64, 0.0))
                    floors[skip] = np.maximum(floors[skip], diff.max(axis=1))
                    seen |= set(np.unique(h64).tolist())
    assert {TR.HIT_NOTHING, TR.HIT_TERRAIN} <= seen and len(seen) > 12  # misses, ground and many bodies
    print("ray distance floors per env: terrain only", floors[True], "with bodies", floors[False])
    for got, const in ((floors[True], TR.RAY_FLOOR_TERRAIN), (floors[False], TR.RAY_FLOOR_BODIES)):
        assert (got <= np.array(const)).all() and (got >= 0.5 * np.array(const)).all(), (got, const)
    # the heading of a rotation about z by a is (cos a, sin a); of one that points x straight up, (1, 0)
    a = 0.7
    c, s = TR.heading(np.array([0, 0, math.sin(a / 2), math.cos(a / 2)]))
    assert abs(c - math.cos(a)) < 1e-12 and abs(s - math.sin(a)) < 1e-12
    assert TR.heading(np.array([0, -math.sqrt(0.5), 0, math.sqrt(0.5)])) == (1, 0)
