"""GPU checks of the per-env terrain in the camera sensors and of the ray-cast sensor against the float64
numpy restatement of their definitions (tests/terrain_reference.py). One engine of 4 envs whose rb_state
holds the render tests' scene (render_reference.scene), the kinds (2, 1, 2, 0) over the envs, 70 x 45
images, 185 rays per env.

Tolerances follow the rule of test_gpu_render.py: 8 x the reference's own float32-against-float64 floor
(test_terrain_render.py measures and holds them), never a figure taken from the kernel. A pixel that does
not agree with the reference must agree with it at a neighbour, and such edge pixels stay within 0.5 % of an
image; a ray may differ from float64 in its hit id in at most 1 % of the rays (the reference alone: none)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_reference as RR  # noqa: E402
import terrain_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
N, H, W = RR.N_ENVS, RR.H, RR.W
MARKERS_RGB, MARKER_RADIUS = [(0.8, 0.0, 0.0), (0.1, 0.9, 0.1), (0.1, 0.2, 0.9)], 0.05


def _cams(dicts):
    from humanoid_amd import render as R
    return [R.camera(**d) for d in dicts]


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(model):
    """One engine whose rb_state holds the shared scene, a renderer that is given terrain, one that never
    hears of it, and the float64 references (each computed once)."""
    import torch
    from humanoid_amd import render as R
    from humanoid_amd.engine import Engine
    c = _Ctx()
    c.model = model
    c.eng = Engine(model, N, device=0)
    rbt = c.eng.rb_state.view(N, 24, 13)
    c.rb = RR.scene(env0_rows=rbt[0].cpu().numpy())  # env 0 stays as he_create_envs left it
    rbt.copy_(torch.from_numpy(c.rb).to(c.eng.device))
    dev = c.eng.device
    c.seg, c.rgb = RR.distinct_seg(), RR.distinct_rgb()
    c.seg_t, c.rgb_t = torch.from_numpy(c.seg).to(dev), torch.from_numpy(c.rgb).to(dev)
    c.mpos = (np.random.default_rng(5).uniform(-0.5, 0.5, (N, 3, 3)).astype(np.float32) + np.float32([0.8, 0, 1]))
    c.mpos_t = torch.from_numpy(c.mpos).to(dev)
    c.ren, c.plain = R.Renderer(c.eng), R.Renderer(c.eng)
    for r in (c.ren, c.plain):
        r.set_appearance(c.rgb_t, c.seg_t)
        r.set_markers(c.mpos_t, MARKERS_RGB, MARKER_RADIUS)
    c.kind_t = torch.tensor(TR.KINDS, dtype=torch.int32, device=dev)
    c.rays = TR.sensor_rays()
    c.refs = {}
    return c


def _set_terrain(c, ter):
    c.ren.set_terrain(c.kind_t, float(ter["slope"]), float(ter["step_height"]), float(ter["step_length"]))


def _draw(ren, cams, flags):
    import torch
    ren.set_cameras(_cams(cams))
    ren.render(flags)
    torch.cuda.synchronize()
    return ren.color.cpu().numpy(), ren.depth.cpu().numpy(), ren.seg.cpu().numpy()


def _image_reference(c, setting, flags):
    key = ("image", setting, flags)
    if key not in c.refs:
        c.refs[key] = TR.render(c.model.geom_type, c.model.geom_params, c.rb, TR.cameras(), TR.settings()[setting], c.rgb,
                                c.seg, (c.mpos, MARKERS_RGB, MARKER_RADIUS), flags, np.float64)
    return c.refs[key]


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("setting", [0, 1])
def test_terrain_images_against_reference(ctx, setting, shadows):
    """The six views on the steps and on the slope (and two on the steps under the rest pose), appearance and
    markers set."""
    from humanoid_amd import render as R
    flags = R.FLAG_CHECKER | (R.FLAG_SHADOWS if shadows else 0)
    cams = TR.cameras()
    _set_terrain(ctx, TR.settings()[setting])
    ref = _image_reference(ctx, setting, flags)
    img = _draw(ctx.ren, cams, flags)
    worst = 0.0
    for k in range(len(cams)):
        a, b = tuple(x[k] for x in img), tuple(x[k] for x in ref)
        agree, edge = RR.compare(a, b, TR.TERRAIN_DEPTH_TOL)
        fin = agree & np.isfinite(b[1])
        worst = max(worst, float(np.abs(np.where(fin, a[1], 0.0) - np.where(fin, b[1], 0.0)).max()))
        print(f"camera {k} (env {cams[k]['env']}): {int(edge.sum())} edge pixels, {int((~(agree | edge)).sum())} failing")
    print(f"largest depth difference on agreeing pixels {worst:.3e} m (tolerance {TR.TERRAIN_DEPTH_TOL:.3e})")
    for k in range(len(cams)):
        RR.check(tuple(x[k] for x in img), tuple(x[k] for x in ref), TR.TERRAIN_DEPTH_TOL)
    # the scene is worth it: the terrain moved most of the ground, markers and many bodies are in view
    flat = _draw(ctx.plain, cams, flags)
    assert (img[1][:6] != flat[1][:6]).mean() > 0.3
    assert R.SEG_MARKER in img[2] and len(np.unique(img[2])) > 40
    # culling never changes a pixel
    full = _draw(ctx.ren, cams, flags | R.FLAG_NO_CULL)
    assert all((a == b).all() for a, b in zip(img, full))


def test_plane_kinds_and_no_terrain_draw_todays_image(ctx):
    """An all-zero kind array, NULL after a real one, and kinds that name no terrain (7, -1) give the image of
    a renderer that never heard of terrain, to the bit."""
    import torch
    from humanoid_amd import render as R
    cams = RR.parity_cameras() + TR.cameras()[:3]
    want = _draw(ctx.plain, cams, R.FLAGS_DEFAULT)
    ter = TR.settings()[1]
    dev = ctx.eng.device
    _set_terrain(ctx, ter)
    real = _draw(ctx.ren, cams, R.FLAGS_DEFAULT)
    assert not np.array_equal(real[1], want[1])
    for kind in (torch.zeros(N, dtype=torch.int32, device=dev), None, torch.tensor([7, -1, 3, 0], dtype=torch.int32, device=dev)):
        ctx.ren.set_terrain(kind, float(ter["slope"]), float(ter["step_height"]), float(ter["step_length"]))
        got = _draw(ctx.ren, cams, R.FLAGS_DEFAULT)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        _set_terrain(ctx, ter)  # a real one in between
    # a refused setting raises and leaves the previous one
    with pytest.raises(R.RenderError, match="step_length"):
        ctx.ren.set_terrain(ctx.kind_t, 0.1, 0.05, 0.0)
    again = _draw(ctx.ren, cams, R.FLAGS_DEFAULT)
    assert all(np.array_equal(a, b) for a, b in zip(again, real))


def test_kind_tensor_is_read_at_render_time(ctx):
    import torch
    from humanoid_amd import render as R
    cams = TR.cameras()[:6]  # env 2
    kind = torch.zeros(N, dtype=torch.int32, device=ctx.eng.device)
    ter = TR.settings()[0]
    ctx.ren.set_terrain(kind, float(ter["slope"]), float(ter["step_height"]), float(ter["step_length"]))
    flat = _draw(ctx.ren, cams, R.FLAGS_DEFAULT)
    images = {}
    for k in (1, 2):
        kind[2] = k  # in place: no call into the library
        ctx.ren.render(R.FLAGS_DEFAULT)
        torch.cuda.synchronize()
        images[k] = ctx.ren.depth.cpu().numpy()
        assert (images[k] != flat[1]).mean() > 0.3
    assert (images[1] != images[2]).mean() > 0.3
    kind[2] = 0
    ctx.ren.render(R.FLAGS_DEFAULT)
    torch.cuda.synchronize()
    assert np.array_equal(ctx.ren.depth.cpu().numpy().view(np.uint32), flat[1].view(np.uint32))
    _set_terrain(ctx, ter)


def _ray_reference(c, setting, mode, skip):
    key = ("rays", setting, mode, skip)
    if key not in c.refs:
        c.refs[key] = TR.cast(c.model.geom_type, c.model.geom_params, c.rb, c.rays, TR.RAY_BODY, mode, TR.settings()[setting],
                              TR.MAX_RANGE, skip, np.float64)
    return c.refs[key]


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("mode", ["position", "heading", "transform"])
def test_ray_sensor_against_reference(ctx, mode, skip):
    import torch
    from humanoid_amd import render as R
    for setting in (0, 1):
        _set_terrain(ctx, TR.settings()[setting])
        ctx.ren.set_rays(ctx.rays, body="Pelvis", frame=mode)
        dist, hit = ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=skip)
        torch.cuda.synchronize()
        assert dist is ctx.ren.ray_dist and tuple(dist.shape) == (N, 185) and hit.dtype == torch.int32
        d, h = dist.cpu().numpy().astype(np.float64), hit.cpu().numpy()
        d64, h64 = _ray_reference(ctx, setting, R.RAY_FRAMES[mode], skip)
        same = h == h64
        floors = TR.RAY_FLOOR_TERRAIN if skip else TR.RAY_FLOOR_BODIES
        for e in range(N):
            fin = same[e] & np.isfinite(d64[e])
            worst = float(np.abs(np.where(fin, d[e], 0.0) - np.where(fin, d64[e], 0.0)).max())
            print(f"setting {setting} env {e}: {int((~same[e]).sum())} of 185 hit ids differ, largest distance difference "
                  f"{worst:.3e} m (tolerance {8 * floors[e]:.3e})")
        for e in range(N):
            fin = same[e] & np.isfinite(d64[e])
            assert (~same[e]).sum() <= TR.HIT_ID_CAP * same[e].size
            assert np.abs(np.where(fin, d[e], 0.0) - np.where(fin, d64[e], 0.0)).max() <= 8 * floors[e]
            assert (np.isinf(d[e]) == (h[e] == R.HIT_NOTHING)).all() and (d[e][h[e] == R.HIT_NOTHING] > 0).all()
        assert skip == (not (h >= 0).any()) and (h == R.HIT_TERRAIN).any()


def test_down_ray_over_a_known_tread(ctx):
    """Straight down from (1.37, 0.2, 2) in env 2, in the position frame of its pelvis: x = 1.37 lies on tread
    3 of the 0.4 m steps (height 3 x 0.05) and on tread 4 of the 0.3 m steps (height 4 x 0.15)."""
    import torch
    p = ctx.rb[2, 0, :3].astype(np.float64)
    ray = np.array([[1.37 - p[0], 0.2 - p[1], 2.0 - p[2], 0, 0, -1]])
    a = ray[0, :3].astype(np.float32)
    oz = np.float32(ctx.rb[2, 0, 2]) + a[2]  # the origin as the device forms it
    for setting, cell in ((0, 3), (1, 4)):
        ter = TR.settings()[setting]
        _set_terrain(ctx, ter)
        ctx.ren.set_rays(ray, body=0, frame="position")
        dist, hit = ctx.ren.cast_rays(5.0)
        torch.cuda.synchronize()
        want = float(oz) - cell * float(ter["step_height"])
        assert int(hit[2, 0]) == -1 and abs(float(dist[2, 0]) - want) <= 8 * TR.RAY_FLOOR_TERRAIN[2]
        assert int(hit[1, 0]) == -1 and int(hit[3, 0]) == -1  # the slope and the plane under the other envs
    ctx.ren.set_rays(ctx.rays)


def test_sensor_ray_and_camera_centre_pixel_agree(ctx):
    """A camera of odd size has a pixel whose ray is the view axis: a sensor ray from the same point along the
    same axis returns the t the depth image holds (depth = -t there, d = f) and the same thing hit. Views 0 and
    4 look at the stairs; the third looks from parity camera 0's place at the origin of the first body of env 2
    that the float64 reference says its axis hits."""
    import torch
    from humanoid_amd import render as R
    ter = TR.settings()[1]
    _set_terrain(ctx, ter)
    p = ctx.rb[2, 0, :3].astype(np.float64)

    def ray_of(pos, target):
        return np.concatenate([np.array(pos, np.float64) - p, np.array(target, np.float64) - np.array(pos, np.float64)])[None, :]

    pos3 = (1.4, -1.2, 1.5)
    for b in range(24):
        ray = ray_of(pos3, ctx.rb[2, b, :3])
        ray[:, 3:] /= np.linalg.norm(ray[:, 3:])
        if TR.cast(ctx.model.geom_type, ctx.model.geom_params, ctx.rb, ray.astype(np.float32), 0, 0, ter, 20.0, False)[1][2, 0] >= 0:
            break
    else:
        raise AssertionError("no body of env 2 is seen from parity camera 0's place")
    ctx.ren.set_markers(None)  # the sensor never hits one
    seen = set()
    for pos, target in (TR.VIEWS[0][:2], TR.VIEWS[4][:2], (pos3, tuple(float(x) for x in ctx.rb[2, b, :3]))):
        ctx.ren.set_rays(ray_of(pos, target), body=0, frame="position")
        dist, hit = ctx.ren.cast_rays(20.0, skip_bodies=False)
        ctx.ren.set_cameras(_cams([RR.cam(2, pos, target, 60.0, width=71, height=45)]))
        ctx.ren.render(R.FLAGS_DEFAULT)
        torch.cuda.synchronize()
        depth, seg = float(ctx.ren.depth[0, 22, 35]), int(ctx.ren.seg[0, 22, 35])
        t, who = float(dist[2, 0]), int(hit[2, 0])
        print(f"sensor t {t:.6f} hit {who}, camera depth {depth:.6f} seg {seg}")
        assert np.isfinite(t) and abs(t + depth) <= TR.TERRAIN_DEPTH_TOL
        assert who >= -1 and seg == (0 if who == -1 else ctx.seg[2, who])
        seen.add(min(who, 0))
    assert seen == {-1, 0}  # the terrain and a body
    ctx.ren.set_markers(ctx.mpos_t, MARKERS_RGB, MARKER_RADIUS)
    ctx.ren.set_rays(ctx.rays)


def test_ray_outputs_null_sentinel_tails_and_side_stream(ctx):
    """A NULL output is not written and the other is as with both; nothing is written past N x R; a launch on
    a side stream gives the same values; a refused ray set keeps the previous one."""
    import torch
    from humanoid_amd import render as R
    _set_terrain(ctx, TR.settings()[0])
    ctx.ren.set_rays(ctx.rays, body=0, frame="heading")
    full_d, full_h = [x.clone() for x in ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=False)]
    dev = ctx.eng.device
    n, tail = N * 185, 1024
    for pick in ((1, 1), (1, 0), (0, 1)):
        d = torch.full((n + tail,), -7.5, dtype=torch.float32, device=dev) if pick[0] else None
        h = torch.full((n + tail,), -77, dtype=torch.int32, device=dev) if pick[1] else None
        ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=False, dist=d, hit=h)
        torch.cuda.synchronize()
        if d is not None:
            assert torch.equal(d[:n].view(N, 185).view(torch.int32), full_d.view(torch.int32)) and bool((d[n:] == -7.5).all())
        if h is not None:
            assert torch.equal(h[:n].view(N, 185), full_h) and bool((h[n:] == -77).all())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    d, h = torch.zeros_like(full_d), torch.zeros_like(full_h)
    with torch.cuda.stream(side):
        ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=False, dist=d, hit=h)
    side.synchronize()
    assert torch.equal(d.view(torch.int32), full_d.view(torch.int32)) and torch.equal(h, full_h)
    with pytest.raises(R.RenderError, match="max_range"):
        ctx.ren.cast_rays(0.0)
    with pytest.raises(R.RenderError, match="1..1024"):
        ctx.ren.set_rays(np.tile(ctx.rays[:1], (1025, 1)))
    with pytest.raises(R.RenderError, match="not finite"):
        ctx.ren.set_rays(np.array([[0, 0, 1, 0, 0, 0.0]]))  # no direction to normalise
    assert ctx.ren.num_rays == 185
    d2, h2 = ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=False)
    torch.cuda.synchronize()
    assert torch.equal(d2.view(torch.int32), full_d.view(torch.int32)) and torch.equal(h2, full_h)
    # the full ray count, in one launch
    many = np.tile(ctx.rays, (6, 1))[:1024]
    ctx.ren.set_rays(many, body=0, frame="heading")
    d3, h3 = ctx.ren.cast_rays(TR.MAX_RANGE, skip_bodies=False)
    torch.cuda.synchronize()
    assert tuple(d3.shape) == (N, 1024) and torch.equal(h3[:, 185:370], full_h) and torch.equal(h3[:, 925:1024], full_h[:, :99])
    ctx.ren.set_rays(ctx.rays)


def test_facade_draws_the_engines_terrain_and_casts_its_rays():
    """A sim whose engine got set_env_properties(terrain_kind=...) renders that terrain, and cast_ray_sensor
    gives what a Renderer made directly on an identically stepped second sim gives."""
    import torch
    from test_facade_env import _facade_sim
    from humanoid_amd import render as R
    from humanoid_amd.isaacgym import gymapi, gymtorch
    n = 4
    rays = R.height_scan_rays(5, 3, 0.25, 1.0, offset=(0.6, 0.0))
    out = []
    for direct in (False, True):
        gym, sim = _facade_sim(n)
        kind = torch.tensor([0, 1, 2, 7], dtype=torch.int32, device=sim.engine.device)
        sim.engine.set_env_properties(terrain_kind=kind)
        gym.simulate(sim)
        gym.simulate(sim)
        if direct:
            gym.fetch_results(sim, True)
            ren = R.Renderer(sim.engine)
            ren.set_terrain_from_engine()
            ren.set_rays(rays, "Pelvis", "heading")
            dist, hit = ren.cast_rays(5.0, skip_bodies=True)
        else:
            dist = torch.zeros(n, 15, device=sim.engine.device)
            hit = torch.zeros(n, 15, dtype=torch.int32, device=sim.engine.device)
            gym.set_ray_sensor(sim, rays, "Pelvis", "heading")
            assert sim.pending_substeps == 0  # the pending simulates were issued first
            gym.cast_ray_sensor(sim, gymtorch.unwrap_tensor(dist), gymtorch.unwrap_tensor(hit), 5.0)
            # and the cameras of this sim show the terrain: env 2 stands on steps, env 3's kind names none
            props = gymapi.CameraProperties()
            props.width, props.height = W, H
            for env in sim.envs:
                gym.create_camera_sensor(env, props)
                gym.set_camera_location(0, env, gymapi.Vec3(-1.0, -2.0, 1.5), gymapi.Vec3(2.0, 0.0, 0.1))
            gym.render_all_camera_sensors(sim)
            depth = [gym.get_camera_image(sim, env, 0, gymapi.IMAGE_DEPTH) for env in sim.envs]
            ground = [gym.get_camera_image(sim, env, 0, gymapi.IMAGE_SEGMENTATION) == 0 for env in sim.envs]
            par = sim.engine.params
            plain = R.Renderer(sim.engine)
            plain.set_cameras(_cams([RR.cam(e, (-1.0, -2.0, 1.5), (2.0, 0.0, 0.1), 90.0, near=0.001, far=2e6) for e in range(n)]))
            plain.render()
            flat = plain.depth.cpu().numpy()
            assert np.array_equal(depth[0], flat[0]) and np.array_equal(depth[3], flat[3])
            for e in (1, 2):
                assert (depth[e] != flat[e]).mean() > 0.1
            plain.set_terrain(kind, par.terrain_slope, par.step_height, par.step_length)
            plain.render()
            assert all(np.array_equal(depth[e], plain.depth[e].cpu().numpy()) for e in range(n))
            assert all(g.mean() > 0.3 for g in ground)
        torch.cuda.synchronize()
        out.append((dist.clone(), hit.clone()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and torch.equal(out[0][1], out[1][1])
    assert (out[0][1] == -1).all() and torch.isfinite(out[0][0]).all()
    d = out[0][0].cpu().numpy()
    assert np.ptp(d[0]) < 1e-5 and np.ptp(d[1]) > 0.05 and np.ptp(d[2]) > 0.04  # plane, slope, steps


def test_env_render_still_returns_its_frame(model):
    import torch
    from test_facade_env import _clip_dict
    from humanoid_amd.env import EnvConfig, HumanoidPHC
    env = HumanoidPHC(EnvConfig(num_envs=4, motion_file=_clip_dict(model), seed=1, camera=True))
    env.reset()
    env.step(torch.zeros(4, 69, device=env.device))
    frame = env.render()
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (360, 640, 4)
    assert env._renderer._terrain is None  # the env sets no terrain: the plane
    depth = env._renderer.depth[0]
    assert torch.isfinite(depth).float().mean() > 0.3
    env.close()
