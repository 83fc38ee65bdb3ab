"""GPU checks of the camera sensors against the float64 numpy restatement of the image definition
(tests/render_reference.py). Scenes are written straight into the zero-copy rb_state tensor, so no
physics is needed: 4 envs (the pose he_create_envs leaves; two with randomly rotated bodies scattered in
a 1 m cube; one with every body 1000 m away), 70 x 45 images (partial tiles on both edges), 3 cameras on
envs (2, 0, 2) with fovs 90 and 40.

The comparison rule (render_reference.compare): a GPU pixel agrees with the reference when the seg id is
equal, the colour within +-1 level per channel and the depth within DEPTH_TOL = 8 x the reference's own
float32-against-float64 floor (2.8e-5 m); a pixel that does not must agree with the reference at one of
its 8 neighbours (a silhouette, shadow-edge or checker-edge pixel) and such pixels may make up 0.5 % of an
image at most."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
N, K, H, W = RR.N_ENVS, 3, RR.H, RR.W


def _cams(dicts):
    from humanoid_amd import render as R
    return [R.camera(**d) for d in dicts]


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(model):
    """One engine whose rb_state holds the shared scene, one renderer, and the references (computed once)."""
    import torch
    from humanoid_amd import render as R
    from humanoid_amd.engine import Engine
    c = _Ctx()
    c.model = model
    c.eng = Engine(model, N, device=0)
    rbt = c.eng.rb_state.view(N, 24, 13)
    c.rb = RR.scene(env0_rows=rbt[0].cpu().numpy())  # env 0 stays as he_create_envs left it
    rbt.copy_(torch.from_numpy(c.rb).to(c.eng.device))
    c.ren = R.Renderer(c.eng)
    c.seg, c.rgb = RR.distinct_seg(), RR.distinct_rgb()
    c.seg_t = torch.from_numpy(c.seg).to(c.eng.device)
    c.rgb_t = torch.from_numpy(c.rgb).to(c.eng.device)
    c.refs = {}
    return c


def _reference(c, name, cams, flags, markers=None, appearance=True):
    key = (name, flags)
    if key not in c.refs:
        c.refs[key] = RR.render(c.model.geom_type, c.model.geom_params, c.rb, cams, c.rgb if appearance else None,
                                c.seg if appearance else None, markers, flags, np.float64)
    return c.refs[key]


def _gpu(c, cams, flags, appearance=True):
    import torch
    c.ren.set_appearance(c.rgb_t if appearance else None, c.seg_t if appearance else None)
    c.ren.set_cameras(_cams(cams))
    c.ren.render(flags)
    torch.cuda.synchronize()
    return c.ren.color.cpu().numpy(), c.ren.depth.cpu().numpy(), c.ren.seg.cpu().numpy()


def _check_all(img, ref):
    edges = []
    for k in range(ref[0].shape[0]):
        edges.append(RR.check(tuple(x[k] for x in img), tuple(x[k] for x in ref), RR.DEPTH_TOL))
    return edges


def test_empty_env_straight_down(ctx):
    """Camera straight down from height h over the env whose bodies are 1000 m away: depth -h, seg 0, and
    the checker squares where the definition puts them."""
    from humanoid_amd import render as R
    h = 3.0
    cams = RR.down_camera(h)
    ctx.ren.set_markers(None)
    col, dep, seg = _gpu(ctx, cams, R.FLAG_CHECKER)
    assert col.shape == (1, H, W, 4) and dep.shape == (1, H, W) and seg.shape == (1, H, W)
    assert not seg.any() and (col[..., 3] == 255).all()
    assert abs(dep[0, H // 2, W // 2] + h) <= RR.DEPTH_TOL
    np.testing.assert_allclose(dep[0], -h, rtol=0, atol=RR.DEPTH_TOL)
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    gx = cams[0]["pos"][0] + h * (2 * (j + 0.5) / W - 1)
    gy = cams[0]["pos"][1] + h * (1 - 2 * (i + 0.5) / H) * H / W
    odd = (np.floor(gx) + np.floor(gy)).astype(int) & 1
    shade = RR.AMBIENT + (1 - RR.AMBIENT) * RR.LIGHT[2]
    want = np.floor(np.where(odd, RR.GROUND_ODD, RR.GROUND_EVEN) * shade * 255 + 0.5)
    # no pixel centre of this camera is within 1e-3 m of a checker line, so every square is exact
    assert np.abs(gx - np.round(gx)).min() > 1e-3 and np.abs(gy - np.round(gy)).min() > 1e-3
    for ch in range(3):
        assert np.abs(col[0, ..., ch].astype(int) - want).max() <= 1
    assert ((col[0, ..., 0] > 150) == (odd == 0)).all()
    # and by the general rule, with shadows on as well
    ref = _reference(ctx, "down", cams, R.FLAGS_DEFAULT)
    print("edge pixels:", _check_all(_gpu(ctx, cams, R.FLAGS_DEFAULT), ref))


@pytest.mark.parametrize("shadows", [True, False])
def test_parity_with_reference(ctx, shadows):
    from humanoid_amd import render as R
    flags = R.FLAG_CHECKER | (R.FLAG_SHADOWS if shadows else 0)
    cams = RR.parity_cameras()
    ctx.ren.set_markers(None)
    ref = _reference(ctx, "parity", cams, flags)
    img = _gpu(ctx, cams, flags)
    for k in range(K):
        agree, edge = RR.compare(tuple(x[k] for x in img), tuple(x[k] for x in ref), RR.DEPTH_TOL)
        fin = agree & np.isfinite(ref[1][k])
        diff = np.abs(np.where(fin, img[1][k], 0.0) - np.where(fin, ref[1][k], 0.0))
        print(f"camera {k}: {int(edge.sum())} edge pixels, {int((~(agree | edge)).sum())} failing, largest depth "
              f"difference on agreeing pixels {diff.max():.3e} m (tolerance "
              f"{RR.DEPTH_TOL:.3e})")
    _check_all(img, ref)
    # the scene exercises every body id of the viewed envs that the reference sees, and shadows matter
    assert set(np.unique(img[2])) == set(np.unique(ref[2])) and len(np.unique(ref[2])) > 20
    if shadows:
        lit = _reference(ctx, "parity", cams, R.FLAG_CHECKER)
        assert (ref[0] != lit[0]).any(-1).mean() > 0.005
    # culling never changes a pixel
    full = _gpu(ctx, cams, flags | R.FLAG_NO_CULL)
    assert all((a == b).all() for a, b in zip(img, full))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_following_camera_equals_fixed_camera_at_host_pose(ctx, mode):
    """A camera attached to a body draws, bit for bit, what a fixed camera draws at the pose computed on
    the host from the same rb_state (the header's operation order, in float32)."""
    from humanoid_amd import render as R
    ctx.ren.set_markers(None)
    follow = []
    for env, pos, target, fov in ((2, (1.3, -1.9, 0.7), (0.1, 0.2, -0.1), 90.0), (1, (-2.1, 0.4, 1.1), (0.0, 0.1, 0.2), 40.0),
                                  (2, (0.5, 2.2, 1.5), (0.0, 0.0, 0.5), 40.0)):
        # of the env's (randomly rotated) bodies, follow the one that carries the camera highest above the ground
        cands = [RR.cam(env, pos, target, fov, follow_body=b, follow_mode=mode) for b in range(24)]
        follow.append(max(cands, key=lambda cm: float(RR.camera_points(cm, ctx.rb, np.float32)[0][2])))
    assert all(RR.camera_points(cm, ctx.rb, np.float32)[0][2] > 0.5 for cm in follow)
    fixed = []
    for cm in follow:
        P, T = RR.camera_points(cm, ctx.rb, np.float32)
        assert P.dtype == np.float32 and T.dtype == np.float32
        fixed.append(RR.cam(cm["env"], [float(x) for x in P], [float(x) for x in T], cm["hfov_deg"]))
    a = _gpu(ctx, follow, R.FLAGS_DEFAULT)
    b = _gpu(ctx, fixed, R.FLAGS_DEFAULT)
    assert (a[0] == b[0]).all() and (a[2] == b[2]).all()
    assert (a[1].view(np.uint32) == b[1].view(np.uint32)).all()
    assert len(np.unique(a[2])) > 5  # bodies are in view
    if mode == 1:  # the rotation matters: the position-mode image of the same offsets differs
        other = _gpu(ctx, [dict(cm, follow_mode=0) for cm in follow], R.FLAGS_DEFAULT)
        assert (other[2] != a[2]).any()


def test_null_outputs_and_sentinel_tails(ctx):
    """A NULL output is not written and the others are as with all three; nothing is written past the end
    of a buffer (70 x 45 leaves partial tiles on the right and bottom edges)."""
    import torch
    from humanoid_amd import render as R
    cams = RR.parity_cameras()
    ctx.ren.set_markers(None)
    full = _gpu(ctx, cams, R.FLAGS_DEFAULT)
    dev = ctx.eng.device
    n, tail = K * H * W, 4096

    def bufs():
        return (torch.full((n * 4 + tail,), 0xAB, dtype=torch.uint8, device=dev),
                torch.full((n + tail,), -7.5, dtype=torch.float32, device=dev),
                torch.full((n + tail,), -77, dtype=torch.int32, device=dev))

    def same(c, d, s):
        ok = True
        if c is not None:
            ok &= bool((c[:n * 4].cpu().numpy().reshape(K, H, W, 4) == full[0]).all()) and bool((c[n * 4:] == 0xAB).all())
        if d is not None:
            ok &= bool((d[:n].cpu().numpy().reshape(K, H, W).view(np.uint32) == full[1].view(np.uint32)).all())
            ok &= bool((d[n:] == -7.5).all())
        if s is not None:
            ok &= bool((s[:n].cpu().numpy().reshape(K, H, W) == full[2]).all()) and bool((s[n:] == -77).all())
        return ok

    for pick in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
        c, d, s = [b if p else None for b, p in zip(bufs(), pick)]
        ctx.ren.render_into(c, d, s, R.FLAGS_DEFAULT)
        torch.cuda.synchronize()
        assert same(c, d, s), pick
    with pytest.raises(R.RenderError, match="no output"):
        ctx.ren.render_into(None, None, None)
    # a refused camera set launches nothing and keeps the previous set
    before = ctx.ren.color.clone()
    with pytest.raises(R.RenderError, match="share one size"):
        ctx.ren.set_cameras(_cams([RR.cam(0, (1, 1, 1), (0, 0, 0)), RR.cam(0, (1, 1, 1), (0, 0, 0), width=W + 1)]))
    with pytest.raises(R.RenderError, match="env 4"):
        ctx.ren.set_cameras(_cams([RR.cam(4, (1, 1, 1), (0, 0, 0))]))
    assert ctx.ren.num_cameras == K and torch.equal(ctx.ren.render(R.FLAGS_DEFAULT), before)


def _project(cm, X):
    """Pixel (row, column) of the world point X for a fixed camera, by the header's camera definition."""
    P, T = np.array(cm["pos"], float), np.array(cm["target"], float)
    f = (T - P) / np.linalg.norm(T - P)
    r = np.cross(f, [0, 0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    v = np.asarray(X, float) - P
    th = np.tan(np.radians(cm["hfov_deg"]) / 2)
    x, y = (v @ r) / (v @ f) / th, (v @ u) / (v @ f) / (th * cm["height"] / cm["width"])
    return int(np.floor((1 - y) / 2 * cm["height"])), int(np.floor((x + 1) / 2 * cm["width"]))


def test_markers_occlude_and_cast_no_shadow(ctx):
    import torch
    from humanoid_amd import render as R
    cm = RR.parity_cameras()[1]  # env 0: the bodies around the origin
    P, T = np.array(cm["pos"]), np.array(cm["target"])
    ctx.ren.set_markers(None)
    plain = _gpu(ctx, [cm], R.FLAGS_DEFAULT)
    ci, cj = H // 2, W // 2
    body_at_centre = plain[2][0, ci - 1:ci + 1, cj - 1:cj + 1]
    assert (body_at_centre > 0).all() and (body_at_centre != R.SEG_MARKER).all()
    # marker 0 on the central ray in front of the bodies, marker 1 over open ground
    mpos = np.zeros((N, 2, 3), np.float32)
    mpos[:, 0] = P + 0.5 * (T - P)
    mpos[:, 1] = (-0.6, 0.5, 0.25)
    radius = 0.05
    mk = torch.from_numpy(mpos).to(ctx.eng.device)
    ctx.ren.set_markers(mk, [(0.8, 0.0, 0.0), (0.1, 0.9, 0.1)], radius)
    img = _gpu(ctx, [cm], R.FLAGS_DEFAULT)
    ctx.ren.set_markers(None)
    centre = img[2][0, ci - 1:ci + 1, cj - 1:cj + 1]
    assert (centre == R.SEG_MARKER).all()
    want_depth = -(0.5 * np.linalg.norm(T - P) - radius)
    assert abs(img[1][0, ci, cj] - want_depth) < 2e-3  # the pixel centre is half a pixel off the axis
    assert img[0][0, ci, cj, 0] > img[0][0, ci, cj, 1] + 40  # red
    # markers cast no shadow: every pixel that is not a marker is exactly as without markers ...
    rest = img[2][0] != R.SEG_MARKER
    assert rest.sum() > 0.9 * H * W and (~rest).sum() > 8
    assert (img[0][0][rest] == plain[0][0][rest]).all() and (img[1][0][rest] == plain[1][0][rest]).all()
    # ... in particular the ground point where marker 1's shadow would fall, which is in view, lit ground
    spot = mpos[0, 1] - np.array(RR.LIGHT) * (mpos[0, 1, 2] / RR.LIGHT[2])
    si, sj = _project(cm, spot)
    assert 0 <= si < H and 0 <= sj < W and img[2][0, si, sj] == 0 and np.isfinite(img[1][0, si, sj])
    lit = _reference(ctx, "marker-lit", [cm], R.FLAG_CHECKER)
    assert np.abs(img[0][0, si, sj].astype(int) - lit[0][0, si, sj].astype(int)).max() <= 1
    # and the whole image agrees with the reference, which draws markers and lets them cast nothing
    ref = _reference(ctx, "markers", [cm], R.FLAGS_DEFAULT, markers=(mpos, [(0.8, 0.0, 0.0), (0.1, 0.9, 0.1)], radius))
    _check_all(img, ref)
    assert (ref[2] == R.SEG_MARKER).sum() > 8


def test_rendering_leaves_the_engine_alone(model):
    import torch
    from humanoid_amd import _abi
    from humanoid_amd import render as R
    from humanoid_amd.body_sets import frozen_dof_mask
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import pd_action_offset_scale
    n = 4
    off, sc = pd_action_offset_scale(model)
    frozen = np.array(frozen_dof_mask(), np.int32)
    g = torch.Generator().manual_seed(3)
    actions = [(0.3 * torch.randn(n, 69, generator=g)).cuda() for _ in range(10)]
    kinds = [k for k in range(12)]
    states = []
    for with_render in (False, True):
        eng = Engine(model, n, device=0)
        eng.set_pd_params(off, sc, frozen)
        root = torch.zeros(n, 13, device=eng.device)
        root[:, 2], root[:, 6] = 0.95, 1.0
        root[:, 0] = torch.arange(n, device=eng.device) * 0.3
        eng.set_root_state_indexed(root, torch.arange(n, dtype=torch.int32, device=eng.device))
        ren = None
        if with_render:
            ren = R.Renderer(eng)
            ren.set_cameras(_cams([RR.cam(e, (0.0, -3.0, 1.5), (0.0, 0.0, 0.8), follow_body=0, follow_mode=2)
                                   for e in (2, 0, 2)]))
        for a in actions:
            eng.step_actions(a, 2)
            if ren is not None:
                before = [eng.buffer(k).clone() for k in kinds]
                ren.render()
                torch.cuda.synchronize()
                assert all(torch.equal(b.view(torch.int32), eng.buffer(k).view(torch.int32))
                           for b, k in zip(before, kinds))
        torch.cuda.synchronize()
        states.append([eng.buffer(k).clone() for k in (_abi.BUF_ROOT_STATE, _abi.BUF_DOF_STATE, _abi.BUF_RB_STATE,
                                                      _abi.BUF_CONTACT_FORCE, _abi.BUF_CONTACT_CACHE)])
        if ren is not None:
            assert len(torch.unique(ren.seg)) == 1 and (ren.color[..., :3].float().std() > 5)  # something was drawn
    for a, b in zip(*states):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(states[0][0][:, 2].min()) > 0.3  # the humanoids were simulated, not left at rest


def test_gym_facade_end_to_end():
    """The reference's recording order (render_env.py:151-171, 218-227, 398-411) through the facade."""
    import torch
    from test_facade_env import _facade_sim
    from humanoid_amd.isaacgym import gymapi, gymtorch
    n = 4
    gym, sim = _facade_sim(n)
    envs = sim.envs
    props = gymapi.CameraProperties()
    props.width, props.height, props.horizontal_fov = W, H, 60.0
    handles = [gym.create_camera_sensor(env, props) for env in envs]  # after prepare_sim, as the reference
    assert handles == [0] * n
    with pytest.raises(NotImplementedError):
        gym.create_camera_sensor(envs[0], gymapi.CameraProperties())
    for e, env in enumerate(envs):
        gym.set_camera_location(handles[e], env, gymapi.Vec3(0.1 * e + 1.2, -2.2, 1.3), gymapi.Vec3(0.1 * e, 0.0, 0.85))
        for b in range(24):
            gym.set_rigid_body_segmentation_id(env, 0, b, b + 1)
    gym.simulate(sim)
    gym.simulate(sim)
    assert sim.pending_substeps == 2
    gym.render_all_camera_sensors(sim)  # flushes the pending simulates first
    assert sim.pending_substeps == 0
    gym.step_graphics(sim)
    e = 1
    col = gym.get_camera_image(sim, envs[e], handles[e], gymapi.IMAGE_COLOR)
    dep = gym.get_camera_image(sim, envs[e], handles[e], gymapi.IMAGE_DEPTH)
    seg = gym.get_camera_image(sim, envs[e], handles[e], gymapi.IMAGE_SEGMENTATION)
    assert isinstance(col, np.ndarray) and col.dtype == np.uint8 and col.shape == (H, W * 4)
    assert dep.dtype == np.float32 and dep.shape == (H, W) and seg.dtype == np.int32 and seg.shape == (H, W)
    rgba = col.reshape(col.shape[0], -1, 4)  # render_env.py:160
    assert (rgba[..., 3] == 255).all() and (dep[np.isfinite(dep)] < 0).all()
    ids = set(np.unique(seg))
    assert 0 in ids and len(ids) > 10 and ids <= set(range(25))
    with pytest.raises(NotImplementedError):
        gym.get_camera_image(sim, envs[e], handles[e], gymapi.IMAGE_OPTICAL_FLOW)
    # the GPU tensor aliases the memory the numpy copy came from
    gym.start_access_image_tensors(sim)
    t = gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, envs[e], handles[e], gymapi.IMAGE_COLOR))
    gym.end_access_image_tensors(sim)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (H, W, 4)
    assert t.data_ptr() == sim.renderer.color[e].data_ptr() and (t.cpu().numpy() == rgba).all()
    td = gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, envs[e], handles[e], gymapi.IMAGE_DEPTH))
    assert td.data_ptr() == sim.renderer.depth[e].data_ptr() and tuple(td.shape) == (H, W)
    # set_rigid_body_color changes only that body's pixels
    body = int(np.bincount(seg[seg > 0]).argmax()) - 1
    gym.set_rigid_body_color(envs[e], 0, body, gymapi.MESH_VISUAL, gymapi.Vec3(0.1, 0.2, 0.9))
    gym.render_all_camera_sensors(sim)
    rgba2 = t.cpu().numpy()  # the alias shows the new render
    changed = (rgba2 != rgba).any(-1)
    assert changed.any() and (changed == (seg == body + 1)).all()
    other = gym.get_camera_image(sim, envs[2], handles[2], gymapi.IMAGE_SEGMENTATION)
    # the image differs after the humanoid has been moved by an indexed root-state write
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    src = root.clone()
    src[e, 0] += 0.6
    ids_t = torch.tensor([e], dtype=torch.int32, device=src.device)
    gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src), gymtorch.unwrap_tensor(ids_t), 1)
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.render_all_camera_sensors(sim)
    seg3 = gym.get_camera_image(sim, envs[e], handles[e], gymapi.IMAGE_SEGMENTATION)
    assert (seg3 != seg).mean() > 0.02
    # env 2 was simulated one more step but not moved: its image stays nearly the same
    other3 = gym.get_camera_image(sim, envs[2], handles[2], gymapi.IMAGE_SEGMENTATION)
    assert (other3 != other).mean() < 0.02


def test_env_render_returns_frames_with_markers(model):
    import torch
    from test_facade_env import _clip_dict
    from humanoid_amd.env import EnvConfig, HumanoidPHC
    clips = _clip_dict(model)
    env = HumanoidPHC(EnvConfig(num_envs=4, motion_file=clips, seed=1, camera=True))
    env.reset()
    for _ in range(10):  # zero actions: the humanoid leaves its reference motion, so the markers show
        env.step(torch.zeros(4, 69, device=env.device))
    env.viewing_env_idx = 2  # chosen before the first frame: palette colour 2, green
    g = env.render().cpu().numpy().astype(int)
    on_body = (env._renderer.seg[0].cpu().numpy() == 0) & np.isfinite(env._renderer.depth[0].cpu().numpy())
    assert ((g[..., 1] > g[..., 0] + 30) & (g[..., 1] > g[..., 2] + 30) & on_body).sum() > 50
    env.viewing_env_idx = 0
    frame = env.render()
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (360, 640, 4)
    f = frame.cpu().numpy().astype(int)
    assert (f != g).any()
    red = (f[..., 0] > 60) & (f[..., 1] < 30) & (f[..., 2] < 30)
    assert red.sum() > 50
    assert (env._renderer.seg[0] == 1000).sum() >= red.sum() > 0
    # the humanoid (palette colour 0, blue) is in view too, and the camera follows the viewed env
    assert ((f[..., 2] > f[..., 0] + 30) & (env._renderer.seg[0].cpu().numpy() == 0)
            & np.isfinite(env._renderer.depth[0].cpu().numpy())).sum() > 50
    env.close()
    off = HumanoidPHC(EnvConfig(num_envs=4, motion_file=clips, seed=1))
    assert off.render() is None
    off.close()
