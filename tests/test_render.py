"""CPU checks of the camera sensors: the render library's ABI, its argument checks, the gym facade's
camera bookkeeping, the numpy reference's own rounding (the cap margin and the depth floor the GPU tests
use), and the PNG writer. The image itself is checked on the GPU (test_gpu_render.py)."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_reference as RR  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_render.h")


def _lib():
    from humanoid_amd import build, render
    if not os.path.exists(render.LIB_PATH):
        build.build()
    return render.load_library()


def test_render_library_exports_every_declared_symbol():
    from humanoid_amd import render
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hr_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) >= 9
    assert not [s for s in syms if not hasattr(lib, s)]
    assert set(syms) == set(render.HR_SYMBOLS)
    assert lib.hr_version() == 1
    # the engine's header scan (test_abi.py) must not pick anything up from this header
    assert not re.findall(r"\bhe_[a-z_0-9]+\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))


def test_render_library_is_not_part_of_the_engine():
    """The renderer is a library of its own: its sources are not among the engine's, and every header
    they include is tracked by the build."""
    from humanoid_amd import build
    libs = build.LIBRARIES
    assert [name for name, lib in libs.items() if any(s.startswith("hr_") for s, _ in lib.sources)] == ["render"]
    assert libs["render"].sources == [("hr_render.hip", [])] and libs["render"].path != libs["engine"].path
    assert any(h.endswith("humanoid_render.h") for h in build.HEADERS)
    # the render kernels (the template's two instantiations by their arguments) and the ray caster: no scratch
    assert build.BUDGETS["hr_render.hip"] == {k: build.Budget(max_scratch=0)
                                              for k in ("render_kernel<false>", "render_kernel<true>", "rays_kernel")}


def test_camera_struct_and_constants_match_header(tmp_path):
    from humanoid_amd import render
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "humanoid_render.h"\n'
                   'int main(){printf("%zu %zu %zu %d %d %u %u %u %d %d %d\\n", sizeof(hr_camera), '
                   "offsetof(hr_camera, follow_body), offsetof(hr_camera, target), HR_SEG_MARKER, HR_MAX_MARKERS, "
                   "HR_FLAG_SHADOWS, HR_FLAG_CHECKER, HR_FLAG_NO_CULL, HR_FOLLOW_POSITION, HR_FOLLOW_TRANSFORM, "
                   "HR_FOLLOW_POSITION_XY);"
                   'printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\\n", HR_AMBIENT, '
                   "HR_SHADOW, HR_SHADOW_EPS, HR_LIGHT_X, HR_LIGHT_Y, HR_LIGHT_Z, HR_SKY_R, HR_SKY_G, HR_SKY_B, "
                   "HR_GROUND_EVEN, HR_GROUND_ODD, HR_BODY_R, HR_BODY_G, HR_BODY_B);}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    ints, floats = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    H = render.HrCamera
    assert [int(x) for x in ints.split()] == [
        C.sizeof(H), H.follow_body.offset, H.target.offset, render.SEG_MARKER, render.MAX_MARKERS, render.FLAG_SHADOWS,
        render.FLAG_CHECKER, render.FLAG_NO_CULL, render.FOLLOW_POSITION, render.FOLLOW_TRANSFORM,
        render.FOLLOW_POSITION_XY]
    # the reference restates the header's constants, the product its default colour
    want = [RR.AMBIENT, RR.SHADOW, RR.SHADOW_EPS, *RR.LIGHT, *RR.SKY, RR.GROUND_EVEN, RR.GROUND_ODD, *RR.BODY_RGB]
    assert np.float32([float(x) for x in floats.split()]).tolist() == np.float32(want).tolist()
    assert tuple(np.float32(render.BODY_RGB)) == tuple(np.float32(RR.BODY_RGB))
    assert RR.SEG_MARKER == render.SEG_MARKER and abs(np.linalg.norm(RR.LIGHT) - 1) < 1e-12


def test_create_without_gpu_reports(he_model):
    import torch
    lib = _lib()
    h = C.c_void_p()
    if not torch.cuda.is_available():
        assert lib.hr_create(0, C.byref(he_model), 4, C.byref(h)) != 0
        assert "HIP device" in lib.hr_last_error().decode() and not h.value
    assert lib.hr_create(0, None, 4, C.byref(h)) != 0 and "model" in lib.hr_last_error().decode()
    assert lib.hr_create(0, C.byref(he_model), 0, C.byref(h)) != 0 and "num_envs" in lib.hr_last_error().decode()


def test_create_refuses_a_model_the_engine_would_refuse(he_model):
    """hr_create runs the structural model check the engine and the dynamics library run, and says why."""
    import copy
    lib = _lib()
    h = C.c_void_p()
    for index, parent, word in ((0, 0, "root"), (5, 7, "DFS")):
        m = copy.deepcopy(he_model)
        m.parents[index] = parent
        assert lib.hr_create(0, C.byref(m), 4, C.byref(h)) != 0 and not h.value
        text = lib.hr_last_error().decode()
        assert text.startswith("hr_create: ") and word in text, text
    for field, value, word in (("num_bodies", 23, "bodies"), ("num_dof", 68, "dofs"), ("num_pairs", 257, "pair")):
        m = copy.deepcopy(he_model)
        setattr(m, field, value)
        assert lib.hr_create(0, C.byref(m), 4, C.byref(h)) != 0 and word in lib.hr_last_error().decode()
    m = copy.deepcopy(he_model)
    m.geom_type[3] = 9
    assert lib.hr_create(0, C.byref(m), 4, C.byref(h)) != 0 and "geom type 9" in lib.hr_last_error().decode()


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def test_render_into_checks_tensors_before_any_library_call():
    """render_into hands the kernel raw pointers it writes K*H*W pixels through: a tensor that is not on the
    device, of another dtype, non-contiguous, no tensor at all or too short is refused by name first."""
    import torch
    from humanoid_amd import render
    k, hgt, w, n_envs = 2, 5, 7, 3
    n = k * hgt * w
    r = object.__new__(render.Renderer)
    r.lib, r.h, r.engine = _NoCalls(), None, None
    r.num_cameras, r.height, r.width, r.num_envs = k, hgt, w, n_envs
    good = {"color": torch.zeros(4 * n, dtype=torch.uint8), "depth": torch.zeros(n), "seg": torch.zeros(n, dtype=torch.int32),
            "rb_state": torch.zeros(n_envs * 24, 13)}
    wrong_dtype = {"color": torch.float32, "depth": torch.float64, "seg": torch.int64, "rb_state": torch.float64}
    for name, ok in good.items():
        bad = {
            "a CPU tensor": (torch.device("cuda", 0), ok),
            "a wrong dtype": (torch.device("cpu"), ok.to(wrong_dtype[name])),
            "non-contiguous": (torch.device("cpu"), torch.stack([ok, ok], -1)[..., 0]),
            "not a tensor": (torch.device("cpu"), ok.numpy()),
            "too short": (torch.device("cpu"), ok.reshape(-1)[:-1]),
        }
        for what, (device, t) in bad.items():
            r.device = device
            assert what != "non-contiguous" or not t.is_contiguous()
            with pytest.raises(render.RenderError, match=name):
                r.render_into(**{name: t})
    # tensors that pass reach the library call, and only then: flat and longer than needed is accepted
    r.device = torch.device("cpu")
    long = {name: torch.cat([t.reshape(-1), t.reshape(-1)]) for name, t in good.items()}
    with pytest.raises(AssertionError, match="library call hr_render"):
        r.render_into(**long)


def test_invalid_camera_sets_are_refused():
    from humanoid_amd import render
    lib = _lib()
    ok = dict(env=1, width=70, height=45, pos=(1, 2, 3), target=(0, 0, 1))

    def refused(cams, n=4, k=None):
        arr = (render.HrCamera * max(len(cams), 1))(*cams)
        rc = lib.hr_validate_cameras(arr, len(cams) if k is None else k, n)
        return lib.hr_last_error().decode() if rc else None

    assert refused([render.camera(**ok), render.camera(**dict(ok, env=3, follow_body=5, follow_mode=1))]) is None
    assert "k = 0" in refused([], k=0)
    assert "k = -1" in refused([render.camera(**ok)], k=-1)
    assert "share one size" in refused([render.camera(**ok), render.camera(**dict(ok, width=71))])
    assert "share one size" in refused([render.camera(**ok), render.camera(**dict(ok, height=44))])
    assert "env 4 outside" in refused([render.camera(**dict(ok, env=4))])
    assert "env -1 outside" in refused([render.camera(**ok), render.camera(**dict(ok, env=-1))])
    assert "not positive" in refused([render.camera(**dict(ok, width=0))])
    assert "not positive" in refused([render.camera(**dict(ok, height=-3))])
    assert "fov" in refused([render.camera(**dict(ok, hfov_deg=0.0))])
    assert "fov" in refused([render.camera(**dict(ok, hfov_deg=-10.0))])
    assert "fov" in refused([render.camera(**dict(ok, hfov_deg=180.0))])
    assert "near plane" in refused([render.camera(**dict(ok, near=0.0))])
    assert "near plane" in refused([render.camera(**dict(ok, near=-1.0))])
    assert "far plane" in refused([render.camera(**dict(ok, near=2.0, far=1.0))])
    assert "follow_body" in refused([render.camera(**dict(ok, follow_body=24))])
    assert "follow_mode" in refused([render.camera(**dict(ok, follow_body=0, follow_mode=3))])
    with pytest.raises(render.RenderError, match="share one size"):
        render.validate_cameras([render.camera(**ok), render.camera(**dict(ok, width=71))], 4)
    # entry points refuse a null handle with a message instead of touching it
    for call in (lambda: lib.hr_set_cameras(None, None, 0), lambda: lib.hr_set_appearance(None, None, None),
                 lambda: lib.hr_set_markers(None, None, 0, None, 0.0),
                 lambda: lib.hr_render(None, None, None, None, None, 3, None)):
        assert call() != 0 and "null handle" in lib.hr_last_error().decode()


def _facade_sim(n=3):
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.Gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    from humanoid_amd.model import DEFAULT_MODEL_JSON
    asset = gym.load_asset(sim, os.path.dirname(DEFAULT_MODEL_JSON), os.path.basename(DEFAULT_MODEL_JSON))
    envs = []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 2)
        gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 0.89)), "humanoid", i, 0, 7 if i == 1 else 0)
        envs.append(env)
    return gymapi, gym, sim, envs


def test_facade_camera_bookkeeping_without_device():
    gymapi, gym, sim, envs = _facade_sim()
    p = gymapi.CameraProperties()
    assert (p.width, p.height, p.horizontal_fov, p.near_plane, p.far_plane, p.enable_tensors) == (
        1600, 900, 90.0, 0.001, 2e6, False)
    assert len({gymapi.IMAGE_COLOR, gymapi.IMAGE_DEPTH, gymapi.IMAGE_SEGMENTATION, gymapi.IMAGE_OPTICAL_FLOW}) == 4
    assert len({gymapi.MESH_NONE, gymapi.MESH_COLLISION, gymapi.MESH_VISUAL, gymapi.MESH_VISUAL_AND_COLLISION}) == 4
    assert gymapi.FOLLOW_POSITION != gymapi.FOLLOW_TRANSFORM
    small = gymapi.CameraProperties()
    small.width, small.height = 70, 45
    # handles count the env's own cameras, as Isaac Gym's do; the sim keeps them in creation order
    assert gym.create_camera_sensor(envs[2], small) == 0
    assert gym.create_camera_sensor(envs[0], small) == 0
    assert gym.create_camera_sensor(envs[2], small) == 1
    assert [c.env for c in sim.cameras] == [2, 0, 2] and envs[2].cameras == [0, 2]
    with pytest.raises(NotImplementedError, match="share one size"):
        gym.create_camera_sensor(envs[1], gymapi.CameraProperties())
    assert len(sim.cameras) == 3
    gym.set_camera_location(1, envs[2], gymapi.Vec3(1, 2, 3), gymapi.Vec3(0, 0, 1))
    assert sim.cameras[2].pos == (1.0, 2.0, 3.0) and sim.cameras[2].target == (0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="no camera 2"):
        gym.set_camera_location(2, envs[2], gymapi.Vec3(), gymapi.Vec3())
    # a transform looks along its +X axis: a quarter turn about z looks along +y
    s = np.sqrt(0.5)
    gym.set_camera_transform(0, envs[0], gymapi.Transform(gymapi.Vec3(1, 1, 1), gymapi.Quat(0, 0, s, s)))
    np.testing.assert_allclose(sim.cameras[1].target, (1, 2, 1), atol=1e-12)
    gym.attach_camera_to_body(0, envs[0], 3, gymapi.Transform(gymapi.Vec3(-2, 0, 1)), gymapi.FOLLOW_TRANSFORM)
    assert (sim.cameras[1].follow_body, sim.cameras[1].follow_mode) == (3, 1)
    np.testing.assert_allclose(sim.cameras[1].target, (-1, 0, 1), atol=1e-12)
    gym.set_camera_location(0, envs[0], gymapi.Vec3(1, 2, 3), gymapi.Vec3(0, 0, 1))
    assert sim.cameras[1].follow_body == -1
    # appearance: create_actor's segmentation id is the actor's default, bodies override it
    assert envs[1].body_seg.tolist() == [7] * 24 and envs[0].body_seg.tolist() == [0] * 24
    gym.set_rigid_body_segmentation_id(envs[1], 0, 5, 9)
    assert envs[1].body_seg[5] == 9 and envs[1].body_seg[4] == 7
    gym.set_rigid_body_color(envs[0], 0, 2, gymapi.MESH_VISUAL, gymapi.Vec3(1, 0, 0))
    assert envs[0].body_rgb[2].tolist() == [1, 0, 0] and envs[0].body_rgb[1].tolist() == list(np.float32(RR.BODY_RGB))
    # nothing has been drawn: images are refused with a reason, optical flow always
    with pytest.raises(RuntimeError, match="before render_all_camera_sensors"):
        gym.get_camera_image(sim, envs[0], 0, gymapi.IMAGE_COLOR)
    with pytest.raises(NotImplementedError, match="OPTICAL_FLOW"):
        gym.get_camera_image(sim, envs[0], 0, gymapi.IMAGE_OPTICAL_FLOW)
    with pytest.raises(RuntimeError, match="before prepare_sim"):
        gym.render_all_camera_sensors(sim)
    with pytest.raises(NotImplementedError, match="viewer"):
        gym.create_viewer(sim, gymapi.CameraProperties())


def test_env_config_camera_defaults():
    from humanoid_amd.env import EnvConfig
    c = EnvConfig()
    assert (c.camera, c.camera_width, c.camera_height) == (False, 640, 360)


def test_reference_self_check(model):
    """The reference against itself, float32 against float64, on the GPU tests' scenes: its own rounding
    moves at most a quarter of the cap's pixels, and its depth differs by at most DEPTH_FLOOR on the pixels
    that agree -- the floor the GPU tests' depth tolerance (8 x) is measured from."""
    rb = RR.scene()
    segs, rgbs = RR.distinct_seg(), RR.distinct_rgb()
    mk = (np.random.default_rng(5).uniform(-0.5, 0.5, (RR.N_ENVS, 3, 3)).astype(np.float32) + np.float32([0, 0, 1]),
          [(0.8, 0.0, 0.0)], 0.05)
    floor, worst = 0.0, 0
    for cams, markers in ((RR.parity_cameras(), None), (RR.parity_cameras(), mk), (RR.down_camera(), None)):
        for flags in (RR.FLAG_SHADOWS | RR.FLAG_CHECKER, RR.FLAG_CHECKER):
            r64 = RR.render(model.geom_type, model.geom_params, rb, cams, rgbs, segs, markers, flags, np.float64)
            r32 = RR.render(model.geom_type, model.geom_params, rb, cams, rgbs, segs, markers, flags, np.float32)
            for k in range(len(cams)):
                a, b = tuple(x[k] for x in r32), tuple(x[k] for x in r64)
                agree, edge = RR.compare(a, b, np.inf)
                assert (agree | edge).all()
                worst = max(worst, int(edge.sum()))
                fin = agree & np.isfinite(b[1])
                with np.errstate(invalid="ignore"):
                    floor = max(floor, float(np.abs(a[1] - b[1])[fin].max()))
                # the scenes are worth testing on: bodies, ground and (first parity camera) sky in view
                if len(cams) == 3:
                    assert len(np.unique(b[2])) >= 8 and (b[2] == 0).any()
            if len(cams) == 3:
                assert np.isinf(r64[1][0]).any() and not np.isinf(r64[1][1]).any()
    quarter = 0.25 * RR.CAP * RR.W * RR.H
    print(f"reference float32 vs float64: at most {worst} edge pixels per image (a quarter of the cap: {quarter:.1f}), "
          f"depth floor {floor:.3e} m, GPU depth tolerance {RR.DEPTH_TOL:.3e} m")
    assert worst <= quarter
    assert 0.5 * RR.DEPTH_FLOOR <= floor <= RR.DEPTH_FLOOR, floor
    assert RR.DEPTH_TOL == 8 * RR.DEPTH_FLOOR and RR.DEPTH_TOL <= 1e-3


def test_reference_down_camera_matches_closed_form(model):
    """The reference itself on the one scene with a closed form: straight down from height h, pixel (i, j)
    sees the ground point (cx + h x, cy + h y), depth -h everywhere."""
    h = 3.0
    cams = RR.down_camera(h)
    col, dep, seg = RR.render(model.geom_type, model.geom_params, RR.scene(), cams, flags=RR.FLAG_CHECKER)
    np.testing.assert_allclose(dep[0], -h, atol=1e-12)
    assert not seg.any()
    j, i = np.meshgrid(np.arange(RR.W), np.arange(RR.H))
    gx = cams[0]["pos"][0] + h * (2 * (j + 0.5) / RR.W - 1)
    gy = cams[0]["pos"][1] + h * (1 - 2 * (i + 0.5) / RR.H) * RR.H / RR.W
    odd = (np.floor(gx) + np.floor(gy)).astype(int) & 1
    shade = RR.AMBIENT + (1 - RR.AMBIENT) * RR.LIGHT[2]
    want = np.floor(np.where(odd, RR.GROUND_ODD, RR.GROUND_EVEN) * shade * 255 + 0.5)
    assert (col[0, ..., 0] == want).all() and (col[0, ..., 3] == 255).all()
    assert 0.3 < odd.mean() < 0.7


def test_save_png_round_trip(tmp_path):
    from humanoid_amd.render import save_png
    g = np.random.default_rng(0)
    for ch in (4, 3):
        img = g.integers(0, 256, (45, 70, ch), dtype=np.uint8)
        path = tmp_path / f"a{ch}.png"
        save_png(str(path), img)
        data = path.read_bytes()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, chunks = 8, []
        while pos < len(data):
            n, tag = struct.unpack(">I4s", data[pos:pos + 8])
            body = data[pos + 8:pos + 8 + n]
            crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
            assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
            chunks.append((tag, body))
            pos += 12 + n
        assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (70, 45, 8, 6 if ch == 4 else 2, 0, 0, 0)
        raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(45, 1 + 70 * ch)
        assert not raw[:, 0].any()  # filter type 0 on every row
        assert (raw[:, 1:].reshape(45, 70, ch) == img).all()
    with pytest.raises(ValueError):
        save_png(str(tmp_path / "b.png"), np.zeros((4, 4), np.uint8))
