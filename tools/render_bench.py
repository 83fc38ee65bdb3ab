"""Time the camera-sensor kernel (hr_render): HIP events around 100 launches after 20 warm-up launches,
one process. Cases: one 1600 x 900 camera and 64 cameras of 320 x 180 (one per env), each with shadows on
and off and with tile culling on and off (HR_FLAG_NO_CULL). The scene is 64 standing humanoids with 24 red
markers each, seen by the env's tracking camera (4 m behind, 2 m up, as HumanoidPHC.render()).

Next to each time the record carries the plain work count of a launch without culling -- pixels x
primitives tested by the primary rays (48 per pixel: 24 geoms + 24 markers) and, with shadows, 24 more for
every pixel that hits something lit -- so the figure can be judged.

Two more groups of cases follow the plane's (--cases picks: plane, terrain, rays, or all): the same two camera
sets with every env on the box steps (hr_set_terrain, shadows and culling on; the sky rays walk the cells of
the steps, so the frame costs more than the plane's), and the ray-cast sensor (hr_cast_rays) as a height scan
of 11 x 11 rays under each of 4096 standing humanoids, terrain only and with the bodies.

--lib times another build of the render library at the same shapes (the parent commit's, say, next to this
one's, alternately, in processes of their own); cases whose entry points that build lacks are left out.

    python tools/render_bench.py [--out profiles/r08/render_bench.json] [--cases all] [--lib PATH]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import NB, ROOT  # noqa: E402


def standing_pose(model, n, rng):
    """rb_state [n,24,13]: the rest pose (identity rotations, joint offsets summed down the tree) at
    z = 0.89 with a sub-metre xy jitter."""
    rb = np.zeros((n, NB, 13), np.float32)
    pos = np.zeros((NB, 3))
    for b in range(NB):
        p = int(model.parents[b])
        pos[b] = (pos[p] if p >= 0 else np.array([0.0, 0.0, 0.89])) + (model.local_pos[b] if p >= 0 else 0.0)
    rb[:, :, :3] = pos[None] + np.concatenate([rng.uniform(-1, 1, (n, 1, 2)), np.zeros((n, 1, 1))], -1)
    rb[:, :, 6] = 1.0
    return rb


def main():
    ap = bc.parser("profiles/r08/render_bench.json", envs=None, warmup=20, calls=None, blocks=None)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--cases", default="all", choices=("all", "plane", "terrain", "rays"))
    ap.add_argument("--lib", default=None, help="another build of libhumanoid_render.so to time")
    args = ap.parse_args()
    import torch
    from humanoid_amd import render as R
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    if args.lib:  # bind what that build exports; a case that needs more is left out below
        import ctypes
        other = ctypes.CDLL(args.lib)
        R._LIBRARY.prototypes = {k: v for k, v in R.HR_PROTOTYPES.items() if hasattr(other, k)}
        R.load_library(args.lib)
    has_new = "hr_set_terrain" in R._LIBRARY.prototypes
    want = lambda group: args.cases in ("all", group) and (group == "plane" or has_new)  # noqa: E731

    def launch_ms(fn):  # ms per call: HIP events around `launches` calls after `warmup` calls
        for _ in range(args.warmup):
            fn()
        return bc.timed(fn, args.launches)

    model = load_default_model()
    n = 64
    eng = Engine(model, n, device=0)
    rng = np.random.default_rng(0)
    rb = standing_pose(model, n, rng)
    eng.rb_state.view(n, NB, 13).copy_(torch.from_numpy(rb).to(eng.device))
    ren = R.Renderer(eng)
    mpos = torch.from_numpy(rb[:, :, :3] + rng.normal(0, 0.08, (n, NB, 3)).astype(np.float32)).to(eng.device).contiguous()
    ren.set_markers(mpos, (0.8, 0.0, 0.0), 0.05)
    results = []
    for name, k, w, h in (("1x1600x900", 1, 1600, 900), ("64x320x180", 64, 320, 180)):
        ren.set_cameras([R.camera(e, w, h, (0.0, -4.0, 2.0), (0.0, 0.0, 1.0), follow_body=0,
                                  follow_mode=R.FOLLOW_POSITION_XY) for e in range(k)])
        ren.render(R.FLAGS_DEFAULT)
        torch.cuda.synchronize()
        pixels = k * w * h
        hit = int(torch.isfinite(ren.depth).sum())
        for shadows in (True, False):
            for cull in (True, False):
                if not want("plane"):
                    continue
                flags = R.FLAG_CHECKER | (R.FLAG_SHADOWS if shadows else 0) | (0 if cull else R.FLAG_NO_CULL)
                ms = launch_ms(lambda: ren.render(flags))
                tests = pixels * 48 + (hit * NB if shadows else 0)
                results.append(dict(case=name, cameras=k, width=w, height=h, shadows=shadows, culling=cull,
                                    ms_per_render=round(ms, 5), pixels=pixels, pixels_hit=hit,
                                    primitive_tests_unculled=tests,
                                    gtests_per_s_unculled_equivalent=round(tests / ms / 1e6, 2)))
                print(json.dumps(results[-1]), flush=True)
        if want("terrain"):  # every env on the steps of the engine's defaults (0.05 m x 0.4 m)
            par = eng.params
            kind = torch.full((n,), 2, dtype=torch.int32, device=eng.device)
            ren.set_terrain(kind, par.terrain_slope, par.step_height, par.step_length)
            ren.render(R.FLAGS_DEFAULT)
            torch.cuda.synchronize()
            hit_t = int(torch.isfinite(ren.depth).sum())
            ms = launch_ms(lambda: ren.render(R.FLAGS_DEFAULT))
            results.append(dict(case=name + "-steps", cameras=k, width=w, height=h, shadows=True, culling=True,
                                terrain="steps", step_height=par.step_height, step_length=par.step_length,
                                ms_per_render=round(ms, 5), pixels=pixels, pixels_hit=hit_t))
            print(json.dumps(results[-1]), flush=True)
            ren.set_terrain(None)
    if want("rays"):  # a height scan under each of 4096 standing humanoids, half of them on the steps
        big, grid = 4096, 11
        eng_r = Engine(model, big, device=0)
        eng_r.rb_state.view(big, NB, 13).copy_(torch.from_numpy(standing_pose(model, big, rng)).to(eng_r.device))
        scan = R.Renderer(eng_r)
        kind = (torch.arange(big, device=eng_r.device) % 2 * 2).to(torch.int32)
        scan.set_terrain(kind, eng_r.params.terrain_slope, eng_r.params.step_height, eng_r.params.step_length)
        scan.set_rays(R.height_scan_rays(grid, grid, 0.1, 1.0), body="Pelvis", frame="heading")
        for skip in (True, False):
            ms = launch_ms(lambda: scan.cast_rays(10.0, skip_bodies=skip))
            rays = big * grid * grid
            results.append(dict(case=f"rays-{big}x{grid * grid}", envs=big, rays_per_env=grid * grid, skip_bodies=skip,
                                ms_per_cast=round(ms, 5), grays_per_s=round(rays / ms / 1e6, 3),
                                rays_hit=int(torch.isfinite(scan.ray_dist).sum())))
            print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/render_bench.py", args, {"render": args.lib}, results, envs=n, primitives_per_env=48,
                    cases=args.cases,
                    render_library=os.path.relpath(args.lib, ROOT) if args.lib else "humanoid_amd/libhumanoid_render.so")


if __name__ == "__main__":
    main()
