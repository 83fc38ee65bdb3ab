"""Time the camera-sensor kernel (hr_render): HIP events around 100 launches after 20 warm-up launches,
one process. Cases: one 1600 x 900 camera and 64 cameras of 320 x 180 (one per env), each with shadows on
and off and with tile culling on and off (HR_FLAG_NO_CULL). The scene is 64 standing humanoids with 24 red
markers each, seen by the env's tracking camera (4 m behind, 2 m up, as HumanoidPHC.render()).

Next to each time the record carries the plain work count of a launch without culling -- pixels x
primitives tested by the primary rays (48 per pixel: 24 geoms + 24 markers) and, with shadows, 24 more for
every pixel that hits something lit -- so the figure can be judged.

    python tools/render_bench.py [--out profiles/r08/render_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def standing_pose(model, n, rng):
    """rb_state [n,24,13]: the rest pose (identity rotations, joint offsets summed down the tree) at
    z = 0.89 with a sub-metre xy jitter."""
    rb = np.zeros((n, 24, 13), np.float32)
    pos = np.zeros((24, 3))
    for b in range(24):
        p = int(model.parents[b])
        pos[b] = (pos[p] if p >= 0 else np.array([0.0, 0.0, 0.89])) + (model.local_pos[b] if p >= 0 else 0.0)
    rb[:, :, :3] = pos[None] + np.concatenate([rng.uniform(-1, 1, (n, 1, 2)), np.zeros((n, 1, 1))], -1)
    rb[:, :, 6] = 1.0
    return rb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "render_bench.json"))
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=100)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd import render as R
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    model = load_default_model()
    n = 64
    eng = Engine(model, n, device=0)
    rng = np.random.default_rng(0)
    rb = standing_pose(model, n, rng)
    eng.rb_state.view(n, 24, 13).copy_(torch.from_numpy(rb).to(eng.device))
    ren = R.Renderer(eng)
    mpos = torch.from_numpy(rb[:, :, :3] + rng.normal(0, 0.08, (n, 24, 3)).astype(np.float32)).to(eng.device).contiguous()
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
                flags = R.FLAG_CHECKER | (R.FLAG_SHADOWS if shadows else 0) | (0 if cull else R.FLAG_NO_CULL)
                for _ in range(args.warmup):
                    ren.render(flags)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.launches):
                    ren.render(flags)
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / args.launches
                tests = pixels * 48 + (hit * 24 if shadows else 0)
                results.append(dict(case=name, cameras=k, width=w, height=h, shadows=shadows, culling=cull,
                                    ms_per_render=round(ms, 5), pixels=pixels, pixels_hit=hit,
                                    primitive_tests_unculled=tests,
                                    gtests_per_s_unculled_equivalent=round(tests / ms / 1e6, 2)))
                print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/render_bench.py", device=torch.cuda.get_device_name(0), warmup=args.warmup,
               launches=args.launches, envs=n, primitives_per_env=48,
               render_library_device_code_id=build.device_code_id(build.RENDER_LIB), results=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
