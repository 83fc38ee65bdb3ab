"""Time the inverse kinematics in one launch (include/humanoid_ik.h, hk_solve) at N = 4096 envs against the
same iteration assembled from what the package offered before it, for k = 9 (both hands and the head,
linear) and k = 30 (both hands, both ankles, the head, all six axes), at 1 and 8 iterations:

    fused      InverseKinematics.solve: every iteration, the residual included, one launch
    assembled  per iteration: the bodies' places and orientations by forward kinematics in torch (quaternions,
               one batched step per tree level), the rows' errors from them (positions, and the rotation
               vectors of the quaternion errors), clamped;
               TaskSpace.control(errors, mode="force", damping, armature, no gravity) for its qdd;
               the integration in torch (the root by its world rates, the joints' exp-map on the right, the
               limits' clamp)

HIP events around `--calls` calls, in alternating blocks (fused, assembled, fused, ...) in one process after
a warm-up of both, `--blocks` blocks each; the record carries every block and reports the median and the
spread per side. The starts are seeded random poses within the limits, the targets the rows' places at
poses up to 0.05 m and 0.15 rad per dof away. The two sides' poses after the timed number of iterations are
compared once before timing.

    python tools/ik_bench.py [--out profiles/ik/ik_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dynamics_bench import random_state  # noqa: E402

BODIES = {9: (("L_Hand", "R_Hand", "Head"), 3), 30: (("L_Hand", "R_Hand", "L_Ankle", "R_Ankle", "Head"), 6)}
DAMPING, CLIP = 1e-4, 0.1


def quat_exp(torch, v):
    """xyzw of exp([v]x), rows of v [..., 3]."""
    t2 = (v * v).sum(-1, keepdim=True)
    th = torch.sqrt(t2.clamp_min(1e-12))
    small = t2 < 1e-6
    s = torch.where(small, 0.5 - t2 / 48, torch.sin(0.5 * th) / th)
    c = torch.where(small, 1 - t2 / 8, torch.cos(0.5 * th))
    return torch.cat([v * s, c], -1)


def quat_mul(torch, a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_rotvec(torch, q):
    q = torch.where(q[..., 3:] < 0, -q, q)
    v, w = q[..., :3], q[..., 3:]
    s2 = (v * v).sum(-1, keepdim=True)
    sn = torch.sqrt(s2.clamp_min(1e-20))
    f = torch.where(s2 < 2.5e-7, (2 - s2 * (2 / 3) / (w * w)) / w, 2 * torch.atan2(sn, w) / sn)
    return v * f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik", "ik_bench.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build, task
    from humanoid_amd.body_sets import BODY_NAMES
    from humanoid_amd.engine import Engine
    from humanoid_amd.ik import InverseKinematics
    from humanoid_amd.model import load_default_model
    n = args.envs
    model = load_default_model()
    eng = Engine(model, n, device=0)
    dev = eng.device
    lo = torch.tensor(np.asarray(model.dof_lower, np.float32), device=dev)
    up = torch.tensor(np.asarray(model.dof_upper, np.float32), device=dev)
    rng = np.random.default_rng(0)
    root, dof = random_state(n, rng)
    root[:, 7:], dof[..., 1] = 0, 0
    root0 = torch.from_numpy(root).to(dev)
    dof0 = torch.from_numpy(dof.reshape(n * 69, 2)).to(dev)
    dof0[:, 0] = torch.minimum(torch.maximum(dof0.view(n, 69, 2)[..., 0], lo), up).reshape(-1)
    ik, ts = InverseKinematics(eng), task.TaskSpace(eng)
    flags = task.FLAG_ARMATURE | task.FLAG_NO_GRAVITY

    parents = [int(p) for p in model.parents]
    depth = [0] * 24
    for b in range(1, 24):
        depth[b] = depth[parents[b]] + 1
    levels = [(torch.tensor([b for b in range(24) if depth[b] == lv], device=dev),
               torch.tensor([parents[b] for b in range(24) if depth[b] == lv], device=dev))
              for lv in range(1, max(depth) + 1)]
    local_pos = torch.tensor(np.asarray(model.local_pos, np.float32), device=dev)

    def rotate(q, v):
        t = 2 * torch.cross(q[..., :3], v, dim=-1)
        return v + q[..., 3:] * t + torch.cross(q[..., :3], t, dim=-1)

    def body_poses(r, d):
        """Forward kinematics in torch: [N,24,7], position and xyzw orientation of every body."""
        ql = quat_exp(torch, d.view(n, 23, 3, 2)[..., 0])
        pos, quat = torch.zeros(n, 24, 3, device=dev), torch.zeros(n, 24, 4, device=dev)
        pos[:, 0], quat[:, 0] = r[:, :3], r[:, 3:7]
        for bs, ps in levels:
            qa = quat[:, ps]
            pos[:, bs] = pos[:, ps] + rotate(qa, local_pos[bs].expand(n, -1, -1))
            quat[:, bs] = quat_mul(torch, qa, ql[:, bs - 1])
        return torch.cat([pos, quat], -1)

    def integrate(r, d, dq):
        r2, d2 = torch.zeros_like(r), torch.zeros_like(d)
        r2[:, :3] = r[:, :3] + dq[:, :3]
        q = quat_mul(torch, quat_exp(torch, dq[:, 3:6]), r[:, 3:7])
        r2[:, 3:7] = q / q.norm(dim=-1, keepdim=True)
        th = d.view(n, 23, 3, 2)[..., 0]
        new = quat_rotvec(torch, quat_mul(torch, quat_exp(torch, th), quat_exp(torch, dq[:, 6:].view(n, 23, 3))))
        d2.view(n, 69, 2)[..., 0] = torch.minimum(torch.maximum(new.reshape(n, 69), lo), up)
        return r2, d2

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.calls

    results = []
    for k, (names, axes) in BODIES.items():
        bodies = [BODY_NAMES.index(b) for b in names]
        rows = [(b, a) for b in bodies for a in range(axes)]
        ik.set_rows(rows)
        ts.set_rows(rows)
        body_idx = torch.tensor(bodies, device=dev)
        # the targets: the bodies' places and orientations at a pose a step away from the start
        dq = torch.from_numpy(np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), np.zeros((n, 3)),
                                              rng.uniform(-0.15, 0.15, (n, 69))], 1).astype(np.float32)).to(dev)
        goal = body_poses(*integrate(root0, dof0, dq)).clone()
        target_rot = goal[:, :, 3:7].contiguous()
        gp = goal.index_select(1, body_idx)[:, :, :3]
        target = (gp if axes == 3 else torch.cat([gp, torch.zeros_like(gp)], -1)).reshape(n, k).contiguous()
        gq = goal.index_select(1, body_idx)[:, :, 3:7]
        out_r, out_d, out_e = torch.empty(n, 13, device=dev), torch.empty(n * 69, 2, device=dev), torch.empty(n, k, device=dev)

        def errors(rb):
            b = rb.index_select(1, body_idx)
            e = gp - b[:, :, :3]
            if axes == 6:
                conj = b[:, :, 3:7] * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=dev)
                e = torch.cat([e, quat_rotvec(torch, quat_mul(torch, gq, conj))], -1)
            return e.reshape(n, k)

        for iterations in (1, 8):
            def fused():
                return ik.solve(target, target_rot, iterations, DAMPING, CLIP, root0, dof0, out_r, out_d, residual=out_e)

            def assembled():
                r, d = root0, dof0
                for _ in range(iterations):
                    e = errors(body_poses(r, d)).clamp(-CLIP, CLIP)
                    _, _, qdd = ts.control(e, None, "force", DAMPING, flags=flags, root_state=r, dof_state=d,
                                           want_gen_force=False, want_task_force=False)
                    r, d = integrate(r, d, qdd)
                return r, d, errors(body_poses(r, d))

            for _ in range(args.warmup):
                a, c = fused(), assembled()
            torch.cuda.synchronize()
            diff = dict(root=float((a[0] - c[0]).abs().max()), dof=float((a[1] - c[1]).abs().max()),
                        residual=float((a[2] - c[2]).abs().max()), worst_fused_residual=float(a[2].abs().max()))
            tf, ta = [], []
            for _ in range(args.blocks):
                tf.append(timed(fused))
                ta.append(timed(assembled))
            mf, ma = statistics.median(tf), statistics.median(ta)
            results.append(dict(case=f"k{k}_it{iterations}", k=k, iterations=iterations, fused_ms=round(mf, 5),
                                fused_blocks_ms=[round(t, 5) for t in tf], assembled_ms=round(ma, 5),
                                assembled_blocks_ms=[round(t, 5) for t in ta], assembled_over_fused=round(ma / mf, 2),
                                fused_ms_per_iteration=round(mf / iterations, 5), max_abs_difference=diff))
            print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/ik_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               calls_per_block=args.calls, blocks=args.blocks, damping=DAMPING, step_clip=CLIP,
               assembled="per iteration: forward kinematics and the rows' errors in torch, TaskSpace.control "
                         "(force mode, no gravity) for qdd, the integration in torch",
               task_library_device_code_id=build.device_code_id(build.LIBRARIES["task"].path),
               engine_device_code_id=build.device_code_id(build.LIB), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
