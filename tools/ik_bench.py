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
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import NB, ND, quat_exp, quat_mul, quat_rotvec  # noqa: E402

BODIES = {9: (("L_Hand", "R_Hand", "Head"), 3), 30: (("L_Hand", "R_Hand", "L_Ankle", "R_Ankle", "Head"), 6)}
DAMPING, CLIP = 1e-4, 0.1


def main():
    args = bc.parser("profiles/ik/ik_bench.json", warmup=3, calls=10).parse_args()
    import torch
    from humanoid_amd import task
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
    root, dof = bc.random_state(n, rng)
    root[:, 7:], dof[..., 1] = 0, 0
    root0 = torch.from_numpy(root).to(dev)
    dof0 = torch.from_numpy(dof.reshape(n * ND, 2)).to(dev)
    dof0[:, 0] = torch.minimum(torch.maximum(dof0.view(n, ND, 2)[..., 0], lo), up).reshape(-1)
    ik, ts = InverseKinematics(eng), task.TaskSpace(eng)
    flags = task.FLAG_ARMATURE | task.FLAG_NO_GRAVITY
    bodies_tree = bc.tree(model, dev)

    def body_poses(r, d):
        """Forward kinematics in torch: [N,24,7], position and xyzw orientation of every body."""
        return torch.cat(bc.forward_kinematics(bodies_tree, r[:, :3], r[:, 3:7],
                                               quat_exp(d.view(n, NB - 1, 3, 2)[..., 0])), -1)

    def integrate(r, d, dq):
        r2, d2 = torch.zeros_like(r), torch.zeros_like(d)
        r2[:, :3] = r[:, :3] + dq[:, :3]
        q = quat_mul(quat_exp(dq[:, 3:6]), r[:, 3:7])
        r2[:, 3:7] = q / q.norm(dim=-1, keepdim=True)
        th = d.view(n, NB - 1, 3, 2)[..., 0]
        new = quat_rotvec(quat_mul(quat_exp(th), quat_exp(dq[:, 6:].view(n, NB - 1, 3))))
        d2.view(n, ND, 2)[..., 0] = torch.minimum(torch.maximum(new.reshape(n, ND), lo), up)
        return r2, d2

    results = []
    for k, (names, axes) in BODIES.items():
        bodies = [BODY_NAMES.index(b) for b in names]
        rows = [(b, a) for b in bodies for a in range(axes)]
        ik.set_rows(rows)
        ts.set_rows(rows)
        body_idx = torch.tensor(bodies, device=dev)
        # the targets: the bodies' places and orientations at a pose a step away from the start
        dq = torch.from_numpy(np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), np.zeros((n, 3)),
                                              rng.uniform(-0.15, 0.15, (n, ND))], 1).astype(np.float32)).to(dev)
        goal = body_poses(*integrate(root0, dof0, dq)).clone()
        target_rot = goal[:, :, 3:7].contiguous()
        gp = goal.index_select(1, body_idx)[:, :, :3]
        target = (gp if axes == 3 else torch.cat([gp, torch.zeros_like(gp)], -1)).reshape(n, k).contiguous()
        gq = goal.index_select(1, body_idx)[:, :, 3:7]
        out_r, out_d, out_e = torch.empty(n, 13, device=dev), torch.empty(n * ND, 2, device=dev), torch.empty(n, k, device=dev)

        def errors(rb):
            b = rb.index_select(1, body_idx)
            e = gp - b[:, :, :3]
            if axes == 6:
                conj = b[:, :, 3:7] * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=dev)
                e = torch.cat([e, quat_rotvec(quat_mul(gq, conj))], -1)
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

            def compare(o):
                a, c = o["fused"], o["assembled"]
                return dict(root=float((a[0] - c[0]).abs().max()), dof=float((a[1] - c[1]).abs().max()),
                            residual=float((a[2] - c[2]).abs().max()), worst_fused_residual=float(a[2].abs().max()))

            t, diff = bc.alternate(dict(fused=fused, assembled=assembled), args.warmup, args.calls, args.blocks, compare)
            tf, ta = t["fused"], t["assembled"]
            results.append(dict(case=f"k{k}_it{iterations}", k=k, iterations=iterations, **bc.side_fields("fused", tf),
                                **bc.side_fields("assembled", ta), assembled_over_fused=bc.over(ta, tf, 2),
                                fused_ms_per_iteration=round(statistics.median(tf) / iterations, 5),
                                max_abs_difference=diff))
            print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/ik_bench.py", args, ["task", "engine"], results, damping=DAMPING, step_clip=CLIP,
                    assembled="per iteration: forward kinematics and the rows' errors in torch, TaskSpace.control "
                              "(force mode, no gravity) for qdd, the integration in torch")


if __name__ == "__main__":
    main()
