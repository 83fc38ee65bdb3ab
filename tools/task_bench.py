"""Time task-space control in one launch (include/humanoid_task.h, ht_task_control) at N = 4096 envs against
the recipe built from what the other libraries offer, for k = 6 (R_Hand, all axes) and k = 30 (both hands,
both ankles, the head, all axes), in both modes:

    fused     TaskSpace.control: u, F and qdd, one launch
    recipe    Dynamics.refresh(jacobian, bias) + the rows gathered from the [N,24,6,75] tensor
              Solver.solve(J)                                   Y = J M^-1
              torch: xdd_free = Y (f - c) + b, A = Y J^T or Yj Yj^T, linalg.cholesky, cholesky_solve,
                     u = J^T F or (0; Yj^T F)
              Solver.forward_dynamics(f + u)                    qdd

The recipe has no source for b = Jdot qd (that is what the task library adds): it takes b from one
TaskSpace.terms call before the timing, so its time leaves that term's cost out. HIP events around
`--calls` calls, in alternating blocks (fused, recipe, fused, ...) in one process after a warm-up of both,
`--blocks` blocks each; the record carries every block and reports the median and the spread per side.
The states are seeded random ones (every joint bent, every velocity nonzero). The two sides' u and qdd are
compared once before timing.

    python tools/task_bench.py [--out profiles/task/task_bench.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import ND, NG  # noqa: E402

BODIES = {6: ("R_Hand",), 30: ("L_Hand", "R_Hand", "L_Ankle", "R_Ankle", "Head")}


def main():
    args = bc.parser("profiles/task/task_bench.json").parse_args()
    import torch
    from humanoid_amd import dynamics as D
    from humanoid_amd.body_sets import BODY_NAMES
    from humanoid_amd.solve import Solver
    from humanoid_amd.task import TaskSpace
    n = args.envs
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)))
    dev = eng.device
    dyn, sol, ts = D.Dynamics(eng), Solver(eng), TaskSpace(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    f = torch.zeros(n, NG, device=dev)
    f[:, 6:] = bc.uniform((n, ND), 100.0, gen)

    results = []
    for k, names in BODIES.items():
        bodies = [BODY_NAMES.index(b) for b in names]
        rows = [(b, a) for b in bodies for a in range(6)]
        ts.set_rows(rows)
        body_idx = torch.tensor(bodies, device=dev)
        xdd = bc.uniform((n, k), 5.0, gen)
        b = ts.terms(want=("bias_acc",))["bias_acc"]  # the recipe's one borrowed term
        out_u, out_f, out_q = torch.empty(n, NG, device=dev), torch.empty(n, k, device=dev), torch.empty(n, NG, device=dev)
        for mode in ("force", "joint"):
            def fused():
                return ts.control(xdd, f, mode, 0.0, out_u, out_f, out_q)

            def recipe():
                dyn.refresh(jacobian=True, mass_matrix=False, bias=True)
                J = dyn.jacobian.index_select(1, body_idx).reshape(n, k, NG)
                Y = sol.solve(J)
                r = xdd - ((Y @ (f - dyn.bias).unsqueeze(-1)).squeeze(-1) + b)
                if mode == "force":
                    A = Y @ J.transpose(1, 2)
                else:
                    Yj = Y[:, :, 6:]
                    A = Yj @ Yj.transpose(1, 2)
                F = torch.cholesky_solve(r.unsqueeze(-1), torch.linalg.cholesky(A))
                if mode == "force":
                    u = (J.transpose(1, 2) @ F).squeeze(-1)
                else:
                    u = torch.cat([torch.zeros(n, 6, device=dev), (Yj.transpose(1, 2) @ F).squeeze(-1)], dim=1)
                return u, F.squeeze(-1), sol.forward_dynamics(f + u)

            t, diff = bc.alternate(dict(fused=fused, recipe=recipe), args.warmup, args.calls, args.blocks, lambda o: {
                name: float((o["fused"][i] - o["recipe"][i]).abs().max() / o["recipe"][i].abs().max())
                for i, name in ((0, "u"), (2, "qdd"))})
            tk, tr = t["fused"], t["recipe"]
            results.append(dict(case=f"k{k}_{mode}", k=k, mode=mode, **bc.side_fields("fused", tk),
                                **bc.side_fields("recipe", tr), recipe_over_fused=bc.over(tr, tk, 2),
                                slowest_fused_over_fastest_recipe=bc.slowest_over_fastest(tk, tr),
                                max_abs_difference_over_max=diff))
            print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/task_bench.py", args, ["task", "solve", "engine"], results,
                    recipe="Dynamics.refresh(jacobian, bias) + row gather, Solver.solve, torch bmm / cholesky / cholesky_solve, "
                           "Solver.forward_dynamics; b = Jdot qd borrowed from the task library, untimed")


if __name__ == "__main__":
    main()
