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

BODIES = {6: ("R_Hand",), 30: ("L_Hand", "R_Hand", "L_Ankle", "R_Ankle", "Head")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task", "task_bench.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd import dynamics as D
    from humanoid_amd.body_sets import BODY_NAMES
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    from humanoid_amd.solve import Solver
    from humanoid_amd.task import TaskSpace
    n = args.envs
    eng = Engine(load_default_model(), n, device=0)
    dev = eng.device
    root, dof = random_state(n, np.random.default_rng(0))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    eng.set_root_state_indexed(torch.from_numpy(root).to(dev), ids)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(dev), ids)
    dyn, sol, ts = D.Dynamics(eng), Solver(eng), TaskSpace(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    f = torch.zeros(n, 75, device=dev)
    f[:, 6:] = (torch.rand(n, 69, device=dev, generator=gen) * 2 - 1) * 100.0

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.calls

    results = []
    for k, names in BODIES.items():
        bodies = [BODY_NAMES.index(b) for b in names]
        rows = [(b, a) for b in bodies for a in range(6)]
        ts.set_rows(rows)
        body_idx = torch.tensor(bodies, device=dev)
        xdd = (torch.rand(n, k, device=dev, generator=gen) * 2 - 1) * 5.0
        b = ts.terms(want=("bias_acc",))["bias_acc"]  # the recipe's one borrowed term
        out_u, out_f, out_q = torch.empty(n, 75, device=dev), torch.empty(n, k, device=dev), torch.empty(n, 75, device=dev)
        for mode in ("force", "joint"):
            def fused():
                return ts.control(xdd, f, mode, 0.0, out_u, out_f, out_q)

            def recipe():
                dyn.refresh(jacobian=True, mass_matrix=False, bias=True)
                J = dyn.jacobian.index_select(1, body_idx).reshape(n, k, 75)
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

            for _ in range(args.warmup):
                a, c = fused(), recipe()
            torch.cuda.synchronize()
            diff = {name: float((a[i] - c[i]).abs().max() / c[i].abs().max()) for i, name in ((0, "u"), (2, "qdd"))}
            tk, tr = [], []
            for _ in range(args.blocks):
                tk.append(timed(fused))
                tr.append(timed(recipe))
            mk, mr = statistics.median(tk), statistics.median(tr)
            results.append(dict(case=f"k{k}_{mode}", k=k, mode=mode, fused_ms=round(mk, 5),
                                fused_blocks_ms=[round(t, 5) for t in tk], recipe_ms=round(mr, 5),
                                recipe_blocks_ms=[round(t, 5) for t in tr], recipe_over_fused=round(mr / mk, 2),
                                slowest_fused_over_fastest_recipe=round(max(tk) / min(tr), 4),
                                max_abs_difference_over_max=diff))
            print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/task_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               calls_per_block=args.calls, blocks=args.blocks,
               recipe="Dynamics.refresh(jacobian, bias) + row gather, Solver.solve, torch bmm / cholesky / cholesky_solve, "
                      "Solver.forward_dynamics; b = Jdot qd borrowed from the task library, untimed",
               task_library_device_code_id=build.device_code_id(build.LIBRARIES["task"].path),
               solve_library_device_code_id=build.device_code_id(build.LIBRARIES["solve"].path),
               engine_device_code_id=build.device_code_id(build.LIB), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
