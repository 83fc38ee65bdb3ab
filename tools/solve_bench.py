"""Time the joint-space solve kernels (include/humanoid_solve.h) at N = 4096 envs against the paths they
replace, each from the dynamics library's tensors in torch:

    forward_dynamics    hs_forward_dynamics           vs  Dynamics.refresh(jacobian=False) + torch.linalg.solve(M, f - c)
    computed_torque     hs_computed_torque            vs  Dynamics.refresh(jacobian=False) + the INTEGRATION.md recipe
    solve_k6            hs_solve, rhs = J of one body  vs  Dynamics.refresh() + torch.linalg.solve(M, J^T)

HIP events around `--calls` calls, in alternating blocks (kernel, replaced path, kernel, ...) in one
process after a warm-up of both, `--blocks` blocks each; the record carries every block and reports
the median and the spread (min, max) per side. The states are seeded random ones (every joint bent,
every velocity nonzero). The two sides' outputs are compared once before timing.

    python tools/solve_bench.py [--out profiles/r12/solve_cost.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "solve_cost.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--body", type=int, default=23, help="the body whose Jacobian block is solve_k6's rhs (23: R_Hand)")
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd import dynamics as D
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    from humanoid_amd.solve import Solver
    n = args.envs
    eng = Engine(load_default_model(), n, device=0)
    dev = eng.device
    root, dof = random_state(n, np.random.default_rng(0))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    eng.set_root_state_indexed(torch.from_numpy(root).to(dev), ids)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(dev), ids)
    dyn, sol = D.Dynamics(eng), Solver(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    f = torch.zeros(n, 75, device=dev)
    f[:, 6:] = (torch.rand(n, 69, device=dev, generator=gen) * 2 - 1) * 100.0
    qdd_des = (torch.rand(n, 69, device=dev, generator=gen) * 2 - 1) * 20.0
    dyn.refresh()
    J = dyn.jacobian[:, args.body].contiguous()  # [N,6,75]
    out_q, out_t, out_a, out_x = (torch.empty(n, 75, device=dev), torch.empty(n, 69, device=dev),
                                  torch.empty(n, 6, device=dev), torch.empty(n, 6, 75, device=dev))
    M, c = dyn.mass_matrix, dyn.bias

    def fd_kernel():
        return sol.forward_dynamics(f, out_q)

    def fd_torch():
        dyn.refresh(jacobian=False)
        return torch.linalg.solve(M, (f - c).unsqueeze(-1)).squeeze(-1)

    def ct_kernel():
        return sol.computed_torque(qdd_des, None, out_t, out_a)[0]

    def ct_torch():
        dyn.refresh(jacobian=False)
        qb = torch.linalg.solve(M[:, :6, :6], -(c[:, :6] + (M[:, :6, 6:] @ qdd_des.unsqueeze(-1)).squeeze(-1)))
        qdd = torch.cat([qb, qdd_des], dim=1)
        return ((M @ qdd.unsqueeze(-1)).squeeze(-1) + c)[:, 6:].contiguous()

    def k6_kernel():
        return sol.solve(J, out_x)

    def k6_torch():
        dyn.refresh()
        return torch.linalg.solve(M, dyn.jacobian[:, args.body].transpose(1, 2)).transpose(1, 2)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.calls

    results = []
    for name, kern, ref in (("forward_dynamics", fd_kernel, fd_torch), ("computed_torque", ct_kernel, ct_torch),
                            ("solve_k6", k6_kernel, k6_torch)):
        for _ in range(args.warmup):
            a, b = kern(), ref()
        torch.cuda.synchronize()
        diff = float((a - b).abs().max() / b.abs().max())
        tk, tr = [], []
        for _ in range(args.blocks):
            tk.append(timed(kern))
            tr.append(timed(ref))
        mk, mr = statistics.median(tk), statistics.median(tr)
        results.append(dict(case=name, kernel_ms=round(mk, 5), kernel_blocks_ms=[round(t, 5) for t in tk],
                            replaced_ms=round(mr, 5), replaced_blocks_ms=[round(t, 5) for t in tr],
                            speedup=round(mr / mk, 1), slowest_kernel_over_fastest_replaced=round(max(tk) / min(tr), 4),
                            max_abs_difference_over_max=diff))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/solve_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               calls_per_block=args.calls, blocks=args.blocks, body=args.body,
               solve_library_device_code_id=build.device_code_id(build.LIBRARIES["solve"].path),
               engine_device_code_id=build.device_code_id(build.LIB), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
