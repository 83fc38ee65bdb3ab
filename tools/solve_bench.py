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
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import ND, NG  # noqa: E402


def main():
    ap = bc.parser("profiles/r12/solve_cost.json")
    ap.add_argument("--body", type=int, default=23, help="the body whose Jacobian block is solve_k6's rhs (23: R_Hand)")
    args = ap.parse_args()
    import torch
    from humanoid_amd import dynamics as D
    from humanoid_amd.solve import Solver
    n = args.envs
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)))
    dev = eng.device
    dyn, sol = D.Dynamics(eng), Solver(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    f = torch.zeros(n, NG, device=dev)
    f[:, 6:] = bc.uniform((n, ND), 100.0, gen)
    qdd_des = bc.uniform((n, ND), 20.0, gen)
    dyn.refresh()
    J = dyn.jacobian[:, args.body].contiguous()  # [N,6,75]
    out_q, out_t, out_a, out_x = (torch.empty(n, NG, device=dev), torch.empty(n, ND, device=dev),
                                  torch.empty(n, 6, device=dev), torch.empty(n, 6, NG, device=dev))
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

    results = []
    for name, kern, ref in (("forward_dynamics", fd_kernel, fd_torch), ("computed_torque", ct_kernel, ct_torch),
                            ("solve_k6", k6_kernel, k6_torch)):
        t, diff = bc.alternate(dict(kernel=kern, replaced=ref), args.warmup, args.calls, args.blocks, lambda o: float(
            (o["kernel"] - o["replaced"]).abs().max() / o["replaced"].abs().max()))
        tk, tr = t["kernel"], t["replaced"]
        results.append(dict(case=name, **bc.side_fields("kernel", tk), **bc.side_fields("replaced", tr),
                            speedup=bc.over(tr, tk, 1), slowest_kernel_over_fastest_replaced=bc.slowest_over_fastest(tk, tr),
                            max_abs_difference_over_max=diff))
        print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/solve_bench.py", args, ["solve", "engine"], results, body=args.body)


if __name__ == "__main__":
    main()
