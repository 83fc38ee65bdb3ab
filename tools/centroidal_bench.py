"""Time the centroidal queries in one launch (include/humanoid_centroidal.h, hc_compute) at N = 4096 envs
against the recipe a user had to assemble before, in two cases: all six outputs, and com, com_vel and
momentum only.

    fused     Centroidal.refresh: one launch
    recipe    Dynamics.refresh(jacobian=False) with armature and gravity off     M [N,75,75], c [N,75]
              the rigid-body tensor: c_b = p_b + R(q_b) com[b], com = sum m_b c_b / m
              torch: r = com - p_0, A_G = M[0:6] with the angular rows less r x the linear rows, the same
                     for c[0:6]; momentum = A_G qd, com_vel = P / m, kinetic = 1/2 qd^T M qd,
                     potential = -m g . com
              (the second case leaves the bias force, the energies and the 6 x 75 output out)

HIP events around `--calls` calls, in alternating blocks (fused, recipe, fused, ...) in one process after a
warm-up of both, `--blocks` blocks each; the record carries every block and reports the median and the
spread per side. The states are seeded random ones advanced by one simulate call, so that the rigid-body
tensor the recipe reads belongs to the root and dof state the kernel reads. The two sides' outputs are
compared once before timing. The fused launch's bytes written over its time are set against the HBM peak.

    python tools/centroidal_bench.py [--out profiles/centroidal/centroidal_bench.json]
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import NB, ND  # noqa: E402

HBM_PEAK_TBS = 8.0        # HBM3E, specification
HBM_ACHIEVABLE_TBS = 6.3  # measured with a float4 copy
CASES = {"all_six": ("com", "com_vel", "momentum", "cmm", "cmm_bias", "energy"),
         "com_vel_momentum": ("com", "com_vel", "momentum")}


def main():
    args = bc.parser("profiles/centroidal/centroidal_bench.json").parse_args()
    import torch
    from humanoid_amd import dynamics as D
    from humanoid_amd.centroidal import OUTPUTS, output_shapes
    from humanoid_amd.model import load_default_model
    n = args.envs
    root, dof = bc.random_state(n, np.random.default_rng(0))
    root[:, 2] += 3.0  # in the air: the one simulate call below meets no ground
    eng = bc.seeded_engine(n, root, dof, simulate=1)  # the rigid-body tensor now belongs to the root and dof state
    dev = eng.device
    dyn = D.Dynamics(eng, armature=False)
    dyn.gravity = False
    cen = dyn.centroidal
    model = load_default_model()
    mass = torch.tensor(np.asarray(model.mass, np.float32), device=dev)
    lcom = torch.tensor(np.asarray(model.com, np.float32), device=dev)
    mtot = mass.sum()
    g = torch.tensor([float(x) for x in eng.params.gravity], device=dev)
    rb = eng.rb_state.view(n, NB, 13)

    def shifted(rows, r):  # [N,6,k]: the angular rows less r x the linear rows
        return torch.cat([rows[:, 0:3], rows[:, 3:6] - torch.cross(r.unsqueeze(-1).expand_as(rows[:, 0:3]), rows[:, 0:3], dim=1)],
                         dim=1)

    results = []
    for case, names in CASES.items():
        full = case == "all_six"
        want = {k: k in names for k in OUTPUTS}

        def fused():
            cen.refresh(**want)
            return {k: getattr(cen, k) for k in names}

        def recipe():
            dyn.refresh(jacobian=False, bias=full)
            q, u = rb[:, :, 3:6], rb[:, :, 6:7]
            t = 2.0 * torch.cross(q, lcom.expand(n, NB, 3), dim=2)
            cb = rb[:, :, 0:3] + lcom + u * t + torch.cross(q, t, dim=2)
            com = (mass[None, :, None] * cb).sum(1) / mtot
            r = com - eng.root_states[:, 0:3]
            qd = dyn.generalized_velocity()
            A = shifted(dyn.mass_matrix[:, 0:6], r)
            mom = (A @ qd.unsqueeze(-1)).squeeze(-1)
            out = dict(com=com, com_vel=mom[:, 0:3] / mtot, momentum=mom)
            if full:
                out["cmm"] = A
                out["cmm_bias"] = shifted(dyn.bias[:, 0:6].unsqueeze(-1), r).squeeze(-1)
                kin = 0.5 * (qd.unsqueeze(1) @ dyn.mass_matrix @ qd.unsqueeze(-1)).reshape(n)
                out["energy"] = torch.stack([kin, -mtot * (com @ g)], dim=1)
            return out

        t, diff = bc.alternate(dict(fused=fused, recipe=recipe), args.warmup, args.calls, args.blocks, lambda o: {
            k: float((o["fused"][k] - o["recipe"][k]).abs().max()) for k in names})
        tk, tr = t["fused"], t["recipe"]
        mk = statistics.median(tk)
        shapes = output_shapes(n)
        written = 4 * sum(int(np.prod(shapes[k])) for k in names)
        read = 4 * n * (13 + ND * 2)
        results.append(dict(case=case, outputs=list(names), **bc.side_fields("fused", tk), **bc.side_fields("recipe", tr),
                            recipe_over_fused=bc.over(tr, tk, 2),
                            slowest_fused_over_fastest_recipe=bc.slowest_over_fastest(tk, tr),
                            max_abs_difference=diff, bytes_written=written, bytes_read=read,
                            written_tb_per_s=round(written / (mk * 1e-3) / 1e12, 4),
                            fraction_of_hbm_peak=round(written / (mk * 1e-3) / 1e12 / HBM_PEAK_TBS, 4)))
        print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/centroidal_bench.py", args, ["dynamics", "engine"], results,
                    recipe="Dynamics.refresh(jacobian=False), armature and gravity off; the centre of mass from the "
                           "rigid-body tensor; torch for the re-referencing, A_G qd and the energies",
                    timing="HIP events around each block of calls, host launch cost included on both sides",
                    hbm_peak_tb_per_s=HBM_PEAK_TBS, hbm_achievable_tb_per_s=HBM_ACHIEVABLE_TBS,
                    bound="one wave per env runs a serial tree pass of 8 levels before it stores 1.9 KB: the launch is "
                          "bound by that latency and by the launch itself, not by HBM (see fraction_of_hbm_peak)")


if __name__ == "__main__":
    main()
