"""Time the dynamics-query kernel (hd_compute, humanoid_amd.dynamics.Dynamics.refresh) at N = 4096 envs:
HIP events around 200 launches after 20 warm-up launches, one process, repeated 3 times (the record
carries every repeat and reports the median). Cases: all three outputs in one launch, and each output
alone. The states are seeded random ones (every joint bent, every velocity nonzero).

The job is bound by its stores, so next to each time the record carries the bytes a launch writes (from
the shapes: J N*24*6*75, M N*75*75, c N*75 floats; the reads, N*(13 + 138) floats, are 2.5 MB), the
rate bytes / time, and that rate's fraction of the plain-store rate MI355X_MICROARCH.md measures for one
dword per lane, 256 B per wave instruction (6.0-6.2 TB/s; 6.0 is used).

    python tools/dynamics_bench.py [--out profiles/r09/dynamics_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORE_RATE = 6.0e12  # B/s


def random_state(n, rng):
    root = np.zeros((n, 13), np.float32)
    root[:, :2] = rng.uniform(-1, 1, (n, 2))
    root[:, 2] = rng.uniform(0.9, 1.6, n)
    q = rng.normal(size=(n, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = rng.normal(0, 1.0, (n, 6))
    dof = np.zeros((n, 69, 2), np.float32)
    dof[..., 0] = rng.uniform(-0.6, 0.6, (n, 69))
    dof[..., 1] = rng.normal(0, 1.0, (n, 69))
    return root, dof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "dynamics_bench.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd import dynamics as D
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    n = args.envs
    eng = Engine(load_default_model(), n, device=0)
    root, dof = random_state(n, np.random.default_rng(0))
    ids = torch.arange(n, dtype=torch.int32, device=eng.device)
    eng.set_root_state_indexed(torch.from_numpy(root).to(eng.device), ids)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(eng.device), ids)
    dyn = D.Dynamics(eng)
    nbytes = {k: 4 * int(np.prod(s)) for k, s in D.output_shapes(n).items()}
    cases = (("all", ("jacobian", "mass_matrix", "bias")), ("jacobian", ("jacobian",)),
             ("mass_matrix", ("mass_matrix",)), ("bias", ("bias",)))
    results = []
    for name, outs in cases:
        kw = {k: k in outs for k in ("jacobian", "mass_matrix", "bias")}
        for _ in range(args.warmup):
            dyn.refresh(**kw)
        times = []
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                dyn.refresh(**kw)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) / args.launches)
        ms = statistics.median(times)
        written = sum(nbytes[k] for k in outs)
        rate = written / (ms * 1e-3)
        results.append(dict(case=name, outputs=list(outs), ms_per_refresh=round(ms, 5),
                            ms_repeats=[round(t, 5) for t in times], bytes_written=written,
                            store_floor_ms=round(written / STORE_RATE * 1e3, 5), tb_per_s=round(rate / 1e12, 3),
                            fraction_of_store_rate=round(rate / STORE_RATE, 3)))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/dynamics_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               launches=args.launches, repeats=args.repeats, store_rate_tb_per_s=STORE_RATE / 1e12,
               dynamics_library_device_code_id=build.device_code_id(build.LIBRARIES["dynamics"].path), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
