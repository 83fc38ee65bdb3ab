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
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402

STORE_RATE = 6.0e12  # B/s


def main():
    ap = bc.parser("profiles/r09/dynamics_bench.json", warmup=20, calls=None, blocks=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from humanoid_amd import dynamics as D
    n = args.envs
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)))
    dyn = D.Dynamics(eng)
    nbytes = {k: 4 * int(np.prod(s)) for k, s in D.output_shapes(n).items()}
    cases = (("all", ("jacobian", "mass_matrix", "bias")), ("jacobian", ("jacobian",)),
             ("mass_matrix", ("mass_matrix",)), ("bias", ("bias",)))
    results = []
    for name, outs in cases:
        kw = {k: k in outs for k in ("jacobian", "mass_matrix", "bias")}
        for _ in range(args.warmup):
            dyn.refresh(**kw)
        times = [bc.timed(lambda: dyn.refresh(**kw), args.launches) for _ in range(args.repeats)]
        ms = statistics.median(times)
        written = sum(nbytes[k] for k in outs)
        rate = written / (ms * 1e-3)
        results.append(dict(case=name, outputs=list(outs), ms_per_refresh=round(ms, 5),
                            ms_repeats=[round(t, 5) for t in times], bytes_written=written,
                            store_floor_ms=round(written / STORE_RATE * 1e3, 5), tb_per_s=round(rate / 1e12, 3),
                            fraction_of_store_rate=round(rate / STORE_RATE, 3)))
        print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/dynamics_bench.py", args, ["dynamics"], results,
                    store_rate_tb_per_s=STORE_RATE / 1e12)


if __name__ == "__main__":
    main()
