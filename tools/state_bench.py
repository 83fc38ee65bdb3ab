"""Time the env-state calls (include/humanoid_engine.h "env state": he_save_envs, he_load_envs, he_clone_envs) at
N = 4096 envs against the same movement assembled from what the engine offered before them: one indexing op
per public buffer on the zero-copy tensors.

    save_all / load_all      every env                 vs  clone() / copy_() of the ten public state buffers
    save_64 / load_64        k = 64 scattered envs     vs  index_select / index_copy_ per buffer
    clone_64                 64 envs onto 64 others    vs  index_copy_(dst, index_select(src)) per buffer
    clone_1_to_4095          env 0 onto every other    vs  the same

The replaced path cannot reach the internal rows (the pending wrench, the actuation): it moves 792 of the
state's 1005 words per env, so it moves LESS than the kernel does, and it cannot restore an env. The record
says so (`replaced_words_per_env`). Effective bytes/s are against 2 k W 4 (every word read once, written once).

HIP events around `--calls` calls, in alternating blocks (kernel, replaced path, kernel, ...) in one process
after a warm-up of both, `--blocks` blocks each; the record carries every block and reports the median and the
spread per side. The two sides' results are compared once before timing.

    python tools/state_bench.py [--out profiles/state/state_bench.json]
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402

PUBLIC = ("root_states", "dof_state", "rb_state", "contact_forces", "dof_force", "dof_targets", "num_contacts",
          "dropped_contacts", "contact_cache", "initial_root_states")
FIELDS = ("root", "dof_state", "rb", "cf", "dof_force", "targets", "num_contacts", "dropped", "cache", "init_root")


def main():
    args = bc.parser("profiles/state/state_bench.json").parse_args()
    import torch
    n = args.envs
    # simulate(2): contacts, a warm-start cache, forces: every field holds something
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)), simulate=2)
    dev = eng.device
    words = eng.state_layout[0]
    rows = [getattr(eng, name).view(n, -1) for name in PUBLIC]  # zero-copy [N, words of the buffer]
    replaced_words = sum(r.shape[1] for r in rows)
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ids64, dst64 = perm[:64].to(torch.int32).contiguous(), perm[64:128].to(torch.int32).contiguous()
    src1 = torch.zeros(n - 1, dtype=torch.int32, device=dev)
    dst1 = torch.arange(1, n, dtype=torch.int32, device=dev)
    full, part = eng.save_envs(), eng.save_envs(ids64)
    full_rows = [r.clone() for r in rows]
    part_rows = [r.index_select(0, ids64.long()) for r in rows]
    out_full, out_part = torch.empty_like(full), torch.empty_like(part)

    def replaced_clone(src, dst):
        s, d = src.long(), dst.long()
        return lambda: [r.index_copy_(0, d, r.index_select(0, s)) for r in rows]

    cases = (
        ("save_all", n, lambda: eng.save_envs(out=out_full), lambda: [r.clone() for r in rows]),
        ("load_all", n, lambda: eng.load_envs(full), lambda: [r.copy_(s) for r, s in zip(rows, full_rows)]),
        ("save_64", 64, lambda: eng.save_envs(ids64, out=out_part),
         lambda: [r.index_select(0, ids64.long()) for r in rows]),
        ("load_64", 64, lambda: eng.load_envs(part, ids64),
         lambda: [r.index_copy_(0, ids64.long(), s) for r, s in zip(rows, part_rows)]),
        ("clone_64", 64, lambda: eng.clone_envs(ids64, dst64), replaced_clone(ids64, dst64)),
        ("clone_1_to_4095", n - 1, lambda: eng.clone_envs(src1, dst1), replaced_clone(src1, dst1)),
    )
    # the two sides move the same public words: compared once, before timing
    for f, r in zip(FIELDS, full_rows):
        assert torch.equal(eng.state_field(full, f), r), f
    for f, r in zip(FIELDS, part_rows):
        assert torch.equal(eng.state_field(part, f), r), f

    results = []
    for name, k, kern, ref in cases:
        t = bc.alternate(dict(kernel=kern, replaced=ref), args.warmup, args.calls, args.blocks)[0]
        tk, tr = t["kernel"], t["replaced"]
        moved = 2 * k * words * 4
        results.append(dict(case=name, k=k, **bc.side_fields("kernel", tk), kernel_bytes=moved,
                            kernel_effective_gb_per_s=round(moved / (statistics.median(tk) * 1e-3) / 1e9, 1),
                            **bc.side_fields("replaced", tr), replaced_over_kernel=bc.over(tr, tk, 2),
                            slowest_kernel_over_fastest_replaced=bc.slowest_over_fastest(tk, tr)))
        print(json.dumps(results[-1]), flush=True)
    bc.write_record(args.out, "tools/state_bench.py", args, ["engine", "engine_phases"], results, words_per_env=words,
                    replaced_words_per_env=replaced_words,
                    note="the replaced path is one indexing op per public buffer; it cannot reach the internal rows (pending "
                         "wrench, actuation), so it moves replaced_words_per_env of words_per_env words per env and cannot "
                         "restore an env; times include the host's launch work (20 back-to-back calls between two events)")


if __name__ == "__main__":
    main()
