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

PUBLIC = ("root_states", "dof_state", "rb_state", "contact_forces", "dof_force", "dof_targets", "num_contacts",
          "dropped_contacts", "contact_cache", "initial_root_states")
FIELDS = ("root", "dof_state", "rb", "cf", "dof_force", "targets", "num_contacts", "dropped", "cache", "init_root")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state", "state_bench.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    n = args.envs
    eng = Engine(load_default_model(), n, device=0)
    dev = eng.device
    root, dof = random_state(n, np.random.default_rng(0))
    every = torch.arange(n, dtype=torch.int32, device=dev)
    eng.set_root_state_indexed(torch.from_numpy(root).to(dev), every)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(dev), every)
    eng.simulate(2)  # contacts, a warm-start cache, forces: every field holds something
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

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.calls

    results = []
    for name, k, kern, ref in cases:
        for _ in range(args.warmup):
            kern()
            ref()
        torch.cuda.synchronize()
        tk, tr = [], []
        for _ in range(args.blocks):
            tk.append(timed(kern))
            tr.append(timed(ref))
        mk, mr = statistics.median(tk), statistics.median(tr)
        moved = 2 * k * words * 4
        results.append(dict(case=name, k=k, kernel_ms=round(mk, 5), kernel_blocks_ms=[round(t, 5) for t in tk],
                            kernel_bytes=moved, kernel_effective_gb_per_s=round(moved / (mk * 1e-3) / 1e9, 1),
                            replaced_ms=round(mr, 5), replaced_blocks_ms=[round(t, 5) for t in tr],
                            replaced_over_kernel=round(mr / mk, 2),
                            slowest_kernel_over_fastest_replaced=round(max(tk) / min(tr), 4)))
        print(json.dumps(results[-1]), flush=True)
    rec = dict(tool="tools/state_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               calls_per_block=args.calls, blocks=args.blocks, words_per_env=words,
               replaced_words_per_env=replaced_words,
               note="the replaced path is one indexing op per public buffer; it cannot reach the internal rows (pending "
                    "wrench, actuation), so it moves replaced_words_per_env of words_per_env words per env and cannot "
                    "restore an env; times include the host's launch work (20 back-to-back calls between two events)",
               engine_device_code_id=build.device_code_id(build.LIB),
               engine_phases_device_code_id=build.device_code_id(build.LIBRARIES["engine_phases"].path),
               results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
