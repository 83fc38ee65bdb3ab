"""What the query benches (tools/*_bench.py) share, stated once: the seeded states, the arguments, the timer, the
alternating blocks, the record, and the torch tree arithmetic of the replaced sides.

The method: HIP events around `calls` calls; every side warmed, one synchronise, the sides' outputs compared
once, then `blocks` blocks that take the sides in turn in one process; the record carries every block and the
median per side. Nothing here falls back when there is no device: `alternate` takes a timer and a synchronise
only so that its ordering can be checked on the CPU (tests/test_bench_common.py).
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from humanoid_amd._abi import NB, ND, NG  # noqa: E402,F401


# ------------------------------------------------------------------ states and draws
def random_state(n, rng):
    root = np.zeros((n, 13), np.float32)
    root[:, :2] = rng.uniform(-1, 1, (n, 2))
    root[:, 2] = rng.uniform(0.9, 1.6, n)
    q = rng.normal(size=(n, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = rng.normal(0, 1.0, (n, 6))
    dof = np.zeros((n, ND, 2), np.float32)
    dof[..., 0] = rng.uniform(-0.6, 0.6, (n, ND))
    dof[..., 1] = rng.normal(0, 1.0, (n, ND))
    return root, dof


def seeded_engine(n, root, dof, simulate=0):
    """The default model's Engine on device 0 holding root [n,13] and dof [n,69,2], advanced by simulate(`simulate`)."""
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    eng = Engine(load_default_model(), n, device=0)
    ids = torch.arange(n, dtype=torch.int32, device=eng.device)
    eng.set_root_state_indexed(torch.from_numpy(root).to(eng.device), ids)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * ND, 2)).to(eng.device), ids)
    if simulate:
        eng.simulate(simulate)
    return eng


def uniform(shape, scale, gen):
    return (torch.rand(shape, device=gen.device, generator=gen) * 2 - 1) * scale


# ------------------------------------------------------------------ arguments
def parser(out_default, envs=4096, warmup=5, calls=20, blocks=5):
    """--out (a path below the repository, or None), --envs, --warmup, --calls, --blocks; None leaves one out."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=out_default and os.path.join(ROOT, out_default))
    for name, default in (("envs", envs), ("warmup", warmup), ("calls", calls), ("blocks", blocks)):
        if default is not None:
            ap.add_argument("--" + name, type=int, default=default)
    return ap


# ------------------------------------------------------------------ timing
def timed(fn, calls):
    """ms per call: HIP events around `calls` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def alternate(sides, warmup, calls, blocks, compare=None, timed=timed, sync=None):
    """Warm every side of `sides` (name -> callable, None: no such side), each its `warmup` calls with the last
    calls side by side; synchronise once; hand each side's last warm-up result to `compare` (the outputs are
    compared here, before any timing); then `blocks` blocks, each timing the sides in the given order, `calls`
    calls a side. `warmup` and `calls` are ints or name -> int. Returns ({name: [ms per call, one per block]},
    what `compare` returned, or the last results themselves without one)."""
    sides = {k: fn for k, fn in sides.items() if fn is not None}
    per_side = lambda x: {k: x[k] if isinstance(x, dict) else x for k in sides}  # noqa: E731
    warmup, calls = per_side(warmup), per_side(calls)
    last = {}
    for i in range(max(warmup.values()), 0, -1):
        for k, fn in sides.items():
            if warmup[k] >= i:
                last[k] = fn()
    (sync or torch.cuda.synchronize)()
    compared = compare(last) if compare else last
    times = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            times[k].append(timed(fn, calls[k]))
    return times, compared


# ------------------------------------------------------------------ the record
def side_fields(name, blocks_ms, digits=5):
    return {f"{name}_ms": round(statistics.median(blocks_ms), digits),
            f"{name}_blocks_ms": [round(t, digits) for t in blocks_ms]}


def over(a_blocks_ms, b_blocks_ms, digits):
    """a over b, the medians."""
    return round(statistics.median(a_blocks_ms) / statistics.median(b_blocks_ms), digits)


def slowest_over_fastest(a_blocks_ms, b_blocks_ms):
    return round(max(a_blocks_ms) / min(b_blocks_ms), 4)


def dump(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


HEAD = (("envs", "envs"), ("warmup", "warmup"), ("calls", "calls_per_block"), ("launches", "launches"),
        ("repeats", "repeats"), ("replaced_calls", "replaced_calls_per_block"), ("blocks", "blocks"))


def write_record(path, tool, args, libraries, results, device=None, code_id=None, **extra):
    """tool, device, the arguments of HEAD that `args` has, `extra`, the device_code_id of every library of
    `libraries` (names of build.LIBRARIES, or name -> the path of another build), results."""
    from humanoid_amd import build
    rec = dict(tool=tool, device=torch.cuda.get_device_name(0) if device is None else device)
    rec.update({key: getattr(args, name) for name, key in HEAD if hasattr(args, name)})
    rec.update(extra)
    paths = libraries if isinstance(libraries, dict) else dict.fromkeys(libraries)
    for name, lib in paths.items():
        key = f"{name}_device_code_id" if name.startswith("engine") else f"{name}_library_device_code_id"
        rec[key] = (code_id or build.device_code_id)(lib or build.LIBRARIES[name].path)
    rec["results"] = results
    dump(path, rec)
    return rec


# ------------------------------------------------------------------ torch: rotations
def quat_exp(v):
    """xyzw of exp([v]x), rows of v [..., 3]."""
    t2 = (v * v).sum(-1, keepdim=True)
    th = torch.sqrt(t2.clamp_min(1e-12))
    small = t2 < 1e-6
    s = torch.where(small, 0.5 - t2 / 48, torch.sin(0.5 * th) / th)
    c = torch.where(small, 1 - t2 / 8, torch.cos(0.5 * th))
    return torch.cat([v * s, c], -1)


def quat_mul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_rotvec(q):
    q = torch.where(q[..., 3:] < 0, -q, q)
    v, w = q[..., :3], q[..., 3:]
    s2 = (v * v).sum(-1, keepdim=True)
    sn = torch.sqrt(s2.clamp_min(1e-20))
    f = torch.where(s2 < 2.5e-7, (2 - s2 * (2 / 3) / (w * w)) / w, 2 * torch.atan2(sn, w) / sn)
    return v * f


def quat_rotate(q, v):
    t = 2 * torch.cross(q[..., :3], v, dim=-1)
    return v + q[..., 3:] * t + torch.cross(q[..., :3], t, dim=-1)


def quat_matrix(q):
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def skew(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(
        v.shape[:-1] + (3, 3))


def rodrigues(v):
    t2 = (v * v).sum(-1, keepdim=True)
    th = torch.sqrt(t2.clamp_min(1e-12))
    small = t2 < 1e-6
    A = torch.where(small, 1 - t2 / 6, torch.sin(th) / th)[..., None]
    B = torch.where(small, 0.5 - t2 / 24, (1 - torch.cos(th)) / t2.clamp_min(1e-12))[..., None]
    K = skew(v)
    return torch.eye(3, dtype=v.dtype, device=v.device) + A * K + B * (K @ K)


def mv(A, v):
    return (A @ v.unsqueeze(-1)).squeeze(-1)


# ------------------------------------------------------------------ torch: the body tree
def tree(model, device):
    """The model as float32 tensors on `device`: per tree level the (bodies, parents) index pair, local_pos [24,3],
    mass [24], com [24,3], inertia [24,3,3], armature [69], and sub [24,24] (sub[j, b]: b in the subtree of j)."""
    f32 = dict(dtype=torch.float32, device=device)
    parents = [int(p) for p in model.parents]
    depth = [0] * NB
    for b in range(1, NB):
        depth[b] = depth[parents[b]] + 1
    levels = [(torch.tensor([b for b in range(NB) if depth[b] == lv], device=device),
               torch.tensor([parents[b] for b in range(NB) if depth[b] == lv], device=device))
              for lv in range(1, max(depth) + 1)]
    sub = torch.zeros(NB, NB, **f32)
    for b in range(NB):
        a = b
        while a >= 0:
            sub[a, b] = 1.0
            a = parents[a]
    field = lambda name: torch.tensor(np.asarray(getattr(model, name), np.float32), **f32)  # noqa: E731
    return SimpleNamespace(parents=parents, levels=levels, sub=sub, **{k: field(k) for k in (
        "local_pos", "mass", "com", "inertia", "armature")})


def forward_kinematics(tr, pos0, rot0, local, visit=None):
    """pos [N,24,3] and rot of every body, one batched step per tree level, from the root's pos0 [N,3] (None: the
    origin) and rot0 and the joints' rotations local [N,23,...]: rotations are xyzw quaternions (rot0 [N,4]) or
    matrices (rot0 [N,3,3]). visit(bodies, parents, the parents' rot, the bodies' rot, the offsets in the world)
    runs per level."""
    compose, rotate = (quat_mul, quat_rotate) if rot0.dim() == 2 else (torch.matmul, mv)
    n = rot0.shape[0]
    pos = torch.zeros(n, NB, 3, dtype=rot0.dtype, device=rot0.device)
    rot = torch.zeros((n, NB) + rot0.shape[1:], dtype=rot0.dtype, device=rot0.device)
    rot[:, 0] = rot0
    if pos0 is not None:
        pos[:, 0] = pos0
    for bs, ps in tr.levels:
        ra = rot[:, ps]
        rb = compose(ra, local[:, bs - 1])
        d = rotate(ra, tr.local_pos[bs].expand(n, -1, -1))
        pos[:, bs], rot[:, bs] = pos[:, ps] + d, rb
        if visit:
            visit(bs, ps, ra, rb, d)
    return pos, rot
