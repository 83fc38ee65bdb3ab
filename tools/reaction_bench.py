"""Time the joint-reaction queries (include/humanoid_wrench.h, hw_compute) at N = 4096 envs against the same
outputs from the reference's algorithm in torch float32, batched over the envs on the device:

    kernel    Reaction.compute: one launch of torque_kernel
    torch     forward kinematics with the bodies' velocities and accelerations, one batched step per tree
              level (rotation matrices), every body's Newton-Euler wrench about its centre of mass, the
              subtree sums as one [24,24] mask product, tau as the joint axes' components of the torques

for a prescribed base with a force and a torque on every body: all four outputs, then `wrench` alone; the
kernel's free base too (no torch side: it adds the 6 x 6 solve). Then the force sensors' refresh for two
ankle sensors (ForceSensors.read, what gym.refresh_force_sensor_tensor runs after its flush): the launch
and the torch lines around it.

HIP events around `--calls` calls, in alternating blocks (kernel, torch, kernel, ...) in one process after a
warm-up of both, `--blocks` blocks each; the record carries every block and reports the median and the
spread per side. The states are seeded random ones (every joint bent, every velocity nonzero). The two
sides' outputs are compared once before timing.

    python tools/reaction_bench.py [--out profiles/reaction/reaction_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reaction", "reaction_bench.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import torch
    from humanoid_amd import build
    from humanoid_amd.body_sets import BODY_NAMES
    from humanoid_amd.engine import Engine
    from humanoid_amd.model import load_default_model
    from humanoid_amd.reaction import Reaction, output_shapes
    from humanoid_amd.sensors import ForceSensors
    from humanoid_amd.solve import Solver
    n = args.envs
    model = load_default_model()
    eng = Engine(model, n, device=0)
    dev = eng.device
    root, dof = random_state(n, np.random.default_rng(0))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    eng.set_root_state_indexed(torch.from_numpy(root).to(dev), ids)
    eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(dev), ids)
    rx, sol = Reaction(eng), Solver(eng)
    gen = torch.Generator(device=dev).manual_seed(1)

    def rand(shape, scale):
        return (torch.rand(shape, device=dev, generator=gen) * 2 - 1) * scale

    qdd_des, base_acc = rand((n, 69), 20.0), rand((n, 6), 10.0)
    force, torque = rand((n * 24, 3), 200.0), rand((n * 24, 3), 20.0)

    f32 = dict(dtype=torch.float32, device=dev)
    parents = [int(p) for p in model.parents]
    depth = [0] * 24
    for b in range(1, 24):
        depth[b] = depth[parents[b]] + 1
    levels = [(torch.tensor([b for b in range(24) if depth[b] == lv], device=dev),
               torch.tensor([parents[b] for b in range(24) if depth[b] == lv], device=dev))
              for lv in range(1, max(depth) + 1)]
    local_pos = torch.tensor(np.asarray(model.local_pos, np.float32), **f32)
    mass = torch.tensor(np.asarray(model.mass, np.float32), **f32)
    com = torch.tensor(np.asarray(model.com, np.float32), **f32)
    inertia = torch.tensor(np.asarray(model.inertia, np.float32), **f32)  # [24,3,3]
    armature = torch.tensor(np.asarray(model.armature, np.float32), **f32)
    gravity = torch.tensor([float(x) for x in eng.params.gravity], **f32)
    sub = torch.zeros(24, 24, **f32)  # sub[j, b]: b in the subtree of j
    for b in range(24):
        a = b
        while a >= 0:
            sub[a, b] = 1.0
            a = parents[a]

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
        return torch.eye(3, **f32) + A * K + B * (K @ K)

    def quat_matrix(q):
        x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)

    def mv(A, v):
        return (A @ v.unsqueeze(-1)).squeeze(-1)

    cross = lambda a, b: torch.cross(a, b, dim=-1)  # noqa: E731

    def reference(want_all=True):
        """The header's definitions in torch: (wrench, tau, base_acc, body_acc), prescribed base."""
        r, d = eng.root_states, eng.dof_state.view(n, 23, 3, 2)
        Rl = rodrigues(d[..., 0])
        u, ud = d[..., 1], qdd_des.view(n, 23, 3)
        R, p = torch.zeros(n, 24, 3, 3, **f32), torch.zeros(n, 24, 3, **f32)
        w, wd, acc = torch.zeros(n, 24, 3, **f32), torch.zeros(n, 24, 3, **f32), torch.zeros(n, 24, 3, **f32)
        R[:, 0], w[:, 0], acc[:, 0], wd[:, 0] = quat_matrix(r[:, 3:7]), r[:, 10:13], base_acc[:, :3], base_acc[:, 3:]
        for bs, ps in levels:
            Ra, wa, wda = R[:, ps], w[:, ps], wd[:, ps]
            Rb = Ra @ Rl[:, bs - 1]
            dd = mv(Ra, local_pos[bs].expand(n, -1, -1))
            wrel = mv(Rb, u[:, bs - 1])
            R[:, bs], p[:, bs], w[:, bs] = Rb, p[:, ps] + dd, wa + wrel
            wd[:, bs] = wda + cross(wa, wrel) + mv(Rb, ud[:, bs - 1])
            acc[:, bs] = acc[:, ps] + cross(wda, dd) + cross(wa, cross(wa, dd))
        rc = mv(R, com.expand(n, -1, -1))
        a_c = acc + cross(wd, rc) + cross(w, cross(w, rc))
        Iw = R @ inertia @ R.transpose(-1, -2)
        Fb = mass[None, :, None] * (a_c - gravity) - force.view(n, 24, 3)
        Tb = mv(Iw, wd) + cross(w, mv(Iw, w)) - torque.view(n, 24, 3)
        F = torch.einsum("jb,nbi->nji", sub, Fb)
        N = torch.einsum("jb,nbi->nji", sub, Tb + cross(p + rc, Fb)) - cross(p, F)
        wrench = torch.cat([F, N], -1)
        if not want_all:
            return (wrench,)
        tau = torch.einsum("njik,nji->njk", R[:, 1:], N[:, 1:]).reshape(n, 69) + armature * qdd_des
        return wrench, tau, base_acc.clone(), torch.cat([acc, wd], -1)

    out = {k: torch.empty(s, **f32) for k, s in output_shapes(n).items()}

    def kernel_all():
        o = rx.compute(qdd_des, base_acc, force, torque, wrench=False, out=out)
        return o["wrench"], o["tau"], o["base_acc"], o["body_acc"]

    def kernel_wrench():
        return (rx.compute(qdd_des, base_acc, force, torque, wrench=False, out={"wrench": out["wrench"]})["wrench"],)

    def kernel_all_free():
        o = rx.compute(qdd_des, None, force, torque, wrench=False, out=out)
        return o["wrench"], o["tau"], o["base_acc"], o["body_acc"]

    def computed_torque():
        return sol.computed_torque(qdd_des, None, out["tau"], out["base_acc"])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.calls

    results = []
    for name, kern, ref in (("all_outputs_prescribed", kernel_all, lambda: reference(True)),
                            ("wrench_alone_prescribed", kernel_wrench, lambda: reference(False)),
                            ("all_outputs_free_base", kernel_all_free, None),
                            ("hs_computed_torque", computed_torque, None)):
        for _ in range(args.warmup):
            a = kern()
            b = ref() if ref else None
        torch.cuda.synchronize()
        diff = None if ref is None else [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b)]
        tk, tr = [], []
        for _ in range(args.blocks):
            tk.append(timed(kern))
            if ref:
                tr.append(timed(ref))
        rec = dict(case=name, kernel_ms=round(statistics.median(tk), 5), kernel_blocks_ms=[round(t, 5) for t in tk])
        if ref:
            mr = statistics.median(tr)
            rec.update(torch_ms=round(mr, 5), torch_blocks_ms=[round(t, 5) for t in tr],
                       torch_over_kernel=round(mr / statistics.median(tk), 1), max_abs_difference_over_max=diff)
        results.append(rec)
        print(json.dumps(rec), flush=True)

    # the force sensors' refresh: two ankle sensors, after a launch of the engine
    ankles = [BODY_NAMES.index("L_Ankle"), BODY_NAMES.index("R_Ankle")]
    fs = ForceSensors(eng, ankles, [[0, 0, 0, 0, 0, 0, 1], [0.03, -0.02, -0.05, 0.1, -0.3, 0.2, 0.9]], reaction=rx)
    reading = torch.zeros(n * 2, 6, **f32)
    fs.before_step()
    eng.simulate(1)
    dt = float(eng.params.dt)
    for _ in range(args.warmup):
        fs.read(dt, reading)
    ts = [timed(lambda: fs.read(dt, reading)) for _ in range(args.blocks)]
    tb = [timed(fs.before_step) for _ in range(args.blocks)]
    results.append(dict(case="force_sensors_two_ankles", read_ms=round(statistics.median(ts), 5),
                        read_blocks_ms=[round(t, 5) for t in ts], before_step_ms=round(statistics.median(tb), 5),
                        before_step_blocks_ms=[round(t, 5) for t in tb]))
    print(json.dumps(results[-1]), flush=True)

    rec = dict(tool="tools/reaction_bench.py", device=torch.cuda.get_device_name(0), envs=n, warmup=args.warmup,
               calls_per_block=args.calls, blocks=args.blocks,
               torch="the header's definitions in float32, batched over the envs: kinematics with accelerations per tree "
                     "level, per-body Newton-Euler wrenches, subtree sums as a mask product",
               solve_library_device_code_id=build.device_code_id(build.LIBRARIES["solve"].path),
               engine_device_code_id=build.device_code_id(build.LIB), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
