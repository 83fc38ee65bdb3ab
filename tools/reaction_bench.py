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
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import NB, ND, mv  # noqa: E402


def main():
    args = bc.parser("profiles/reaction/reaction_bench.json").parse_args()
    import torch
    from humanoid_amd.body_sets import BODY_NAMES
    from humanoid_amd.model import load_default_model
    from humanoid_amd.reaction import Reaction, output_shapes
    from humanoid_amd.sensors import ForceSensors
    from humanoid_amd.solve import Solver
    n = args.envs
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)))
    dev = eng.device
    rx, sol = Reaction(eng), Solver(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    qdd_des, base_acc = bc.uniform((n, ND), 20.0, gen), bc.uniform((n, 6), 10.0, gen)
    force, torque = bc.uniform((n * NB, 3), 200.0, gen), bc.uniform((n * NB, 3), 20.0, gen)

    f32 = dict(dtype=torch.float32, device=dev)
    tr = bc.tree(load_default_model(), dev)
    gravity = torch.tensor([float(x) for x in eng.params.gravity], **f32)
    cross = lambda a, b: torch.cross(a, b, dim=-1)  # noqa: E731

    def reference(want_all=True):
        """The header's definitions in torch: (wrench, tau, base_acc, body_acc), prescribed base."""
        r, d = eng.root_states, eng.dof_state.view(n, NB - 1, 3, 2)
        u, ud = d[..., 1], qdd_des.view(n, NB - 1, 3)
        w, wd, acc = torch.zeros(n, NB, 3, **f32), torch.zeros(n, NB, 3, **f32), torch.zeros(n, NB, 3, **f32)
        w[:, 0], acc[:, 0], wd[:, 0] = r[:, 10:13], base_acc[:, :3], base_acc[:, 3:]

        def rates(bs, ps, Ra, Rb, dd):  # the level's angular velocities and both accelerations
            wa, wda = w[:, ps], wd[:, ps]
            wrel = mv(Rb, u[:, bs - 1])
            w[:, bs] = wa + wrel
            wd[:, bs] = wda + cross(wa, wrel) + mv(Rb, ud[:, bs - 1])
            acc[:, bs] = acc[:, ps] + cross(wda, dd) + cross(wa, cross(wa, dd))

        p, R = bc.forward_kinematics(tr, None, bc.quat_matrix(r[:, 3:7]), bc.rodrigues(d[..., 0]), rates)
        rc = mv(R, tr.com.expand(n, -1, -1))
        a_c = acc + cross(wd, rc) + cross(w, cross(w, rc))
        Iw = R @ tr.inertia @ R.transpose(-1, -2)
        Fb = tr.mass[None, :, None] * (a_c - gravity) - force.view(n, NB, 3)
        Tb = mv(Iw, wd) + cross(w, mv(Iw, w)) - torque.view(n, NB, 3)
        F = torch.einsum("jb,nbi->nji", tr.sub, Fb)
        N = torch.einsum("jb,nbi->nji", tr.sub, Tb + cross(p + rc, Fb)) - cross(p, F)
        wrench = torch.cat([F, N], -1)
        if not want_all:
            return (wrench,)
        tau = torch.einsum("njik,nji->njk", R[:, 1:], N[:, 1:]).reshape(n, ND) + tr.armature * qdd_des
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

    results = []
    for name, kern, ref in (("all_outputs_prescribed", kernel_all, lambda: reference(True)),
                            ("wrench_alone_prescribed", kernel_wrench, lambda: reference(False)),
                            ("all_outputs_free_base", kernel_all_free, None),
                            ("hs_computed_torque", computed_torque, None)):
        t, diff = bc.alternate(dict(kernel=kern, torch=ref), args.warmup, args.calls, args.blocks, lambda o: ref and [
            float((x - y).abs().max() / y.abs().max()) for x, y in zip(o["kernel"], o["torch"])])
        rec = dict(case=name, **bc.side_fields("kernel", t["kernel"]))
        if ref:
            rec.update(**bc.side_fields("torch", t["torch"]), torch_over_kernel=bc.over(t["torch"], t["kernel"], 1),
                       max_abs_difference_over_max=diff)
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
    ts = [bc.timed(lambda: fs.read(dt, reading), args.calls) for _ in range(args.blocks)]
    tb = [bc.timed(fs.before_step, args.calls) for _ in range(args.blocks)]
    results.append(dict(case="force_sensors_two_ankles", **bc.side_fields("read", ts), **bc.side_fields("before_step", tb)))
    print(json.dumps(results[-1]), flush=True)

    bc.write_record(args.out, "tools/reaction_bench.py", args, ["solve", "engine"], results,
                    torch="the header's definitions in float32, batched over the envs: kinematics with accelerations per "
                          "tree level, per-body Newton-Euler wrenches, subtree sums as a mask product")


if __name__ == "__main__":
    main()
