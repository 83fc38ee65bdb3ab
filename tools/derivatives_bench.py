"""Time the dynamics derivatives (include/humanoid_derivatives.h, hg_compute) at N = 4096 envs against the
path they replace, and hold the existing entries of libhumanoid_solve.so to a build of the parent commit.

Default: the bench.

    kernel    Derivatives.inverse_dynamics: one launch of torque_kernel for dtau_dq and dtau_dv together, and
              for each alone; Derivatives.forward_dynamics (the solve, the derivatives at a = qdd, M^-1 on both
              matrices in chunks of 32 rows)
    replaced  central differences in float32 through torque_kernel on states perturbed in torch: per direction
              the pose q (+) h e_j (quaternion products for the root and the ball joints) or the velocity
              qd + h e_j, two launches each, 72 pose and 75 velocity directions = 294 launches. The launch
              is hw_compute with a prescribed base, the entry that gives all 75 rows of M a + c (the root
              wrench and the joint torques); it is hs_computed_torque's kernel and costs what it costs. The
              forward form's replaced path is the same with hs_forward_dynamics as the launch.

HIP events around `--calls` calls (replaced: `--replaced-calls`), in alternating blocks (kernel, replaced,
kernel, ...) in one process after a warm-up of both, `--blocks` blocks each; the record carries every block
and reports the median per side. The states are seeded random ones (every joint bent, every velocity
nonzero). Both sides' errors against the float64 reference of tests/derivative_reference.py are recorded
on the first `--check-envs` envs: max|x - x64| / max|x64|, the largest over those envs.

    python tools/derivatives_bench.py [--out profiles/derivatives/derivatives_bench.json]

--ab PARENT_DIR: the hs_ and hw_ entries of this tree's libhumanoid_solve.so against the one in PARENT_DIR (a
build of the parent commit), each run in a process of its own: their outputs on the six states of
dynamics_reference.test_states compared byte for byte (printed; exit status 1 when any differs), then their
times at 4096 envs in `--passes` alternating passes (new, parent, new, ...), per pass the median of the
blocks; the record (--out) carries the median over the passes and the spread of one side's passes.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_common as bc  # noqa: E402
from bench_common import NB, ND, NG, ROOT, quat_exp, quat_mul, quat_rotvec  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

H_Q, H_V = 5e-3, 1.0  # float32 steps: (3 eps)^(1/3) of an angle of order 1; tau is quadratic in qd


# ------------------------------------------------------------------ the replaced path's pose arithmetic
def moved_states(root, dof, j, h):
    """(root', dof') at q (+) h e_j: torch float32, batched over the envs."""
    import torch
    r, d = root.clone(), dof.clone()
    if j < 3:
        r[:, j] += h
    elif j < 6:
        e = torch.zeros(1, 3, device=root.device)
        e[0, j - 3] = h
        r[:, 3:7] = quat_mul(quat_exp(e).expand(root.shape[0], 4), root[:, 3:7])
    else:
        b, i = (j - 6) // 3, (j - 6) % 3
        e = torch.zeros(1, 3, device=root.device)
        e[0, i] = h
        th = d.view(-1, ND, 2)[:, 3 * b:3 * b + 3, 0]
        d.view(-1, ND, 2)[:, 3 * b:3 * b + 3, 0] = quat_rotvec(quat_mul(quat_exp(th), quat_exp(e).expand(th.shape[0], 4)))
    return r, d


def bumped_states(root, dof, j, h):
    """(root', dof') at qd + h e_j."""
    r, d = root.clone(), dof.clone()
    if j < 6:
        r[:, 7 + j] += h
    else:
        d.view(-1, ND, 2)[:, j - 6, 1] += h
    return r, d


def differences(fun, root, dof, pose, out):
    """out[:, :, j] = (fun(state+) - fun(state-)) / 2 h for every direction that can change fun."""
    move, h = (moved_states, H_Q) if pose else (bumped_states, H_V)
    out.zero_()
    for j in range(3, NG):  # neither the root position nor its linear velocity enters
        out[:, :, j] = (fun(*move(root, dof, j, h)) - fun(*move(root, dof, j, -h))) / (2 * h)
    return out


# ------------------------------------------------------------------ the bench
def bench(args):
    import torch
    import derivative_reference as GR
    from humanoid_amd.derivatives import Derivatives
    from humanoid_amd.reaction import Reaction
    from humanoid_amd.solve import Solver
    n = args.envs
    eng = bc.seeded_engine(n, *bc.random_state(n, np.random.default_rng(0)))
    dev = eng.device
    dv, rx, sol = Derivatives(eng), Reaction(eng), Solver(eng)
    gen = torch.Generator(device=dev).manual_seed(1)
    acc, f = bc.uniform((n, NG), 20.0, gen), bc.uniform((n, NG), 50.0, gen)
    root, dof = eng.root_states.clone(), eng.dof_state.clone()
    base_acc, qdd_des = acc[:, :6].contiguous(), acc[:, 6:].contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    outs = {k: torch.empty(n, NG, NG, **f32) for k in ("dtau_dq", "dtau_dv")}
    fd_q, fd_v = torch.empty(n, NG, NG, **f32), torch.empty(n, NG, NG, **f32)
    hw = dict(wrench=torch.empty(n, NB, 6, **f32), tau=torch.empty(n, ND, **f32))
    qdd_buf, ab_buf = torch.empty(n, NG, **f32), torch.empty(n, 6, **f32)

    def tau_by_launch(r, d):  # all 75 rows of M a + c from one launch of torque_kernel
        o = rx.compute(qdd_des, base_acc, wrench=False, out=hw, root_state=r, dof_state=d)
        return torch.cat([o["wrench"][:, 0], o["tau"]], dim=1)

    def qdd_by_launch(r, d):
        return sol.forward_dynamics(f, qdd_buf, root_state=r, dof_state=d).clone()

    cases = (
        ("dtau_dq_and_dtau_dv", lambda: dv.inverse_dynamics(acc, out=outs, dtau_dq=False, dtau_dv=False),
         lambda: (differences(tau_by_launch, root, dof, True, fd_q), differences(tau_by_launch, root, dof, False, fd_v))),
        ("dtau_dq_alone", lambda: dv.inverse_dynamics(acc, out={"dtau_dq": outs["dtau_dq"]}, dtau_dq=False, dtau_dv=False),
         lambda: differences(tau_by_launch, root, dof, True, fd_q)),
        ("dtau_dv_alone", lambda: dv.inverse_dynamics(acc, out={"dtau_dv": outs["dtau_dv"]}, dtau_dq=False, dtau_dv=False),
         lambda: differences(tau_by_launch, root, dof, False, fd_v)),
        ("forward_dynamics_derivatives", lambda: dv.forward_dynamics(f),
         lambda: (differences(qdd_by_launch, root, dof, True, fd_q), differences(qdd_by_launch, root, dof, False, fd_v))),
    )

    # the errors, once, on the first envs: both sides against the float64 reference
    m = args.check_envs
    from humanoid_amd import _abi
    from humanoid_amd.model import load_default_model
    hm = _abi.make_model(load_default_model())
    g = tuple(eng.params.gravity)
    r_h, d_h = root.cpu().numpy()[:m], dof.cpu().numpy().reshape(n, ND, 2)[:m]
    x64 = GR.exact(hm, r_h, d_h, acc.cpu().numpy()[:m], g)
    fwd64 = GR.forward(hm, r_h, d_h, f.cpu().numpy()[:m], g)
    x32 = GR.exact(hm, r_h, d_h, acc.cpu().numpy()[:m], g, np.float32)
    err = lambda x, ref: float(GR.error(x.cpu().numpy()[:m], ref).max())  # noqa: E731
    cases[0][1]()
    cases[0][2]()
    errors = {
        "dtau_dq": dict(kernel=err(outs["dtau_dq"], x64["dtau_dq"]), replaced=err(fd_q, x64["dtau_dq"]),
                        float32_floor=float(GR.error(x32["dtau_dq"], x64["dtau_dq"]).max())),
        "dtau_dv": dict(kernel=err(outs["dtau_dv"], x64["dtau_dv"]), replaced=err(fd_v, x64["dtau_dv"]),
                        float32_floor=float(GR.error(x32["dtau_dv"], x64["dtau_dv"]).max())),
    }
    fw = cases[3][1]()
    cases[3][2]()
    errors["dqdd_dq"] = dict(kernel=err(fw["dqdd_dq"], fwd64["dqdd_dq"]), replaced=err(fd_q, fwd64["dqdd_dq"]))
    errors["dqdd_dv"] = dict(kernel=err(fw["dqdd_dv"], fwd64["dqdd_dv"]), replaced=err(fd_v, fwd64["dqdd_dv"]))
    print(json.dumps(dict(errors_against_float64=errors)), flush=True)

    results = []
    for name, kern, rep in cases:
        t = bc.alternate(dict(kernel=kern, replaced=rep), dict(kernel=args.warmup, replaced=1),
                         dict(kernel=args.calls, replaced=args.replaced_calls), args.blocks)[0]
        results.append(dict(case=name, **bc.side_fields("kernel", t["kernel"]), **bc.side_fields("replaced", t["replaced"], 3),
                            replaced_over_kernel=bc.over(t["replaced"], t["kernel"], 1)))
        print(json.dumps(results[-1]), flush=True)
    t_ct = statistics.median(bc.timed(lambda: sol.computed_torque(qdd_des, None, hw["tau"], ab_buf), args.calls)
                             for _ in range(args.blocks))
    t_hw = statistics.median(bc.timed(lambda: tau_by_launch(root, dof), args.calls) for _ in range(args.blocks))
    bc.write_record(args.out, "tools/derivatives_bench.py", args, ["solve", "engine"], results,
                    replaced="central differences in float32 (pose step %g, velocity step %g) through torque_kernel launches "
                             "(hw_compute, prescribed base: all 75 rows) on states perturbed in torch, 2 x 72 + 2 x 75 "
                             "launches for both matrices; the forward form through hs_forward_dynamics likewise" % (H_Q, H_V),
                    one_launch_ms=dict(hs_computed_torque=round(t_ct, 5),
                                       hw_compute_with_the_torch_concatenation=round(t_hw, 5)),
                    check_envs=m, errors_against_float64=errors)
    del dv, rx, sol, eng
    return 0


# ------------------------------------------------------------------ against the parent's build
def ab_side(args):
    """One process of --ab: load the solve library at args.side (before any constructor: the first load is
    the one that stays), then either dump the entries' outputs on the six test states or time them."""
    import torch
    from humanoid_amd import _abi, reaction, solve
    solve.load_library(args.side)
    reaction.load_library(args.side)
    if args.dump:
        import dynamics_reference as DR
        from humanoid_amd.model import load_default_model
        root_h, dof_h = DR.test_states(_abi.make_model(load_default_model()))
        n = root_h.shape[0]
    else:
        n = args.envs
        root_h, dof_h = bc.random_state(n, np.random.default_rng(0))
    eng = bc.seeded_engine(n, root_h, dof_h)
    sol, rx = solve.Solver(eng), reaction.Reaction(eng)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    rand = lambda shape, s: bc.uniform(shape, s, gen)  # noqa: E731
    f, qdd_des, base_acc = rand((n, NG), 100.0), rand((n, ND), 20.0), rand((n, 6), 10.0)
    force, torque, rhs = rand((n * NB, 3), 200.0), rand((n * NB, 3), 20.0), rand((n, 6, NG), 1.0)
    entries = {
        "hs_forward_dynamics": lambda: (sol.forward_dynamics(f),),
        "hs_computed_torque": lambda: sol.computed_torque(qdd_des, f),
        "hs_solve_k6": lambda: (sol.solve(rhs),),
        "hw_compute_prescribed": lambda: tuple(rx.compute(qdd_des, base_acc, force, torque, "body", tau=True,
                                                          base_acc_out=True, body_acc=True).values()),
        "hw_compute_free": lambda: tuple(rx.compute(qdd_des, None, force, torque, tau=True, base_acc_out=True,
                                                    body_acc=True).values()),
    }
    if args.dump:
        out = {}
        for name, fn in entries.items():
            for flags in range(4):
                sol.armature = rx.armature = bool(flags & 1)
                sol.gravity = rx.gravity = not flags & 2
                for i, t in enumerate(fn()):
                    out[f"{name}_flags{flags}_{i}"] = t.cpu().numpy().copy()
        torch.cuda.synchronize()
        np.savez(args.dump, **out)
    else:
        res = {}
        for name, fn in entries.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            res[name] = [bc.timed(fn, args.calls) for _ in range(args.blocks)]
        print("AB_SIDE " + json.dumps(res), flush=True)
    del sol, rx, eng
    return 0


def ab(args):
    from humanoid_amd import build
    name = os.path.basename(build.LIBRARIES["solve"].path)
    libs = {"new": build.LIBRARIES["solve"].path, "parent": os.path.abspath(os.path.join(args.ab, name))}
    ids = {k: build.device_code_id(v) for k, v in libs.items()}
    me = [sys.executable, os.path.abspath(__file__)]
    differs = False
    with tempfile.TemporaryDirectory() as tmp:
        dumps = {}
        for side, lib in libs.items():
            dumps[side] = os.path.join(tmp, side + ".npz")
            subprocess.run(me + ["--side", lib, "--dump", dumps[side]], check=True, timeout=300)
        a, b = np.load(dumps["parent"]), np.load(dumps["new"])
        print(f"the hs_ and hw_ entries on the six states of dynamics_reference.test_states, under the four flag "
              f"combinations: parent {ids['parent']}, this tree {ids['new']}")
        for key in a.files:
            same = a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes()
            differs |= not same
            print(key, a[key].shape, "identical" if same else
                  f"differs ({int((a[key].view(np.uint32) != b[key].view(np.uint32)).sum())} words)", flush=True)
    passes = {"new": [], "parent": []}
    for _ in range(args.passes):
        for side, lib in libs.items():
            r = subprocess.run(me + ["--side", lib, "--envs", str(args.envs), "--calls", str(args.calls), "--blocks",
                                     str(args.blocks)], check=True, timeout=300, capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB_SIDE ")][-1]
            passes[side].append(json.loads(line[len("AB_SIDE "):]))
    results = []
    for case in passes["new"][0]:
        rec = dict(case=case)
        for side in ("new", "parent"):
            per_pass = [statistics.median(p[case]) for p in passes[side]]
            blocks = [t for p in passes[side] for t in p[case]]
            med = statistics.median(per_pass)
            rec.update({f"{side}_ms_per_pass": [round(t, 5) for t in per_pass], f"{side}_ms": round(med, 5),
                        f"{side}_blocks_ms_min_max": [round(min(blocks), 5), round(max(blocks), 5)],
                        f"{side}_pass_spread": round((max(per_pass) - min(per_pass)) / med, 4)})
        rec["new_over_parent"] = round(rec["new_ms"] / rec["parent_ms"], 4)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    import torch
    rec = dict(what="the hs_ and hw_ entries at 4096 envs, this tree's libhumanoid_solve.so against a build of the parent "
                    "commit's, alternating passes of one process each (new, parent, new, ...); per pass the median of the "
                    "blocks; here the median over the passes, and the spread of the passes of one side (max - min over "
                    "the median), the A/B's own run-to-run figure",
               tool="tools/derivatives_bench.py --ab", device=torch.cuda.get_device_name(0), envs=args.envs,
               calls_per_block=args.calls, blocks=args.blocks, passes=args.passes,
               new_solve_library_device_code_id=ids["new"], parent_solve_library_device_code_id=ids["parent"],
               outputs_identical=not differs, results=results)
    bc.dump(args.out, rec)
    return 1 if differs else 0


def main():
    ap = bc.parser(None)
    ap.add_argument("--replaced-calls", type=int, default=1)
    ap.add_argument("--check-envs", type=int, default=8)
    ap.add_argument("--ab", metavar="PARENT_DIR", help="a directory with the parent commit's libhumanoid_solve.so")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--side", help=argparse.SUPPRESS)
    ap.add_argument("--dump", help=argparse.SUPPRESS)
    args = ap.parse_args()
    here = os.path.join(ROOT, "profiles", "derivatives")
    if args.side:
        return ab_side(args)
    if args.ab:
        args.out = args.out or os.path.join(here, "solve_ab.json")
        return ab(args)
    args.out = args.out or os.path.join(here, "derivatives_bench.json")
    return bench(args)


if __name__ == "__main__":
    sys.exit(main())
