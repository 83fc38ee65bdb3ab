"""Bit-identity of two engine builds (e.g. a scheduler-flag variant, or a refactored kernel against
its parent): the same run with each library in its own process, the final states compared.

  python tools/lib_identity.py LIB_A LIB_B [--fused] [--config NAME] [--scheme NAME]
  python tools/lib_identity.py LIB_A LIB_B --lying [--max-contacts N]
  python tools/lib_identity.py --queries DIR_A DIR_B

Default: the bench rollout (configs[2], tracking actions, 4096 envs, TGS, <= 32 rows) for 20 steps;
--fused runs it as the one-launch env step. --config / --scheme go to bench.Rollout as in
tools/phase_profile.py (512 envs: envs never interact): `--config dr` reaches the terrain kinds and
the per-env properties, `--scheme pgs` physics_kernel. --lying: 512 lying bodies lowered into the
plane (25-40 contacts, most solves past 32 rows: the TGS wide class) under random targets, 10 policy
steps; with --max-contacts below the contacts generated it reaches the overflow reduction, and the
count of envs that dropped contacts is printed (0: the mode did not reach it, lower the cap).
--queries: the query libraries (libhumanoid_dynamics.so, libhumanoid_solve.so, and libhumanoid_task.so when
both directories hold one: its terms under the four flag combinations and both control modes at k = 1, 6,
32) of each directory on
the same engine library and 305 seeded states that reach the branches of csrc/he_tree_state.h (the five
of tests/test_gpu_dynamics.py, roots at the origin and 1 km away, all dofs zero, a joint below, at and
above rodrigues' 1e-3 rad threshold, a joint near pi): J, M, c under the four flag combinations,
forward dynamics with and without a force, computed torque, hs_solve at k = 1, 6, 32."""
import argparse
import os
import subprocess
import sys

# argv: out, fused (0/1), config, scheme, num_envs
CODE = r"""
import argparse, sys, numpy as np, torch
sys.path.insert(0, '.')
import bench
from humanoid_amd.model import load_default_model
out, fused, config, scheme, n = sys.argv[1], sys.argv[2] == '1', sys.argv[3], sys.argv[4], int(sys.argv[5])
args = argparse.Namespace(config=config, num_envs=n, clips=128, seed=0, max_contacts=40, fused=fused, scheme=scheme)
ro = bench.Rollout(args, load_default_model(), 0, 0)
for _ in range(20):
    if config == 'imitation':
        ro.tracking_actions()
    ro.step()
torch.cuda.synchronize()
e = ro.eng
np.savez(out, root=e.root_states.cpu().numpy(), dof=e.dof_state.cpu().numpy(), obs=ro.obs.cpu().numpy(),
         rb=e.rb_state.cpu().numpy(), force=e.dof_force.cpu().numpy(), contacts=e.num_contacts.cpu().numpy(),
         cache=e.contact_cache.cpu().numpy())
"""


# argv: out, max_contacts
CODE_LYING = r"""
import sys, numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import cases
from humanoid_amd import _abi
from humanoid_amd.engine import Engine
from humanoid_amd.model import load_default_model
n = 512
hm = _abi.make_model(load_default_model())
rng = np.random.default_rng(5)
root, dof = cases.lying_state(n, rng)
root[:, 2] = 0.08 + rng.uniform(0, 0.04, n).astype(np.float32)
eng = Engine(hm, n, device=0, sim_params=_abi.default_sim_params(max_contacts=int(sys.argv[2])))
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
eng.root_states.copy_(cu(root))
eng.dof_state.copy_(cu(dof.reshape(n * 69, 2)))
caches = []
dropped = np.zeros(n, bool)
for _ in range(10):
    eng.dof_targets.copy_(cu(rng.uniform(-0.5, 0.5, (n, 69)).astype(np.float32)))
    eng.simulate(2)
    caches.append(eng.contact_cache.cpu().numpy().copy())
    dropped |= eng.dropped_contacts.cpu().numpy() > 0
torch.cuda.synchronize()
print('envs with dropped contacts:', int(dropped.sum()), 'of', n)
np.savez(sys.argv[1], root=eng.root_states.cpu().numpy(), dof=eng.dof_state.cpu().numpy(),
         rb=eng.rb_state.cpu().numpy(), force=eng.dof_force.cpu().numpy(), cache=np.asarray(caches),
         contacts=eng.num_contacts.cpu().numpy())
"""


# argv: out, libhumanoid_dynamics.so, libhumanoid_solve.so[, libhumanoid_task.so]
CODE_QUERIES = r"""
import sys, numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import cases
from humanoid_amd import dynamics, solve
dynamics.load_library(sys.argv[2])  # before any constructor: the first load is the one that stays
solve.load_library(sys.argv[3])
if len(sys.argv) > 4:
    from humanoid_amd import task
    task.load_library(sys.argv[4])
from humanoid_amd.engine import Engine
from humanoid_amd.model import load_default_model
G = 50  # envs per group
n = 5 + 6 * G
rng = np.random.default_rng(13)
root, dof = np.zeros((n, 13), np.float32), np.zeros((n, 69, 2), np.float32)
# 0..4: the five states of tests/test_gpu_dynamics.py (env 0 stays as he_create_envs left it)
r5, d5 = cases.random_state(4, np.random.default_rng(11), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
root[1:5], dof[1:5] = r5, d5
dof[4, :, 0] = 0.0
# six groups of random states, every velocity nonzero: as drawn; the root 1 km away; all dofs zero; one
# joint per env on the series branch of rodrigues (|q| < 1e-3); one straddling that threshold; one near pi
root[5:], dof[5:] = cases.random_state(n - 5, rng)
grp = lambda g: slice(5 + g * G, 5 + (g + 1) * G)
root[grp(1), :2] += rng.choice([-1000.0, 1000.0], (G, 2)).astype(np.float32)
dof[grp(2), :, 0] = 0.0
for g, norms in ((3, rng.uniform(0.0, 1e-3, G)), (4, 1e-3 * (1 + rng.uniform(-1e-3, 1e-3, G))),
                 (5, np.pi * (1 + rng.uniform(-0.01, 0.01, G)))):
    for e, j, t in zip(range(*grp(g).indices(n)), rng.integers(0, 23, G), norms):
        v = dof[e, 3 * j:3 * j + 3, 0].astype(np.float64)
        dof[e, 3 * j:3 * j + 3, 0] = (v * (t / np.linalg.norm(v))).astype(np.float32)
th = np.linalg.norm(dof[5:, :, 0].reshape(n - 5, 23, 3), axis=2)
print('joints below 1e-3 rad:', int((th < 1e-3).sum()), ' within 1% of pi:', int((abs(th - np.pi) < 0.0315).sum()),
      ' roots 1 km away:', int((abs(root[:, 0]) > 900).sum()))
eng = Engine(load_default_model(), n, device=0)
dev = eng.device
ids = torch.arange(1, n, dtype=torch.int32, device=dev)
eng.set_root_state_indexed(torch.from_numpy(root).to(dev), ids)
eng.set_dof_state_indexed(torch.from_numpy(dof.reshape(n * 69, 2)).to(dev), ids)
dyn, sol = dynamics.Dynamics(eng), solve.Solver(eng)
out = {}
for flags in range(4):  # armature x gravity
    t = {k: torch.zeros(s, device=dev) for k, s in dynamics.output_shapes(n).items()}
    dyn.refresh_into(t['jacobian'], t['mass_matrix'], t['bias'], flags=flags)
    out.update({f'{k}_flags{flags}': v.cpu().numpy() for k, v in t.items()})
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
f = np.zeros((n, 75), np.float32)
f[:, 6:] = rng.uniform(-100, 100, (n, 69))
out['fd'] = sol.forward_dynamics().cpu().numpy()
out['fd_force'] = sol.forward_dynamics(cu(f)).cpu().numpy()
tau, a_b = sol.computed_torque(cu(rng.uniform(-20, 20, (n, 69))), cu(f))
out['ct_tau'], out['ct_base_acc'] = tau.cpu().numpy(), a_b.cpu().numpy()
for k in (1, 6, 32):
    out[f'solve_k{k}'] = sol.solve(cu(rng.normal(size=(n, k, 75)))).cpu().numpy()
if len(sys.argv) > 4:  # the task library: every term and both modes at k = 1, 6 (offset points), 32
    import task_reference as TR
    from humanoid_amd.body_sets import BODY_NAMES
    sets = TR.row_sets(list(BODY_NAMES))
    off = (0.03, -0.02, 0.01)
    sets[6] = [(b, a, off) for b, a, _ in sets[6]]
    ts = task.TaskSpace(eng)
    for k in (1, 6, 32):
        ts.set_rows(sets[k])
        xdd = cu(rng.uniform(-5, 5, (n, k)))
        for flags in range(4):
            out.update({f'task_{name}_k{k}_flags{flags}': v.cpu().numpy() for name, v in ts.terms(cu(f), flags=flags).items()})
        for mode in ('force', 'joint'):
            for lam in (0.0, 0.01):
                names = (f'task_{x}_k{k}_{mode}_damping{lam}' for x in ('u', 'F', 'qdd'))
                out.update({name: v.cpu().numpy() for name, v in zip(names, ts.control(xdd, cu(f), mode, lam))})
    del ts
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
del dyn, sol, eng  # before the interpreter takes the modules their destructors use
"""


def queries(dirs):
    """--queries: the dynamics and solve libraries of two directories on the same seeded states (the same
    product engine library on both sides), every output compared byte for byte; the task library's outputs
    too when both directories hold one."""
    import tempfile
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from humanoid_amd import build
    env = {k: v for k, v in os.environ.items() if k != "HE_ENGINE_LIB"}
    differs = False
    with tempfile.TemporaryDirectory() as tmp:  # 70 MB a side: not among the records
        outs = []
        dynamics, solve, task = (os.path.basename(build.LIBRARIES[n].path) for n in ("dynamics", "solve", "task"))
        with_task = all(os.path.exists(os.path.join(d, task)) for d in dirs)
        if not with_task:
            print(f"no {task} on both sides: the task library's outputs are left out", flush=True)
        for k, d in enumerate(dirs):
            libs = [os.path.abspath(os.path.join(d, name)) for name in (dynamics, solve) + ((task,) if with_task else ())]
            print(f"side {'AB'[k]}: {d}  device code: dynamics {build.device_code_id(libs[0])}, "
                  f"solve {build.device_code_id(libs[1])}" + (f", task {build.device_code_id(libs[2])}" if with_task else ""),
                  flush=True)
            outs.append(os.path.join(tmp, f"queries_{k}.npz"))
            subprocess.run([sys.executable, "-c", CODE_QUERIES, outs[-1]] + libs, check=True, env=env, timeout=300)
        a, b = np.load(outs[0]), np.load(outs[1])
        for key in a.files:
            same = a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes()
            differs |= not same
            print(key, a[key].shape, "identical" if same else
                  f"differs (max {np.nanmax(np.abs(a[key].astype(np.float64) - b[key])):.3g}, "
                  f"{int((a[key].view(np.uint32) != b[key].view(np.uint32)).sum())} words)")
    return 1 if differs else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--queries", action="store_true", help="libs are two directories, each with the query libraries")
    ap.add_argument("--lying", action="store_true")
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--config", default="imitation")
    ap.add_argument("--scheme", choices=["default", "pgs", "r02", "tgs_small"], default="default")
    ap.add_argument("--max-contacts", type=int, default=40, help="--lying: the contact capacity in the sim params")
    ap.add_argument("--num-envs", type=int, default=None)
    args = ap.parse_args()
    if args.queries:
        return queries(args.libs)
    n = args.num_envs or (4096 if (args.config, args.scheme) == ("imitation", "default") else 512)
    outs = []
    for k, lib in enumerate(args.libs):
        out = f"gpurun_out/ident_{k}.npz"
        os.makedirs(os.path.dirname(out), exist_ok=True)
        env = dict(os.environ, HE_ENGINE_LIB=os.path.abspath(lib))
        if args.lying:
            cmd = [sys.executable, "-c", CODE_LYING, out, str(args.max_contacts)]
        else:
            cmd = [sys.executable, "-c", CODE, out, "1" if args.fused else "0", args.config, args.scheme, str(n)]
        subprocess.run(cmd, check=True, env=env, timeout=300)
        outs.append(out)
    import numpy as np
    a, b = np.load(outs[0]), np.load(outs[1])
    differs = False
    for key in a.files:
        same = a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes()  # the bits (NaN payloads too)
        differs |= not same
        print(key, "identical" if same else f"differs (max {np.nanmax(np.abs(a[key].astype(np.float64) - b[key])):.3g})")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
