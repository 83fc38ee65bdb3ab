"""Bit-identity of two engine builds (e.g. a scheduler-flag variant, or a refactored kernel against
its parent): the same run with each library in its own process, the final states compared.

  python tools/lib_identity.py LIB_A LIB_B [--fused] [--config NAME] [--scheme NAME]
  python tools/lib_identity.py LIB_A LIB_B --lying [--max-contacts N]

Default: the bench rollout (configs[2], tracking actions, 4096 envs, TGS, <= 32 rows) for 20 steps;
--fused runs it as the one-launch env step. --config / --scheme go to bench.Rollout as in
tools/phase_profile.py (512 envs: envs never interact): `--config dr` reaches the terrain kinds and
the per-env properties, `--scheme pgs` physics_kernel. --lying: 512 lying bodies lowered into the
plane (25-40 contacts, most solves past 32 rows: the TGS wide class) under random targets, 10 policy
steps; with --max-contacts below the contacts generated it reaches the overflow reduction, and the
count of envs that dropped contacts is printed (0: the mode did not reach it, lower the cap)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--lying", action="store_true")
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--config", default="imitation")
    ap.add_argument("--scheme", choices=["default", "pgs", "r02", "tgs_small"], default="default")
    ap.add_argument("--max-contacts", type=int, default=40, help="--lying: the contact capacity in the sim params")
    ap.add_argument("--num-envs", type=int, default=None)
    args = ap.parse_args()
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
