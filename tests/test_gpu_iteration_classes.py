"""The TGS kernel's three iteration-loop instantiations in one launch, against the fp64 oracle.

physics_kernel_tgs runs its position iterations in one of three loops, chosen per env and physics step
by the row count: up to 32 rows (solve_tgs<32>; a standing body: 28 rows, all on the feet, the leg
class), 33-63 rows (solve_tgs<MAXR>, the wide class with its 48- and 63-row sweeps) and no rows
(tgs_free_iterations). The three differ in what they keep in registers over the iterations, and a
change to that (spills) is compared bit for bit with its parent on the bench rollouts only;
this test holds each loop to the oracle, 16 envs over 8 policy steps:

* 6 standing on the plane, PD stand-still (as test_physics_standing_matches_oracle);
* 6 lying with folded limbs: lying bodies settled on the plane by the oracle (3 s), then driven
  toward joint targets 0.05 rad off their pose; four or five of them hold 33 to 63 rows in every step
  (both of the wide class's sweeps, 33-48 and 49-63 rows), the others 27 to 33;
* 4 dropped from 1 m above the standing height under random targets: no rows at first.

That each class occurs is asserted from word 7 of the warm-start cache (the last solve's row count),
of the oracle's cache alone (a CPU test) and then of the engine's.

Tolerances: those of tests/test_gpu_parity.py (_physics_compare, which tests/test_gpu_pgs.py uses too):
positions, joint angles, the centre of mass and quaternions 1e-4, velocities 1e-2 + 1e-3 rel, dof
forces 0.5 N m + 1e-3 rel, widened by 4 x the oracle's own sensitivity only where that exceeds the
tolerance (_cond_close, 8 probes as for runs past 5 steps), at most 5 % of the elements widened. The
rigid-body rows beyond the positions _physics_compare checks take the root's tolerances (quaternions
1e-4, velocities 1e-2 + 1e-3 rel); the contact forces take the dof forces' (0.5 N + 1e-3 rel: both are
the solve's impulses over dt, and a joint-limit row's impulse appears in both). An env is left out only
when the oracle itself says its contact set is within rounding of changing (a probe's contact keys
differ from the oracle's in some step): decided on the CPU, never by the engine's result, and at most
one env of each class; every other env's contact keys and row counts must equal the oracle's in every
step."""
import numpy as np
import pytest

from humanoid_amd import _abi
from oracle import oracle as O

import cases

N_STAND, N_LYING, N_DROP = 6, 6, 4
N = N_STAND + N_LYING + N_DROP
STEPS, CALLS, NPROBES = 8, 2, 8
STAND = slice(0, N_STAND)
LYING = slice(N_STAND, N_STAND + N_LYING)
DROP = slice(N_STAND + N_LYING, N)
LEG_BODIES = set(range(9))  # Pelvis, L/R Hip, Knee, Ankle, Toe


def _keys(cache):
    n, keys, _ = _abi.cache_rows(cache)
    return [tuple(sorted(int(k) for k in keys[e, :n[e]] if (k >> 14) == 0)) for e in range(keys.shape[0])]


def _rows(cache):
    return _abi.cache_rows(cache)[0].copy()


@pytest.fixture(scope="module")
def reference(model, he_model):
    """The start states, and the oracle's run with its probes: computed once, read by both tests."""
    rng = np.random.default_rng(40)
    sp = _abi.default_sim_params()
    rs, ds = cases.standing_state(model, N_STAND, rng, xy_jitter=1.0)
    ts = np.zeros((N_STAND, 69), np.float32)
    # lying, half of them face down, settled by the oracle for 90 policy steps (3 s)
    rl, dl = cases.lying_state(N_LYING, rng, on_floor=True, model=model)
    rl[N_LYING // 2:, 3] *= -1
    rb = O.forward_kinematics(he_model, rl, dl)
    rl[:, 2] += (0.005 - cases.ground_gaps(model, rb).min(-1)).astype(np.float32)
    hold = dl[..., 0].copy()
    cl = O.new_cache(N_LYING)
    for _ in range(90):
        O.physics_step(he_model, sp, rl, dl, hold, CALLS, cache=cl)
    tl = (dl[..., 0] + rng.uniform(-0.05, 0.05, (N_LYING, 69))).astype(np.float32)
    rd, dd = cases.standing_state(model, N_DROP, rng, xy_jitter=1.0)
    rd[:, 2] += 1.0
    td = rng.uniform(-0.3, 0.3, (N_DROP, 69)).astype(np.float32)
    root = np.concatenate([rs, rl, rd]).astype(np.float32)
    dof = np.concatenate([ds, dl, dd]).astype(np.float32)
    targets = np.concatenate([ts, tl, td])

    r_o, d_o, c_o = root.copy(), dof.copy(), O.new_cache(N)
    probes = [[root.copy(), dof.copy(), None, O.new_cache(N)] for _ in range(NPROBES)]
    rows, keys, row_bodies = [], [], []
    fragile = np.zeros(N, bool)  # a probe's contact set differs from the oracle's in some step
    out = None
    for step in range(STEPS):
        out = O.physics_step(he_model, sp, r_o, d_o, targets, CALLS, cache=c_o)
        for k, pr in enumerate(probes):
            pr[2] = cases.probe_physics_step(he_model, sp, pr[0], pr[1], targets, CALLS, pr[3], 123 + 1000 * k + step)
            fragile |= np.array([a != b for a, b in zip(_keys(pr[3]), _keys(c_o))])
        rows.append(_rows(c_o))
        keys.append(_keys(c_o))
        n, kk, _ = _abi.cache_rows(c_o)
        row_bodies.append([{b for k in kk[e, :n[e]] for b in _abi.key_fields(k)[:2] if b >= 0} for e in range(N)])
    return dict(root=root, dof=dof, targets=targets, r=r_o, d=d_o, out=out, probes=probes, rows=np.array(rows),
                keys=keys, row_bodies=row_bodies, fragile=fragile)


def test_oracle_reaches_every_iteration_class(reference):
    """The condition of the GPU test, from the oracle alone: the poses reach the three loops."""
    rows, fragile = reference["rows"], reference["fragile"]
    print("oracle rows per step:\n", rows, "\nfragile contact sets:", np.flatnonzero(fragile).tolist())
    # <= 32 rows, leg class: every standing env in every step, every row on the root and the legs
    assert ((rows[:, STAND] > 0) & (rows[:, STAND] <= 32)).all()
    assert all(b <= LEG_BODIES for step in reference["row_bodies"] for b in step[STAND])
    # > 32 rows: in every step at least four of the six lying envs, with both sweeps of the wide class
    # (33-48 rows, 49-63 rows) in every step
    wide = rows[:, LYING] > 32
    assert (wide.sum(1) >= 4).all()
    assert (wide & (rows[:, LYING] <= 48)).any(1).all() and (rows[:, LYING] > 48).any(1).all()
    # no rows at first: every dropped env
    assert (rows[0, DROP] == 0).all()
    for cls in (STAND, LYING, DROP):
        assert fragile[cls].sum() <= 1


@pytest.mark.gpu
def test_iteration_classes_match_oracle(reference, he_model, model):
    torch = pytest.importorskip("torch")
    from test_gpu_parity import CondStats, _cond_close, cu, make_engine
    ref = reference
    eng = make_engine(he_model, N)
    eng.root_states.copy_(cu(ref["root"]))
    eng.dof_state.copy_(cu(ref["dof"].reshape(N * 69, 2)))
    eng.dof_targets.copy_(cu(ref["targets"]))
    ok = ~ref["fragile"]
    for step in range(STEPS):
        eng.simulate(CALLS)
        torch.cuda.synchronize()
        cg = eng.contact_cache.cpu().numpy()
        rows_g, keys_g = _rows(cg), _keys(cg)
        print(f"step {step}: engine rows {rows_g.tolist()}")
        # each class occurred on the engine as on the oracle, with the oracle's contact set
        assert (rows_g[ok] == ref["rows"][step][ok]).all(), f"step {step}: row counts {rows_g} vs {ref['rows'][step]}"
        bad = [e for e in np.flatnonzero(ok) if keys_g[e] != ref["keys"][step][e]]
        assert not bad, f"step {step}: contact keys differ in envs {bad}"
    out = ref["out"]
    assert (eng.num_contacts.cpu().numpy()[ok] == out["num_contacts"][ok]).all()
    rg = eng.root_states.cpu().numpy()
    dg = eng.dof_state.view(N, 69, 2).cpu().numpy()
    rbg = eng.rb_state.view(N, 24, 13).cpu().numpy()
    fg = eng.dof_force.view(N, 69).cpu().numpy()
    cfg = eng.contact_forces.view(N, 24, 3).cpu().numpy()
    r_o, d_o = ref["r"], ref["d"]
    R = [p[0] for p in ref["probes"]]
    D = [p[1] for p in ref["probes"]]
    OS = [p[2] for p in ref["probes"]]

    def align(q, to):  # quaternions up to sign
        return np.where((q * to).sum(-1, keepdims=True) < 0, -q, q)

    pos_tol, vel_tol = 1e-4, 1e-2
    st = CondStats()
    kw = dict(stats=st)
    rbo = out["rb_state"]
    _cond_close("root pos", rg[ok, :3], r_o[ok, :3], [r[ok, :3] for r in R], pos_tol, **kw)
    _cond_close("root quat", align(rg[ok, 3:7], r_o[ok, 3:7]), r_o[ok, 3:7],
                [align(r[ok, 3:7], r_o[ok, 3:7]) for r in R], pos_tol, **kw)
    _cond_close("dof pos", dg[ok, :, 0], d_o[ok, :, 0], [d[ok, :, 0] for d in D], pos_tol, **kw)
    _cond_close("root vel", rg[ok, 7:], r_o[ok, 7:], [r[ok, 7:] for r in R], vel_tol, 1e-3, **kw)
    _cond_close("dof vel", dg[ok, :, 1], d_o[ok, :, 1], [d[ok, :, 1] for d in D], vel_tol, 1e-3, **kw)
    _cond_close("body pos", rbg[ok, :, :3], rbo[ok, :, :3], [o["rb_state"][ok, :, :3] for o in OS], pos_tol, **kw)
    _cond_close("body quat", align(rbg[ok, :, 3:7], rbo[ok, :, 3:7]), rbo[ok, :, 3:7],
                [align(o["rb_state"][ok, :, 3:7], rbo[ok, :, 3:7]) for o in OS], pos_tol, **kw)
    _cond_close("body vel", rbg[ok, :, 7:], rbo[ok, :, 7:], [o["rb_state"][ok, :, 7:] for o in OS], vel_tol, 1e-3, **kw)
    com_g = cases.center_of_mass(model, rbg[ok])
    com_o = cases.center_of_mass(model, rbo[ok])
    _cond_close("CoM", com_g, com_o, [cases.center_of_mass(model, o["rb_state"][ok]) for o in OS], pos_tol, **kw)
    _cond_close("dof force", fg[ok], out["dof_force"][ok], [o["dof_force"][ok] for o in OS], 0.5, 1e-3, **kw)
    _cond_close("contact force", cfg[ok], out["contact_forces"][ok], [o["contact_forces"][ok] for o in OS], 0.5, 1e-3,
                **kw)
    print(f"sensitivity-widened elements: {st.widened}/{st.total} ({100 * st.frac:.2f}%) {st.by_name}")
    assert st.frac <= 0.05, f"{st.widened}/{st.total} elements needed the widening: {st.by_name}"
