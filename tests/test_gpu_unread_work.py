"""The physics step's left-out work (DESIGN §4.1 "Unread work") on the paths the bench rollouts do not
reach: a launch in which an env leaves the leg class between two physics steps, the reported forces of
launches of one, two and three physics steps, and boxes with more than four candidate corners beside
boxes with four or fewer.

Every condition a GPU test relies on is established on the CPU, from the fp64 oracle alone
(test_oracle_*), and the oracle's runs are computed once per module."""
import os

import numpy as np
import pytest

from humanoid_amd import _abi
from oracle import oracle as O

import cases
import contact_cases as CC

LEG_BODIES = set(range(9))  # Pelvis, L/R Hip, Knee, Ankle, Toe


def _row_bodies(cache):
    n, keys, _ = _abi.cache_rows(cache)
    return [{b for k in keys[e, :n[e]] for b in _abi.key_fields(k)[:2] if b >= 0} for e in range(keys.shape[0])]


# ---------------------------------------------------------------------------- class flip inside a launch
N_STAND = 4
# A body leaning forward on its toes, arms hanging straight down, held by its drives and tipping over: the
# hands' distance to the plane at the start decides the physics step (1/120 s) at which a hand comes within
# the contact offset. With these four the oracle's first hand row is in physics step 4, 7, 10 and 12 of the
# 12 (three launches of four), each at least 1 mm of start height away from the neighbouring step: inside
# a launch, after a step of the same launch that had leg rows only.
HAND_GAPS = (0.0226, 0.0306, 0.0456, 0.058)
FLIP_STEPS = (4, 7, 10, 12)
POLICY_STEPS, CALLS = 3, 2


def _leaning_pose(model, he_model, theta, lift=0.01):
    """Root pitched by theta about y, the shoulders turned so that both arms point straight down, the
    lowest leg point `lift` above the plane. Returns root, dof and the bodies' ground gaps."""
    root = np.zeros((1, 13), np.float32)
    dof = np.zeros((1, 69, 2), np.float32)
    root[0, 3:7] = [0, np.sin(theta / 2), 0, np.cos(theta / 2)]
    c, s = np.cos(theta), np.sin(theta)
    down = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T @ np.array([0, 0, -1.0])  # world down in the root frame
    for joint, y in ((15, 1.0), (20, -1.0)):  # L_Shoulder, R_Shoulder: the arm's rest direction is +-y
        a = np.array([0, y, 0.0])
        ax = np.cross(a, down)
        dof[0, 3 * (joint - 1):3 * joint, 0] = ax / np.linalg.norm(ax) * np.arctan2(np.linalg.norm(ax), a @ down)
    gaps = cases.ground_gaps(model, O.forward_kinematics(he_model, root, dof))[0]
    root[0, 2] += lift - gaps[:9].min()
    return root, dof, cases.ground_gaps(model, O.forward_kinematics(he_model, root, dof))[0]


def _leaning_state(model, he_model, hand_gap):
    lo, hi = 1.1, 1.35  # the hands' gap falls from 0.18 m to below the plane over this range
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        if _leaning_pose(model, he_model, mid)[2][9:].min() > hand_gap:
            lo = mid
        else:
            hi = mid
    return _leaning_pose(model, he_model, 0.5 * (lo + hi))[:2]


@pytest.fixture(scope="module")
def flip_case(model, he_model):
    rs, ds = cases.standing_state(model, N_STAND, np.random.default_rng(3), xy_jitter=1.0)
    lean = [_leaning_state(model, he_model, g) for g in HAND_GAPS]
    root = np.concatenate([rs] + [r for r, _ in lean]).astype(np.float32)
    dof = np.concatenate([ds] + [d for _, d in lean]).astype(np.float32)
    targets = dof[..., 0].copy()
    # the oracle, one physics step per call (dt / substeps of the engine's defaults), for the rows' bodies
    sp = _abi.default_sim_params(dt=1.0 / 120.0, substeps=1)
    r, d, c = root.copy(), dof.copy(), O.new_cache(len(root))
    bodies, rows = [], []
    for _ in range(POLICY_STEPS * CALLS * 2):
        O.physics_step(he_model, sp, r, d, targets, 1, cache=c)
        bodies.append(_row_bodies(c))
        rows.append(_abi.cache_rows(c)[0].copy())
    return dict(root=root, dof=dof, targets=targets, bodies=bodies, rows=np.array(rows))


def test_oracle_leaves_the_leg_class_inside_a_launch(flip_case):
    bodies, rows = flip_case["bodies"], flip_case["rows"]
    assert ((rows > 0) & (rows <= 32)).all(), rows  # the <= 32-row class throughout
    for e in range(N_STAND):
        assert all(step[e] <= LEG_BODIES for step in bodies)
    for k, want in enumerate(FLIP_STEPS):
        first = next(s + 1 for s, step in enumerate(bodies) if not step[N_STAND + k] <= LEG_BODIES)
        assert first == want, (k, first)
        assert (first - 1) % (2 * CALLS) != 0  # not a launch's first step: the step before it is of the same launch


@pytest.mark.gpu
def test_class_flip_inside_a_launch_leaves_the_step_unchanged(flip_case, he_model):
    """State, caches, rb rows and dof forces of the eight envs, bit for bit against HE_TGS_LEGS=0 (every
    env over all 75 dofs), with the leaning envs' hands arriving inside the first, second and third launch."""
    torch = pytest.importorskip("torch")
    from test_gpu_parity import cu, make_engine
    n = len(flip_case["root"])
    outs, left = [], []
    for v in ("0", "1"):
        os.environ["HE_TGS_LEGS"] = v
        try:
            eng = make_engine(he_model, n)
        finally:
            os.environ.pop("HE_TGS_LEGS", None)
        eng.root_states.copy_(cu(flip_case["root"]))
        eng.dof_state.copy_(cu(flip_case["dof"].reshape(n * 69, 2)))
        eng.dof_targets.copy_(cu(flip_case["targets"]))
        per_step = []
        for _ in range(POLICY_STEPS):
            eng.simulate(CALLS)
            torch.cuda.synchronize()
            per_step.append([t.clone() for t in (eng.root_states, eng.dof_state, eng.contact_cache, eng.rb_state,
                                                 eng.dof_force, eng.contact_forces)])
            left.append([not b <= LEG_BODIES for b in _row_bodies(eng.contact_cache.cpu().numpy())])
        outs.append(per_step)
    # the engine took the oracle's course: after each launch, the envs whose hand has arrived
    for launch in range(POLICY_STEPS):
        want = [False] * N_STAND + [s <= 2 * CALLS * (launch + 1) for s in FLIP_STEPS]
        assert left[launch] == want and left[POLICY_STEPS + launch] == want, (launch, left)
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert torch.isfinite(x).all()
            assert torch.equal(x, y), "the leg class must not change any env's step"


# ---------------------------------------------------------------------------- reported forces, 1-3 steps
N_FORCE, FORCE_STEPS, FORCE_PROBES = 4, 2, 3
KNEE_Y = 4  # L_Knee's y dof


def _force_state(model):
    """Env 0 and 3 stand on the plane under small targets; env 1 hangs 1.5 m up with its left knee held at
    the angle limit (a limit row, and the folded leg's self pairs); env 2 hangs there with no row at all."""
    rng = np.random.default_rng(17)
    root, dof = cases.standing_state(model, N_FORCE, rng, xy_jitter=0.5)
    root[1:3, 2] += 1.5
    targets = rng.uniform(-0.1, 0.1, (N_FORCE, 69)).astype(np.float32)
    targets[0] = 0.0
    dof[1, KNEE_Y, 0] = np.pi - 0.03
    targets[1] = 0.0
    targets[1, KNEE_Y] = 5.0
    return root, dof, targets


@pytest.fixture(scope="module")
def force_reference(model, he_model):
    root, dof, targets = _force_state(model)
    ref = {}
    for sub in (1, 2, 3):
        sp = _abi.default_sim_params(substeps=sub)
        r, d, c = root.copy(), dof.copy(), O.new_cache(N_FORCE)
        probes = [[root.copy(), dof.copy(), None, O.new_cache(N_FORCE)] for _ in range(FORCE_PROBES)]
        for step in range(FORCE_STEPS):
            out = O.physics_step(he_model, sp, r, d, targets, 1, cache=c)
            for k, pr in enumerate(probes):
                pr[2] = cases.probe_physics_step(he_model, sp, pr[0], pr[1], targets, 1, pr[3], 123 + 1000 * k + step)
        ref[sub] = dict(out=out, probes=[p[2] for p in probes], cache=c)
    return dict(root=root, dof=dof, targets=targets, ref=ref)


def test_oracle_force_case_has_a_limit_row_and_a_free_env(force_reference):
    for sub, ref in force_reference["ref"].items():
        n, keys, lam = _abi.cache_rows(ref["cache"])
        assert n[0] > 0 and n[3] > 0 and n[2] == 0, (sub, n)
        k1 = [_abi.key_fields(k) for k in keys[1, :n[1]]]
        assert k1[0][:2] == (2, -2) and lam[1, 0] > 0, (sub, k1)  # L_Knee's limit row, holding the joint
        assert all(b1 >= 0 for _, b1, _, _ in k1[1:])  # beside it only the folded leg's self pairs: no terrain
        assert np.abs(ref["out"]["contact_forces"][[0, 3]]).max() > 100.0  # the standing envs' feet carry them
        assert (ref["out"]["contact_forces"][2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 2, 3])
def test_reported_forces_are_the_last_physics_steps(force_reference, he_model, substeps):
    """dof_force and contact_forces after two launches of `substeps` physics steps against the oracle's, at
    the parity tests' tolerances for them (0.5 + 1e-3 rel, widened by the oracle's own sensitivity only where
    that exceeds the tolerance, at most 5 % of the elements: test_gpu_parity._physics_compare,
    test_gpu_iteration_classes)."""
    torch = pytest.importorskip("torch")
    from test_gpu_parity import CondStats, _cond_close, cu, make_engine
    fr = force_reference
    eng = make_engine(he_model, N_FORCE, substeps=substeps)
    eng.root_states.copy_(cu(fr["root"]))
    eng.dof_state.copy_(cu(fr["dof"].reshape(N_FORCE * 69, 2)))
    eng.dof_targets.copy_(cu(fr["targets"]))
    for _ in range(FORCE_STEPS):
        eng.simulate(1)
    torch.cuda.synchronize()
    ref = fr["ref"][substeps]
    out, probes = ref["out"], ref["probes"]
    assert (_abi.cache_rows(eng.contact_cache.cpu().numpy())[0] == _abi.cache_rows(ref["cache"])[0]).all()
    fg = eng.dof_force.view(N_FORCE, 69).cpu().numpy()
    cfg = eng.contact_forces.view(N_FORCE, 24, 3).cpu().numpy()
    print(f"substeps {substeps}: |dof force - oracle| max {np.abs(fg - out['dof_force']).max():.3e}, "
          f"|contact force - oracle| max {np.abs(cfg - out['contact_forces']).max():.3e}")
    st = CondStats()
    _cond_close("dof force", fg, out["dof_force"], [o["dof_force"] for o in probes], 0.5, 1e-3, stats=st)
    _cond_close("contact force", cfg, out["contact_forces"], [o["contact_forces"] for o in probes], 0.5, 1e-3, stats=st)
    assert st.frac <= 0.05, f"{st.widened}/{st.total} elements needed the widening: {st.by_name}"
    assert (cfg[2] == 0).all()  # no contact: nothing left over from an earlier step or launch


# ---------------------------------------------------------------------------- corner ranking
N_BOX = 8
BOXES = (3, 4, 7, 8)  # the ankle and toe boxes
SUNK = {2: (4, 8), 6: (3, 4, 7, 8)}  # env: its boxes with all eight corners within the contact offset


def _box_case(model):
    """Plane (kind 0) and steps (kind 2). Env 0, 1, 4: standing (four bottom corners per box, env 4 on the
    second step); env 2: 0.03 m into the plane (the toe boxes, 0.04 m high, entirely within the offset);
    env 6: 0.08 m into the first step (the ankle boxes, 0.092 m high, too); env 3, 5: pitched and rolled by
    0.3 rad (one or two corners per box); env 7: 0.5 m up (none)."""
    root, dof = cases.standing_state(model, N_BOX)
    kind = np.array([0, 0, 0, 0, 2, 2, 2, 0], np.int32)
    sp = _abi.default_sim_params()
    root[:, 0] = [0.0, 0.7, -0.3, 0.2, 2.5 * sp.step_length, 1.5 * sp.step_length, 1.5 * sp.step_length, 0.0]
    root[4, 2] += 2 * sp.step_height
    root[5:7, 2] += sp.step_height
    root[2, 2] -= 0.03
    root[6, 2] -= 0.08
    root[7, 2] += 0.5
    for e, axis in ((3, 1), (5, 0)):
        root[e, 3 + axis], root[e, 6] = np.sin(0.15), np.cos(0.15)
        root[e, 2] += 0.02
    return dict(root=root, dof=dof, sim=dict(substeps=1, terrain=1), terrain_kind=kind)


def _corner_candidates(model, he_model, case):
    """Corners within the contact offset of the terrain, per env and box: counted here from the rigid-body
    rows, by the terrain rule of DESIGN §5 (plane z = 0; steps of step_height every step_length for x > 0)."""
    sp = _abi.default_sim_params(**case["sim"])
    rb = O.forward_kinematics(he_model, case["root"], case["dof"]).astype(np.float64)
    count = np.zeros((N_BOX, len(BOXES)), int)
    for j, b in enumerate(BOXES):
        g = np.asarray(model.geom_params[b], np.float64)
        sg = np.array([[(c & 1) * 2 - 1, ((c >> 1) & 1) * 2 - 1, ((c >> 2) & 1) * 2 - 1] for c in range(8)], np.float64)
        pts = g[None, 0:3] + (sg * g[3:6]) @ cases._qmat(g[6:10]).T
        w = rb[:, b, None, :3] + np.einsum("nij,kj->nki", cases._qmat(rb[:, b, 3:7]), pts)
        h = np.where((case["terrain_kind"][:, None] == 2) & (w[..., 0] > 0),
                     sp.step_height * np.floor(w[..., 0] / sp.step_length), 0.0)
        count[:, j] = ((w[..., 2] - h) < sp.contact_offset).sum(1)
    return count


@pytest.fixture(scope="module")
def box_case(model, he_model):
    case = _box_case(model)
    slots, out = CC.oracle_contacts(case)
    return dict(case=case, slots=slots, out=out, candidates=_corner_candidates(model, he_model, case))


def test_oracle_keeps_the_four_deepest_corners_of_a_sunk_box(box_case):
    cand, slots = box_case["candidates"], box_case["slots"]
    print("candidate corners per env and box:\n", cand)
    keys = slots[:, :, 7].astype(np.int64)
    for e in range(N_BOX):
        for j, b in enumerate(BOXES):
            want = 8 if b in SUNK.get(e, ()) else cand[e, j]
            assert cand[e, j] == want and (want == 8 or want <= 4), (e, b, cand[e, j])
            mine = [s for s in range(keys.shape[1]) if keys[e, s] >= 0 and _abi.key_fields(keys[e, s])[:2] == (b, -1)]
            assert len(mine) == min(cand[e, j], 4), (e, b, len(mine))
            if want == 8:  # the kept four are the bottom face, by the gaps, in corner order
                assert slots[e, mine, 6].max() < 0.0
                subs = [_abi.key_fields(keys[e, s])[2] for s in mine]
                assert subs == sorted(subs)
    assert (cand[[0, 1, 4]] == 4).all() and (cand[7] == 0).all() and cand[[3, 5]].max() <= 2 and cand[[3, 5]].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("solver_type", [1, 0])
def test_corner_ranking_matches_the_oracle(box_case, solver_type):
    """The normal rows' keys in slot order and the slot counts equal the oracle's gen_contacts, sunk boxes
    beside boxes with four or fewer candidates in one launch. (The engine exports no gaps; the oracle's are
    checked above, and a slot's key names its body and corner.)"""
    from test_gpu_contact_generation import run_engine
    got = run_engine(box_case["case"], solver_type)
    keys = box_case["slots"][:, :, 7].astype(np.int64)
    for e in range(N_BOX):
        ko = [int(k) for k in keys[e] if k >= 0 and ((k >> 5) & 31) != 0]
        assert got["contact"][e] == ko, (e, got["contact"][e], ko)
    assert (got["num"] == box_case["out"]["num_contacts"]).all()
    assert (got["dropped"] == box_case["out"]["dropped"]).all()
