"""Contact generation on the GPU against the independent reference (tests/contact_reference.py), not
through the oracle: the kept normal-row keys of the warm-start cache in slot order, ``num_contacts`` and
``dropped_contacts`` of a fresh engine after one physics step (substeps 1, simulate(1)), for both
solvers (the template picks different scratch). The inputs (tests/contact_cases.py) reach the pair
cull's second compaction pass, the upper half of the deepest-first reduction and the 128-candidate pool;
each test asserts from the reference that its input does. Envs whose reference margin is under 2e-5 m
(contact_reference.BORDERLINE) are left out, at most 5 % of a case. The oracle is held to the same
reference on the same inputs by tests/test_contact_generation.py."""
import numpy as np
import pytest

from humanoid_amd import _abi

import contact_cases as CC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SOLVERS = pytest.mark.parametrize("solver_type", [1, 0])


def run_engine(case, solver_type):
    """One step of a fresh engine from the case's state: per env the contact keys and the limit keys of
    the cache's normal rows (row order = slot order), num_contacts, dropped_contacts, contact_forces."""
    from humanoid_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    _, hm, _ = CC.models()
    n = case["root"].shape[0]
    sp = (_abi.default_sim_params if solver_type == 1 else _abi.pgs_sim_params)(**case["sim"])
    eng = Engine(hm, n, device=0, sim_params=sp)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")  # noqa: E731
    if case["terrain_kind"] is not None:
        eng.set_env_properties(None, None, dev(case["terrain_kind"]))
    eng.root_states.copy_(dev(case["root"]))
    eng.dof_state.copy_(dev(case["dof"].reshape(n * 69, 2)))
    eng.dof_targets.copy_(dev(np.zeros((n, 69), np.float32)))
    eng.simulate(1)
    torch.cuda.synchronize()
    rows, keys, _ = _abi.cache_rows(eng.contact_cache.cpu().numpy())
    contact, limit = [], []
    for e in range(n):
        k = keys[e, :rows[e]]
        k = k[(k >> 14) == 0]
        lim = ((k >> 5) & 31) == 0
        contact.append(k[~lim].tolist())
        limit.append(k[lim].tolist())
    return dict(contact=contact, limit=limit, num=eng.num_contacts.cpu().numpy().copy(),
                dropped=eng.dropped_contacts.cpu().numpy().copy(),
                forces=eng.contact_forces.view(n, 24, 3).cpu().numpy().copy())


def assert_engine_equals_reference(case, got, oracle_limit_keys=None):
    ref, ok = case["ref"], case["ok"]
    print(CC.describe(case))
    CC.assert_borderline_share(case)
    bad = []
    for e in np.flatnonzero(ok):
        kr = ref["key"][e][ref["key"][e] >= 0].tolist()
        same = (got["contact"][e] == kr and got["num"][e] == ref["kept"][e] and got["dropped"][e] == ref["dropped"][e]
                and len(got["limit"][e]) == min(case["nlim"][e], ref["kept"][e]))
        if same and oracle_limit_keys is not None:
            same = got["limit"][e] == oracle_limit_keys[e]
        if not same:
            bad.append(e)
    e = bad[0] if bad else 0
    assert not bad, (f"{len(bad)} envs differ from the reference, first env {e}: candidates {ref['candidates'][e]}, "
                     f"survivors {ref['survivors'][e]}, margin {ref['margin'][e]:.2e}; slots {got['num'][e]} vs "
                     f"{ref['kept'][e]}, dropped {got['dropped'][e]} vs {ref['dropped'][e]}, limit rows "
                     f"{len(got['limit'][e])} vs {case['nlim'][e]}; keys only on the GPU "
                     f"{sorted(set(got['contact'][e]) - set(CC.CR.sorted_keys(ref, e)))}, only in the reference "
                     f"{sorted(set(CC.CR.sorted_keys(ref, e)) - set(got['contact'][e]))}")


@SOLVERS
@pytest.mark.parametrize("cap", [40, 16])
def test_crowded_poses(solver_type, cap):
    case = CC.crowded(cap)
    CC.assert_reaches_crowded_paths(case)
    assert_engine_equals_reference(case, run_engine(case, solver_type))


@SOLVERS
@pytest.mark.parametrize("cap", [40, 16])
def test_crowded_poses_with_limits(solver_type, cap):
    """Joint angles up to 3.1 rad, limits on: the limit keys equal the oracle's, their count the
    reference's."""
    case = CC.crowded(cap, limits=True)
    CC.assert_reaches_crowded_paths(case)
    assert case["nlim"].max() >= 3
    slots, _ = CC.oracle_contacts(case)
    keys = slots[:, :, 7].astype(np.int64)
    lim = [k[(k >= 0) & (((k >> 5) & 31) == 0)].tolist() for k in keys]
    assert_engine_equals_reference(case, run_engine(case, solver_type), oracle_limit_keys=lim)


@SOLVERS
def test_past_the_candidate_pool(solver_type):
    case = CC.past_pool()
    c = case["ref"]["candidates"]
    assert c.min() >= 129 and c.max() <= 160
    assert_engine_equals_reference(case, run_engine(case, solver_type))


@SOLVERS
def test_ordinary_poses(solver_type):
    case = CC.ordinary()
    assert_engine_equals_reference(case, run_engine(case, solver_type))


@SOLVERS
def test_terrain_kinds(solver_type):
    case = CC.terrain_kinds()
    assert_engine_equals_reference(case, run_engine(case, solver_type))


@SOLVERS
def test_contact_offset_threshold(solver_type):
    """The lowest terrain point 1e-4 m under the contact offset is a contact on the GPU, 1e-4 m over it
    no terrain point is, on each terrain kind and for upright, lying and head-down bodies."""
    case = CC.threshold()
    assert case["ok"].all()
    got = run_engine(case, solver_type)
    assert_engine_equals_reference(case, got)
    terr = np.array([sum(1 for k in ks if ((k >> 5) & 31) == 1) for ks in got["contact"]])
    assert (terr[case["above"]] == 0).all() and (terr[~case["above"]] >= 1).all(), terr


@SOLVERS
def test_forces_follow_the_reference_normals(solver_type):
    """Friction 0: a body touched by one contact only reports a force along the reference's normal, +n
    on a pair's first body and -n on its partner, within 1e-4 rad."""
    case = CC.force_direction()
    got = run_engine(case, solver_type)
    assert_engine_equals_reference(case, got)
    CC.assert_forces_along_normals(case, got["forces"])
