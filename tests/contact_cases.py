"""Inputs of the contact-generation tests (tests/test_contact_generation.py on the oracle,
tests/test_gpu_contact_generation.py on the engine), seeded and small, each with its reference result
(tests/contact_reference.py) computed once per session and shared.

A case is a dict: root [N,13] and dof [N,69,2] (fp32), sim (he_sim_params overrides; always substeps 1),
terrain_kind [N] or None, nlim [N] (the joint-limit slots the state raises, from the limit rule of
DESIGN §5), ref (the reference's result) and ok [N] (envs that are not borderline)."""
import functools

import numpy as np

from humanoid_amd import _abi
from humanoid_amd.model import load_default_model
from oracle import oracle as O

import cases
import contact_reference as CR

LIMIT_GUARD, LIMIT_MARGIN = 0.02, 0.1  # DESIGN §5 "Joint limits"; he_sim_params.limit_margin's default


@functools.lru_cache(None)
def models():
    model = load_default_model()
    hm = _abi.make_model(model)
    return model, hm, CR.Model(hm)


def _random_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def folded_state(n, rng, angle=(1.5, 3.0), height=(0.1, 0.3)):
    """Joints bent by `angle` rad about random axes, the root at `height` at any tilt: limbs folded
    onto the trunk and each other, on the ground."""
    root = np.zeros((n, 13), np.float32)
    root[:, :2] = rng.uniform(-1, 1, (n, 2))
    root[:, 2] = rng.uniform(*height, n)
    root[:, 3:7] = _random_quat(rng, n)
    ax = rng.normal(size=(n, 23, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    dof = np.zeros((n, 69, 2), np.float32)
    dof[..., 0] = (ax * rng.uniform(*angle, (n, 23, 1))).reshape(n, 69)
    return root, dof


def limit_slots(dof):
    """The joint-limit slots of a state at rest (one row per joint whose rotation angle is
    within limit_margin of pi - 0.02) and the distance (rad) of the nearest joint to that threshold."""
    ang = np.linalg.norm(dof[..., 0].astype(np.float64).reshape(dof.shape[0], 23, 3), axis=-1)
    th = np.pi - LIMIT_GUARD - LIMIT_MARGIN
    return (ang > th).sum(1), np.abs(ang - th).min(1)


def finish(root, dof, terrain_kind=None, **sim):
    """The case dict of a state: its reference result and the envs that are not borderline."""
    _, _, M = models()
    sp = _abi.default_sim_params(substeps=1, **sim)
    n = root.shape[0]
    nlim, lim_margin = limit_slots(dof) if sp.joint_limits else (np.zeros(n, np.int64), np.full(n, np.inf))
    ref = CR.generate(M, root, dof[..., 0], contact_offset=sp.contact_offset, terrain_kind=terrain_kind,
                      terrain_slope=sp.terrain_slope, step_height=sp.step_height, step_length=sp.step_length,
                      max_contacts=sp.max_contacts, nlim=nlim, self_collision=bool(sp.self_collision))
    ok = (ref["margin"] >= CR.BORDERLINE) & (lim_margin >= CR.BORDERLINE)
    return dict(root=root, dof=dof, sim=dict(sim, substeps=1), terrain_kind=terrain_kind, nlim=nlim, ref=ref, ok=ok)


def describe(case):
    ref, ok = case["ref"], case["ok"]
    return (f"borderline {(~ok).sum()}/{ok.size} ({100 * (~ok).mean():.1f} %), cull survivors max "
            f"{ref['survivors'].max()}, candidates max {ref['candidates'].max()}, dropped max {ref['dropped'].max()}")


def oracle_contacts(case):
    """The oracle's kept slots [N, 64, 8] (point, normal, gap, key) and step outputs for a case."""
    _, hm, _ = models()
    n = case["root"].shape[0]
    sp = _abi.default_sim_params(**case["sim"])
    slots = np.zeros((n, O.CONTACT_OUT_SLOTS, 8))
    O.set_contact_out(slots)
    try:
        out = O.physics_step(hm, sp, case["root"].copy(), case["dof"].copy(), np.zeros((n, 69), np.float32), 1,
                             terrain_kind=case["terrain_kind"])
    finally:
        O.set_contact_out(None)
    return slots, out


def assert_reaches_crowded_paths(case):
    """Of the envs that are compared: at least 16 with more than 64 cull survivors (the pair cull's
    second compaction pass), at least 8 with more than 64 candidates (the reduction's upper half), none
    past 127 candidates (under the pool)."""
    ref, ok = case["ref"], case["ok"]
    assert (ref["survivors"][ok] > 64).sum() >= 16
    assert (ref["candidates"][ok] > 64).sum() >= 8
    assert ref["candidates"].max() <= 127


def assert_borderline_share(case):
    assert (~case["ok"]).mean() <= 0.05, describe(case)


@functools.lru_cache(None)
def crowded(cap, limits=False):
    """256 folded envs: the second compaction pass of the pair cull (more than 64 survivors), the upper
    half of the reduction (more than 64 candidates), under the candidate pool."""
    rng = np.random.default_rng(11 if limits else 5)
    root, dof = folded_state(256, rng, angle=(1.5, 3.1) if limits else (1.5, 3.0))
    return finish(root, dof, joint_limits=int(limits), max_contacts=cap)


@functools.lru_cache(None)
def past_pool():
    """32 envs with 129-160 candidates, the root at 0-0.15 m: the pool's cap itself."""
    _, _, M = models()
    rng = np.random.default_rng(4)
    # joints folded almost fully: about 1.5 % of these poses pass 128 candidates
    root, dof = folded_state(3072, rng, angle=(3.05, 3.14), height=(0.0, 0.15))
    cnt = CR.generate(M, root, dof[..., 0], count_only=True)["candidates"]
    pick = np.flatnonzero((cnt >= 129) & (cnt <= 160))[:32]
    assert pick.size == 32, f"{pick.size} envs with 129-160 candidates"
    return finish(root[pick].copy(), dof[pick].copy(), joint_limits=0)


@functools.lru_cache(None)
def ordinary():
    """64 standing, lying and random poses (the suite's easy regime)."""
    model = models()[0]
    rng = np.random.default_rng(21)
    r0, d0 = cases.standing_state(model, 16, rng, xy_jitter=1.0)
    d0[..., 0] = rng.uniform(-0.1, 0.1, (16, 69))
    r1, d1 = cases.lying_state(24, rng, on_floor=True, model=model)
    r2, d2 = cases.random_state(24, rng, height=(0.2, 0.9), ang=0.8, vel=0.0, tilt=1.5)
    root, dof = np.concatenate([r0, r1, r2]), np.concatenate([d0, d1, d2])
    root[:, 7:] = 0
    return finish(root, dof, joint_limits=0)


def _settle(root, dof, terrain_kind, lift, **sim):
    """Move each root along z so that its lowest terrain point's gap becomes lift [N] (the slope turns
    a z shift by cos s: iterated)."""
    _, _, M = models()
    sp = _abi.default_sim_params(**sim)
    for _ in range(3):
        ref = CR.generate(M, root, dof[..., 0], terrain_kind=terrain_kind, terrain_slope=sp.terrain_slope,
                          step_height=sp.step_height, step_length=sp.step_length, count_only=True)
        low = ref["point_gap"].min(1)
        c = np.where(np.asarray(terrain_kind) == 1, np.cos(sp.terrain_slope), 1.0)
        root[:, 2] = (root[:, 2].astype(np.float64) + (lift - low) / c).astype(np.float32)
    return root


def _poses(n, rng):
    """Upright, lying and head-down bodies in turn, joints within +-0.3 rad."""
    root = np.zeros((n, 13), np.float32)
    root[:, 6] = 1.0
    th = np.array([0.0, np.pi / 2, np.pi])[np.arange(n) % 3] + rng.uniform(-0.2, 0.2, n)
    root[:, 3], root[:, 6] = np.sin(th / 2), np.cos(th / 2)
    root[:, 2] = 1.0
    dof = np.zeros((n, 69, 2), np.float32)
    dof[..., 0] = rng.uniform(-0.3, 0.3, (n, 69))
    return root, dof


@functools.lru_cache(None)
def terrain_kinds():
    """96 envs over plane, slope and steps, roots at x in [-1, 2]: bodies before the first step, on one
    step and across an edge, resting up to 15 mm deep or up to 10 mm above."""
    rng = np.random.default_rng(8)
    n = 96
    root, dof = _poses(n, rng)
    root[:, 0] = rng.uniform(-1, 2, n)
    root[:, 1] = rng.uniform(-1, 1, n)
    tk = ((np.arange(n) // 3) % 3).astype(np.int32)
    root = _settle(root, dof, tk, rng.uniform(-0.015, 0.01, n), terrain=1)
    return finish(root, dof, terrain_kind=tk, joint_limits=0, terrain=1)


THRESHOLD_DELTA = 1e-4


@functools.lru_cache(None)
def threshold():
    """Upright, lying and head-down bodies on each terrain kind, lifted until the lowest terrain point's
    gap is the contact offset -1e-4 m (even envs) or +1e-4 m (odd envs)."""
    rng = np.random.default_rng(13)
    n = 36
    root, dof = _poses(n // 2, rng)
    root[:, 0] = rng.uniform(-1, 2, n // 2)
    root, dof = np.repeat(root, 2, 0), np.repeat(dof, 2, 0)
    tk = ((np.arange(n) // 6) % 3).astype(np.int32)
    off = _abi.default_sim_params().contact_offset
    sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    root = _settle(root, dof, tk, off + sign * THRESHOLD_DELTA, terrain=1)
    case = finish(root, dof, terrain_kind=tk, joint_limits=0, terrain=1)
    case["above"] = sign > 0
    return case


@functools.lru_cache(None)
def force_direction():
    """128 bodies with joints bent 0.5-2 rad resting 3 mm deep on the plane (even envs) and the slope
    (odd envs), friction 0: a body touched by one contact only feels a force along its normal."""
    rng = np.random.default_rng(31)
    n = 128
    root, dof = folded_state(n, rng, angle=(0.5, 2.0), height=(1.0, 1.0))
    tk = (np.arange(n) % 2).astype(np.int32)
    root = _settle(root, dof, tk, np.full(n, -0.003), terrain=1)
    return finish(root, dof, terrain_kind=tk, joint_limits=0, terrain=1, friction=0.0)


MIN_SEPARATION = 0.02  # m between a pair's closest points: fp32 positions then turn its normal by ~1e-5 rad
FORCE_ANGLE = 1e-4     # rad


def single_contact_bodies(case):
    """(env, body, slot, sign) of every body of a compared env whose only kept contact is one terrain
    point or one self pair (closest points at least MIN_SEPARATION apart): the force on it is along
    sign x the slot's normal, + on a terrain point's body and a pair's first body, - on the partner."""
    ref = case["ref"]
    out = []
    for e in np.flatnonzero(case["ok"]):
        on = np.flatnonzero(ref["key"][e] >= 0)
        touched = np.bincount(np.concatenate([ref["b0"][e, on], ref["b1"][e, on][ref["b1"][e, on] >= 0]]), minlength=24)
        for s in on:
            b0, b1 = int(ref["b0"][e, s]), int(ref["b1"][e, s])
            if b1 >= 0 and ref["sep"][e, s] < MIN_SEPARATION:
                continue
            if touched[b0] == 1:
                out.append((e, b0, s, 1.0))
            if b1 >= 0 and touched[b1] == 1:
                out.append((e, b1, s, -1.0))
    return out


def assert_forces_along_normals(case, forces):
    """contact_forces [N,24,3] of one step against the reference normals: within FORCE_ANGLE on every
    single-contact body with a nonzero force; at least 20 of them, and every class of a segment pair's
    minimiser (interior, edge, corner) beside the terrain points, must occur."""
    ref = case["ref"]
    f = np.asarray(forces, np.float64)
    seen, worst, count = set(), 0.0, 0
    for e, b, s, sign in single_contact_bodies(case):
        if np.linalg.norm(f[e, b]) < 1e-3:  # N: a speculative contact that carries nothing
            continue
        n = sign * ref["n"][e, s]
        angle = np.arctan2(np.linalg.norm(np.cross(f[e, b], n)), f[e, b] @ n)
        assert angle <= FORCE_ANGLE, f"env {e} body {b}: force {f[e, b]} is {angle:.2e} rad off the normal {n}"
        worst, count = max(worst, angle), count + 1
        seen.add(int(ref["cls"][e, s]))
    print(f"{count} single-contact bodies with a force, largest angle {worst:.2e} rad, classes {sorted(seen)}")
    assert count >= 20 and seen == {-1, CR.INTERIOR, CR.EDGE, CR.CORNER}, (count, seen)
