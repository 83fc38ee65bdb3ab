"""GPU checks of the joint-reaction queries (include/humanoid_wrench.h) against the float64 numpy reference
of tests/reaction_reference.py, which tests/test_reaction.py pins (the header's identities, computed
torque, the rest case, a finite difference of the bodies' velocities). The five states are those of
tests/test_gpu_dynamics.py's `ctx`: env 0 as created, 1-3 random tumbling, 4 all-zero dof angles with nonzero
rates. Inputs: qdd_des in +-20, base accelerations in +-10, forces in +-200 N and torques in +-20 N m on every
body.

Tolerance per output: 8 x that output's own float32 floor (MARGIN of tests/test_gpu_dynamics.py). The figure
is the normwise error per env, max|x - x64| / max|x64|, the largest over the five envs; the floor is the
same figure of reaction_reference evaluated in float32 on the same inputs. It is computed and printed here
and never taken from the kernel. With a free base the root's wrench is exactly zero: it is held relative to
the root's wrench at a_b = 0, against the same figure of the float32 reference.

Floors and the kernel's measured figures (MI355X; world frame, armature and gravity on):

    case                         output     float32 floor  tolerance (8 x)  kernel
    prescribed base, no wrench   wrench     1.19e-07       9.54e-07         4.46e-07
                                 tau        2.74e-07       2.20e-06         1.07e-07
                                 body_acc   2.56e-07       2.05e-06         1.90e-07
    prescribed base, f and t     wrench     2.88e-07       2.31e-06         3.19e-07
                                 tau        5.64e-07       4.51e-06         2.24e-07
    free base, no wrench         wrench     3.31e-06       2.65e-05         1.87e-06
                                 tau        6.02e-07       4.81e-06         5.85e-07
                                 base_acc   5.15e-07       4.12e-06         2.54e-07
                                 body_acc   3.17e-07       2.54e-06         2.92e-07
    free base, f and t           wrench     1.21e-06       9.68e-06         5.45e-07
                                 tau        5.30e-07       4.24e-06         3.88e-07
                                 base_acc   6.12e-07       4.90e-06         4.99e-07
                                 body_acc   4.02e-07       3.21e-06         4.34e-07
    free base, root wrench over the root wrench at a_b = 0 (no wrench / f and t)
                                            2.48e-07       1.98e-06         6.87e-08
                                            3.84e-07       3.07e-06         1.14e-07

base_acc with a prescribed base is the input's bits (floor and figure 0). The body frame's figures are within
15 % of the world frame's. Free base with f and t against Solver.computed_torque with gen_force = J^T (f, t):
tau 3.62e-07 of max|tau| (the two floors sum to 8.34e-07), base_acc 7.30e-07 (1.11e-06); with no external
wrench the two are bit-equal. With the root 1 km away every output has the bits of the near call.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import reaction_reference as RR  # noqa: E402
import solve_reference as SR  # noqa: E402
from test_gpu_dynamics import MARGIN, N, ctx  # noqa: E402,F401  (the five states, one engine, one Dynamics)

pytestmark = pytest.mark.gpu
NB, ND, NG = DR.NB, DR.ND, DR.NG
SENTINEL = 12345.0
OUTPUTS = ("wrench", "tau", "base_acc", "body_acc")


def cu(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _held(name, fig, floor):
    print(f"{name}: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    assert np.isfinite(fig) and fig <= MARGIN * floor, (name, fig, MARGIN * floor)


@pytest.fixture(scope="module")
def rx(ctx, he_model):  # noqa: F811
    """A Reaction on ctx's engine, the module's inputs, and a cache of the reference per case in both dtypes
    (computed once per case, left unchanged)."""
    from humanoid_amd import reaction

    class S:
        pass

    s = S()
    s.mod = reaction
    s.rx = reaction.Reaction(ctx.eng)
    rng = np.random.default_rng(29)
    s.qdd_des = rng.uniform(-20.0, 20.0, (N, ND)).astype(np.float32)
    s.base_acc = rng.uniform(-10.0, 10.0, (N, 6)).astype(np.float32)
    s.f = rng.uniform(-200.0, 200.0, (N * NB, 3)).astype(np.float32)
    s.t = rng.uniform(-20.0, 20.0, (N * NB, 3)).astype(np.float32)
    cache = {}

    def ref(prescribed, external, frame="world", armature=True, gravity=True, base_acc=None):
        key = (prescribed, external, frame, armature, gravity, base_acc is not None)
        if key not in cache:
            ab = (s.base_acc if base_acc is None else base_acc) if prescribed else None
            f, t = (s.f, s.t) if external else (None, None)
            cache[key] = tuple(RR.evaluate(he_model, ctx.root, ctx.dof, ctx.g, s.qdd_des, ab, f, t,
                                           reaction.FRAMES[frame], dt, armature, not gravity)
                               for dt in (np.float64, np.float32))
        return cache[key]

    def run(prescribed, external, frame="world", armature=True, gravity=True, want=OUTPUTS, **kw):
        s.rx.armature, s.rx.gravity = armature, gravity
        try:
            out = s.rx.compute(cu(s.qdd_des), cu(s.base_acc) if prescribed else None, cu(s.f) if external else None,
                               cu(s.t) if external else None, frame, wrench="wrench" in want, tau="tau" in want,
                               base_acc_out="base_acc" in want, body_acc="body_acc" in want, **kw)
        finally:
            s.rx.armature, s.rx.gravity = True, True
        return {k: host(v) for k, v in out.items()}

    s.ref, s.run = ref, run
    yield s
    del s.rx


# ------------------------------------------------------------------ every output against the reference
@pytest.mark.parametrize("frame", ["world", "body"])
@pytest.mark.parametrize("external", [False, True], ids=["noext", "ext"])
@pytest.mark.parametrize("prescribed", [True, False], ids=["prescribed", "free"])
def test_outputs_match_the_float64_reference(ctx, rx, prescribed, external, frame):  # noqa: F811
    """wrench, tau, base_acc and body_acc for a prescribed and a free base, without and with an external
    force and torque on every body, in both frames, armature on and off, gravity on and off."""
    shapes = rx.mod.output_shapes(N)
    for armature in (True, False):
        for gravity in (True, False):
            x64, x32 = rx.ref(prescribed, external, frame, armature, gravity)
            got = rx.run(prescribed, external, frame, armature, gravity)
            tag = (f"{'prescribed' if prescribed else 'free'} {'ext' if external else 'noext'} {frame} "
                   f"armature={armature} gravity={gravity}")
            for name in OUTPUTS:
                assert got[name].shape == shapes[name] and got[name].dtype == np.float32
                _held(f"{tag}, {name}", RR.error(got[name], x64[name]).max(), RR.error(x32[name], x64[name]).max())
            if prescribed:
                assert np.array_equal(got["base_acc"], rx.base_acc)  # a copy of the input


@pytest.mark.parametrize("external", [False, True], ids=["noext", "ext"])
def test_free_base_root_wrench_is_the_solves_residual(ctx, rx, he_model, external):  # noqa: F811
    """With a free base nothing acts on the root: its wrench, exactly zero, is the 6 x 6 solve's rounding
    residual. Relative to the root's wrench at a_b = 0 (what the solve cancels), per env, against the same
    figure of the float32 reference."""
    zero = np.zeros((N, 6), np.float32)
    at0, _ = rx.ref(True, external, base_acc=zero)
    scale = np.abs(at0["wrench"][:, 0]).max(axis=1)
    _, x32 = rx.ref(False, external)
    got = rx.run(False, external, want=("wrench",))["wrench"]
    fig = (np.abs(got[:, 0]).max(axis=1) / scale).max()
    floor = (np.abs(x32["wrench"][:, 0]).max(axis=1) / scale).max()
    _held(f"free base {'ext' if external else 'noext'}, root wrench / root wrench at a_b = 0", fig, floor)


# ------------------------------------------------------------------ agreement with the existing entry points
def test_free_base_agrees_with_computed_torque(ctx, rx, he_model):  # noqa: F811
    """Free base: tau and base_acc against Solver.computed_torque with gen_force = J^T (f, t) built from
    Dynamics' Jacobian (the force at the centre of mass: its moment about the origin joins the torque). Both
    are float32 computations of the same numbers, each held to 8 x its floor against float64, so they differ
    by no more than the sum of the two tolerances. With no external wrench the two take the same
    instructions: bit-equal."""
    from humanoid_amd import solve
    solver = solve.Solver(ctx.eng)
    q = cu(rx.qdd_des)
    tau_s, ab_s = solver.computed_torque(q)
    got = rx.run(False, False, want=("tau", "base_acc"))
    assert np.array_equal(got["tau"], host(tau_s)) and np.array_equal(got["base_acc"], host(ab_s))

    Mo = DR.Model(he_model, np.float64)
    J = ctx.J.astype(np.float64)
    f, t = rx.f.reshape(N, NB, 3).astype(np.float64), rx.t.reshape(N, NB, 3).astype(np.float64)
    G = np.zeros((N, NG))
    for e in range(N):
        R, _ = DR.fk(Mo, ctx.root[e], ctx.dof[e])
        for b in range(NB):
            G[e] += J[e, b, 0:3].T @ f[e, b] + J[e, b, 3:6].T @ (t[e, b] + np.cross(R[b] @ Mo.com[b], f[e, b]))
    G32 = G.astype(np.float32)
    tau_s, ab_s = (host(x) for x in solver.computed_torque(q, cu(G32)))
    got = rx.run(False, True, want=("tau", "base_acc"))
    x64, x32 = rx.ref(False, True)
    (M64, c64), (M32, c32) = (SR.terms(he_model, ctx.root, ctx.dof, ctx.g, dt) for dt in (np.float64, np.float32))
    tau64, ab64 = SR.computed_torque(M64, c64, rx.qdd_des, G32)
    tau32, ab32 = SR.computed_torque(M32, c32, rx.qdd_des, G32)
    for name, a, b, r64, fl_s in (("tau", got["tau"], tau_s, x64["tau"], SR.forward_error(tau32, tau64).max()),
                                  ("base_acc", got["base_acc"], ab_s, x64["base_acc"], SR.forward_error(ab32, ab64).max())):
        floor = RR.error(x32[name], x64[name]).max() + fl_s
        d = (np.abs(a.astype(np.float64) - b).max(axis=1) / np.abs(r64).max(axis=1)).max()
        _held(f"free base ext, {name} against Solver.computed_torque (sum of the two floors)", d, floor)
    del solver


# ------------------------------------------------------------------ a far-away env
def test_a_root_one_kilometre_away_changes_nothing(ctx, rx):  # noqa: F811
    """No output depends on where the root stands, and the kernel forms every lever relative to the root
    origin: with the root moved 1 km, every output stays within its floor of the same reference."""
    root = ctx.root.copy()
    root[:, 0] += 1000.0
    root[:, 1] -= 1000.0
    near = rx.run(True, True)
    far = rx.run(True, True, root_state=cu(root))
    x64, x32 = rx.ref(True, True)
    for name in OUTPUTS:
        _held(f"1 km away, {name}", RR.error(far[name], x64[name]).max(), RR.error(x32[name], x64[name]).max())
        print(f"  {name}: bit-equal to the near call: {np.array_equal(far[name], near[name])}")


# ------------------------------------------------------------------ what is written
@pytest.mark.parametrize("prescribed", [True, False], ids=["prescribed", "free"])
def test_outputs_alone_and_together_and_nothing_else_written(ctx, rx, prescribed):  # noqa: F811
    """An output's bits are the same alone and with the other three; an output not asked for is not written;
    inputs and the engine's state are never written."""
    shapes = rx.mod.output_shapes(N)
    inputs = dict(qdd=cu(rx.qdd_des), acc=cu(rx.base_acc), f=cu(rx.f), t=cu(rx.t))
    before = {k: host(v) for k, v in inputs.items()}
    state = host(ctx.eng.root_states), host(ctx.eng.dof_state)

    def call(names):
        outs = {k: torch.full(shapes[k], SENTINEL, dtype=torch.float32, device="cuda:0") for k in OUTPUTS}
        rx.rx.compute(inputs["qdd"], inputs["acc"] if prescribed else None, inputs["f"], inputs["t"], "body",
                      wrench=False, out={k: outs[k] for k in names})
        return {k: host(v) for k, v in outs.items()}

    together = call(OUTPUTS)
    for k in OUTPUTS:
        assert not (together[k] == SENTINEL).any(), k
        alone = call((k,))
        assert np.array_equal(alone[k], together[k]), k
        for other in OUTPUTS:
            if other != k:
                assert (alone[other] == SENTINEL).all(), (k, other)
    # this object's own storage of an output that is not asked for stays as it was
    rx.rx.compute(inputs["qdd"], tau=True)
    rx.rx._tau.fill_(SENTINEL)
    rx.rx.compute(inputs["qdd"])
    assert (host(rx.rx._tau) == SENTINEL).all()
    for k, v in inputs.items():
        assert np.array_equal(host(v), before[k]), k
    assert np.array_equal(host(ctx.eng.root_states), state[0]) and np.array_equal(host(ctx.eng.dof_state), state[1])


def test_dynamics_hands_over_one_reaction_and_the_facade_uses_it(ctx, rx):  # noqa: F811
    """Dynamics.reaction is made once with the object's settings, and computes what a Reaction computes."""
    r = ctx.dyn.reaction
    assert r is ctx.dyn.reaction and isinstance(r, rx.mod.Reaction) and r.armature == ctx.dyn.armature
    got = host(r.compute(cu(rx.qdd_des), cu(rx.base_acc))["wrench"])
    assert np.array_equal(got, rx.run(True, False, want=("wrench",))["wrench"])
