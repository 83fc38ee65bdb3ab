"""GPU checks of the dynamics derivatives (include/humanoid_derivatives.h) against the float64 numpy reference
of tests/derivative_reference.py, which tests/test_derivatives.py pins to the definition (differences of tau
along q (+) delta). Six envs: env 0 as created (at rest), 1-5 the states 1-5 of
dynamics_reference.test_states (three tumbling, one with every dof angle exactly 0 and nonzero rates, one
with a joint near 2.5 rad); and one engine of a single env in the last of them. acc in +-20, and NULL.

Tolerance per output: 8 x that output's own float32 floor (MARGIN of tests/test_gpu_dynamics.py, DESIGN
§4.9). The figure is the normwise error per env, max|x - x64| / max|x64|, the largest over the envs; the
floor is the same figure of derivative_reference evaluated in float32 on the same inputs. It is computed and
printed here and never taken from the kernel.

Floors and the kernel's measured figures are in DESIGN.md §4.14.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import derivative_reference as GR  # noqa: E402
import dynamics_reference as DR  # noqa: E402
import solve_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu
NB, ND, NG = DR.NB, DR.ND, DR.NG
N = 6
MARGIN = 8.0
SENTINEL = 12345.0
OUTPUTS = ("dtau_dq", "dtau_dv", "tau")
HI = slice(64, NG)  # the directions of the second lane pass


def cu(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _held(name, fig, floor):
    print(f"{name}: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    assert np.isfinite(fig) and fig <= MARGIN * floor, (name, fig, MARGIN * floor)


class _Ctx:
    pass


def _engine(model, root, dof, keep_first):
    """An engine in the given states (env 0 left as created when keep_first), and the states read back."""
    from humanoid_amd.engine import Engine
    n = root.shape[0]
    eng = Engine(model, n, device=0)
    first = 1 if keep_first else 0
    ids = torch.arange(first, n, dtype=torch.int32, device=eng.device)
    eng.set_root_state_indexed(cu(root), ids)
    eng.set_dof_state_indexed(cu(dof.reshape(n * ND, 2)), ids)
    torch.cuda.synchronize()
    r, d = host(eng.root_states), host(eng.dof_state).reshape(n, ND, 2)
    assert np.array_equal(r[first:], root[first:]) and np.array_equal(d[first:], dof[first:])
    return eng, r, d


@pytest.fixture(scope="module")
def dx(model, he_model):
    """One engine of six envs and one of a single env with a Derivatives each, the module's inputs, and a
    cache of the reference per case in both dtypes (computed once per case, left unchanged)."""
    from humanoid_amd import derivatives

    c = _Ctx()
    c.mod = derivatives
    root, dof = DR.test_states(he_model)
    assert root.shape[0] == N
    c.eng, c.root, c.dof = _engine(model, root, dof, keep_first=True)
    assert c.root[0, 6] == 1.0 and not c.dof[0].any()  # at rest
    c.eng1, c.root1, c.dof1 = _engine(model, root[5:6], dof[5:6], keep_first=False)
    c.g = tuple(c.eng.params.gravity)
    c.dv, c.dv1 = derivatives.Derivatives(c.eng), derivatives.Derivatives(c.eng1)
    rng = np.random.default_rng(37)
    c.acc = rng.uniform(-20.0, 20.0, (N, NG)).astype(np.float32)
    c.f = rng.uniform(-50.0, 50.0, (N, NG)).astype(np.float32)
    c.mask = DR.mass_mask(DR.Model(he_model).parents)
    cache = {}

    def ref(with_acc=True, armature=True, gravity=True):
        key = (with_acc, armature, gravity)
        if key not in cache:
            cache[key] = tuple(GR.exact(he_model, c.root, c.dof, c.acc if with_acc else None, c.g, dt, armature,
                                        not gravity) for dt in (np.float64, np.float32))
        return cache[key]

    def run(with_acc=True, armature=True, gravity=True, single=False, **kw):
        d = c.dv1 if single else c.dv
        acc = (c.acc[5:6] if single else c.acc) if with_acc else None
        d.armature, d.gravity = armature, gravity
        try:
            out = d.inverse_dynamics(cu(acc), tau=True, **kw)
        finally:
            d.armature, d.gravity = True, True
        return {k: host(v) for k, v in out.items()}

    c.ref, c.run = ref, run
    yield c
    del c.dv, c.dv1, c.eng, c.eng1


# ------------------------------------------------------------------ every output against the reference
@pytest.mark.parametrize("with_acc", [True, False], ids=["acc", "null"])
def test_outputs_match_the_float64_reference(dx, with_acc):
    """dtau_dq, dtau_dv and tau, armature on and off, gravity on and off, at N = 6 and the last state alone
    at N = 1; the directions of the second lane pass (64-74) on their own as well."""
    shapes = dx.mod.output_shapes(N)
    for armature in (True, False):
        for gravity in (True, False):
            x64, x32 = dx.ref(with_acc, armature, gravity)
            got = dx.run(with_acc, armature, gravity)
            one = dx.run(with_acc, armature, gravity, single=True)
            tag = f"{'acc' if with_acc else 'null'} armature={armature} gravity={gravity}"
            for name in OUTPUTS:
                assert got[name].shape == shapes[name] and got[name].dtype == np.float32
                floor = GR.error(x32[name], x64[name])
                _held(f"{tag}, {name}", GR.error(got[name], x64[name]).max(), floor.max())
                _held(f"{tag}, {name}, N = 1", GR.error(one[name], x64[name][5:6]).max(), floor[5])
            for name in ("dtau_dq", "dtau_dv"):
                _held(f"{tag}, {name}, directions 64-74", GR.error(got[name][:, :, HI], x64[name][:, :, HI]).max(),
                      GR.error(x32[name][:, :, HI], x64[name][:, :, HI]).max())


@pytest.mark.parametrize("armature", [True, False], ids=["armature", "bare"])
def test_forward_form_matches_the_float64_reference(dx, he_model, armature):
    """Derivatives.forward_dynamics: qdd, d qdd / d q, d qdd / d qd and M^-1 under a generalised force,
    against the reference's forward form in float64; the floor is its float32 path."""
    x64, x32 = (GR.forward(he_model, dx.root, dx.dof, dx.f, dx.g, dt, armature) for dt in (np.float64, np.float32))
    dx.dv.armature = armature
    try:
        got = {k: host(v) for k, v in dx.dv.forward_dynamics(cu(dx.f), dqdd_dtau=True).items()}
    finally:
        dx.dv.armature = True
    for name in ("qdd", "dqdd_dq", "dqdd_dv", "dqdd_dtau"):
        assert got[name].shape == x64[name].shape and got[name].dtype == np.float32
        _held(f"forward, armature={armature}, {name}", GR.error(got[name], x64[name]).max(),
              GR.error(x32[name], x64[name]).max())


# ------------------------------------------------------------------ the header's consequences
def test_exact_zeros_and_layouts(dx):
    """Exactly zero outside the pattern of M and in columns 0-2, under both layouts; the by-direction
    output is the bitwise transpose of the default."""
    for with_acc in (True, False):
        got = dx.run(with_acc)
        by = dx.run(with_acc, by_direction=True)
        for name in ("dtau_dq", "dtau_dv"):
            assert not got[name][:, ~dx.mask].any(), name
            assert not got[name][:, :, 0:3].any(), name
            assert np.array_equal(by[name].view(np.uint32), got[name].transpose(0, 2, 1).view(np.uint32)), name
            assert np.isfinite(got[name]).all()
        assert np.array_equal(by["tau"], got["tau"])
    assert np.abs(got["dtau_dq"][1:, :, 3:]).max(axis=(0, 1)).all()  # every other direction reaches some row


def test_velocity_derivative_ignores_acceleration_gravity_and_armature(dx):
    """dtau_dv's bits are the same under every acc and flag; dtau_dq ignores the armature, tau does not."""
    base = dx.run()
    for kw in (dict(with_acc=False), dict(gravity=False), dict(armature=False), dict(with_acc=False, gravity=False)):
        other = dx.run(**kw)
        assert np.array_equal(other["dtau_dv"].view(np.uint32), base["dtau_dv"].view(np.uint32)), kw
        assert not np.array_equal(other["tau"], base["tau"]), kw
    bare = dx.run(armature=False)
    assert np.array_equal(bare["dtau_dq"].view(np.uint32), base["dtau_dq"].view(np.uint32))


def test_tau_agrees_with_the_dynamics_tensors(dx, he_model):
    """tau against Dynamics.inverse_dynamics(acc) = M a + c from hd_compute's tensors: two float32
    computations of the same numbers, so they differ by no more than the sum of the two tolerances."""
    from humanoid_amd.dynamics import Dynamics
    dyn = Dynamics(dx.eng)
    dyn.refresh()
    tau_d = host(dyn.inverse_dynamics(cu(dx.acc)))
    x64, x32 = dx.ref()
    (_, M64, c64), (_, M32, c32) = (DR.evaluate(he_model, dx.root, dx.dof, dx.g, dt) for dt in (np.float64, np.float32))
    t64 = np.einsum("eij,ej->ei", M64, dx.acc.astype(np.float64)) + c64
    t32 = np.einsum("eij,ej->ei", M32, dx.acc) + c32
    floor = GR.error(x32["tau"], x64["tau"]).max() + SR.forward_error(t32, t64).max()
    got = dx.run()["tau"]
    fig = (np.abs(got.astype(np.float64) - tau_d).max(axis=1) / np.abs(x64["tau"]).max(axis=1)).max()
    _held("tau against Dynamics.inverse_dynamics (sum of the two floors)", fig, floor)
    del dyn


def test_velocity_derivative_gives_twice_the_bias_force(dx, he_model):
    """dtau_dv . qd = 2 c, c from hd_compute under the no-gravity flag: the product of the kernel's matrix
    with qd (in float64) against twice the dynamics kernel's bias force, within the sum of the two floors
    (the reference's float32 matrix times qd, and dynamics_reference's float32 c, each against float64)."""
    from humanoid_amd.dynamics import Dynamics
    dyn = Dynamics(dx.eng)
    dyn.gravity = False
    dyn.refresh(jacobian=False, mass_matrix=False)
    c_hd = host(dyn.bias).astype(np.float64)
    qd = np.stack([GR.split_state(dx.root[e], dx.dof[e])[3] for e in range(N)])
    x64, x32 = dx.ref()
    (_, _, c64), (_, _, c32) = (DR.evaluate(he_model, dx.root, dx.dof, dx.g, dt, no_gravity=True)
                                for dt in (np.float64, np.float32))
    prod = lambda dv: np.einsum("eij,ej->ei", dv.astype(np.float64), qd)  # noqa: E731
    moving = slice(1, N)  # env 0 is at rest: both sides are exactly zero there
    assert not prod(dx.run()["dtau_dv"])[0].any() and not c_hd[0].any()
    assert GR.error(prod(x64["dtau_dv"])[moving], 2 * c64[moving]).max() < 1e-12
    floor = GR.error(prod(x32["dtau_dv"])[moving], 2 * c64[moving]).max() + GR.error(c32[moving], c64[moving]).max()
    got = prod(dx.run()["dtau_dv"])
    fig = (np.abs(got - 2 * c_hd)[moving].max(axis=1) / np.abs(2 * c64[moving]).max(axis=1)).max()
    _held("dtau_dv . qd against 2 c of hd_compute (sum of the two floors)", fig, floor)
    del dyn


# ------------------------------------------------------------------ mechanics
def _buffers():
    shapes = {"dtau_dq": N * NG * NG, "dtau_dv": N * NG * NG, "tau": N * NG}
    bufs = {k: torch.full((n + NG,), SENTINEL, dtype=torch.float32, device="cuda:0") for k, n in shapes.items()}
    views = {"dtau_dq": bufs["dtau_dq"][:N * NG * NG].view(N, NG, NG), "dtau_dv": bufs["dtau_dv"][:N * NG * NG].view(N, NG, NG),
             "tau": bufs["tau"][:N * NG].view(N, NG)}
    return shapes, bufs, views


def test_second_call_outputs_alone_and_sentinels(dx):
    """Unchanged state, same bits; an output's bits are the same alone and with the others; an output not
    asked for is not written; nothing is written past the last env of any output; inputs and the engine's
    state are never written."""
    acc = cu(dx.acc)
    state = host(dx.eng.root_states), host(dx.eng.dof_state)
    first = dx.run()
    shapes, bufs, views = _buffers()
    dx.dv.inverse_dynamics(acc, dtau_dq=False, dtau_dv=False, out=views)
    for k in OUTPUTS:
        h = host(bufs[k])
        assert np.array_equal(h[:shapes[k]].reshape(first[k].shape), first[k]), k
        assert (h[shapes[k]:] == SENTINEL).all() and not (h[:shapes[k]] == SENTINEL).any(), k
    for k in OUTPUTS:
        shapes, bufs, views = _buffers()
        dx.dv.inverse_dynamics(acc, dtau_dq=False, dtau_dv=False, out={k: views[k]})
        for other in OUTPUTS:
            h = host(bufs[other])
            if other == k:
                assert np.array_equal(h[:shapes[k]].reshape(first[k].shape), first[k]), k
                assert (h[shapes[k]:] == SENTINEL).all()
            else:
                assert (h == SENTINEL).all(), (k, other)
    assert np.array_equal(host(acc), dx.acc)
    assert np.array_equal(host(dx.eng.root_states), state[0]) and np.array_equal(host(dx.eng.dof_state), state[1])


def test_launch_on_a_side_stream(dx):
    want = dx.run()
    acc = cu(dx.acc)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert dx.dv.engine.stream.value == side.cuda_stream
        out = dx.dv.inverse_dynamics(acc, tau=True, out={k: torch.empty_like(cu(want[k])) for k in OUTPUTS})
    side.synchronize()
    for k in OUTPUTS:
        assert np.array_equal(host(out[k]), want[k]), k


def test_refusals_leave_the_outputs_unchanged(dx):
    d, E = dx.dv, dx.mod.DerivativesError
    dev = dx.eng.device
    acc = cu(dx.acc)
    out = {"dtau_dq": torch.full((N, NG, NG), SENTINEL, device=dev), "dtau_dv": torch.full((N, NG, NG), SENTINEL, device=dev),
           "tau": torch.full((N, NG), SENTINEL, device=dev)}
    with pytest.raises(E, match="acc"):
        d.inverse_dynamics(torch.zeros(N, ND, device=dev), out=out)  # shape
    with pytest.raises(E, match="acc"):
        d.inverse_dynamics(torch.zeros(N, NG, dtype=torch.float64, device=dev), out=out)  # dtype
    with pytest.raises(E, match="acc"):
        d.inverse_dynamics(torch.zeros(N, NG), out=out)  # device
    with pytest.raises(E, match="acc"):
        d.inverse_dynamics(torch.zeros(NG, N, device=dev).t(), out=out)  # contiguity
    with pytest.raises(E, match="dtau_dq"):
        d.inverse_dynamics(acc, out=dict(out, dtau_dq=torch.zeros(N, NG, NG)))
    with pytest.raises(E, match="unknown flag"):
        d.inverse_dynamics(acc, out=out, flags=8)
    with pytest.raises(E, match="also an input"):
        d.inverse_dynamics(acc, dtau_dq=False, dtau_dv=False, out={"tau": acc})
    with pytest.raises(E, match="root_state"):
        d.inverse_dynamics(acc, out=out, root_state=torch.zeros(N, 12, device=dev))
    # the library's own checks, below the binding's
    o = dx.mod.HgOutputs(tau=acc.data_ptr())
    ptrs = (dx.eng.root_states.data_ptr(), dx.eng.dof_state.data_ptr(), acc.data_ptr())
    import ctypes as C
    assert d.lib.hg_compute(d.h, *ptrs, C.byref(o), 1, None) != 0 and "also an input" in d.lib.hg_last_error().decode()
    o = dx.mod.HgOutputs(dtau_dq=out["dtau_dq"].data_ptr(), dtau_dv=out["dtau_dq"].data_ptr())
    assert d.lib.hg_compute(d.h, *ptrs, C.byref(o), 1, None) != 0 and "same buffer" in d.lib.hg_last_error().decode()
    o = dx.mod.HgOutputs()
    assert d.lib.hg_compute(d.h, *ptrs, C.byref(o), 1, None) != 0 and "no output buffer" in d.lib.hg_last_error().decode()
    torch.cuda.synchronize()
    for t in out.values():
        assert (t == SENTINEL).all().item()
    assert np.array_equal(host(acc), dx.acc)


# ------------------------------------------------------------------ Dynamics and the gym facade
def test_dynamics_hands_over_one_derivatives(dx):
    from humanoid_amd.dynamics import Dynamics
    dyn = Dynamics(dx.eng)
    d = dyn.derivatives
    assert d is dyn.derivatives and isinstance(d, dx.mod.Derivatives) and d.armature == dyn.armature
    got = d.inverse_dynamics(cu(dx.acc), tau=True)
    want = dx.run()
    for k in OUTPUTS:
        assert np.array_equal(host(got[k]), want[k]), k
    del dyn


def test_facade_entries_see_the_pending_simulate_calls():
    """Two gym.simulate calls and no fetch_results: solve_dynamics_derivatives first issues them, so it sees
    the state after the steps, and both entries equal bit for bit a direct Derivatives on a second sim's
    engine stepped the same way."""
    from humanoid_amd.derivatives import Derivatives
    from humanoid_amd.isaacgym import gymtorch
    from test_facade_env import _facade_sim
    n = 4
    gym, sim = _facade_sim(n)
    gym2, sim2 = _facade_sim(n)
    dev = sim.engine.device
    w = gymtorch.unwrap_tensor
    acc = torch.full((n, NG), 3.0, device=dev)
    dq, dv, tau = torch.zeros(n, NG, NG, device=dev), torch.zeros(n, NG, NG, device=dev), torch.zeros(n, NG, device=dev)
    gym.solve_dynamics_derivatives(sim, w(acc), w(dq), w(dv), w(tau))
    before = host(dq)
    for g, s in ((gym, sim), (gym2, sim2)):
        g.simulate(s)
        g.simulate(s)
    assert sim.pending_substeps == 2
    gym.solve_dynamics_derivatives(sim, w(acc), w(dq), w(dv), w(tau))
    assert sim.pending_substeps == 0
    gym2.fetch_results(sim2, True)
    assert torch.equal(sim.engine.dof_state, sim2.engine.dof_state)
    direct = Derivatives(sim2.engine)
    want = direct.inverse_dynamics(acc, tau=True)
    assert torch.equal(dq, want["dtau_dq"]) and torch.equal(dv, want["dtau_dv"]) and torch.equal(tau, want["tau"])
    assert not np.array_equal(host(dq), before) and dq.abs().max().item() > 1.0
    by = torch.zeros(n, NG, NG, device=dev)
    gym.solve_dynamics_derivatives(sim, w(acc), w(by), by_direction=True)
    assert torch.equal(by, dq.transpose(1, 2))
    f = torch.full((n, NG), 2.0, device=dev)
    qdd, a, b, minv = (torch.zeros(n, NG, device=dev), torch.zeros(n, NG, NG, device=dev),
                       torch.zeros(n, NG, NG, device=dev), torch.zeros(n, NG, NG, device=dev))
    gym.solve_forward_dynamics_derivatives(sim, w(f), w(qdd), w(a), w(b), w(minv))
    want = direct.forward_dynamics(f, dqdd_dtau=True)
    for got, name in ((qdd, "qdd"), (a, "dqdd_dq"), (b, "dqdd_dv"), (minv, "dqdd_dtau")):
        assert torch.equal(got, want[name]) and got.abs().max().item() > 0, name
    torch.cuda.synchronize()
