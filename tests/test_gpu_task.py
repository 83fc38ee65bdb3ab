"""GPU checks of task-space control (include/humanoid_task.h) against the float64 numpy reference of
tests/task_reference.py, which tests/test_task.py pins (Jdot qd by finite differences, the task equation,
the two modes' defining properties). The five states are those of tests/test_gpu_dynamics.py's `ctx`: env 0
as created and at rest, 1-3 random tumbling, 4 all-zero dof angles with nonzero rates. The six row sets are
task_reference.row_sets: k = 1, 6, 12 (offset points), 30, 31, 32, every one with R_Hand's rows, whose own
columns 72..74 are in the kernel's 11-column register tail.

Tolerance per figure: 8 x that figure's own float32 floor (MARGIN of tests/test_gpu_dynamics.py). The
floor is task_reference evaluated in float32 against float64 on the same states, rows and inputs, the
largest over the envs; it is computed and printed here and never taken from the kernel. The figure of an
output is its forward error max|x - x64| / max|x64| per env, the largest over the envs. The unforced
free acceleration of env 0, which is at rest, is in exact arithmetic J (g, 0), zero in most rows: there the
scale is |g|. cond(A64) < 1e6 is asserted first, so that no comparison is against a singular system.

Floors and the kernel's measured figures on the five states (MI355X; floor / kernel; default flags, with
the joint force where the output depends on it):

    k           jac              jminv            lambda_inv       bias_acc         free_acc
    1           3.4e-7 / 9.8e-8  1.9e-6 / 1.8e-6  8.8e-7 / 3.1e-7  9.9e-6 / 1.7e-6  2.9e-6 / 2.6e-6
    6           3.6e-7 / 2.5e-7  4.2e-7 / 5.8e-7  2.2e-7 / 2.0e-7  6.4e-7 / 2.9e-7  4.2e-7 / 1.2e-6
    12          3.6e-7 / 1.8e-7  1.1e-6 / 1.2e-6  6.2e-7 / 4.3e-7  6.3e-7 / 2.9e-7  1.1e-6 / 1.6e-6
    30, 31, 32  3.4e-7 / 2.5e-7  4.2e-7 / 7.9e-7  2.2e-7 / 2.9e-7  3.8e-7 / 3.8e-7  3.6e-7 / 9.5e-7

    k   mode   cond(A64)  F                u                qdd              residual of J qdd + b = xdd_des
    1   force  1.0        2.6e-6 / 2.3e-6  2.6e-6 / 2.3e-6  2.0e-5 / 1.5e-5  1.9e-4 / 7.9e-5
    1   joint  1.0        2.7e-6 / 2.3e-6  2.6e-6 / 2.8e-6  2.0e-5 / 1.5e-5  2.1e-4 / 1.2e-4
    6   force  3.5e3      6.2e-6 / 1.8e-6  6.2e-6 / 1.8e-6  2.0e-5 / 1.5e-5  4.7e-4 / 4.1e-4
    6   joint  1.1e4      4.1e-6 / 2.3e-6  2.7e-6 / 3.1e-6  2.0e-5 / 1.7e-5  2.0e-4 / 4.3e-4
    12  force  1.5e1      1.3e-6 / 1.3e-6  2.7e-6 / 3.2e-6  2.0e-5 / 1.6e-5  2.0e-4 / 8.9e-5
    12  joint  3.9e1      4.3e-6 / 9.1e-6  3.0e-6 / 3.8e-6  1.9e-5 / 1.5e-5  1.6e-4 / 1.2e-4
    30  force  9.2e3      6.6e-6 / 1.2e-5  8.3e-6 / 1.2e-5  2.0e-5 / 1.6e-5  3.6e-4 / 6.4e-4
    30  joint  2.8e5      1.1e-5 / 1.7e-5  1.0e-5 / 1.1e-5  1.4e-5 / 1.8e-5  3.1e-4 / 4.4e-4
    31  force  9.2e3      6.9e-6 / 2.4e-5  1.4e-5 / 4.0e-5  2.0e-5 / 1.6e-5  4.6e-4 / 5.6e-4
    31  joint  2.8e5      3.5e-5 / 5.4e-5  1.3e-5 / 1.5e-5  1.5e-5 / 1.4e-5  3.5e-4 / 5.4e-4
    32  force  1.1e4      7.2e-6 / 3.1e-5  9.4e-6 / 3.8e-5  2.0e-5 / 1.5e-5  5.7e-4 / 5.2e-4
    32  joint  3.2e5      1.0e-5 / 1.2e-5  9.2e-6 / 3.0e-5  1.1e-5 / 1.1e-5  5.3e-4 / 7.7e-4

(lambda = 0, forced.) Over all 340 asserted figures the kernel's worst is 0.56 of its tolerance: qdd at
k = 32, force mode, no force, 1.6e-5 against a floor of 3.5e-6. Round trip through hs_forward_dynamics:
4.1e-4 ... 6.4e-4 of max|xdd_des| against the float32 reference's own 2.0e-4 ... 4.7e-4. The module runs in
4 s.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import solve_reference as SR  # noqa: E402
import task_reference as TR  # noqa: E402
from test_gpu_dynamics import MARGIN, N, ctx  # noqa: E402,F401  (the five states, one engine, one Dynamics)

from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
NB, ND, NG = DR.NB, DR.ND, DR.NG
SENTINEL = 12345.0
KS = (1, 6, 12, 30, 31, 32)
FLAGS = [(True, True), (True, False), (False, True), (False, False)]  # (armature, gravity)


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _held(name, fig, floor):
    print(f"{name}: floor {floor:.3e}  tolerance {MARGIN * floor:.3e}  kernel {fig:.3e}")
    assert np.isfinite(fig) and fig <= MARGIN * floor, (name, fig, MARGIN * floor)


def _fe(x, x64, envs=slice(None)):
    return SR.forward_error(np.asarray(x)[envs], x64[envs]).max()


@pytest.fixture(scope="module")
def tk(ctx, he_model):  # noqa: F811
    """A TaskSpace on ctx's engine, the module's inputs, and a cache of the reference's terms per (row set,
    armature, gravity) in both dtypes (M and c formed once per setting; everything left unchanged)."""
    from humanoid_amd import task

    class T:
        pass

    t = T()
    t.task = task
    t.ts = task.TaskSpace(ctx.eng)
    t.sets = TR.row_sets(list(BODY_NAMES))
    rng = np.random.default_rng(29)
    t.f = np.concatenate([np.zeros((N, 6)), rng.uniform(-100.0, 100.0, (N, ND))], axis=1).astype(np.float32)
    t.xdd = {k: rng.uniform(-5.0, 5.0, (N, k)).astype(np.float32) for k in KS}
    bodies, terms = {}, {}

    def ref(k, armature=True, gravity=True):
        """(float64 terms, float32 terms) of row set k."""
        out = []
        for dt in (np.float64, np.float32):
            key = (dt, armature, gravity)
            if key not in bodies:
                bodies[key] = TR.body_terms(he_model, ctx.root, ctx.dof, ctx.g, dt, armature=armature, no_gravity=not gravity)
            if (k,) + key not in terms:
                terms[(k,) + key] = TR.evaluate(he_model, ctx.root, ctx.dof, t.sets[k], ctx.g, dt, bodies=bodies[key])
            out.append(terms[(k,) + key])
        return out

    t.ref = ref
    t.parents = np.array(he_model.parents[:NB])
    assert not ctx.root[0, 7:].any() and not ctx.dof[0].any()  # env 0 is at rest

    def run_terms(k, f=None, armature=True, gravity=True, **kw):
        t.ts.set_rows(t.sets[k])
        t.ts.armature, t.ts.gravity = armature, gravity
        try:
            return {name: host(v) for name, v in t.ts.terms(None if f is None else cu(f), **kw).items()}
        finally:
            t.ts.armature, t.ts.gravity = True, True

    def run_control(k, mode, damping=0.0, f=None, **kw):
        t.ts.set_rows(t.sets[k])
        return [None if v is None else host(v)
                for v in t.ts.control(cu(t.xdd[k]), None if f is None else cu(f), mode, damping, **kw)]

    t.terms, t.control = run_terms, run_control
    yield t
    del t.ts


# ------------------------------------------------------------------ T1: the terms
@pytest.mark.parametrize("k", KS)
def test_terms(ctx, tk, k):  # noqa: F811
    """jac, jminv, lambda_inv, bias_acc and free_acc against float64, forced and unforced, under the four flag
    combinations; the exact properties the header states."""
    rows = tk.sets[k]
    mask = TR.pattern(tk.parents, rows)
    gvec = np.zeros(NG)
    gvec[:3] = ctx.g
    for armature, gravity in FLAGS:
        t64, t32 = tk.ref(k, armature, gravity)
        tag = f"k={k} armature={armature} gravity={gravity}"
        for f in (None, tk.f):
            Y64, L64, free64 = TR.task_terms(t64, f)
            Y32, L32, free32 = TR.task_terms(t32, f)
            out = tk.terms(k, f, armature, gravity)
            assert {n: v.shape for n, v in out.items()} == {"jac": (N, k, NG), "jminv": (N, k, NG), "lambda_inv": (N, k, k),
                                                            "bias_acc": (N, k), "free_acc": (N, k)}
            if f is None:  # these three do not depend on the force
                _held(tag + " jac", _fe(out["jac"], t64.J), _fe(t32.J, t64.J))
                _held(tag + " jminv", _fe(out["jminv"], Y64), _fe(Y32, Y64))
                _held(tag + " lambda_inv", _fe(out["lambda_inv"], L64), _fe(L32, L64))
                _held(tag + " bias_acc", _fe(out["bias_acc"], t64.b), _fe(t32.b, t64.b))
                assert not (out["jac"][:, ~mask] != 0.0).any()  # exact zeros off the tree's pattern
                assert np.array_equal(out["lambda_inv"], out["lambda_inv"].transpose(0, 2, 1))  # exactly symmetric
                assert (np.linalg.eigvalsh(out["lambda_inv"].astype(np.float64)) > 0).all()
                assert not out["bias_acc"][0].any()  # env 0 is at rest
                # env 0, unforced: J (g, 0) with gravity, nothing without; the scale is |g|
                want0 = t64.J[0] @ gvec if gravity else np.zeros(k)
                gn = np.linalg.norm(ctx.g)
                _held(tag + " free_acc of the resting env / |g|", np.abs(out["free_acc"][0] - want0).max() / gn,
                      np.abs(free32[0] - want0).max() / gn)
                _held(tag + " free_acc unforced", _fe(out["free_acc"], free64, slice(1, None)),
                      _fe(free32, free64, slice(1, None)))
            else:
                _held(tag + " free_acc forced", _fe(out["free_acc"], free64), _fe(free32, free64))
    # zero-offset linear and angular rows against the dynamics kernel's own Jacobian rows, within J's tolerance
    out = tk.terms(k, want=("jac",))
    for r, (body, axis, point) in enumerate(rows):
        if not any(point):
            assert np.abs(out["jac"][:, r].astype(np.float64) - ctx.J[:, body, axis]).max() <= ctx.tol["J"]


# ------------------------------------------------------------------ T2: control
@pytest.mark.parametrize("mode", ["force", "joint"])
@pytest.mark.parametrize("k", KS)
def test_control(ctx, tk, k, mode):  # noqa: F811
    """F, u and qdd against float64 at lambda = 0 and at lambda = 1e-2 x the median diagonal of A64; at
    lambda = 0 the residual of the task equation with the float64 J and b; joint mode's base entries."""
    m = tk.task.MODES[mode]
    t64, t32 = tk.ref(k)
    Y64, L64, _ = TR.task_terms(t64)
    A64 = TR.system_matrix(t64, Y64, L64, m, 0.0)
    cond = max(np.linalg.cond(a) for a in A64)
    print(f"k={k} {mode}: cond(A64) {cond:.2e}")
    assert cond < 1e6
    lam = float(np.float32(1e-2 * np.median(np.diagonal(A64, axis1=1, axis2=2))))
    xdd = tk.xdd[k]
    for damping in (0.0, lam):
        for f in (None, tk.f):
            tag = f"k={k} {mode} lambda={damping:.3g} {'forced' if f is not None else 'free'}"
            u64, F64, q64 = TR.task_control(t64, xdd, f, m, damping)
            u32, F32, q32 = TR.task_control(t32, xdd, f, m, damping)
            u, F, q = tk.control(k, mode, damping, f)
            assert u.shape == (N, NG) and F.shape == (N, k) and q.shape == (N, NG)
            _held(tag + " F", _fe(F, F64), _fe(F32, F64))
            _held(tag + " u", _fe(u, u64), _fe(u32, u64))
            _held(tag + " qdd", _fe(q, q64), _fe(q32, q64))
            if mode == "joint":
                assert not u[:, :6].any()
            if damping == 0.0:
                scale = np.abs(xdd).max(axis=1)
                fig = (np.abs(TR.task_acceleration(t64, q) - xdd).max(axis=1) / scale).max()
                floor = (np.abs(TR.task_acceleration(t64, q32) - xdd).max(axis=1) / scale).max()
                _held(tag + " residual of J qdd + b = xdd_des", fig, floor)


# ------------------------------------------------------------------ T3: round trip through the solve library
@pytest.mark.parametrize("mode", ["force", "joint"])
def test_round_trip_through_forward_dynamics(ctx, tk, mode):  # noqa: F811
    """hs_forward_dynamics(gen_force + u), then J qdd + b against xdd_des; the floor is the float32
    reference's own round trip."""
    from humanoid_amd.solve import Solver
    solver = Solver(ctx.eng)
    m = tk.task.MODES[mode]
    for k in (6, 30):
        t64, t32 = tk.ref(k)
        xdd = tk.xdd[k]
        u, _, q = tk.control(k, mode, 0.0, tk.f)
        back = host(solver.forward_dynamics(cu(tk.f + u)))
        u32, _, _ = TR.task_control(t32, xdd, tk.f, m)
        back32 = SR.forward_dynamics(t32.M, t32.c, tk.f + u32)
        scale = np.abs(xdd).max(axis=1)
        fig = (np.abs(TR.task_acceleration(t64, back) - xdd).max(axis=1) / scale).max()
        floor = (np.abs(TR.task_acceleration(t64, back32) - xdd).max(axis=1) / scale).max()
        _held(f"k={k} {mode} round trip", fig, floor)
    del solver


# ------------------------------------------------------------------ T4: invariance
def test_an_output_does_not_depend_on_the_others_asked_for(ctx, tk):  # noqa: F811
    for k in (6, 31):
        every = tk.terms(k, tk.f)
        for name in tk.task.TERMS:
            alone = tk.terms(k, tk.f, want=(name,))
            assert list(alone) == [name] and np.array_equal(alone[name], every[name]), (k, name)
        pair = tk.terms(k, tk.f, want=("jminv", "bias_acc"))
        assert all(np.array_equal(pair[n], every[n]) for n in pair)
        for mode in ("force", "joint"):
            u, F, q = tk.control(k, mode, 0.0, tk.f)
            u1, n1, n2 = tk.control(k, mode, 0.0, tk.f, want_task_force=False, want_qdd=False)
            assert n1 is None and n2 is None and np.array_equal(u1, u)
            n1, F1, n2 = tk.control(k, mode, 0.0, tk.f, want_gen_force=False, want_qdd=False)
            assert n1 is None and n2 is None and np.array_equal(F1, F)
            n1, n2, q1 = tk.control(k, mode, 0.0, tk.f, want_gen_force=False, want_task_force=False)
            assert n1 is None and n2 is None and np.array_equal(q1, q)


def test_a_row_has_the_same_bits_in_every_row_set(ctx, tk):  # noqa: F811
    """The k = 1 row (R_Hand linear x) is row 6 of the k = 30 set."""
    assert tk.sets[30][6] == tk.sets[1][0]
    one, many = tk.terms(1, tk.f), tk.terms(30, tk.f)
    for name in ("jac", "jminv", "bias_acc", "free_acc"):
        assert np.array_equal(one[name][:, 0], many[name][:, 6]), name
    assert np.abs(one["jminv"]).max() > 0


def test_a_second_row_set_replaces_the_first(ctx, tk):  # noqa: F811
    fresh = tk.task.TaskSpace(ctx.eng)
    fresh.set_rows(tk.sets[6])
    want = {n: host(v) for n, v in fresh.terms(cu(tk.f)).items()}
    want_c = [host(v) for v in fresh.control(cu(tk.xdd[6]), cu(tk.f), "joint", 0.25)]
    tk.ts.set_rows(tk.sets[30])
    tk.ts.terms(cu(tk.f))
    got = tk.terms(6, tk.f)
    assert all(np.array_equal(got[n], want[n]) for n in want)
    got_c = tk.control(6, "joint", 0.25, tk.f)
    assert all(np.array_equal(a, b) for a, b in zip(got_c, want_c))
    # a refused set leaves the rows in place
    with pytest.raises(tk.task.TaskError, match="body 24"):
        tk.ts.set_rows([(24, 0)])
    again = {n: host(v) for n, v in tk.ts.terms(cu(tk.f)).items()}
    assert tk.ts.num_rows == 6 and all(np.array_equal(again[n], want[n]) for n in want)
    del fresh


# ------------------------------------------------------------------ T5: memory discipline
def test_sentinels_null_outputs_and_alignment(ctx, tk):  # noqa: F811
    """Nothing is written past an output's last element or into a buffer that was not passed, and the
    results do not depend on whether a buffer sits on an 8-byte boundary (N = 5 is odd, and here every
    buffer starts one float into its allocation)."""
    k = 31
    shapes = {"jac": (N, k, NG), "jminv": (N, k, NG), "lambda_inv": (N, k, k), "bias_acc": (N, k), "free_acc": (N, k)}
    want = tk.terms(k, tk.f)

    def buf(shape):
        b = torch.full((int(np.prod(shape)) + 1 + NG,), SENTINEL, dtype=torch.float32, device="cuda:0")
        return b, b[1:1 + int(np.prod(shape))].view(shape)

    def shifted(x):  # the same values one float into an allocation
        b = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda:0")
        b[1:] = cu(x).reshape(-1)
        return b[1:].view(x.shape)

    bufs = {n: buf(s) for n, s in shapes.items()}
    assert all(v.data_ptr() % 8 == 4 for _, v in bufs.values())
    tk.ts.set_rows(tk.sets[k])
    tk.ts.terms(shifted(tk.f), out={n: v for n, (_, v) in bufs.items()})
    for n, (b, v) in bufs.items():
        h = host(b)
        assert h[0] == SENTINEL and (h[1 + v.numel():] == SENTINEL).all(), n
        assert np.array_equal(h[1:1 + v.numel()].reshape(shapes[n]), want[n]), n
    # outputs that are not passed are not written: the buffers of the call above keep their contents
    keep = {n: host(b) for n, (b, _) in bufs.items()}
    b_only, v_only = buf(shapes["free_acc"])
    tk.ts.terms(cu(tk.f), want=(), out={"free_acc": v_only})
    assert np.array_equal(host(v_only), want["free_acc"]) and (host(b_only)[1 + v_only.numel():] == SENTINEL).all()
    assert all(np.array_equal(host(b), keep[n]) for n, (b, _) in bufs.items())
    for mode in ("force", "joint"):
        u, F, q = tk.control(k, mode, 0.0, tk.f)
        (bu, vu), (bf, vf), (bq, vq) = buf((N, NG)), buf((N, k)), buf((N, NG))
        tk.ts.control(shifted(tk.xdd[k]), shifted(tk.f), mode, 0.0, out=vu, task_force=vf, qdd=vq)
        for b, v, x in ((bu, vu, u), (bf, vf, F), (bq, vq, q)):
            h = host(b)
            assert h[0] == SENTINEL and (h[1 + v.numel():] == SENTINEL).all()
            assert np.array_equal(h[1:1 + v.numel()].reshape(x.shape), x)
        keep = [host(b) for b in (bu, bf, bq)]
        tk.ts.control(cu(tk.xdd[k]), cu(tk.f), mode, 0.0, want_gen_force=False, want_task_force=False)
        assert all(np.array_equal(host(b), kept) for b, kept in zip((bu, bf, bq), keep))


def test_refusals_leave_the_outputs_unchanged(ctx, tk):  # noqa: F811
    E = tk.task.TaskError
    dev = ctx.eng.device
    k = 6
    tk.ts.set_rows(tk.sets[k])
    u = torch.full((N, NG), SENTINEL, device=dev)
    lam = torch.full((N, k, k), SENTINEL, device=dev)
    xdd = cu(tk.xdd[k])
    with pytest.raises(E, match="xdd_des"):
        tk.ts.control(cu(tk.xdd[12]), out=u)  # the row count of another set
    with pytest.raises(E, match="gen_force"):
        tk.ts.control(xdd, torch.zeros(N, NG), out=u)  # a CPU tensor
    with pytest.raises(E, match="unknown flag"):
        tk.ts.control(xdd, out=u, flags=4)
    with pytest.raises(E, match="unknown mode"):
        tk.ts.control(xdd, out=u, mode=3)
    with pytest.raises(E, match="damping"):
        tk.ts.control(xdd, out=u, damping=-0.5)
    with pytest.raises(E, match="lambda_inv"):
        tk.ts.terms(out={"lambda_inv": torch.zeros(N, k, k + 1, device=dev)})
    with pytest.raises(E, match="unknown flag"):
        tk.ts.terms(out={"lambda_inv": lam}, flags=8)
    with pytest.raises(E, match="root_state"):
        tk.ts.terms(out={"lambda_inv": lam}, root_state=torch.zeros(N, 12, device=dev))
    rc = tk.ts.lib.ht_task_control(tk.ts.h, ctx.eng.root_states.data_ptr(), ctx.eng.dof_state.data_ptr(), xdd.data_ptr(), None,
                                   0, float("nan"), u.data_ptr(), None, None, 1, None)  # below the binding's check
    assert rc != 0 and "damping" in tk.ts.lib.ht_last_error().decode()
    fresh = tk.task.TaskSpace(ctx.eng)
    with pytest.raises(E, match="no rows set"):
        fresh.terms()
    rc = fresh.lib.ht_task_terms(fresh.h, ctx.eng.root_states.data_ptr(), ctx.eng.dof_state.data_ptr(), None, None, None,
                                 lam.data_ptr(), None, None, 1, None)
    assert rc != 0 and "no rows set" in fresh.lib.ht_last_error().decode()
    torch.cuda.synchronize()
    assert (u == SENTINEL).all().item() and (lam == SENTINEL).all().item()
    del fresh


def test_launch_on_a_side_stream(ctx, tk):  # noqa: F811
    want = tk.control(6, "joint", 0.0, tk.f)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert tk.ts.engine.stream.value == side.cuda_stream
        got = tk.ts.control(cu(tk.xdd[6]), cu(tk.f), "joint", 0.0)
    side.synchronize()
    assert all(np.array_equal(host(a), b) for a, b in zip(got, want))


# ------------------------------------------------------------------ T6: Dynamics.task and the gym facade
def test_facade_and_dynamics_task(ctx, tk):  # noqa: F811
    """The same numbers through Dynamics.task and through set_task_rows / solve_task_space, which see the
    state after the pending simulate calls; refusals surface as TaskError."""
    from humanoid_amd.isaacgym import gymtorch
    from test_facade_env import _facade_sim
    # Dynamics.task: ctx's engine, ctx's Dynamics
    k = 6
    want = tk.control(k, "joint", 0.0, tk.f)
    ctx.dyn.task.set_rows(tk.sets[k])
    got = ctx.dyn.task.control(cu(tk.xdd[k]), cu(tk.f), "joint")
    assert ctx.dyn.task is ctx.dyn.task and all(np.array_equal(host(a), b) for a, b in zip(got, want))
    # the facade against a direct TaskSpace on a second sim stepped the same way
    n = 4
    gym, sim = _facade_sim(n)
    gym2, sim2 = _facade_sim(n)
    dev = sim.engine.device
    rows = [("R_Hand", axis, (0.02, 0.0, 0.01)) for axis in range(3)]
    xdd = torch.tensor([[1.0, -2.0, 3.0]], device=dev).repeat(n, 1).contiguous()
    tau, force, qdd = torch.zeros(n, ND, device=dev), torch.zeros(n, NG, device=dev), torch.zeros(n, NG, device=dev)
    with pytest.raises(tk.task.TaskError, match="no rows set"):
        gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(tau))
    assert gym.set_task_rows(sim, rows)
    gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(tau))
    before = host(tau)
    for g, s in ((gym, sim), (gym2, sim2)):
        g.simulate(s)
        g.simulate(s)
    assert sim.pending_substeps == 2
    gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(tau), mode="joint",
                         qdd_out_desc=gymtorch.unwrap_tensor(qdd))
    assert sim.pending_substeps == 0
    gym2.fetch_results(sim2, True)
    assert torch.equal(sim.engine.dof_state, sim2.engine.dof_state)
    direct = tk.task.TaskSpace(sim2.engine)
    direct.set_rows(rows)
    u_d, _, q_d = direct.control(xdd, mode="joint")
    assert np.array_equal(host(tau), host(u_d)[:, 6:]) and np.array_equal(host(qdd), host(q_d))
    assert not np.array_equal(host(tau), before) and np.abs(host(tau)).max() > 0.1
    # force mode with a posture force inside gen_force and a damping
    u0 = torch.zeros(n, NG, device=dev)
    u0[:, 6:] = 3.0
    gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(force), mode="force", damping=1e-3,
                         gen_force_desc=gymtorch.unwrap_tensor(u0))
    u_f, _, _ = direct.control(xdd, u0, "force", 1e-3)
    assert torch.equal(force, u_f)
    # refusals
    with pytest.raises(tk.task.TaskError, match="unknown mode"):
        gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(tau), mode="torque")
    with pytest.raises(tk.task.TaskError, match="tau_out"):
        gym.solve_task_space(sim, gymtorch.unwrap_tensor(xdd), gymtorch.unwrap_tensor(force), mode="joint")
    with pytest.raises(tk.task.TaskError, match="axis"):
        gym.set_task_rows(sim, [("R_Hand", 7)])
    with pytest.raises(tk.task.TaskError, match="outside 1..32"):
        gym.set_task_rows(sim, [("R_Hand", 0)] * 33)
    torch.cuda.synchronize()
    del direct
