"""CPU checks of the joint-space solves (include/humanoid_solve.h): the library's header, symbols,
build lists and argument errors, the binding's tensor checks, and the numpy reference of
tests/solve_reference.py (the yardstick of tests/test_gpu_solve.py) against its pins: its own residual,
the tree-sparse L^T D L, free fall, the computed-torque round trip and one explicit step of the fp64
oracle. The kernels themselves are checked on the GPU (test_gpu_solve.py)."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
import dynamics_reference as DR  # noqa: E402
import solve_reference as SR  # noqa: E402

from humanoid_amd import _abi  # noqa: E402
from oracle import oracle as O  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_solve.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG
EPS64 = float(np.finfo(np.float64).eps)


def _lib():
    from humanoid_amd import build, solve
    if not os.path.exists(solve.LIB_PATH):
        build.build()
    return solve.load_library()


# ------------------------------------------------------------------ header, symbols, build lists
def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import solve
    src = tmp_path / "hs.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_solve.h"\n'
                   'int main(void){printf("%u %u %u %u %d %d\\n", HS_FLAG_ARMATURE, HS_FLAG_NO_GRAVITY, '
                   "HS_FLAGS_DEFAULT, HS_FLAGS_ALL, HS_MAX_RHS, HE_NUM_GEN); return 0;}\n")
    exe = tmp_path / "hs"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [solve.FLAG_ARMATURE, solve.FLAG_NO_GRAVITY, solve.FLAGS_DEFAULT,
                   solve.FLAG_ARMATURE | solve.FLAG_NO_GRAVITY, solve.MAX_RHS, solve.NG]


def test_solve_library_exports_every_declared_symbol():
    from humanoid_amd import solve
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hs_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 8
    assert not [s for s in syms if not hasattr(lib, s)]
    assert set(syms) == set(solve.HS_PROTOTYPES) == set(solve.HS_SYMBOLS)
    assert lib.hs_version() == 1
    # the other libraries' header scans must not pick anything up from this header
    assert not re.findall(r"\bh[ed]_[a-z_0-9]+\s*\(", text)
    # and the shared object exports nothing of the engine's or the dynamics library's
    nm = subprocess.run(["nm", "-D", "--defined-only", solve.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert not [s for s in exported if re.match(r"h[edr]_", s)]
    assert {s for s in exported if s.startswith("hs_")} == set(solve.HS_PROTOTYPES)


def test_solve_library_is_a_library_of_its_own():
    from humanoid_amd import build
    libs = build.LIBRARIES
    assert libs["solve"].sources == [("hs_solve.hip", ["-fno-slp-vectorize"])]
    assert [name for name, lib in libs.items() if any(s.startswith("hs_") for s, _ in lib.sources)] == ["solve"]
    assert libs["dynamics"].sources == [("hd_dynamics.hip", [])]
    assert len({libs[n].path for n in ("solve", "dynamics", "engine", "render", "engine_phases")}) == 5
    assert any(h.endswith("humanoid_solve.h") for h in build.HEADERS)
    assert build.BUDGETS["hs_solve.hip"] == {k: build.Budget(max_scratch=0) for k in ("solve_kernel", "torque_kernel")}
    build.build()
    ids = {build.device_code_id(libs[n].path) for n in ("engine", "render", "dynamics", "solve")}
    assert len(ids) == 4


def test_scratch_check_takes_one_name_or_several():
    from humanoid_amd import build
    from resource_reports import report

    build.check_resources("hs_solve.hip", report({"solve_kernel": {}, "torque_kernel": {}}))
    build.check_resources("hs_solve.hip", report({"torque_kernel": {}, "solve_kernel": {}}))
    with pytest.raises(RuntimeError, match="torque_kernel: 8 bytes/lane of scratch"):
        build.check_resources("hs_solve.hip", report({"solve_kernel": {}, "torque_kernel": {"scratch": 8}}))
    with pytest.raises(RuntimeError, match="torque_kernel: not in the compiler's resource report"):
        build.check_resources("hs_solve.hip", report({"solve_kernel": {}}))
    with pytest.raises(RuntimeError, match="torque_kernel: no scratch size"):
        build.check_resources("hs_solve.hip", report({"solve_kernel": {}, "torque_kernel": {"scratch": None}}))
    with pytest.raises(RuntimeError, match="dynamics_kernel: 4 bytes/lane of scratch"):
        build.check_resources("hd_dynamics.hip", report({"dynamics_kernel": {"scratch": 4}}))


# ------------------------------------------------------------------ argument errors, no GPU
def test_abi_errors_are_reported_without_gpu(he_model):
    """Argument errors come back as a nonzero code with a reason, before any device is touched."""
    from humanoid_amd import solve
    lib = _lib()
    g = (C.c_float * 3)(0.0, 0.0, -9.81)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.hs_last_error().decode()

    assert "hs_forward_dynamics: null handle" in reason(lib.hs_forward_dynamics(None, None, None, None, None, 1, None))
    assert "hs_computed_torque: null handle" in reason(
        lib.hs_computed_torque(None, None, None, None, None, None, None, 1, None))
    assert "hs_solve: null handle" in reason(lib.hs_solve(None, None, None, None, None, 1, 1, None))
    assert "num_envs" in reason(lib.hs_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "null output" in reason(lib.hs_create(0, C.byref(he_model), g, 4, None))
    assert "gravity" in reason(lib.hs_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.hs_create(0, None, g, 4, C.byref(h)))
    assert lib.hs_validate_model(C.byref(he_model)) == 0
    solve.validate_model(he_model)
    for field, value, word in (("num_bodies", 23, "bodies"), ("num_dof", 68, "dofs"), ("num_pairs", 257, "pair")):
        m = copy.deepcopy(he_model)
        setattr(m, field, value)
        assert word in reason(lib.hs_validate_model(C.byref(m)))
        with pytest.raises(solve.SolveError):
            solve.validate_model(m)
    m = copy.deepcopy(he_model)
    m.parents[0] = 0
    assert "root" in reason(lib.hs_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    m.parents[5] = 7
    assert "DFS" in reason(lib.hs_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    m.geom_type[3] = 9
    assert "geom type" in reason(lib.hs_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    for b in range(1, NB):
        m.parents[b] = b - 1  # one chain of 23 joints
    assert "joints from the root" in reason(lib.hs_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    m.parents[5] = 1  # a valid DFS tree, but not the one the factorisation is unrolled for
    assert "unrolled" in reason(lib.hs_validate_model(C.byref(m)))
    # a valid model and arguments: the only thing missing here is the device
    rc = lib.hs_create(0, C.byref(he_model), g, 4, C.byref(h))
    if rc != 0:
        assert "device" in lib.hs_last_error().decode().lower() or "hip" in lib.hs_last_error().decode().lower()
    else:  # on a GPU machine the handle exists: the remaining argument checks, none of which launches
        one = C.c_void_p(4096)  # never dereferenced: every call below is refused first
        assert "state pointer" in reason(lib.hs_forward_dynamics(h, None, None, None, one, 1, None))
        assert "null output" in reason(lib.hs_forward_dynamics(h, one, one, None, None, 1, None))
        assert "unknown flag" in reason(lib.hs_forward_dynamics(h, one, one, None, one, 4, None))
        assert "state pointer" in reason(lib.hs_computed_torque(h, one, None, one, None, one, one, 1, None))
        assert "desired acceleration" in reason(lib.hs_computed_torque(h, one, one, None, None, one, one, 1, None))
        assert "no output" in reason(lib.hs_computed_torque(h, one, one, one, None, None, None, 1, None))
        assert "unknown flag" in reason(lib.hs_computed_torque(h, one, one, one, None, one, None, 9, None))
        two = C.c_void_p(8192)
        assert "right-hand side" in reason(lib.hs_solve(h, one, one, None, two, 1, 1, None))
        assert "null output" in reason(lib.hs_solve(h, one, one, one, None, 1, 1, None))
        assert "same buffer" in reason(lib.hs_solve(h, one, one, one, one, 1, 1, None))
        assert "outside 1..32" in reason(lib.hs_solve(h, one, one, one, two, 0, 1, None))
        assert "outside 1..32" in reason(lib.hs_solve(h, one, one, one, two, 33, 1, None))
        assert "unknown flag" in reason(lib.hs_solve(h, one, one, one, two, 1, 16, None))
        assert "4-byte aligned" in reason(lib.hs_solve(h, one, one, C.c_void_p(4098), two, 1, 1, None))
        lib.hs_destroy(h)


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


class _NoEngine:
    stream = None

    def __getattr__(self, name):
        raise AssertionError(f"engine attribute {name} read before the argument check")


def test_binding_checks_tensors_before_any_library_call():
    import torch
    from humanoid_amd import solve
    n = 3
    s = object.__new__(solve.Solver)
    s.lib, s.h, s.engine = _NoCalls(), None, _NoEngine()
    s.device, s.num_envs, s.armature, s.gravity = torch.device("cuda", 0), n, True, True
    assert s.flags == solve.FLAG_ARMATURE
    s.armature, s.gravity = False, False
    assert s.flags == solve.FLAG_NO_GRAVITY
    with pytest.raises(solve.SolveError, match="gen_force"):
        s.forward_dynamics(torch.zeros(n, NG))  # a CPU tensor
    with pytest.raises(solve.SolveError, match="out"):
        s.forward_dynamics(None, torch.zeros(n, NG, dtype=torch.float64))
    with pytest.raises(solve.SolveError, match="qdd_des"):
        s.computed_torque(torch.zeros(n, NG))
    with pytest.raises(solve.SolveError, match="no output"):
        s.computed_torque(torch.zeros(n, ND), want_tau=False, want_base_acc=False)
    with pytest.raises(solve.SolveError, match="rhs"):
        s.solve(torch.zeros(n, NG))
    with pytest.raises(solve.SolveError, match="outside 1..32"):
        s.solve(torch.zeros(n, 33, NG))
    with pytest.raises(solve.SolveError, match="outside 1..32"):
        s.solve(torch.zeros(n, 0, NG))
    with pytest.raises(solve.SolveError, match="rhs"):
        s.solve(torch.zeros(n, NG, 6).transpose(1, 2))
    with pytest.raises(solve.SolveError, match="rhs"):
        s.solve(np.zeros((n, 6, NG), np.float32))


def test_dynamics_delegates_to_a_lazily_created_solver():
    from humanoid_amd import dynamics, solve
    calls = []

    class _Solver:
        armature, gravity = None, None

        def forward_dynamics(self, *a):
            calls.append(("fd", a, self.armature, self.gravity))
            return "qdd"

        def computed_torque(self, *a):
            calls.append(("ct", a, self.armature, self.gravity))
            return "tau", "acc"

        def solve(self, *a):
            calls.append(("solve", a, self.armature, self.gravity))
            return "x"

    d = object.__new__(dynamics.Dynamics)
    d.armature, d.gravity = False, True
    d._solver = _Solver()
    assert d.forward_dynamics("f", "o") == "qdd" and calls[-1] == ("fd", ("f", "o"), False, True)
    d.gravity = False
    assert d.computed_torque("q", None, "t", "b") == ("tau", "acc") and calls[-1] == ("ct", ("q", None, "t", "b"), False, False)
    d.armature = True
    assert d.solve("r", None) == "x" and calls[-1] == ("solve", ("r", None), True, False)
    assert set(("forward_dynamics", "computed_torque", "solve")) <= set(dir(solve.Solver))


def test_facade_solves_before_prepare_sim_raise():
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    with pytest.raises(RuntimeError, match="solve_forward_dynamics before prepare_sim"):
        gym.solve_forward_dynamics(sim, None, None)
    with pytest.raises(RuntimeError, match="solve_computed_torque before prepare_sim"):
        gym.solve_computed_torque(sim, None, None)
    with pytest.raises(RuntimeError, match="solve_mass_matrix before prepare_sim"):
        gym.solve_mass_matrix(sim, None, None)
    assert sim.dynamics is None


# ------------------------------------------------------------------ the reference against its pins
@pytest.fixture(scope="module")
def ref(he_model):
    """The shared states of the dynamics tests (4 random, one all-zero dofs, one with joints near 2.5 rad),
    float64 M (armature on) and c there, and right-hand sides; computed once, left unchanged."""
    root, dof = DR.test_states(he_model)
    sp = _abi.default_sim_params()
    g = tuple(sp.gravity)
    M, c = SR.terms(he_model, root, dof, g, np.float64, armature=True)
    M0, _ = SR.terms(he_model, root, dof, g, np.float64, armature=False)
    rng = np.random.default_rng(5)
    n = root.shape[0]
    f = np.concatenate([np.zeros((n, 6)), rng.uniform(-100.0, 100.0, (n, ND))], axis=1)
    rhs = rng.normal(size=(n, 4, NG))
    qdd_des = rng.uniform(-20.0, 20.0, (n, ND))
    parents = np.array(he_model.parents[:NB])
    return dict(root=root, dof=dof, g=g, M=M, M0=M0, c=c, f=f, rhs=rhs, qdd_des=qdd_des, n=n,
                lam=SR.dof_parents(parents), mask=DR.mass_mask(parents))


def test_reference_residual_is_float64_rounding(ref):
    """|M x - b| <= 1e-12 (|M||x| + |b|) componentwise for the three solves, armature on and off (the
    harder matrix: cond 1.9e6 against 3.8e3)."""
    worst = 0.0
    for M in (ref["M"], ref["M0"]):
        x = SR.forward_dynamics(M, ref["c"], ref["f"])
        worst = max(worst, SR.residual(M, x, ref["f"] - ref["c"]).max())
        X = SR.solve(M, ref["rhs"])
        worst = max(worst, SR.residual(M, X, ref["rhs"]).max())
        tau, ab = SR.computed_torque(M, ref["c"], ref["qdd_des"], ref["f"])
        worst = max(worst, SR.torque_residual(M, ref["c"], ref["qdd_des"], tau, ab, ref["f"]).max())
    print("reference residual, componentwise:", worst)
    assert worst < 1e-12


def test_sparse_ltdl_equals_the_dense_solve(ref):
    """The tree-sparse L^T D L reproduces M (so it needs no fill-in) and its solve equals the dense
    Cholesky's within cond(M) eps."""
    lam = ref["lam"]
    assert lam[0] == -1 and (lam[1:] < np.arange(1, NG)).all() and (lam[1:] >= 0).all()
    worst = 0.0
    for M in (ref["M"], ref["M0"]):
        for e in range(ref["n"]):
            L, D = SR.ltdl(M[e], lam)
            rebuilt = L.T @ np.diag(D) @ L
            assert np.abs(rebuilt - M[e]).max() <= 1e-13 * np.abs(M[e]).max()
            assert (D > 0).all()
            # no fill-in: L is zero off the tree's pattern, where M is
            assert not (~ref["mask"] & (M[e] != 0.0)).any()
            assert not (~ref["mask"] & (L - np.eye(NG) != 0.0)).any()
            b = ref["f"][e] - ref["c"][e]
            xs = SR.ltdl_solve(M[e], lam, b)
            xd = SR.spd_solve(M[e], b)
            err = np.abs(xs - xd).max() / np.abs(xd).max()
            bound = 10.0 * np.linalg.cond(M[e]) * EPS64
            worst = max(worst, err / bound)
            assert err <= bound, (e, err, bound)
    print("sparse against dense, worst error / (10 cond eps):", worst)


def test_free_fall(he_model, ref):
    """A body at rest with no generalised force falls: qdd[0:3] = g, every other entry 0."""
    root, dof = ref["root"].copy(), ref["dof"].copy()
    root[:, 7:13] = 0
    dof[..., 1] = 0
    M, c = SR.terms(he_model, root, dof, ref["g"])
    qdd = SR.forward_dynamics(M, c)
    want = np.zeros((ref["n"], NG))
    want[:, :3] = np.asarray(ref["g"], np.float64)
    print("free fall, max deviation:", np.abs(qdd - want).max())
    np.testing.assert_allclose(qdd, want, rtol=0, atol=1e-9)


def test_computed_torque_round_trip(ref):
    """forward_dynamics(gen_force + (0, tau)) of computed_torque's tau returns (a_b, qdd_des), within
    cond(M) eps of the largest acceleration."""
    tau, ab = SR.computed_torque(ref["M"], ref["c"], ref["qdd_des"], ref["f"])
    f = ref["f"].copy()
    f[:, 6:] += tau
    qdd = SR.forward_dynamics(ref["M"], ref["c"], f)
    want = np.concatenate([ab, ref["qdd_des"]], axis=1)
    err = SR.forward_error(qdd, want)
    bound = 10.0 * np.array([np.linalg.cond(m) for m in ref["M"]]) * EPS64
    print("round trip, relative:", err, "bound", bound)
    assert (err <= bound).all()
    # and without a generalised force, the tau of gravity compensation holds the joints still
    tau0, ab0 = SR.computed_torque(ref["M"], ref["c"], np.zeros((ref["n"], ND)))
    f0 = np.concatenate([np.zeros((ref["n"], 6)), tau0], axis=1)
    q0 = SR.forward_dynamics(ref["M"], ref["c"], f0)
    assert np.abs(q0[:, 6:]).max() <= bound.max() * np.abs(q0).max()
    assert (SR.forward_error(q0[:, :6], ab0) <= bound).all()


def test_forward_dynamics_is_the_oracles_explicit_step(he_model):
    """One explicit PGS step of the fp64 oracle (no midpoint bias, one substep, no drive gains, no
    damping, no limits, the velocity clamps out of reach, in flight): (u1 - u0) / dt is
    forward_dynamics(0) with the armature on M. The oracle computes in float64 but hands the state back
    in float32: u0 is exact, u1 carries a rounding of at most 2^-24 |u1| per entry, so the step's
    acceleration differs from the reference by at most 2^-24 |u1| / dt in that entry, plus the float64
    level at which tests/test_dynamics.py holds M and c to the oracle (5e-15 of the largest entry) taken
    through the solve (times cond(M))."""
    n = 6
    rng = np.random.default_rng(43)
    root, dof = cases.random_state(n, rng, height=(3.0, 4.0), vel=0.5, ang=0.5)
    sp = _abi.pgs_sim_params(bias_midpoint=0, substeps=1, angular_damping=0.0, joint_limits=0, self_collision=0,
                             kp_scale=0.0, kd_scale=0.0, max_joint_velocity=1e6, max_angular_velocity=1e6)
    dt = float(sp.dt)
    M, c = SR.terms(he_model, root, dof, tuple(sp.gravity), np.float64, armature=True)
    qdd = SR.forward_dynamics(M, c)
    r1, d1 = root.copy(), dof.copy()
    out = O.physics_step(he_model, sp, r1, d1, dof[..., 0].copy(), 1)
    assert int(out["num_contacts"].max()) == 0
    u0 = np.stack([DR.gen_velocity(root[e], dof[e]) for e in range(n)])
    u1 = np.stack([DR.gen_velocity(r1[e], d1[e]) for e in range(n)])
    a = (u1 - u0) / dt
    cond = np.array([np.linalg.cond(m) for m in M])
    bound = 2.0 ** -24 * np.abs(u1) / dt + (5e-15 * cond * np.abs(qdd).max(axis=1))[:, None]
    err = np.abs(a - qdd)
    print("oracle step against forward_dynamics(0): max |a - qdd|", err.max(), "of max |qdd|", np.abs(qdd).max(),
          "relative", err.max() / np.abs(qdd).max(), "; worst entry / its bound", (err / bound).max())
    assert np.abs(qdd).max() > 5.0  # gravity and the tumbling both show
    assert (err <= bound).all()
