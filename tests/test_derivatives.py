"""CPU checks of the dynamics derivatives (include/humanoid_derivatives.h): the header, the hg_ symbols and
refusals of libhumanoid_solve.so, the binding, and the numpy reference of tests/derivative_reference.py (the
yardstick of tests/test_gpu_derivatives.py) against the definition it restates: the exact tangent
propagation in float64 against Richardson-extrapolated central differences of tau along q (+) delta, the
header's consequences (the zero pattern, the position columns, dtau_dv . qd = 2 c, what dtau_dv and the
armature do not touch, dtau_dq affine in a), and the forward form against differences of
solve_reference.forward_dynamics. The kernel itself is checked on the GPU.

States: the six of dynamics_reference.test_states (four tumbling, one with every dof angle exactly 0, one
with a joint near 2.5 rad), taken as the float32 values exactly; acc in +-20.

Bounds. EXACT = 1e-8 of the largest entry for the exact derivative against the differences: with the steps
1e-4 and 5e-5 the h^4 remainder of the extrapolation and the rounding of a float64 tau (1e-13 of ~1e3,
over 2 h) are both some 1e-9 of entries up to several hundred. The velocity differences are exact up to
rounding (tau is quadratic in qd). IDENTITY = 1e-12 of the largest entry for equalities of float64
expressions that sum the same terms in another order. FORWARD = 1e-6: the same differences, of qdd, whose
rounding is that of tau's through M^-1 (the condition of M with the armature is some 1e3).

The refusals that a handle must get past its null check are sent with a stand-in handle, a zeroed block of
memory: hg_compute checks its arguments before it reads the handle."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import derivative_reference as GR  # noqa: E402
import dynamics_reference as DR  # noqa: E402

from humanoid_amd import _abi  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_derivatives.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG
G = (0.0, 0.0, -9.81)
EXACT, IDENTITY, FORWARD = 1e-8, 1e-12, 1e-6
G64 = np.asarray(G, np.float32).astype(np.float64)  # the gravity vector as the device holds it


def _lib():
    from humanoid_amd import build, derivatives
    if not os.path.exists(derivatives.LIB_PATH):
        build.build()
    return derivatives.load_library()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------ header, symbols
def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import derivatives
    src = tmp_path / "hg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "humanoid_derivatives.h"\n'
                   'int main(void){printf("%u %u %u %u %u %d %d %d %d %d\\n", HG_FLAG_ARMATURE, HG_FLAG_NO_GRAVITY, '
                   "HG_FLAG_BY_DIRECTION, HG_FLAGS_DEFAULT, HG_FLAGS_ALL, HG_NUM_OUTPUTS, (int)sizeof(hg_outputs), "
                   "(int)offsetof(hg_outputs, dtau_dq), (int)offsetof(hg_outputs, dtau_dv), "
                   "(int)offsetof(hg_outputs, tau)); return 0;}\n")
    exe = tmp_path / "hg"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O = derivatives.HgOutputs
    assert out == [derivatives.FLAG_ARMATURE, derivatives.FLAG_NO_GRAVITY, derivatives.FLAG_BY_DIRECTION,
                   derivatives.FLAGS_DEFAULT,
                   derivatives.FLAG_ARMATURE | derivatives.FLAG_NO_GRAVITY | derivatives.FLAG_BY_DIRECTION,
                   len(derivatives.OUTPUTS), C.sizeof(O), O.dtau_dq.offset, O.dtau_dv.offset, O.tau.offset]
    assert [n for n, _ in O._fields_] == list(derivatives.OUTPUTS) == ["dtau_dq", "dtau_dv", "tau"]


def test_header_states_the_definitions():
    """The definitions and their consequences stand in the public header."""
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("qd[0:3] is the root origin's linear velocity in the world",
                   "qd[3:6] is the root's angular velocity in the world",
                   "qd[6+d] is the child-frame relative rate of the ball joints",
                   "the pose after flowing for unit time at generalised velocity delta",
                   "the root rotation becomes exp([delta[3:6]]x) R_0",
                   "joint b becomes R_a exp([theta_b]x) exp([delta_b]x)",
                   "keep their values, in their own coordinates",
                   "dtau_dq[e, i, j] = d/d eps tau_i(q (+) eps e_j, qd, a) at eps = 0",
                   "dtau_dv[e, i, j] = d tau_i / d qd_j",
                   "are not ancestor-or-self related",
                   "Columns 0-2 of dtau_dq are exactly zero, because gravity is uniform",
                   "dtau_dv does not depend on a, on gravity or on the armature",
                   "The armature does not enter either derivative",
                   "dtau_dv . qd = 2 c",
                   "a null handle; a null state pointer; a null `out`; all three outputs null; an output that is also "
                   "an input"):
        assert phrase in text, phrase


def test_library_exports_every_declared_symbol_and_the_other_families_are_unchanged():
    from humanoid_amd import derivatives, reaction, solve
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text)))
    assert syms == sorted(["hg_last_error", "hg_version", "hg_validate_model", "hg_create", "hg_destroy", "hg_compute"])
    assert set(syms) == set(derivatives.HG_PROTOTYPES) == set(derivatives.HG_SYMBOLS)
    assert lib.hg_version() == 1
    assert not re.findall(r"\bh[edsrtckw]_[a-z_0-9]+\s*\(", text)  # no other family's scan picks this header up
    assert derivatives.LIB_PATH == solve.LIB_PATH
    nm = subprocess.run(["nm", "-D", "--defined-only", derivatives.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("hg_")} == set(derivatives.HG_PROTOTYPES)
    assert {s for s in exported if s.startswith("hw_")} == set(reaction.HW_PROTOTYPES)
    assert {s for s in exported if s.startswith("hs_")} == set(solve.HS_PROTOTYPES)
    assert len(solve.HS_PROTOTYPES) == 8


def test_device_code_is_a_header_of_the_solve_source():
    from humanoid_amd import build
    assert build.LIBRARIES["solve"].sources == [("hs_solve.hip", ["-fno-slp-vectorize"])]
    assert not [f for f in os.listdir(build.CSRC) if f.startswith("hg_")]
    assert '#include "hs_derivs.h"' in open(os.path.join(build.CSRC, "hs_solve.hip")).read()
    assert any(h.endswith("hs_derivs.h") for h in build.HEADERS)
    assert any(h.endswith("humanoid_derivatives.h") for h in build.HEADERS)
    assert set(build.BUDGETS["hs_solve.hip"]) == {"solve_kernel", "torque_kernel"}
    assert all(b.max_scratch == 0 for b in build.BUDGETS["hs_solve.hip"].values())
    # the headers the other libraries share are not the place of the extension
    for shared in ("he_joint_space.h", "he_tree_state.h"):
        assert "dtau" not in open(os.path.join(build.CSRC, shared)).read()


def test_binding_is_a_query_binding():
    from humanoid_amd import derivatives, dynamics
    from humanoid_amd.isaacgym import gymapi
    cls = derivatives.Derivatives
    assert issubclass(cls, _abi.QueryBinding) and cls is not _abi.QueryBinding
    for name in ("__init__", "__del__", "flags", "_flags", "_states", "_out"):  # the constructor too is the base's
        assert name not in vars(cls) and hasattr(cls, name), name
    assert cls.LIBRARY.prefix == "hg" and cls.LIBRARY.error_cls is derivatives.DerivativesError
    assert cls.LIBRARY.prototypes is derivatives.HG_PROTOTYPES and cls.LIBRARY.path == derivatives.LIB_PATH
    assert cls.NO_CPU_PATH.endswith("no CPU path")
    for name in ("LIB_PATH", "load_library", "validate_model", "check_tensor", "HG_PROTOTYPES", "HG_SYMBOLS",
                 "FLAG_ARMATURE", "FLAG_NO_GRAVITY", "FLAG_BY_DIRECTION", "FLAGS_DEFAULT", "NG"):
        assert hasattr(derivatives, name), name
    assert issubclass(derivatives.DerivativesError, RuntimeError)
    assert derivatives.DerivativesError.__module__ == derivatives.__name__
    with pytest.raises(derivatives.DerivativesError, match="x: expected a torch tensor"):
        derivatives.check_tensor(None, None, (1,), None, "x")
    assert isinstance(dynamics.Dynamics.derivatives, property)
    assert derivatives.output_shapes(3) == {"dtau_dq": (3, 75, 75), "dtau_dv": (3, 75, 75), "tau": (3, 75)}
    for name in ("solve_dynamics_derivatives", "solve_forward_dynamics_derivatives"):
        assert callable(getattr(gymapi.Gym, name))
    with pytest.raises(RuntimeError, match="solve_dynamics_derivatives before prepare_sim"):
        gymapi.Gym().solve_dynamics_derivatives(gymapi.Sim(0, gymapi.SimParams()), None)


def test_binding_refuses_before_any_library_call():
    import torch
    from humanoid_amd import derivatives

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name} before the argument check")

    class Eng:
        root_states, dof_state = torch.zeros(3, 13), torch.zeros(3 * ND, 2)

    o = object.__new__(derivatives.Derivatives)
    o.lib, o.h, o.engine = NoCalls(), None, Eng()
    o.device, o.num_envs, o.armature, o.gravity = torch.device("cpu"), 3, True, True
    E = derivatives.DerivativesError
    with pytest.raises(E, match="no output asked for"):
        o.inverse_dynamics(dtau_dq=False, dtau_dv=False)
    with pytest.raises(E, match="out names"):
        o.inverse_dynamics(out={"dtau": torch.zeros(3, NG, NG)})
    with pytest.raises(E, match="acc"):
        o.inverse_dynamics(torch.zeros(3, ND))
    with pytest.raises(E, match="acc"):
        o.inverse_dynamics(torch.zeros(3, NG, dtype=torch.float64))
    with pytest.raises(E, match="dtau_dq"):
        o.inverse_dynamics(out={"dtau_dq": torch.zeros(3, NG, ND)})
    with pytest.raises(E, match="tau"):
        o.inverse_dynamics(out={"tau": torch.zeros(3, ND)})
    acc = torch.zeros(3, NG)
    with pytest.raises(E, match="also an input"):
        o.inverse_dynamics(acc, dtau_dq=False, dtau_dv=False, out={"tau": acc})
    both = torch.zeros(3, NG, NG)
    with pytest.raises(E, match="another output"):
        o.inverse_dynamics(acc, out={"dtau_dq": both, "dtau_dv": both})
    with pytest.raises(E, match="root_state"):
        o.inverse_dynamics(acc, root_state=torch.zeros(3, 12))


def test_refusals_in_the_headers_order_without_gpu(he_model):
    import copy
    from humanoid_amd import derivatives
    lib = _lib()
    g = (C.c_float * 3)(*G)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.hg_last_error().decode()

    assert "hg_create: num_envs" in reason(lib.hg_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "hg_create: null output" in reason(lib.hg_create(0, C.byref(he_model), g, 4, None))
    assert "hg_create: null gravity" in reason(lib.hg_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.hg_create(0, None, g, 4, C.byref(h)))
    assert h.value is None
    assert lib.hg_validate_model(C.byref(he_model)) == 0
    derivatives.validate_model(he_model)
    m = copy.deepcopy(he_model)
    m.parents[5] = 1  # hs_validate_model's refusal: not the tree the library is unrolled for
    assert "unrolled" in reason(lib.hg_validate_model(C.byref(m)))
    with pytest.raises(derivatives.DerivativesError, match="unrolled"):
        derivatives.validate_model(m)
    assert lib.hg_destroy(None) == 0

    one, acc_p, two, three, four, odd = (C.c_void_p(v) for v in (4096, 6144, 8192, 12288, 16384, 8194))
    block = C.create_string_buffer(4096)
    fake = C.cast(block, C.c_void_p)

    def outputs(**kw):
        return derivatives.HgOutputs(**{k: v.value for k, v in kw.items()})

    full = outputs(dtau_dq=two, dtau_dv=three, tau=four)

    def compute(handle=fake, root=one, dof=C.c_void_p(5120), acc=acc_p, out=full, flags=1):
        return lib.hg_compute(handle, root, dof, acc, None if out is None else C.byref(out), flags, None)

    # each refusal with everything after it in the order wrong as well: the earlier one is the one reported
    none = outputs()
    bad_out = outputs(dtau_dq=odd)
    alias = outputs(dtau_dq=acc_p, dtau_dv=odd)
    assert "hg_compute: null handle" in reason(compute(handle=None, root=None, out=None, flags=8, acc=odd))
    assert "hg_compute: null state pointer" in reason(compute(root=None, out=None, flags=8, acc=odd))
    assert "hg_compute: null state pointer" in reason(compute(dof=None, out=None, flags=8, acc=odd))
    assert "hg_compute: null output struct" in reason(compute(out=None, flags=8, acc=odd))
    assert "hg_compute: no output buffer" in reason(compute(out=none, flags=8, acc=odd))
    assert "hg_compute: an output is also an input" in reason(compute(out=alias, flags=8))
    assert "hg_compute: an output is also an input" in reason(compute(out=outputs(tau=one), flags=8))
    assert "hg_compute: two outputs are the same buffer" in reason(compute(out=outputs(dtau_dq=two, tau=two), flags=8))
    assert "hg_compute: unknown flag bits 0x8" in reason(compute(out=bad_out, flags=8 | 1))
    assert "hg_compute: every buffer must be 4-byte aligned" in reason(compute(out=bad_out, flags=7))
    for name in ("root", "dof", "acc"):  # every pointer is looked at
        assert "4-byte aligned" in reason(compute(**{name: C.c_void_p(8195)}))
    for name in derivatives.OUTPUTS:
        assert "4-byte aligned" in reason(compute(out=outputs(**{name: C.c_void_p(8193)})))
    assert block.raw == bytes(4096)  # the stand-in handle was never written


# ------------------------------------------------------------------ the reference against the definition
@pytest.fixture(scope="module")
def ref(he_model):
    """The module's states and acceleration, the exact derivative in float64 and the definition by
    differences (computed once, left unchanged)."""
    class S:
        pass

    s = S()
    s.root, s.dof = DR.test_states(he_model)
    s.n = n = s.root.shape[0]
    assert n == 6 and not s.dof[4, :, 0].any() and s.dof[4, :, 1].any()
    rng = np.random.default_rng(31)
    s.acc = rng.uniform(-20.0, 20.0, (n, NG)).astype(np.float32)
    s.exact = GR.exact(he_model, s.root, s.dof, s.acc, G)
    s.fd = GR.differences(he_model, s.root, s.dof, s.acc, G)
    s.mask = DR.mass_mask(DR.Model(he_model).parents)
    return s


def test_tau_is_the_headers(ref, he_model):
    """tau by Newton-Euler sums equals M a + c with dynamics_reference's mass matrix and a bias force by
    virtual power, and at the float32-rounded state dynamics_reference.evaluate's own M a + c."""
    Mo = DR.Model(he_model, np.float64)
    g = G64
    for e in range(ref.n):
        st = GR.split_state(ref.root[e], ref.dof[e])
        a = ref.acc[e].astype(np.float64)
        assert _rel(ref.exact["tau"][e], GR.tau_by_matrices(Mo, *st, a, g, True)) < IDENTITY
    _, M, c = DR.evaluate(he_model, ref.root, ref.dof, G, np.float64, armature=True)
    want = np.einsum("eij,ej->ei", M, ref.acc.astype(np.float64)) + c
    assert _rel(ref.exact["tau"], want) < IDENTITY


def test_exact_derivative_equals_the_definition(ref):
    for name in ("dtau_dq", "dtau_dv"):
        for e in range(ref.n):
            fig = _rel(ref.exact[name][e], ref.fd[name][e])
            print(f"{name} env {e}: exact against differences {fig:.2e} of {np.abs(ref.fd[name][e]).max():.1f}")
            assert fig < EXACT, (name, e, fig)
    assert _rel(ref.exact["tau"], ref.fd["tau"]) < IDENTITY


def test_difference_steps_agree(ref, he_model):
    """The two steps of the pose differences and their extrapolation on one state: the h^2 term is there
    and the extrapolation removes it (the reading the EXACT bound rests on)."""
    Mo = DR.Model(he_model, np.float64)
    e = 5
    st, a, g = GR.split_state(ref.root[e], ref.dof[e]), ref.acc[e].astype(np.float64), G64
    pos, quat, theta, qd = st
    fun = lambda d: GR.tau_at(Mo, *GR.moved(pos, quat, theta, d), qd, a, g, True)  # noqa: E731
    d1, d2 = GR._central(fun, GR.H_Q[0]), GR._central(fun, GR.H_Q[1])
    scale = np.abs(ref.exact["dtau_dq"][e]).max()
    e1, e2 = np.abs(d1 - ref.exact["dtau_dq"][e]).max() / scale, np.abs(d2 - ref.exact["dtau_dq"][e]).max() / scale
    print(f"h = {GR.H_Q[0]}: {e1:.2e}; h = {GR.H_Q[1]}: {e2:.2e}; extrapolated {_rel(ref.exact['dtau_dq'][e], ref.fd['dtau_dq'][e]):.2e}")
    assert 3.0 < e1 / e2 < 5.0  # second order


def test_zero_pattern_and_position_columns(ref):
    """Exactly zero where the two joints are not ancestor-or-self related, in the exact derivative and in
    the differences alike; the root position and root linear velocity columns are exactly zero."""
    for src in (ref.exact, ref.fd):
        for name in ("dtau_dq", "dtau_dv"):
            assert not src[name][:, ~ref.mask].any(), name
    for name in ("dtau_dq", "dtau_dv"):
        assert not ref.exact[name][:, :, 0:3].any(), name
    assert not ref.fd["dtau_dv"][:, :, 0:3].any()
    # a moved root position reaches the differences only through the rounding of the bodies' world positions
    assert np.abs(ref.fd["dtau_dq"][:, :, 0:3]).max() < EXACT * np.abs(ref.fd["dtau_dq"]).max()


def test_twice_the_bias_force(ref, he_model):
    """c without gravity is homogeneous of degree 2 in qd: dtau_dv . qd = 2 c."""
    Mo = DR.Model(he_model, np.float64)
    zero = np.zeros(NG)
    for e in range(ref.n):
        st = GR.split_state(ref.root[e], ref.dof[e])
        c0 = GR.tau_at(Mo, *st, zero, np.zeros(3), False)
        assert _rel(ref.exact["dtau_dv"][e] @ st[3], 2.0 * c0) < IDENTITY


def test_what_the_derivatives_do_not_depend_on(ref, he_model):
    """dtau_dv: not on a, gravity or the armature (the same numbers, bit for bit); dtau_dq: not on the
    armature; tau: on all three."""
    base = ref.exact
    for kw in (dict(acc=None), dict(acc=ref.acc, no_gravity=True), dict(acc=ref.acc, armature=False)):
        other = GR.exact(he_model, ref.root, ref.dof, gravity=G, **kw)
        assert np.array_equal(other["dtau_dv"], base["dtau_dv"]), kw
        assert not np.array_equal(other["tau"], base["tau"]), kw
        if "armature" in kw:
            assert np.array_equal(other["dtau_dq"], base["dtau_dq"])
        else:
            assert not np.array_equal(other["dtau_dq"], base["dtau_dq"])


def test_pose_derivative_is_affine_in_the_acceleration(ref, he_model):
    rng = np.random.default_rng(32)
    a2 = rng.uniform(-20.0, 20.0, (ref.n, NG)).astype(np.float32)
    d = {k: GR.exact(he_model, ref.root, ref.dof, v, G)["dtau_dq"] for k, v in (("2", a2), ("0", None))}
    # the sum in float64, unrounded: exact() takes float32 inputs, so the sum goes in by hand
    Mo = DR.Model(he_model, np.float64)
    for e in range(ref.n):
        st = GR.split_state(ref.root[e], ref.dof[e])
        _, dsum, _ = GR.exact_env(Mo, st, ref.acc[e].astype(np.float64) + a2[e], G64, True)
        resid = dsum - ref.exact["dtau_dq"][e] - d["2"][e] + d["0"][e]
        assert np.abs(resid).max() < IDENTITY * np.abs(dsum).max()


def test_forward_form_against_differences(ref, he_model):
    """d qdd / d q and d qdd / d qd (-M^-1 dtau at a = qdd) against float64 differences of
    solve_reference.forward_dynamics on the two hardest states, with a generalised force acting and the
    armature on; d qdd / d tau is M^-1."""
    Mo = DR.Model(he_model, np.float64)
    g = G64
    rng = np.random.default_rng(33)
    for e in (4, 5):
        st = GR.split_state(ref.root[e], ref.dof[e])
        f = rng.uniform(-50.0, 50.0, NG)
        qdd, dq, dv, minv = GR.forward_env(Mo, st, f, g, True)
        fq, fv = GR.forward_differences_env(Mo, st, f, g, True)
        M, c = GR.mass_and_bias(Mo, st, g, True)
        assert _rel(M @ qdd + c, f) < IDENTITY * 1e3 and _rel(minv @ M, np.eye(NG)) < IDENTITY * 1e3
        print(f"env {e}: dqdd_dq {_rel(dq, fq):.2e} of {np.abs(fq).max():.1f}, dqdd_dv {_rel(dv, fv):.2e} of {np.abs(fv).max():.1f}")
        assert _rel(dq, fq) < FORWARD and _rel(dv, fv) < FORWARD


def test_float32_floor_is_a_rounding(ref, he_model):
    """The float32 path of the reference, the floor of the GPU tolerances, is a few roundings and no more."""
    x32 = GR.exact(he_model, ref.root, ref.dof, ref.acc, G, np.float32)
    for name in ("tau", "dtau_dq", "dtau_dv"):
        assert x32[name].dtype == np.float32
        fig = GR.error(x32[name], ref.exact[name]).max()
        print(f"{name}: float32 floor {fig:.2e}")
        assert fig < 5e-6
