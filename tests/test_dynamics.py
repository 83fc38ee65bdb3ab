"""CPU checks of the dynamics-query tensors: the numpy reference of ``include/humanoid_dynamics.h``
(tests/dynamics_reference.py, the yardstick of tests/test_gpu_dynamics.py) is pinned to the
finite-difference mechanics of tests/test_independent_dynamics.py and to the fp64 oracle; then the
library's ABI, the binding's argument checks, the gym facade's guards and the engine library's
device-code identity. The kernel itself is checked on the GPU (test_gpu_dynamics.py)."""
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import test_independent_dynamics as TI  # noqa: E402  (Body, _jacobians: the central-difference yardstick)

from humanoid_amd import _abi  # noqa: E402
from oracle import oracle as O  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_dynamics.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG


@pytest.fixture(scope="module")
def ref(he_model):
    """The shared states (4 random, one all-zero dofs, one with joints near 2.5 rad) and the float64
    reference at them, armature off; computed once, left unchanged."""
    root, dof = DR.test_states(he_model)
    sp = _abi.default_sim_params()
    J, M, c = DR.evaluate(he_model, root, dof, tuple(sp.gravity), np.float64, armature=False)
    return dict(root=root, dof=dof, sp=sp, J=J, M=M, c=c)


def _lib():
    from humanoid_amd import build, dynamics
    if not os.path.exists(dynamics.LIB_PATH):
        build.build()
    return dynamics.load_library()


# ------------------------------------------------------------------ the reference against its pins
def test_states_cover_the_branches(ref):
    dof = ref["dof"]
    assert ref["root"].shape[0] == 6
    assert np.all(dof[4, :, 0] == 0.0) and np.abs(dof[4, :, 1]).max() > 0.1  # small-angle branch, moving
    ang = np.linalg.norm(dof[5, :, 0].reshape(NB - 1, 3), axis=1)
    assert 2.4 < ang.max() < 2.6


def test_reference_jacobian_against_central_differences(he_model, ref):
    """J against the central-difference Jacobians of the poses alone (origins and rotations flowed along
    each generalised velocity). The difference's roundoff is about eps / h = 1e-10 / 1e-6 of a lever arm,
    its truncation h^2 = 1e-12."""
    B = TI.Body(he_model)
    worst = 0.0
    for e in range(ref["root"].shape[0]):
        _, Jo, Jp = TI._jacobians(B, ref["root"][e], ref["dof"][e])
        fd = np.concatenate([Jp, Jo], axis=1)[:, :, DR.PERM]  # (w, v, dofs) -> (v, w, dofs)
        worst = max(worst, np.abs(ref["J"][e] - fd).max())
    print("reference J - central differences, max abs:", worst)
    assert worst < 5.2e-9  # 10 x the measured 5.2e-10


def test_reference_mass_matrix_and_bias_against_the_oracle(he_model, ref):
    """M (armature off) and c against the oracle's CRBA H and RNEA bias after the (w, v) -> (v, w) block
    permutation: two different algorithms in float64, so the bound is rounding, relative to the largest
    entry."""
    H, bias = O.dynamics_terms(he_model, ref["sp"], ref["root"], ref["dof"])
    P = DR.PERM
    em = ec = 0.0
    for e in range(ref["root"].shape[0]):
        em = max(em, np.abs(ref["M"][e] - H[e][P][:, P]).max() / np.abs(ref["M"][e]).max())
        ec = max(ec, np.abs(ref["c"][e] - bias[e][P]).max() / np.abs(ref["c"][e]).max())
    print("reference M, c - oracle, relative to the largest entry:", em, ec)
    assert em < 1e-15  # 10 x the measured 9.7e-17
    assert ec < 5e-15  # 10 x the measured 4.9e-16


def test_armature_adds_exactly_the_dof_diagonal(he_model, ref):
    Mo = DR.Model(he_model)
    assert Mo.armature.max() > 0.0
    for e in (0, 5):
        R, p = DR.fk(Mo, ref["root"][e], ref["dof"][e])
        J = DR.jacobian(Mo, R, p)
        d = DR.mass_matrix(Mo, R, J, True) - DR.mass_matrix(Mo, R, J, False)
        want = np.zeros((NG, NG))
        want[np.arange(6, NG), np.arange(6, NG)] = Mo.armature
        assert np.array_equal(d != 0.0, want != 0.0)
        np.testing.assert_allclose(d, want, rtol=0, atol=1e-12)


def test_jacobian_times_velocity_is_the_rigid_body_velocity(he_model, ref):
    """The defining property, against the oracle's rigid-body rows (float32 outputs of float64 work)."""
    rb = O.forward_kinematics(he_model, ref["root"], ref["dof"]).astype(np.float64)
    for e in range(ref["root"].shape[0]):
        qd = DR.gen_velocity(ref["root"][e], ref["dof"][e])
        v = ref["J"][e] @ qd  # [24,6]
        # float32 rows: half an ulp of the largest velocity (about 10 m/s at the chain ends) is 5e-7
        np.testing.assert_allclose(v, rb[e, :, 7:13], rtol=0, atol=2e-6)


def test_mass_matrix_is_the_kinetic_energy_metric(he_model, ref):
    me = O.momentum_energy(he_model, ref["sp"], ref["root"], ref["dof"])
    for e in range(ref["root"].shape[0]):
        qd = DR.gen_velocity(ref["root"][e], ref["dof"][e])
        np.testing.assert_allclose(0.5 * qd @ ref["M"][e] @ qd, me[e, 6], rtol=1e-12)
        assert np.array_equal(ref["M"][e], ref["M"][e].T) or np.abs(ref["M"][e] - ref["M"][e].T).max() < 1e-13


def test_inverse_dynamics_of_gravity_free_rest_is_zero(he_model, ref):
    """Without gravity and at rest the bias vanishes; with gravity at rest it is minus the gravity
    force's generalised components (root linear part: -m_total g)."""
    root, dof = ref["root"].copy(), ref["dof"].copy()
    root[:, 7:13] = 0
    dof[..., 1] = 0
    _, _, c0 = DR.evaluate(he_model, root, dof, no_gravity=True)
    assert np.abs(c0).max() == 0.0
    g = tuple(ref["sp"].gravity)
    _, _, cg = DR.evaluate(he_model, root, dof, g)
    mtot = float(np.sum(np.array(he_model.mass[:NB], np.float64)))
    np.testing.assert_allclose(cg[:, 0:3], np.broadcast_to(-mtot * np.asarray(g), (cg.shape[0], 3)), rtol=1e-12, atol=1e-12)


def test_jacobian_sparsity_is_the_subtree_mask(he_model, ref):
    """A dof column of joint j is nonzero only in j's subtree, and its angular rows (a unit vector) are
    nonzero in all of it: the angular block's pattern is exactly the mask built from `parents`."""
    parents = np.array(he_model.parents[:NB])
    mask = DR.jacobian_mask(parents)  # [24,75]
    assert mask[:, :6].all() and mask.sum() < mask.size / 2
    for e in range(ref["root"].shape[0]):
        nz = ref["J"][e] != 0.0  # [24,6,75]
        assert not (nz & ~mask[:, None, :]).any()
        ang = nz[:, 3:6, :].any(axis=1)
        assert np.array_equal(ang[:, 3:], mask[:, 3:]) and not ang[:, :3].any()  # root linear columns: (e_i, 0)
        lin = nz[:, 0:3, 6:].any(axis=1)  # linear rows: the subtree without the joint's own body
        own = np.zeros((NB, NG - 6), bool)
        for c in range(6, NG):
            own[DR.col_joint(c), c - 6] = True
        assert np.array_equal(lin, mask[:, 6:] & ~own)
    mm = DR.mass_mask(parents)
    assert np.array_equal(mm, mm.T)
    for e in range(ref["root"].shape[0]):
        assert not ((ref["M"][e] != 0.0) & ~mm).any()


def test_float32_floor_of_the_reference(he_model, ref):
    """The reference evaluated in float32 against float64: the floor the GPU tolerance is 8 x of. Pinned
    loosely here so that a change of the reference that moves the floor is seen."""
    g = tuple(ref["sp"].gravity)
    J32, M32, c32 = DR.evaluate(he_model, ref["root"], ref["dof"], g, np.float32, armature=False)
    assert J32.dtype == M32.dtype == c32.dtype == np.float32
    fj = np.abs(J32 - ref["J"]).max()
    fm = np.abs(M32 - ref["M"]).max() / np.abs(ref["M"]).max()
    fc = np.abs(c32 - ref["c"]).max()
    print("float32 floors: J", fj, "M / max", fm, "c", fc, "N, max |c|", np.abs(ref["c"]).max())
    # measured 3.6e-7, 5.0e-8, 1.5e-4 N (of 727 N): a few float32 ulps of each output's largest entry
    assert 1e-8 < fj < 2e-6 and 1e-9 < fm < 5e-7 and 1e-6 < fc < 1e-3


# ------------------------------------------------------------------ ABI
def test_dynamics_library_exports_every_declared_symbol():
    from humanoid_amd import dynamics
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hd_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 6
    assert not [s for s in syms if not hasattr(lib, s)]
    assert set(syms) == set(dynamics.HD_SYMBOLS)
    assert lib.hd_version() == 1
    # the engine's header scan (test_abi.py) must not pick anything up from this header
    assert not re.findall(r"\bhe_[a-z_0-9]+\s*\(", text)


def test_dynamics_library_is_not_part_of_the_engine():
    from humanoid_amd import build
    libs = build.LIBRARIES
    assert [name for name, lib in libs.items() if any(s.startswith("hd_") for s, _ in lib.sources)] == ["dynamics"]
    assert libs["dynamics"].sources == [("hd_dynamics.hip", [])]
    assert len({libs[n].path for n in ("dynamics", "engine", "render", "engine_phases")}) == 4
    assert any(h.endswith("humanoid_dynamics.h") for h in build.HEADERS)
    assert build.BUDGETS["hd_dynamics.hip"]["dynamics_kernel"] == build.Budget(max_scratch=0)


def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import dynamics
    src = tmp_path / "hd.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_dynamics.h"\n'
                   'int main(void){printf("%u %u %u %u %d %d\\n", HD_FLAG_ARMATURE, HD_FLAG_NO_GRAVITY, '
                   "HD_FLAGS_DEFAULT, HD_FLAGS_ALL, HD_JAC_ROWS, HE_NUM_GEN); return 0;}\n")
    exe = tmp_path / "hd"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [dynamics.FLAG_ARMATURE, dynamics.FLAG_NO_GRAVITY, dynamics.FLAGS_DEFAULT,
                   dynamics.FLAG_ARMATURE | dynamics.FLAG_NO_GRAVITY, dynamics.JAC_ROWS, dynamics.NG]


def test_abi_errors_are_reported_without_gpu(he_model):
    """Argument errors come back as a nonzero code with a reason, before any device is touched."""
    import copy
    from humanoid_amd import dynamics
    lib = _lib()
    g = (C.c_float * 3)(0.0, 0.0, -9.81)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.hd_last_error().decode()

    assert "null handle" in reason(lib.hd_compute(None, None, None, None, None, None, 1, None))
    assert "num_envs" in reason(lib.hd_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "null output" in reason(lib.hd_create(0, C.byref(he_model), g, 4, None))
    assert "gravity" in reason(lib.hd_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.hd_create(0, None, g, 4, C.byref(h)))
    assert lib.hd_validate_model(C.byref(he_model)) == 0
    dynamics.validate_model(he_model)
    for field, value, word in (("num_bodies", 23, "bodies"), ("num_dof", 68, "dofs"), ("num_pairs", 257, "pair")):
        m = copy.deepcopy(he_model)
        setattr(m, field, value)
        assert word in reason(lib.hd_validate_model(C.byref(m)))
        with pytest.raises(dynamics.DynamicsError):
            dynamics.validate_model(m)
    m = copy.deepcopy(he_model)
    m.parents[0] = 0
    assert "root" in reason(lib.hd_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    m.parents[5] = 7
    assert "DFS" in reason(lib.hd_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    m.geom_type[3] = 9
    assert "geom type" in reason(lib.hd_validate_model(C.byref(m)))
    m = copy.deepcopy(he_model)
    for b in range(1, NB):
        m.parents[b] = b - 1  # one chain of 23 joints
    assert "joints from the root" in reason(lib.hd_validate_model(C.byref(m)))
    # a valid model and arguments: the only thing missing here is the device
    rc = lib.hd_create(0, C.byref(he_model), g, 4, C.byref(h))
    if rc != 0:
        assert "device" in lib.hd_last_error().decode().lower() or "hip" in lib.hd_last_error().decode().lower()
    else:  # on a GPU machine the handle exists: the remaining argument checks of hd_compute
        assert "state pointer" in reason(lib.hd_compute(h, None, None, None, None, None, 1, None))
        lib.hd_destroy(h)


# ------------------------------------------------------------------ the binding's argument checks
class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def _unbound_dynamics(n, device):
    from humanoid_amd import dynamics
    d = object.__new__(dynamics.Dynamics)
    d.lib, d.h, d.engine = _NoCalls(), None, None
    d.device, d.num_envs, d.armature, d.gravity = device, n, True, True
    return d


def test_binding_checks_tensors_before_any_library_call():
    import torch
    from humanoid_amd import dynamics
    dev = torch.device("cuda", 0)
    n = 3
    shapes = dynamics.output_shapes(n)
    assert shapes == {"jacobian": (3, 24, 6, 75), "mass_matrix": (3, 75, 75), "bias": (3, 75)}
    d = _unbound_dynamics(n, dev)
    assert d.flags == dynamics.FLAG_ARMATURE
    d.gravity, d.armature = False, False
    assert d.flags == dynamics.FLAG_NO_GRAVITY
    with pytest.raises(dynamics.DynamicsError, match="no output"):
        d.refresh_into()
    bad = {
        "CPU tensor": torch.zeros(shapes["bias"]),
        "wrong shape": torch.zeros(n, 74),
        "wrong dtype": torch.zeros(shapes["bias"], dtype=torch.float64),
        "non-contiguous": torch.zeros(75, n).t(),
        "not a tensor": np.zeros(shapes["bias"], np.float32),
    }
    for what, t in bad.items():
        with pytest.raises(dynamics.DynamicsError, match="bias"):
            d.refresh_into(bias=t)
        # each fault on its own (the device right, where the fault is not the device)
        with pytest.raises(dynamics.DynamicsError, match=what):
            dynamics.check_tensor(t, torch.float32, shapes["bias"], dev if what == "CPU tensor" else torch.device("cpu"),
                                  what)
    with pytest.raises(dynamics.DynamicsError, match="jacobian"):
        d.refresh_into(jacobian=torch.zeros(n, 24, 6, 64))
    with pytest.raises(dynamics.DynamicsError, match="mass_matrix"):
        d.refresh_into(mass_matrix=torch.zeros(n, 75, 75).transpose(1, 2))
    # a tensor that passes hands out its pointer
    ok = torch.zeros(shapes["bias"])
    assert dynamics.check_tensor(ok, torch.float32, shapes["bias"], torch.device("cpu"), "bias").value == ok.data_ptr()


def test_inverse_dynamics_is_mass_times_acceleration_plus_bias():
    import torch
    from humanoid_amd import dynamics
    d = _unbound_dynamics(2, torch.device("cpu"))
    gen = torch.Generator().manual_seed(3)
    d.mass_matrix = torch.randn(2, 75, 75, generator=gen)
    d.bias = torch.randn(2, 75, generator=gen)
    qdd = torch.randn(2, 75, generator=gen)
    want = torch.einsum("nij,nj->ni", d.mass_matrix, qdd) + d.bias
    torch.testing.assert_close(d.inverse_dynamics(qdd), want, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ facade guards
def test_facade_acquire_before_prepare_sim_raises():
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    for acquire in (gym.acquire_jacobian_tensor, gym.acquire_mass_matrix_tensor, gym.acquire_bias_force_tensor):
        with pytest.raises(RuntimeError, match="before prepare_sim"):
            acquire(sim, "humanoid")
    # a refresh before its acquire is a no-op that reports success, as in Isaac Gym
    assert gym.refresh_jacobian_tensors(sim) is True
    assert gym.refresh_mass_matrix_tensors(sim) is True
    assert gym.refresh_bias_force_tensors(sim) is True
    assert sim.dynamics is None


# ------------------------------------------------------------------ the engine's device code stays
def test_engine_device_code_is_the_recorded_one():
    """Adding the dynamics library must not move the engine's device code: after build(), the engine
    library's id equals the one in the newest committed parity record, and the three libraries' device
    codes are three different ones."""
    from humanoid_amd import build
    build.build()
    recs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "parity_configs1.json")))
    assert recs
    with open(recs[-1]) as f:
        want = json.load(f)["device_code"]
    assert build.device_code_id(build.LIBRARIES["engine"].path) == want
    ids = {build.device_code_id(build.LIBRARIES[n].path) for n in ("engine", "render", "dynamics")}
    assert len(ids) == 3
