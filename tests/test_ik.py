"""CPU checks of the inverse kinematics (include/humanoid_ik.h): the header, the hk_ symbols and refusals of
libhumanoid_task.so, the binding's checks, the facade's guards, and the numpy reference of
tests/ik_reference.py (the yardstick of tests/test_gpu_ik.py) against its pins: an undamped step meets
J dq = e with the least kinetic energy, the integration agrees with the Jacobian on every body, a limit
that binds is met exactly, and the iteration converges on the shared inputs. The kernel itself is checked
on the GPU (test_gpu_ik.py).

Measured here, float64 reference (bounds in the tests):

    J dq - e after one undamped step                                 4.2e-16
    FK(q + eps dq) - FK(q) - eps J dq, eps = 1e-3 / 1e-4, / eps^2    2.201 / 2.200 (positions), 2.4396 / 2.4397 (rotations)
    what a clipped step leaves beyond |e| - clip, clip 0.02 / 0.002  3.3e-3 / 5.1e-5
    worst residual after 8 iterations, k = 6 / 9 / 12 / 15           4.1e-8 / 1.2e-8 / 1.0e-8 / 3.1e-8 (m or rad)
    the same with the float32 reference                              2.1e-7 / 1.4e-7 / 1.9e-7 / 2.5e-7

The refusals that a handle must get past its null check are sent with a stand-in handle, a zeroed block
of memory: hk_solve checks its arguments before it reads the handle, and a zeroed handle is one without rows."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_reference as DR  # noqa: E402
import ik_reference as IK  # noqa: E402
import task_reference as TR  # noqa: E402

from humanoid_amd import _abi  # noqa: E402
from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_ik.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG


def _lib():
    from humanoid_amd import build, ik
    if not os.path.exists(ik.LIB_PATH):
        build.build()
    return ik.load_library()


# ------------------------------------------------------------------ header, symbols, build rules
def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import ik, task
    src = tmp_path / "hk.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_ik.h"\n'
                   'int main(void){printf("%u %u %u %u %d %d\\n", HK_FLAG_ARMATURE, HK_FLAG_LIMITS, HK_FLAGS_DEFAULT, '
                   "HK_FLAGS_ALL, HK_MAX_ITERATIONS, HT_MAX_ROWS); return 0;}\n")
    exe = tmp_path / "hk"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ik.FLAG_ARMATURE, ik.FLAG_LIMITS, ik.FLAGS_DEFAULT, ik.FLAG_ARMATURE | ik.FLAG_LIMITS,
                   ik.MAX_ITERATIONS, ik.MAX_ROWS]
    assert ik.MAX_ITERATIONS == IK.MAX_ITERATIONS == 64 and ik.FLAG_ARMATURE == task.FLAG_ARMATURE
    assert not ik.FLAGS_DEFAULT & task.FLAG_NO_GRAVITY  # the kernel sets that bit itself
    # the ABI has no struct of its own: the handle is opaque and the rows are humanoid_task.h's
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"\bstruct\s+(\w+)", text) == ["hk_solver"] and "{" not in text.replace('extern "C" {', "")
    assert '#include "humanoid_task.h"' in text


def test_library_exports_exactly_the_declared_symbols_of_both_families():
    from humanoid_amd import ik, task
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hk_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 7
    assert set(syms) == set(ik.HK_PROTOTYPES) == set(ik.HK_SYMBOLS)
    assert not [s for s in syms if not hasattr(lib, s)]
    assert lib.hk_version() == 1
    # the other families' header scans must not pick anything up from this header
    assert not re.findall(r"\bh[cedrst]_[a-z_0-9]+\s*\(", text)
    assert ik.LIB_PATH == task.LIB_PATH
    nm = subprocess.run(["nm", "-D", "--defined-only", ik.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("hk_")} == set(ik.HK_PROTOTYPES)
    assert {s for s in exported if s.startswith("ht_")} == set(task.HT_PROTOTYPES)
    assert not [s for s in exported if re.match(r"h[cedrs]_", s)]
    # the argument lists are the header's: a pointer is a pointer, the scalars in their places
    proto = re.search(r"int hk_solve\((.*?)\);", text, flags=re.S).group(1)
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "float": C.c_float, "uint32_t": C.c_uint32}[a.split()[0]]
             for a in proto.split(",")]
    assert kinds == ik.HK_PROTOTYPES["hk_solve"]


def test_the_family_lives_in_the_task_translation_unit():
    from humanoid_amd import build
    assert [s for s, _ in build.LIBRARIES["task"].sources] == ["ht_task.hip"] and len(build.LIBRARIES) == 6
    assert any(h.endswith("humanoid_ik.h") for h in build.HEADERS)
    assert any(h.endswith("ht_ik.h") for h in build.HEADERS)
    src = open(os.path.join(build.CSRC, "ht_task.hip")).read()
    assert src.rstrip().endswith('#include "ht_ik.h"')
    assert not [f for f in os.listdir(build.CSRC) if f.startswith("hk_")]
    # one kernel, in its budget: the family adds no __global__ function
    both = src + open(os.path.join(build.CSRC, "ht_ik.h")).read()
    assert len(re.findall(r"__global__", both)) == 1
    assert build.BUDGETS["ht_task.hip"] == {"task_kernel": build.Budget(min_waves=2, max_scratch=0)}


# ------------------------------------------------------------------ refusals, no GPU
def test_refusals_come_with_their_reason_and_in_the_stated_order(he_model):
    import copy
    from humanoid_amd import ik, task
    lib = _lib()
    g = (C.c_float * 3)(0.0, 0.0, -9.81)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.hk_last_error().decode()

    assert "hk_create: num_envs" in reason(lib.hk_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "hk_create: null output" in reason(lib.hk_create(0, C.byref(he_model), g, 4, None))
    assert "hk_create: null gravity" in reason(lib.hk_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.hk_create(0, None, g, 4, C.byref(h)))
    assert h.value is None
    assert lib.hk_validate_model(C.byref(he_model)) == 0
    ik.validate_model(he_model)
    m = copy.deepcopy(he_model)
    m.parents[5] = 1  # a valid DFS tree, but not the one the factorisation is unrolled for
    assert "unrolled" in reason(lib.hk_validate_model(C.byref(m)))
    with pytest.raises(ik.IKError, match="unrolled"):
        ik.validate_model(m)
    assert lib.hk_destroy(None) == 0

    one, two, odd = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(8194)
    block = C.create_string_buffer(4096)
    fake = C.cast(block, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def solve(handle=fake, root=one, dof=one, target=one, trot=None, iters=8, damping=1e-4, clip=0.1, root_out=two,
              dof_out=two, res=None, flags=ik.FLAGS_DEFAULT):
        return lib.hk_solve(handle, root, dof, target, trot, iters, damping, clip, root_out, dof_out, res, flags, None)

    # each refusal with everything after it in the order wrong as well: the earlier one is the one reported
    later = dict(flags=8, iters=0, damping=-1.0, clip=0.0, res=odd)
    assert "hk_solve: null handle" in reason(solve(handle=None, root=None, target=None, root_out=None, **later))
    assert "hk_solve: null state pointer" in reason(solve(root=None, target=None, root_out=None, **later))
    assert "hk_solve: null state pointer" in reason(solve(dof=None, target=None, root_out=None, **later))
    assert "hk_solve: null target" in reason(solve(target=None, root_out=None, **later))
    assert "hk_solve: null output state" in reason(solve(root_out=None, **later))
    assert "hk_solve: null output state" in reason(solve(dof_out=None, **later))
    assert "hk_solve: unknown flag bits 0x8" in reason(solve(**later))
    assert "unknown flag bits 0x2" in reason(solve(flags=task.FLAG_NO_GRAVITY | 1))
    later.pop("flags")
    assert "hk_solve: iterations = 0 outside 1..64" in reason(solve(**later))
    assert "iterations = 65" in reason(solve(**dict(later, iters=65)))
    later.pop("iters")
    assert "hk_solve: damping" in reason(solve(**later))
    for bad in (nan, inf):
        assert "damping" in reason(solve(**dict(later, damping=bad)))
    later.pop("damping")
    assert "hk_solve: step_clip" in reason(solve(**later))
    for bad in (-0.1, nan, inf):
        assert "step_clip" in reason(solve(**dict(later, clip=bad)))
    later.pop("clip")
    assert "hk_solve: every buffer must be 4-byte aligned" in reason(solve(**later))
    for name in ("root", "dof", "target", "trot", "root_out", "dof_out", "res"):  # every pointer is looked at
        assert "4-byte aligned" in reason(solve(**{name: C.c_void_p(8195)}))
    assert "hk_solve: no rows set" in reason(solve())
    assert block.raw == bytes(4096)  # the stand-in handle was never written
    # rows: hk_set_rows has ht_set_rows' refusals, and an angular row wants target_rot
    rows = lambda *r: task.make_rows(r)  # noqa: E731
    assert "hk_set_rows: null handle" in reason(lib.hk_set_rows(None, *rows((23, 0))))
    assert "hk_set_rows: null row array" in reason(lib.hk_set_rows(fake, None, 1))
    assert "outside 1..32" in reason(lib.hk_set_rows(fake, rows((23, 0))[0], 0))
    assert "outside 1..32" in reason(lib.hk_set_rows(fake, *rows(*[(23, 0)] * 33)))
    assert "body 24" in reason(lib.hk_set_rows(fake, *rows((23, 0), (24, 0))))
    assert "axis 6" in reason(lib.hk_set_rows(fake, *rows((23, 6))))
    assert "not finite" in reason(lib.hk_set_rows(fake, *rows((23, 1, (0.0, nan, 0.0)))))
    assert block.raw == bytes(4096)
    assert lib.hk_set_rows(fake, *rows((23, 0, (0.01, 0.02, 0.03)), (13, 5))) == 0
    good = block.raw
    assert "body -1" in reason(lib.hk_set_rows(fake, *rows((-1, 0)))) and block.raw == good
    assert "hk_solve: row 1 is angular and target_rot is null" in reason(solve())
    assert "4-byte aligned" in reason(solve(res=odd))  # still in front of the rows' checks
    assert lib.hk_set_rows(fake, *rows((23, 0), (13, 2))) == 0
    assert lib.hk_set_rows(fake, *rows((23, 0, (0.01, 0.02, 0.03)), (13, 5))) == 0
    assert block.raw == good  # a second set replaces the first whole
    # a real handle needs a device
    rc = lib.hk_create(0, C.byref(he_model), g, 4, C.byref(h))
    if rc != 0:
        assert "device" in lib.hk_last_error().decode().lower() or "hip" in lib.hk_last_error().decode().lower()
        assert h.value is None
    else:
        assert "no rows set" in reason(lib.hk_solve(h, one, one, one, None, 8, 1e-4, 0.1, two, two, None, 5, None))
        lib.hk_destroy(h)


# ------------------------------------------------------------------ the binding and the facade
class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


class _Engine:
    stream = None

    def __init__(self, n):
        import torch
        self.root_states, self.dof_state = torch.zeros(n, 13), torch.zeros(n * ND, 2)


def test_binding_follows_the_query_binding_rules_and_checks_before_any_call():
    import torch
    from humanoid_amd import dynamics, ik, solve, task
    cls, error = ik.InverseKinematics, ik.IKError
    assert issubclass(cls, _abi.QueryBinding) and cls is not _abi.QueryBinding
    for name in ("__del__", "flags", "_flags", "_states", "_out"):
        assert name not in vars(cls) and hasattr(cls, name), name
    assert cls.LIBRARY.prefix == "hk" and cls.LIBRARY.error_cls is error and cls.LIBRARY.path == task.LIB_PATH
    assert cls.LIBRARY.prototypes is ik.HK_PROTOTYPES and cls.LIBRARY is not task.TaskSpace.LIBRARY
    assert cls.NO_CPU_PATH.endswith("no CPU path") and ik.HK_SYMBOLS == tuple(ik.HK_PROTOTYPES)
    assert issubclass(error, RuntimeError) and error.__module__ == ik.__name__
    assert ik.make_rows is task.make_rows

    n = 3
    o = object.__new__(cls)
    o.lib, o.h, o.engine = _NoCalls(), None, _Engine(n)
    o.device, o.num_envs, o.armature, o.gravity, o.num_rows, o.angular = torch.device("cpu"), n, True, True, 0, False
    tgt = torch.zeros(n, 6)
    with pytest.raises(error, match="no rows set") as e:
        o.solve(tgt)
    assert not isinstance(e.value, (dynamics.DynamicsError, solve.SolveError, task.TaskError))
    o.num_rows, o.angular = 6, True
    for bad in (0, 65):
        with pytest.raises(error, match="iterations"):
            o.solve(tgt, iterations=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(error, match="damping"):
            o.solve(tgt, damping=bad)
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(error, match="step_clip"):
            o.solve(tgt, step_clip=bad)
    with pytest.raises(error, match="target:"):
        o.solve(torch.zeros(n, 5))
    with pytest.raises(error, match="target_rot is None"):
        o.solve(tgt)
    trot = torch.zeros(n, NB, 4)
    with pytest.raises(error, match="target_rot:"):
        o.solve(tgt, torch.zeros(n, NB, 3))
    with pytest.raises(error, match="root_out:"):
        o.solve(tgt, trot, root_out=torch.zeros(n, 12))
    with pytest.raises(error, match="dof_out:"):
        o.solve(tgt, trot, dof_out=torch.zeros(n, ND, 2))
    with pytest.raises(error, match="residual:"):
        o.solve(tgt, trot, residual=torch.zeros(n, 7))
    # an output that is, or lies inside, the engine's live state is refused
    with pytest.raises(error, match="root_out aliases the engine's state"):
        o.solve(tgt, trot, root_out=o.engine.root_states)
    with pytest.raises(error, match="dof_out aliases the engine's state"):
        o.solve(tgt, trot, dof_out=o.engine.dof_state.view(n * ND, 2))
    with pytest.raises(error, match="root_state:"):
        o.solve(tgt, trot, root_state=torch.zeros(n, 12))
    # everything passes: the library is reached (and here stands for the failure)
    with pytest.raises(AssertionError, match="library call hk_solve"):
        o.solve(tgt, trot)


def test_dynamics_creates_its_ik_object_on_first_use_and_hands_over_armature():
    from humanoid_amd import dynamics
    assert isinstance(dynamics.Dynamics.ik, property)

    class _Ik:
        armature = None

    d = object.__new__(dynamics.Dynamics)
    d.armature, d.gravity = False, True
    d._ik = _Ik()
    assert d.ik is d._ik and d._ik.armature is False


def test_facade_ik_calls_before_prepare_sim_raise():
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    with pytest.raises(RuntimeError, match="set_ik_rows before prepare_sim"):
        gym.set_ik_rows(sim, [("R_Hand", 0)])
    with pytest.raises(RuntimeError, match="solve_inverse_kinematics before prepare_sim"):
        gym.solve_inverse_kinematics(sim, None, None, None)
    assert sim.dynamics is None
    assert "set_ik_rows" in gymapi.__doc__ and "solve_inverse_kinematics" in gymapi.__doc__


# ------------------------------------------------------------------ the reference against its pins
@pytest.fixture(scope="module")
def ref(he_model):
    """Three starts and goals of the convergence inputs, the row sets, per set the targets (left unchanged)."""
    names = list(BODY_NAMES)
    root, dof, g_root, g_dof = IK.convergence_inputs(he_model, 3, 5)
    sets = dict(IK.convergence_rows(names))
    assert sorted(sets) == [6, 9, 12, 15] and all(len(r) == k for k, r in sets.items())
    targets = {k: IK.targets_of(he_model, g_root, g_dof, rows) for k, rows in sets.items()}
    lo, up = IK.limits_of(he_model, np.float32)
    assert (dof[..., 0] >= lo).all() and (dof[..., 0] <= up).all()
    return dict(root=root, dof=dof, sets=sets, targets=targets, n=3, lo=lo, up=up)


def test_the_rotation_helpers_invert_each_other():
    rng = np.random.default_rng(3)
    for dt, tol in ((np.float64, 1e-15), (np.float32, 4e-7)):
        for scale in (0.0, 1e-9, 3e-4, 9.9e-4, 1.1e-3, 0.1, 1.0, 3.0):
            v = (rng.normal(size=3) * scale / np.sqrt(3)).astype(dt)
            back = IK.quat_rotvec(IK.quat_exp(v, dt))
            assert back.dtype == dt and np.abs(back - v).max() <= tol * max(1.0, scale), (dt, scale)
            R = DR._exp(v.astype(np.float64), np.float64)
            assert np.abs(IK.quat_rotvec(IK.matrix_quat(R)) - v).max() < 1e-6 + 1e-12 / max(scale, 1e-3)
    # every branch of the matrix's quaternion, against the quaternion it came from (up to sign)
    for axis in np.eye(3):
        for angle in (0.5, 2.0, 3.1, np.pi):
            q = IK.quat_exp(axis * angle + 0.01, np.float64)
            got = IK.matrix_quat(DR._qmat(q, np.float64))
            assert min(np.abs(got - q).max(), np.abs(got + q).max()) < 1e-14
    # the angle is in [0, pi]
    v = np.array([0.0, 0.0, 4.0])
    assert np.allclose(IK.quat_rotvec(IK.quat_exp(v, np.float64)), [0.0, 0.0, 4.0 - 2 * np.pi])


def test_an_undamped_step_meets_the_errors_with_the_least_kinetic_energy(he_model, ref):
    """damping = 0 and a clip that does not bind: J dq = e to 1e-10, and dq^T M dq is not larger than that of
    dq + n for random n with J n = 0."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for k, rows in ref["sets"].items():
        tgt, trot = ref["targets"][k]
        e = IK.row_errors(he_model, ref["root"], ref["dof"], rows, tgt, trot)
        assert 0.01 < np.abs(e).max() < 1.0
        dq, t = IK.step(he_model, ref["root"], ref["dof"], rows, e, 0.0)
        worst = max(worst, np.abs(np.einsum("ekc,ec->ek", t.J, dq) - e).max())
        for i in range(ref["n"]):
            J, M = t.J[i], t.M[i]
            for _ in range(4):
                nv = rng.normal(size=NG)
                nv -= np.linalg.pinv(J) @ (J @ nv)
                assert np.abs(J @ nv).max() < 1e-10
                assert (dq[i] + nv) @ M @ (dq[i] + nv) >= dq[i] @ M @ dq[i]
    print("worst |J dq - e|:", worst)
    assert worst < 1e-10


def test_the_integration_agrees_with_the_jacobian(he_model, ref):
    """FK(q + eps dq) - FK(q) = eps J dq + O(eps^2) on all 24 bodies, origins and rotations (the rotation's
    change as the rotation vector of R' R^T, which the angular rows of J give): at eps = 1e-3 and 1e-4 the
    remainder over eps^2 stays bounded and equal, so it is the second-order term and no first-order one. A
    root rate applied in the body frame, or a joint rate on the left, leaves a first-order remainder."""
    Mo = DR.Model(he_model, np.float64)
    rng = np.random.default_rng(9)
    ratios = {}
    for eps in (1e-3, 1e-4):
        worst_p = worst_r = 0.0
        rng = np.random.default_rng(9)
        for i in range(ref["n"]):
            root, dof = ref["root"][i].astype(np.float64), ref["dof"][i].astype(np.float64)
            dq = rng.uniform(-1.0, 1.0, NG)
            R, p = IK.fk_pose(Mo, root[:3], root[3:7], dof[:, 0])
            R0, p0 = DR.fk(Mo, ref["root"][i], ref["dof"][i])
            assert np.array_equal(R, R0) and np.array_equal(p, p0)
            Jb = DR.jacobian(Mo, R, p)
            r2, d2 = IK.integrate(root, dof, eps * dq, np.float64)
            assert not r2[7:].any() and not d2[:, 1].any() and abs(r2[3:7] @ r2[3:7] - 1) < 1e-15
            R2, p2 = IK.fk_pose(Mo, r2[:3], r2[3:7], d2[:, 0])
            for b in range(NB):
                worst_p = max(worst_p, np.abs(p2[b] - p[b] - eps * Jb[b, :3] @ dq).max())
                rot = IK.quat_rotvec(IK.matrix_quat(R2[b] @ R[b].T))
                worst_r = max(worst_r, np.abs(rot - eps * Jb[b, 3:] @ dq).max())
        ratios[eps] = (worst_p / eps ** 2, worst_r / eps ** 2)
    print("remainder / eps^2 (positions, rotations):", ratios)
    # a first-order term c eps would make the two quotients differ by 9000 c; the third-order one moves them by
    # a part in a thousand (eps times a ratio of derivatives of order one)
    for a, b in zip(ratios[1e-3], ratios[1e-4]):
        assert a > 0 and abs(a / b - 1) < 0.05


def test_a_binding_limit_is_met_exactly(he_model, ref):
    k = 9
    rows = ref["sets"][k]
    tgt, trot = ref["targets"][k]
    lo, up = ref["lo"].copy(), ref["up"].copy()
    free = IK.solve(he_model, ref["root"], ref["dof"], rows, tgt, trot, 2, limits=False)
    moved = np.abs(free[1][..., 0] - ref["dof"][..., 0]).max(axis=0)
    d = int(np.argmax(moved))  # the dof the unconstrained iteration moves most
    assert moved[d] > 0.02
    import copy
    m = copy.deepcopy(he_model)
    # a box of 5 mrad about every env's start: the move leaves it
    start = ref["dof"][:, d, 0]
    m.dof_lower[d], m.dof_upper[d] = float(start.min() - 0.005), float(start.max() + 0.005)
    lo32, up32 = IK.limits_of(m, np.float32)
    held = IK.solve(m, ref["root"], ref["dof"], rows, tgt, trot, 2, limits=True)
    loose = IK.solve(m, ref["root"], ref["dof"], rows, tgt, trot, 2, limits=False)
    assert np.array_equal(loose[1], free[1])
    th = held[1][:, d, 0]
    assert ((th == lo32[d]) | (th == up32[d])).any() and (th >= lo32[d]).all() and (th <= up32[d]).all()
    assert ((loose[1][:, d, 0] > up32[d]) | (loose[1][:, d, 0] < lo32[d])).any()
    assert (held[1][..., 0] >= lo32).all() and (held[1][..., 0] <= up32).all()


def test_eight_iterations_reach_the_storage_floor(he_model, ref):
    """8 iterations, damping 1e-4, step_clip 0.1 from targets up to 0.05 m and 0.15 rad per dof away: the float64
    reference's worst residual is at most 1e-6 (m or rad) on every row set, and the reported residual is
    the error at the returned pose."""
    worst = {}
    for k, rows in ref["sets"].items():
        tgt, trot = ref["targets"][k]
        e0 = IK.row_errors(he_model, ref["root"], ref["dof"], rows, tgt, trot)
        root, dof, res = IK.solve(he_model, ref["root"], ref["dof"], rows, tgt, trot, 8, 1e-4, 0.1)
        assert root.dtype == np.float32 and dof.dtype == np.float32 and res.dtype == np.float64
        assert not root[:, 7:].any() and not dof[..., 1].any()
        assert np.abs(np.linalg.norm(root[:, 3:7].astype(np.float64), axis=1) - 1).max() < 1e-6
        assert np.array_equal(res, IK.row_errors(he_model, root, dof, rows, tgt, trot))
        assert (dof[..., 0] >= ref["lo"]).all() and (dof[..., 0] <= ref["up"]).all()
        worst[k] = np.abs(res).max()
        assert np.abs(e0).max() > 0.1
    print("worst residual after 8 iterations:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-6


def test_the_step_clip_bounds_a_step(he_model, ref):
    k = 9  # linear rows: a large orientation error's components do not fall at the rate of the angular velocity
    rows = ref["sets"][k]
    tgt, trot = ref["targets"][k]
    e0 = IK.row_errors(he_model, ref["root"], ref["dof"], rows, tgt, trot)
    big = np.abs(e0) > 0.05
    assert big.any()
    # a clipped row moves by its clip to first order (J dq = eb, undamped): what is left of it is |e0| - clip up
    # to the step's curvature, which is second order in the clip: a tenth of the clip leaves a hundredth of it
    # (held to a fiftieth), and at the smaller clip the first-order term stands out tenfold
    rem = {}
    for clip in (0.02, 0.002):
        _, _, e1 = IK.solve(he_model, ref["root"], ref["dof"], rows, tgt, trot, 1, 0.0, clip, limits=False)
        rem[clip] = np.abs(np.abs(e0[big]) - np.abs(e1[big]) - clip).max()
    print("remainder of a clipped step:", rem)
    assert rem[0.002] < rem[0.02] / 50 and rem[0.002] < 0.1 * 0.002
