"""CPU checks of task-space control (include/humanoid_task.h): the library's header, symbols, build lists
and refusals, the binding's checks, and the numpy reference of tests/task_reference.py (the yardstick of
tests/test_gpu_task.py) against its pins: Jdot qd as a finite difference of J qd along the configuration
flow, the task equation J qdd + b = xdd_des in both modes, the modes' defining properties and the
null-space projection of a posture force. The kernel itself is checked on the GPU (test_gpu_task.py).

The refusals that a handle must get past its null check are sent with a stand-in handle, a zeroed block
of memory: every entry point checks its arguments before it reads the handle, and a zeroed handle is one
without rows."""
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
import solve_reference as SR  # noqa: E402
import task_reference as TR  # noqa: E402

from humanoid_amd import _abi  # noqa: E402
from humanoid_amd.body_sets import BODY_NAMES  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_task.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG


def _lib():
    from humanoid_amd import build, task
    if not os.path.exists(task.LIB_PATH):
        build.build()
    return task.load_library()


# ------------------------------------------------------------------ header, symbols, build lists
def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import task
    src = tmp_path / "ht.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "humanoid_task.h"\n'
                   'int main(void){printf("%u %u %u %u %d %d %d %d %d %d %d\\n", HT_FLAG_ARMATURE, HT_FLAG_NO_GRAVITY, '
                   "HT_FLAGS_DEFAULT, HT_FLAGS_ALL, HT_MAX_ROWS, HT_MODE_FORCE, HT_MODE_JOINT, HE_NUM_GEN, "
                   "(int)sizeof(ht_row), (int)offsetof(ht_row, axis), (int)offsetof(ht_row, point)); return 0;}\n")
    exe = tmp_path / "ht"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [task.FLAG_ARMATURE, task.FLAG_NO_GRAVITY, task.FLAGS_DEFAULT, task.FLAG_ARMATURE | task.FLAG_NO_GRAVITY,
                   task.MAX_ROWS, task.MODE_FORCE, task.MODE_JOINT, task.NG, C.sizeof(task.HtRow), task.HtRow.axis.offset,
                   task.HtRow.point.offset]
    assert (task.MAX_ROWS, task.MODE_FORCE, task.MODE_JOINT) == (TR.MAX_ROWS, TR.MODE_FORCE, TR.MODE_JOINT)
    # the flags mean what they mean in the dynamics and solve headers
    from humanoid_amd import dynamics, solve
    assert (task.FLAG_ARMATURE, task.FLAG_NO_GRAVITY) == (solve.FLAG_ARMATURE, solve.FLAG_NO_GRAVITY) == \
        (dynamics.FLAG_ARMATURE, dynamics.FLAG_NO_GRAVITY)


def test_task_library_exports_exactly_the_declared_symbols():
    from humanoid_amd import task
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ht_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 8
    assert set(syms) == set(task.HT_PROTOTYPES) == set(task.HT_SYMBOLS)
    assert not [s for s in syms if not hasattr(lib, s)]
    assert lib.ht_version() == 1
    # the other libraries' header scans must not pick anything up from this header
    assert not re.findall(r"\bh[edrs]_[a-z_0-9]+\s*\(", text)
    nm = subprocess.run(["nm", "-D", "--defined-only", task.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert not [s for s in exported if re.match(r"h[edrs]_", s)]
    assert {s for s in exported if s.startswith("ht_")} == set(task.HT_PROTOTYPES)


def test_task_library_is_an_extension_library_of_its_own():
    from humanoid_amd import build
    # one entry of the one table, its sources ht_task.hip alone; no other library lists an ht_ source
    libs = build.LIBRARIES
    assert [s for s, _ in libs["task"].sources] == ["ht_task.hip"]
    assert [name for name, lib in libs.items() if any(s.startswith("ht_") for s, _ in lib.sources)] == ["task"]
    assert len({lib.path for lib in libs.values()}) == len(libs) == 6
    assert dict(libs["task"].sources)["ht_task.hip"] == dict(libs["solve"].sources)["hs_solve.hip"] == ["-fno-slp-vectorize"]
    assert any(h.endswith("humanoid_task.h") for h in build.HEADERS)
    assert any(h.endswith("he_joint_space.h") for h in build.HEADERS)
    assert build.BUDGETS["ht_task.hip"] == {"task_kernel": build.Budget(min_waves=2, max_scratch=0)}
    # the compile line follows the others' rules: the common flags, an id from the file name, the source's flags
    import hashlib
    cmd = build.compile_command("ht_task.hip")
    assert "-cuid=" + hashlib.md5(b"ht_task.hip").hexdigest()[:16] in cmd and "-fno-slp-vectorize" in cmd
    assert cmd[-4:] == ["-c", os.path.join(build.CSRC, "ht_task.hip"), "-o", os.path.join(build.BUILD, "ht_task.hip.o")]
    build.build()
    ids = {build.device_code_id(libs[n].path) for n in ("engine", "render", "dynamics", "solve", "task")}
    assert len(ids) == 5
    # the shared header is included, not copied
    solve_src = open(os.path.join(build.CSRC, "hs_solve.hip")).read()
    task_src = open(os.path.join(build.CSRC, "ht_task.hip")).read()
    for src in (solve_src, task_src):
        assert '#include "he_joint_space.h"' in src and "struct Lds" not in src and "void crba_row" not in src


# ------------------------------------------------------------------ refusals, no GPU
def _rows(*rows):
    from humanoid_amd import task
    return task.make_rows(rows)


def test_refusals_are_reported_without_gpu(he_model):
    from humanoid_amd import task
    lib = _lib()
    g = (C.c_float * 3)(0.0, 0.0, -9.81)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.ht_last_error().decode()

    # creation and the model check, as the solve library's
    assert "num_envs" in reason(lib.ht_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "null output" in reason(lib.ht_create(0, C.byref(he_model), g, 4, None))
    assert "gravity" in reason(lib.ht_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.ht_create(0, None, g, 4, C.byref(h)))
    assert lib.ht_validate_model(C.byref(he_model)) == 0
    task.validate_model(he_model)
    import copy
    m = copy.deepcopy(he_model)
    m.num_bodies = 23
    assert "bodies" in reason(lib.ht_validate_model(C.byref(m)))
    with pytest.raises(task.TaskError):
        task.validate_model(m)
    m = copy.deepcopy(he_model)
    m.parents[5] = 1  # a valid DFS tree, but not the one the factorisation is unrolled for
    assert "unrolled" in reason(lib.ht_validate_model(C.byref(m)))
    assert lib.ht_destroy(None) == 0

    # null handles
    one, two = C.c_void_p(4096), C.c_void_p(8192)  # never dereferenced: every call below is refused first
    arr, k = _rows((23, 0))
    assert "ht_set_rows: null handle" in reason(lib.ht_set_rows(None, arr, k))
    assert "ht_task_terms: null handle" in reason(lib.ht_task_terms(None, one, one, None, one, None, None, None, None, 1, None))
    assert "ht_task_control: null handle" in reason(
        lib.ht_task_control(None, one, one, one, None, 0, 0.0, one, None, None, 1, None))

    # a stand-in handle: zeroed memory, which is a handle without rows
    block = C.create_string_buffer(4096)
    fake = C.cast(block, C.c_void_p)
    terms = lambda *a: lib.ht_task_terms(fake, *a)  # noqa: E731
    control = lambda *a: lib.ht_task_control(fake, *a)  # noqa: E731
    assert "state pointer" in reason(terms(None, one, None, two, None, None, None, None, 1, None))
    assert "state pointer" in reason(terms(one, None, None, two, None, None, None, None, 1, None))
    assert "no output" in reason(terms(one, one, None, None, None, None, None, None, 1, None))
    assert "unknown flag" in reason(terms(one, one, None, two, None, None, None, None, 4, None))
    assert "4-byte aligned" in reason(terms(one, one, None, C.c_void_p(8194), None, None, None, None, 1, None))
    assert "4-byte aligned" in reason(terms(one, one, C.c_void_p(4097), two, None, None, None, None, 1, None))
    assert "no rows set" in reason(terms(one, one, None, two, None, None, None, None, 1, None))
    assert "state pointer" in reason(control(None, one, one, None, 0, 0.0, two, None, None, 1, None))
    assert "desired acceleration" in reason(control(one, one, None, None, 0, 0.0, two, None, None, 1, None))
    assert "no output" in reason(control(one, one, one, None, 0, 0.0, None, None, None, 1, None))
    assert "unknown flag" in reason(control(one, one, one, None, 0, 0.0, two, None, None, 8, None))
    assert "unknown mode" in reason(control(one, one, one, None, 2, 0.0, two, None, None, 1, None))
    assert "unknown mode" in reason(control(one, one, one, None, -1, 0.0, two, None, None, 1, None))
    for bad in (-1e-3, float("nan"), float("inf")):
        assert "damping" in reason(control(one, one, one, None, 0, bad, two, None, None, 1, None))
    assert "4-byte aligned" in reason(control(one, one, one, None, 1, 0.0, None, C.c_void_p(8195), None, 1, None))
    assert "no rows set" in reason(control(one, one, one, None, 1, 0.5, None, None, two, 1, None))

    # ht_set_rows: each refusal leaves the handle as it was (still without rows, then with the good set)
    def refused(word, *rows, k=None):
        arr, n = _rows(*rows)
        assert word in reason(lib.ht_set_rows(fake, arr, n if k is None else k))

    def check_refusals():
        assert "null row array" in reason(lib.ht_set_rows(fake, None, 1))
        refused("outside 1..32", (23, 0), k=0)
        refused("outside 1..32", *[(23, 0)] * 33)
        refused("body 24", (23, 0), (24, 0))
        refused("body -1", (-1, 0))
        refused("axis 6", (23, 6))
        refused("axis -1", (0, 0), (0, 1), (23, -1))
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("not finite", (23, 0), (23, 1, (0.0, bad, 0.0)))

    check_refusals()
    assert "no rows set" in reason(terms(one, one, None, two, None, None, None, None, 1, None))
    before = block.raw
    assert lib.ht_set_rows(fake, *_rows((23, 0, (0.01, 0.02, 0.03)), (13, 5))) == 0
    good = block.raw
    assert good != before
    check_refusals()
    assert block.raw == good  # nothing changed
    # a second set replaces the first whole: the same bytes as on a fresh handle
    assert lib.ht_set_rows(fake, *_rows((23, 0, (0.5, 0.5, 0.5)), (13, 5), (2, 2, (1.0, 1.0, 1.0)))) == 0
    assert lib.ht_set_rows(fake, *_rows((23, 0, (0.01, 0.02, 0.03)), (13, 5))) == 0
    assert block.raw == good
    # a real handle needs a device
    rc = lib.ht_create(0, C.byref(he_model), g, 4, C.byref(h))
    if rc != 0:
        assert "device" in lib.ht_last_error().decode().lower() or "hip" in lib.ht_last_error().decode().lower()
    else:
        assert "no rows set" in reason(lib.ht_task_terms(h, one, one, None, two, None, None, None, None, 1, None))
        lib.ht_destroy(h)


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


class _NoEngine:
    stream = None

    def __getattr__(self, name):
        raise AssertionError(f"engine attribute {name} read before the argument check")


def test_binding_checks_before_any_library_call():
    import torch
    from humanoid_amd import task
    n = 3
    t = object.__new__(task.TaskSpace)
    t.lib, t.h, t.engine = _NoCalls(), None, _NoEngine()
    t.device, t.num_envs, t.armature, t.gravity, t.num_rows = torch.device("cuda", 0), n, True, True, 0
    assert t.flags == task.FLAG_ARMATURE
    t.armature, t.gravity = False, False
    assert t.flags == task.FLAG_NO_GRAVITY
    with pytest.raises(task.TaskError, match="no rows set"):
        t.terms()
    with pytest.raises(task.TaskError, match="no rows set"):
        t.control(torch.zeros(n, 6))
    t.num_rows = 6
    with pytest.raises(task.TaskError, match="unknown output"):
        t.terms(want=("jacobian",))
    with pytest.raises(task.TaskError, match="no output"):
        t.terms(want=())
    with pytest.raises(task.TaskError, match="gen_force"):
        t.terms(torch.zeros(n, NG))  # a CPU tensor
    with pytest.raises(task.TaskError, match="lambda_inv"):
        t.terms(want=(), out={"lambda_inv": torch.zeros(n, 6, 6)})
    with pytest.raises(task.TaskError, match="xdd_des"):
        t.control(torch.zeros(n, 6))
    with pytest.raises(task.TaskError, match="unknown mode"):
        t.control(torch.zeros(n, 6), mode="torque")
    with pytest.raises(task.TaskError, match="damping"):
        t.control(torch.zeros(n, 6), damping=-1.0)
    with pytest.raises(task.TaskError, match="damping"):
        t.control(torch.zeros(n, 6), damping=float("nan"))
    with pytest.raises(task.TaskError, match="no output"):
        t.control(torch.zeros(n, 6), want_gen_force=False, want_task_force=False, want_qdd=False)
    # rows: names resolve, malformed rows are refused here
    arr, k = task.make_rows([("R_Hand", 0), ("Head", 5, (0.1, 0.0, 0.0)), (3, 4)])
    assert k == 3 and [(r.body, r.axis) for r in arr] == [(BODY_NAMES.index("R_Hand"), 0), (BODY_NAMES.index("Head"), 5), (3, 4)]
    assert abs(arr[1].point[0] - 0.1) < 1e-8
    for bad, word in (([("R_Paw", 0)], "no body named"), ([(1, 2, (0.0, 1.0))], "components"), ([(1,)], "expected")):
        with pytest.raises(task.TaskError, match=word):
            task.make_rows(bad)


def test_dynamics_hands_its_settings_to_a_lazily_created_task_space():
    from humanoid_amd import dynamics

    class _Task:
        armature, gravity = None, None

    d = object.__new__(dynamics.Dynamics)
    d.armature, d.gravity = False, True
    d._task = _Task()
    assert d.task is d._task and (d._task.armature, d._task.gravity) == (False, True)
    d.armature, d.gravity = True, False
    assert (d.task.armature, d.task.gravity) == (True, False)


def test_facade_task_calls_before_prepare_sim_raise():
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    with pytest.raises(RuntimeError, match="set_task_rows before prepare_sim"):
        gym.set_task_rows(sim, [("R_Hand", 0)])
    with pytest.raises(RuntimeError, match="solve_task_space before prepare_sim"):
        gym.solve_task_space(sim, None, None)
    assert sim.dynamics is None
    assert "set_task_rows" in gymapi.__doc__ and "solve_task_space" in gymapi.__doc__


# ------------------------------------------------------------------ the reference against its pins
@pytest.fixture(scope="module")
def ref(he_model):
    """The five states of the GPU tests, the six row sets, float64 terms per set (computed once, left
    unchanged), and per set a desired acceleration, a generalised force and a posture force."""
    root, dof = TR.five_states()
    g = tuple(_abi.default_sim_params().gravity)
    sets = TR.row_sets(list(BODY_NAMES))
    assert sorted(sets) == [1, 6, 12, 30, 31, 32] and all(len(r) == k for k, r in sets.items())
    rng = np.random.default_rng(23)
    n = root.shape[0]
    terms = {k: TR.evaluate(he_model, root, dof, rows, g, np.float64) for k, rows in sets.items()}
    xdd = {k: rng.uniform(-5.0, 5.0, (n, k)) for k in sets}
    f = np.concatenate([np.zeros((n, 6)), rng.uniform(-100.0, 100.0, (n, ND))], axis=1)
    u0 = np.concatenate([np.zeros((n, 6)), rng.uniform(-30.0, 30.0, (n, ND))], axis=1)
    return dict(root=root, dof=dof, g=g, sets=sets, terms=terms, xdd=xdd, f=f, u0=u0, n=n,
                parents=np.array(he_model.parents[:NB]))


def test_row_jacobians_follow_the_header(he_model, ref):
    """J_r is exactly zero off the body's ancestor chain; a zero point gives the body Jacobian's own row; J_r qd
    is the point's velocity component, v_body + w_body x (R_body point), from the body's own velocity."""
    Mo = DR.Model(he_model, np.float64)
    for k, rows in ref["sets"].items():
        t = ref["terms"][k]
        mask = TR.pattern(ref["parents"], rows)
        assert not (t.J[:, ~mask] != 0.0).any()
        assert (np.abs(t.J[1:])[:, mask] > 0).mean() > 0.5
    t = ref["terms"][12]
    assert np.abs(t.J[:, :, 72:]).max() > 0.01  # the hand's own columns: the register tail is exercised
    rows = ref["sets"][12] + ref["sets"][6]
    for e in range(1, ref["n"]):
        R, p = DR.fk(Mo, ref["root"][e], ref["dof"][e])
        Jb = DR.jacobian(Mo, R, p)
        qd = DR.gen_velocity(ref["root"][e], ref["dof"][e], np.float64)
        Jr = TR.task_jacobian(Mo, R, Jb, rows)
        for r, (body, axis, point) in enumerate(rows):
            v, w = Jb[body, :3] @ qd, Jb[body, 3:] @ qd
            want = w[axis - 3] if axis >= 3 else (v + np.cross(w, R[body] @ np.asarray(point, np.float32).astype(np.float64)))[axis]
            assert abs(Jr[r] @ qd - want) < 1e-12
            if not any(point):
                assert np.array_equal(Jr[r], Jb[body, axis])


def test_bias_acceleration_is_the_derivative_of_j_qd(he_model, ref):
    """b = Jdot qd against a central difference of J(q) qd along the configuration flow at constant qd: the
    root advanced by its velocities, R_b <- R_b exp([h u_b]x) for every joint. float64, h = 1e-5: the
    truncation is h^2 |x'''| / 6 (1e-10 of accelerations of a few m/s^2 built on rates of ~1 rad/s) and the
    rounding 1e-16 |J qd| / h = 1e-11; held to 1e-7 of the largest |b|."""
    Mo = DR.Model(he_model, np.float64)
    h = 1e-5
    rows = ref["sets"][12] + ref["sets"][32]  # offset points, angular rows, pelvis rows
    worst = 0.0
    for e in range(1, ref["n"]):
        root, dof = ref["root"][e], ref["dof"][e]
        qd = DR.gen_velocity(root, dof, np.float64)
        R, p = DR.fk(Mo, root, dof)
        b = TR.bias_acceleration(Mo, R, p, root, dof, rows)

        def jqd(s):
            R2, p2 = np.zeros_like(R), np.zeros_like(p)
            R2[0] = DR._exp(s * h * qd[3:6], np.float64) @ R[0]
            p2[0] = p[0] + s * h * qd[0:3]
            for bb in range(1, NB):
                a = Mo.parents[bb]
                Rl = R[a].T @ R[bb]  # the joint's rotation
                R2[bb] = R2[a] @ Rl @ DR._exp(s * h * qd[6 + 3 * (bb - 1):9 + 3 * (bb - 1)], np.float64)
                p2[bb] = p2[a] + R2[a] @ Mo.local_pos[bb]
            return TR.task_jacobian(Mo, R2, DR.jacobian(Mo, R2, p2), rows) @ qd

        fd = (jqd(+1) - jqd(-1)) / (2 * h)
        worst = max(worst, np.abs(fd - b).max() / np.abs(b).max())
        assert np.abs(b).max() > 0.5
    print("Jdot qd against the central difference, relative:", worst)
    assert worst < 1e-7
    # at rest nothing is left
    R, p = DR.fk(Mo, ref["root"][0], ref["dof"][0])
    assert not TR.bias_acceleration(Mo, R, p, ref["root"][0], ref["dof"][0], rows).any()


@pytest.mark.parametrize("mode", [TR.MODE_FORCE, TR.MODE_JOINT], ids=["force", "joint"])
def test_undamped_control_reaches_the_desired_acceleration(ref, mode):
    """lambda = 0: J qdd + b = xdd_des to 1e-9, every row set, with and without a generalised force; cond(A)
    stays below 1e6 (the GPU tests' precondition), at most 1.1e4 / 3.2e5 on the zero-offset sets."""
    worst, conds = 0.0, {}
    for k in ref["sets"]:
        t = ref["terms"][k]
        Y, Li, _ = TR.task_terms(t)
        conds[k] = max(np.linalg.cond(a) for a in TR.system_matrix(t, Y, Li, mode, 0.0))
        assert conds[k] < 1e6
        for f in (None, ref["f"]):
            u, F, qdd = TR.task_control(t, ref["xdd"][k], f, mode)
            worst = max(worst, np.abs(TR.task_acceleration(t, qdd) - ref["xdd"][k]).max())
            if mode == TR.MODE_JOINT:
                assert not u[:, :6].any()
    print("cond(A) per row set:", {k: f"{v:.2e}" for k, v in conds.items()}, " worst |J qdd + b - xdd_des|:", worst)
    assert max(v for k, v in conds.items() if k != 12) <= (1.1e4 if mode == TR.MODE_FORCE else 3.2e5) * 1.05
    assert worst < 1e-9


def test_force_mode_is_the_operational_space_force(ref):
    """u = J^T (J M^-1 J^T)^-1 r by numpy's own inverse, and it is the minimum of u^T M^-1 u among the forces
    that reach xdd_des: any other solution u + n, with J M^-1 n = 0, costs more."""
    rng = np.random.default_rng(2)
    for k in (6, 30):
        t = ref["terms"][k]
        u, F, _ = TR.task_control(t, ref["xdd"][k], ref["f"], TR.MODE_FORCE)
        for e in range(ref["n"]):
            Mi = np.linalg.inv(t.M[e])
            J = t.J[e]
            r = ref["xdd"][k][e] - (J @ Mi @ (ref["f"][e] - t.c[e]) + t.b[e])
            want = J.T @ np.linalg.solve(J @ Mi @ J.T, r)
            assert np.abs(u[e] - want).max() <= 1e-9 * np.abs(want).max()
            nvec = rng.normal(size=NG)
            nvec -= J.T @ np.linalg.solve(J @ Mi @ J.T, J @ Mi @ nvec)  # J M^-1 n = 0
            assert np.abs(J @ Mi @ nvec).max() < 1e-9
            assert (u[e] + nvec) @ Mi @ (u[e] + nvec) > u[e] @ Mi @ u[e]


def test_joint_mode_is_the_least_norm_joint_torque(ref):
    """u[:6] is exactly 0, u[6:] lies in the row space of Yj (so it is the least-norm solution of
    Yj tau = r), and it reaches r."""
    for k in (6, 30):
        t = ref["terms"][k]
        Y, _, free = TR.task_terms(t, ref["f"])
        u, F, _ = TR.task_control(t, ref["xdd"][k], ref["f"], TR.MODE_JOINT)
        assert not u[:, :6].any()
        for e in range(ref["n"]):
            Yj = Y[e][:, 6:]
            coef = np.linalg.lstsq(Yj.T, u[e, 6:], rcond=None)[0]
            assert np.abs(Yj.T @ coef - u[e, 6:]).max() <= 1e-9 * np.abs(u[e]).max()
            assert np.abs(Yj @ u[e, 6:] - (ref["xdd"][k][e] - free[e])).max() < 1e-9
            want = np.linalg.pinv(Yj) @ (ref["xdd"][k][e] - free[e])
            assert np.abs(want - u[e, 6:]).max() <= 1e-7 * np.abs(want).max()


def test_damping_is_added_to_the_diagonal_as_given(ref):
    t = ref["terms"][6]
    Y, Li, free = TR.task_terms(t)
    for mode in (TR.MODE_FORCE, TR.MODE_JOINT):
        A0 = TR.system_matrix(t, Y, Li, mode, 0.0)
        lam = 1e-2 * np.median(np.diagonal(A0, axis1=1, axis2=2))
        A = TR.system_matrix(t, Y, Li, mode, lam)
        assert np.allclose(A - A0, lam * np.eye(6)[None], rtol=0, atol=1e-12)
        _, F, _ = TR.task_control(t, ref["xdd"][6], None, mode, lam)
        for e in range(ref["n"]):
            assert np.abs(A[e] @ F[e] - (ref["xdd"][6][e] - free[e])).max() < 1e-9


def test_a_posture_force_inside_gen_force_is_projected_into_the_null_space(ref):
    """u0 + u(f + u0) = u(f) + (1 - J^T Lambda J M^-1) u0: passing the posture force inside gen_force is the
    explicit null-space projection, and the task acceleration is still xdd_des."""
    k = 12
    t = ref["terms"][k]
    f, u0 = ref["f"], ref["u0"]
    u_with, _, qdd = TR.task_control(t, ref["xdd"][k], f + u0, TR.MODE_FORCE)
    u_task, _, _ = TR.task_control(t, ref["xdd"][k], f, TR.MODE_FORCE)
    for e in range(ref["n"]):
        Mi = np.linalg.inv(t.M[e])
        J = t.J[e]
        Nt = np.eye(NG) - J.T @ np.linalg.solve(J @ Mi @ J.T, J @ Mi)
        want = u_task[e] + Nt @ u0[e]
        assert np.abs(u0[e] + u_with[e] - want).max() <= 1e-9 * np.abs(want).max()
        assert np.abs(J @ Mi @ (Nt @ u0[e])).max() < 1e-9  # the projected force does not move the task
    assert np.abs(TR.task_acceleration(t, qdd) - ref["xdd"][k]).max() < 1e-9


def test_float32_floors_are_where_the_tolerances_expect_them(he_model, ref):
    """The floors the GPU tests multiply by 8, on the zero-offset sets: F, u and free_acc between 6e-7 and
    5e-5, relative (so that 8 x a floor is a real check and not a vacuous one)."""
    lo, hi = np.inf, 0.0
    for k in (1, 6, 30, 31, 32):
        t64 = ref["terms"][k]
        t32 = TR.evaluate(he_model, ref["root"], ref["dof"], ref["sets"][k], ref["g"], np.float32)
        x = ref["xdd"][k].astype(np.float32)
        f = ref["f"].astype(np.float32)
        _, _, free64 = TR.task_terms(t64, f)
        _, _, free32 = TR.task_terms(t32, f)
        figs = [SR.forward_error(free32, free64).max()]
        for mode in (TR.MODE_FORCE, TR.MODE_JOINT):
            u64, F64, _ = TR.task_control(t64, x, f, mode)
            u32, F32, _ = TR.task_control(t32, x, f, mode)
            figs += [SR.forward_error(F32, F64).max(), SR.forward_error(u32, u64).max()]
        lo, hi = min(lo, min(figs)), max(hi, max(figs))
    print(f"float32 floors of F, u and free_acc: {lo:.2e} .. {hi:.2e}")
    assert 1e-7 < lo and hi < 5e-5
