"""CPU checks of the joint-reaction queries (include/humanoid_wrench.h): the header, the hw_ symbols and
refusals of libhumanoid_solve.so, the binding, the facade's host-side refusals for force sensors, and the
numpy reference of tests/reaction_reference.py (the yardstick of tests/test_gpu_reaction.py and
tests/test_gpu_force_sensors.py) against pins that do not use its own sums: the header's identities with
dynamics_reference's M, c and J, solve_reference's computed torque, the rest case, the body frame, and a
central finite difference of the bodies' velocities along the state advanced with qdd held. The kernel
itself is checked on the GPU.

Inputs on dynamics_reference.test_states: qdd_des in +-20, base accelerations in +-10, forces in +-200 N and
torques in +-20 N m on every body. Every identity is an equality of float64 expressions that sum the same
terms in another order; its bound is 1e-12 of the largest entry (some thousand roundings of 1.1e-16).

The refusals that a handle must get past its null check are sent with a stand-in handle, a zeroed block of
memory: hw_compute checks its arguments before it reads the handle."""
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
import reaction_reference as RR  # noqa: E402
import solve_reference as SR  # noqa: E402

from humanoid_amd import _abi  # noqa: E402

HEADER = os.path.join(ROOT, "include", "humanoid_wrench.h")
NB, ND, NG = DR.NB, DR.ND, DR.NG
G = (0.0, 0.0, -9.81)
IDENTITY = 1e-12


def _lib():
    from humanoid_amd import build, reaction
    if not os.path.exists(reaction.LIB_PATH):
        build.build()
    return reaction.load_library()


# ------------------------------------------------------------------ header, symbols
def test_header_compiles_as_c_and_constants_match(tmp_path):
    from humanoid_amd import reaction
    src = tmp_path / "hw.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "humanoid_wrench.h"\n'
                   'int main(void){printf("%u %u %u %u %d %d %d %d %d %d %d %d %d\\n", HW_FLAG_ARMATURE, '
                   "HW_FLAG_NO_GRAVITY, HW_FLAGS_DEFAULT, HW_FLAGS_ALL, HW_FRAME_WORLD, HW_FRAME_BODY, HW_WRENCH_ROWS, "
                   "HW_NUM_OUTPUTS, (int)sizeof(hw_outputs), (int)offsetof(hw_outputs, wrench), "
                   "(int)offsetof(hw_outputs, tau), (int)offsetof(hw_outputs, base_acc), "
                   "(int)offsetof(hw_outputs, body_acc)); return 0;}\n")
    exe = tmp_path / "hw"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O = reaction.HwOutputs
    assert out == [reaction.FLAG_ARMATURE, reaction.FLAG_NO_GRAVITY, reaction.FLAGS_DEFAULT,
                   reaction.FLAG_ARMATURE | reaction.FLAG_NO_GRAVITY, reaction.FRAMES["world"], reaction.FRAMES["body"],
                   reaction.WRENCH_ROWS, len(reaction.OUTPUTS), C.sizeof(O), O.wrench.offset, O.tau.offset,
                   O.base_acc.offset, O.body_acc.offset]
    assert [n for n, _ in O._fields_] == list(reaction.OUTPUTS) == ["wrench", "tau", "base_acc", "body_acc"]
    assert (RR.FRAME_WORLD, RR.FRAME_BODY) == (reaction.FRAMES["world"], reaction.FRAMES["body"])


def test_library_exports_every_declared_symbol_and_the_hs_set_is_unchanged():
    from humanoid_amd import reaction, solve
    lib = _lib()  # loads without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(hw_[a-z_0-9]+)\s*\(", text)))
    assert syms == sorted(["hw_last_error", "hw_version", "hw_validate_model", "hw_create", "hw_destroy", "hw_compute"])
    assert set(syms) == set(reaction.HW_PROTOTYPES) == set(reaction.HW_SYMBOLS)
    assert lib.hw_version() == 1
    assert not re.findall(r"\bh[edsrtck]_[a-z_0-9]+\s*\(", text)  # no other family's scan picks this header up
    assert reaction.LIB_PATH == solve.LIB_PATH
    nm = subprocess.run(["nm", "-D", "--defined-only", reaction.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("hw_")} == set(reaction.HW_PROTOTYPES)
    assert {s for s in exported if s.startswith("hs_")} == set(solve.HS_PROTOTYPES)
    assert len(solve.HS_PROTOTYPES) == 8


def test_device_code_is_a_header_of_the_solve_source():
    from humanoid_amd import build
    assert build.LIBRARIES["solve"].sources == [("hs_solve.hip", ["-fno-slp-vectorize"])]
    assert not [f for f in os.listdir(build.CSRC) if f.startswith("hw_")]
    assert '#include "hs_wrench.h"' in open(os.path.join(build.CSRC, "hs_solve.hip")).read()
    assert any(h.endswith("hs_wrench.h") for h in build.HEADERS) and any(h.endswith("humanoid_wrench.h") for h in build.HEADERS)
    assert set(build.BUDGETS["hs_solve.hip"]) == {"solve_kernel", "torque_kernel"}
    # the header the task library shares is not the place of the extension
    assert "body_force" not in open(os.path.join(build.CSRC, "he_joint_space.h")).read()


def test_binding_is_a_query_binding():
    from humanoid_amd import dynamics, reaction
    cls = reaction.Reaction
    assert issubclass(cls, _abi.QueryBinding) and cls is not _abi.QueryBinding
    for name in ("__init__", "__del__", "flags", "_flags", "_states", "_out"):  # the constructor too is the base's
        assert name not in vars(cls) and hasattr(cls, name), name
    assert cls.LIBRARY.prefix == "hw" and cls.LIBRARY.error_cls is reaction.ReactionError
    assert cls.LIBRARY.prototypes is reaction.HW_PROTOTYPES and cls.LIBRARY.path == reaction.LIB_PATH
    assert cls.NO_CPU_PATH.endswith("no CPU path")
    for name in ("LIB_PATH", "load_library", "validate_model", "check_tensor", "HW_PROTOTYPES", "HW_SYMBOLS",
                 "FLAG_ARMATURE", "FLAG_NO_GRAVITY", "FLAGS_DEFAULT", "NG"):
        assert hasattr(reaction, name), name
    assert issubclass(reaction.ReactionError, RuntimeError) and reaction.ReactionError.__module__ == reaction.__name__
    with pytest.raises(reaction.ReactionError, match="x: expected a torch tensor"):
        reaction.check_tensor(None, None, (1,), None, "x")
    assert isinstance(dynamics.Dynamics.reaction, property)
    assert reaction.output_shapes(3) == {"wrench": (3, 24, 6), "tau": (3, 69), "base_acc": (3, 6), "body_acc": (3, 24, 6)}


def test_binding_refuses_before_any_library_call():
    import torch
    from humanoid_amd import reaction

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name} before the argument check")

    class Eng:
        root_states, dof_state = torch.zeros(3, 13), torch.zeros(3 * ND, 2)

    o = object.__new__(reaction.Reaction)
    o.lib, o.h, o.engine = NoCalls(), None, Eng()
    o.device, o.num_envs, o.armature, o.gravity = torch.device("cpu"), 3, True, True
    with pytest.raises(reaction.ReactionError, match="unknown frame"):
        o.compute(frame="joint")
    with pytest.raises(reaction.ReactionError, match="no output asked for"):
        o.compute(wrench=False)
    with pytest.raises(reaction.ReactionError, match="out names"):
        o.compute(out={"torque": torch.zeros(3, ND)})
    with pytest.raises(reaction.ReactionError, match="qdd_des"):
        o.compute(torch.zeros(3, NG))
    with pytest.raises(reaction.ReactionError, match="base_acc"):
        o.compute(None, torch.zeros(3, 5))
    with pytest.raises(reaction.ReactionError, match="body_force"):
        o.compute(body_force=torch.zeros(3, NB, 3))
    with pytest.raises(reaction.ReactionError, match="body_torque"):
        o.compute(body_torque=torch.zeros(3 * NB, 3, dtype=torch.float64))
    with pytest.raises(reaction.ReactionError, match="wrench"):
        o.compute(out={"wrench": torch.zeros(3, NB, 5)})


def test_refusals_in_the_headers_order_without_gpu(he_model):
    import copy
    from humanoid_amd import reaction
    lib = _lib()
    g = (C.c_float * 3)(*G)
    h = C.c_void_p()

    def reason(rc):
        assert rc != 0
        return lib.hw_last_error().decode()

    assert "hw_create: num_envs" in reason(lib.hw_create(0, C.byref(he_model), g, 0, C.byref(h)))
    assert "hw_create: null output" in reason(lib.hw_create(0, C.byref(he_model), g, 4, None))
    assert "hw_create: null gravity" in reason(lib.hw_create(0, C.byref(he_model), None, 4, C.byref(h)))
    assert "null model" in reason(lib.hw_create(0, None, g, 4, C.byref(h)))
    assert h.value is None
    assert lib.hw_validate_model(C.byref(he_model)) == 0
    reaction.validate_model(he_model)
    m = copy.deepcopy(he_model)
    m.parents[5] = 1  # hs_validate_model's refusal: not the tree the library is unrolled for
    assert "unrolled" in reason(lib.hw_validate_model(C.byref(m)))
    with pytest.raises(reaction.ReactionError, match="unrolled"):
        reaction.validate_model(m)
    assert lib.hw_destroy(None) == 0

    one, two, odd = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(8194)
    block = C.create_string_buffer(4096)
    fake = C.cast(block, C.c_void_p)

    def outputs(**kw):
        return reaction.HwOutputs(**{k: v.value for k, v in kw.items()})

    full = outputs(wrench=two, tau=two, base_acc=two, body_acc=two)

    def compute(handle=fake, root=one, dof=one, qdd=one, acc=one, force=one, torque=one, out=full, frame=0, flags=1):
        return lib.hw_compute(handle, root, dof, qdd, acc, force, torque, None if out is None else C.byref(out), frame,
                              flags, None)

    # each refusal with everything after it in the order wrong as well: the earlier one is the one reported
    none = outputs()
    bad_out = outputs(wrench=odd)
    assert "hw_compute: null handle" in reason(compute(handle=None, root=None, out=None, frame=2, flags=4, qdd=odd))
    assert "hw_compute: null state pointer" in reason(compute(root=None, out=None, frame=2, flags=4, qdd=odd))
    assert "hw_compute: null state pointer" in reason(compute(dof=None, out=None, frame=2, flags=4, qdd=odd))
    assert "hw_compute: null output struct" in reason(compute(out=None, frame=2, flags=4, qdd=odd))
    assert "hw_compute: no output buffer" in reason(compute(out=none, frame=2, flags=4, qdd=odd))
    assert "hw_compute: frame 2 outside 0..1" in reason(compute(out=bad_out, frame=2, flags=4))
    assert "hw_compute: frame -1 outside 0..1" in reason(compute(frame=-1))
    assert "hw_compute: unknown flag bits 0x4" in reason(compute(out=bad_out, flags=4 | 1))
    assert "hw_compute: every buffer must be 4-byte aligned" in reason(compute(out=bad_out))
    for name in ("root", "dof", "qdd", "acc", "force", "torque"):  # every pointer is looked at
        assert "4-byte aligned" in reason(compute(**{name: C.c_void_p(8195)}))
    for name in reaction.OUTPUTS:
        assert "4-byte aligned" in reason(compute(out=outputs(**{name: C.c_void_p(8193)})))
    assert block.raw == bytes(4096)  # the stand-in handle was never written


# ------------------------------------------------------------------ the facade's host-side refusals
def test_facade_refuses_sensors_it_cannot_read(model):
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.Gym()
    asset = gymapi.Asset(model, gymapi.AssetOptions())
    pose = gymapi.Transform()
    with pytest.raises(ValueError, match="body 0"):
        gym.create_asset_force_sensor(asset, 0, pose)
    with pytest.raises(ValueError, match="outside"):
        gym.create_asset_force_sensor(asset, 24, pose)
    for field in ("enable_forward_dynamics_forces", "enable_constraint_solver_forces"):
        props = gymapi.ForceSensorProperties()
        setattr(props, field, False)
        with pytest.raises(NotImplementedError, match=field):
            gym.create_asset_force_sensor(asset, 3, pose, props)
    assert asset.force_sensors == []
    props = gymapi.ForceSensorProperties()
    assert (props.enable_forward_dynamics_forces, props.enable_constraint_solver_forces, props.use_world_frame) == \
        (True, True, False)
    props.use_world_frame = True
    assert gym.create_asset_force_sensor(asset, 3, pose) == 0
    assert gym.create_asset_force_sensor(asset, 7, pose, props) == 1
    assert [(b, w) for b, _, w in asset.force_sensors] == [(3, False), (7, True)]


def test_facade_acquire_without_a_sensor_names_the_call(model):
    from humanoid_amd.isaacgym import gymapi
    gym = gymapi.Gym()
    sim = gymapi.Sim(0, gymapi.SimParams())
    with pytest.raises(RuntimeError, match="before prepare_sim"):
        gym.acquire_force_sensor_tensor(sim)
    sim.asset = gymapi.Asset(model, gymapi.AssetOptions())
    sim.engine = object()  # stands in: the refusal comes before the engine is touched
    with pytest.raises(ValueError, match="create_asset_force_sensor"):
        gym.acquire_force_sensor_tensor(sim)
    assert sim.force_sensors is None and sim.dynamics is None
    sim.engine = None
    # and the refresh before any acquire stays the flush alone: no pending steps, nothing touched
    assert gym.refresh_force_sensor_tensor(sim) is True


# ------------------------------------------------------------------ the reference against its pins
@pytest.fixture(scope="module")
def ref(he_model):
    """The module's states and inputs, and per state what dynamics_reference gives (computed once)."""
    class S:
        pass

    s = S()
    s.root, s.dof = DR.test_states(he_model)
    s.n = n = s.root.shape[0]
    rng = np.random.default_rng(23)
    s.qdd_des = rng.uniform(-20.0, 20.0, (n, ND)).astype(np.float32)
    s.base_acc = rng.uniform(-10.0, 10.0, (n, 6)).astype(np.float32)
    s.f = rng.uniform(-200.0, 200.0, (n, NB, 3)).astype(np.float32)
    s.t = rng.uniform(-20.0, 20.0, (n, NB, 3)).astype(np.float32)
    s.J, s.M, s.c = DR.evaluate(he_model, s.root, s.dof, G, np.float64, armature=False)
    s.Mo = DR.Model(he_model, np.float64)
    s.G = np.zeros((n, NG))
    s.R = np.zeros((n, NB, 3, 3))
    for e in range(n):
        R, p = DR.fk(s.Mo, s.root[e], s.dof[e])
        s.R[e] = R
        Jc = DR._com_jacobian(s.Mo, R, s.J[e])
        s.G[e] = sum(Jc[b].T @ s.f[e, b].astype(np.float64) + s.J[e, b, 3:6].T @ s.t[e, b].astype(np.float64)
                     for b in range(NB))
    return s


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("external", [False, True], ids=["noext", "ext"])
def test_root_and_tau_identities(he_model, ref, external):
    """(F_0, N_0) = (M qdd + c - G)[0:6] and tau without armature = (M qdd + c - G)[6:], prescribed base;
    with armature the dof diagonal's term on top."""
    s = ref
    f, t = (s.f, s.t) if external else (None, None)
    out = RR.evaluate(he_model, s.root, s.dof, G, s.qdd_des, s.base_acc, f, t, armature=False)
    qdd = np.concatenate([s.base_acc, s.qdd_des], axis=1).astype(np.float64)
    want = np.einsum("eij,ej->ei", s.M, qdd) + s.c - (s.G if external else 0.0)
    fig = _rel(out["wrench"][:, 0], want[:, :6]), _rel(out["tau"], want[:, 6:])
    print(f"root wrench {fig[0]:.2e}, tau {fig[1]:.2e} (bound {IDENTITY:.0e})")
    assert max(fig) <= IDENTITY
    assert np.array_equal(out["base_acc"], s.base_acc.astype(np.float64))
    arm = RR.evaluate(he_model, s.root, s.dof, G, s.qdd_des, s.base_acc, f, t, armature=True)
    assert _rel(arm["tau"] - out["tau"], s.Mo.armature * s.qdd_des.astype(np.float64)) <= IDENTITY
    assert np.array_equal(arm["wrench"], out["wrench"])  # armature is no wrench


@pytest.mark.parametrize("external", [False, True], ids=["noext", "ext"])
def test_free_base_is_computed_torque(he_model, ref, external):
    """Free base: tau and base_acc are solve_reference.computed_torque's with gen_force = G, and the root's
    wrench is zero to rounding."""
    s = ref
    f, t = (s.f, s.t) if external else (None, None)
    _, Ma, _ = DR.evaluate(he_model, s.root, s.dof, G, np.float64, armature=True)
    out = RR.evaluate(he_model, s.root, s.dof, G, s.qdd_des, None, f, t)
    tau, ab = SR.computed_torque(Ma, s.c, s.qdd_des, s.G if external else None)
    fig = _rel(out["tau"], tau), _rel(out["base_acc"], ab)
    scale = np.abs(RR.evaluate(he_model, s.root, s.dof, G, s.qdd_des, np.zeros((s.n, 6), np.float32), f, t)["wrench"][:, 0]).max()
    root = np.abs(out["wrench"][:, 0]).max() / scale
    print(f"tau {fig[0]:.2e}, base_acc {fig[1]:.2e}, root wrench / root wrench at a_b = 0: {root:.2e} (bound {IDENTITY:.0e})")
    assert max(fig) <= IDENTITY and root <= IDENTITY


def test_rest_case_carries_the_subtree_weights(he_model, ref):
    """qd = 0, qdd = 0 with a prescribed base, no external wrench: F_j = -m_sub(j) g, and the torque is the
    subtree's weight at its centre of mass about p_j."""
    s = ref
    root, dof = s.root.copy(), s.dof.copy()
    root[:, 7:] = 0.0
    dof[:, :, 1] = 0.0
    out = RR.evaluate(he_model, root, dof, G, None, np.zeros((s.n, 6), np.float32))
    g = np.array(G, np.float32).astype(np.float64)  # the gravity vector is a float32 of the ABI
    m_sub = s.Mo.sub @ s.Mo.mass
    want = -m_sub[None, :, None] * g[None, None, :]
    assert _rel(out["wrench"][:, :, :3], np.broadcast_to(want, (s.n, NB, 3))) <= IDENTITY
    assert np.abs(out["body_acc"]).max() == 0.0
    nog = RR.evaluate(he_model, root, dof, G, None, np.zeros((s.n, 6), np.float32), no_gravity=True)
    assert np.abs(nog["wrench"]).max() == 0.0 and np.abs(nog["tau"]).max() == 0.0


def test_body_frame_is_the_world_wrench_rotated(he_model, ref):
    s = ref
    args = (he_model, s.root, s.dof, G, s.qdd_des, s.base_acc, s.f, s.t)
    w, b = RR.evaluate(*args, frame=RR.FRAME_WORLD), RR.evaluate(*args, frame=RR.FRAME_BODY)
    for k in (0, 3):
        want = np.einsum("ebji,ebj->ebi", s.R, w["wrench"][:, :, k:k + 3])
        assert _rel(b["wrench"][:, :, k:k + 3], want) <= IDENTITY
    for name in ("tau", "base_acc", "body_acc"):
        assert np.array_equal(w[name], b[name])


def _log(R):
    """The rotation vector of a rotation matrix (angles below pi)."""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    s, c = np.linalg.norm(v), (np.trace(R) - 1.0) / 2.0
    return v if s < 1e-12 else v * (np.arctan2(s, c) / s)


def _advanced_velocities(Mo, root, dof, qdd, h):
    """The bodies' (origin velocity, angular velocity) [24,6] at the state advanced by h with qdd held:
    velocities qd + h qdd; the root moved along its velocity and turned by its world angular velocity, the
    dofs integrated on the joint manifold (R_j exp(h u_j), the rates being child-frame)."""
    dt = np.float64
    qd = DR.gen_velocity(root, dof, dt)
    R0 = DR._qmat(root[3:7].astype(dt), dt)
    R0h = DR._exp(h * qd[3:6], dt) @ R0
    p0h = root[:3].astype(dt) + h * qd[:3]
    th = dof[:, 0].astype(dt).reshape(NB - 1, 3)
    u = qd[6:].reshape(NB - 1, 3)
    thh = np.stack([_log(DR._exp(th[j], dt) @ DR._exp(h * u[j], dt)) for j in range(NB - 1)])
    qdh = qd + h * qdd
    R, p = np.zeros((NB, 3, 3)), np.zeros((NB, 3))
    R[0], p[0] = R0h, p0h
    for b in range(1, NB):
        a = Mo.parents[b]
        R[b] = R[a] @ DR._exp(thh[b - 1], dt)
        p[b] = p[a] + R[a] @ Mo.local_pos[b]
    J = DR.jacobian(Mo, R, p)
    rooth = np.concatenate([p0h, root[3:7], qdh[:6]])
    dofh = np.stack([thh.reshape(-1), qdh[6:]], axis=1)
    w, _, _ = DR.body_velocities(Mo, R, p, rooth, dofh)
    # body_velocities casts its velocities through float32; the linear ones come from J in float64
    v = np.einsum("bij,j->bi", J[:, 0:3], qdh)
    wj = np.einsum("bij,j->bi", J[:, 3:6], qdh)
    assert np.abs(w - wj).max() <= 1e-5  # body_velocities' own w, to the float32 cast of its inputs
    return np.concatenate([v, wj], axis=1)


def test_body_acc_is_the_derivative_of_the_body_velocities(he_model, ref):
    """body_acc against the central difference (v(+h) - v(-h)) / 2h. The difference's own error: truncation
    h^2/6 |v'''|, estimated by Richardson from the same difference at 2h (D(2h) - D(h) = 3 x the truncation at
    h), and rounding eps max|v| / h. With jerks of order 1e4 m/s^3 (rates of a few rad/s, qdd to 20) h = 1e-5
    puts the truncation near 2e-7 and the rounding near 1e-10, against accelerations of 50 to 70; the bound is
    twice their sum (the Richardson estimate is itself a leading-order figure)."""
    s, h = ref, 1e-5
    out = RR.evaluate(he_model, s.root, s.dof, G, s.qdd_des, s.base_acc)
    eps = np.finfo(np.float64).eps
    for e in range(s.n):
        qdd = np.concatenate([s.base_acc[e], s.qdd_des[e]]).astype(np.float64)
        vp, vm = (_advanced_velocities(s.Mo, s.root[e], s.dof[e], qdd, k) for k in (h, -h))
        vp2, vm2 = (_advanced_velocities(s.Mo, s.root[e], s.dof[e], qdd, k) for k in (2 * h, -2 * h))
        D, D2 = (vp - vm) / (2 * h), (vp2 - vm2) / (4 * h)
        trunc = np.abs(D2 - D).max() / 3.0
        rounding = eps * max(np.abs(vp).max(), np.abs(vm).max()) / h
        err = np.abs(out["body_acc"][e] - D).max()
        print(f"env {e}: |body_acc - difference| {err:.2e}  truncation {trunc:.2e}  rounding {rounding:.2e}  "
              f"max|body_acc| {np.abs(out['body_acc'][e]).max():.1f}")
        assert err <= 2.0 * (trunc + rounding)
        assert trunc + rounding <= 1e-5 * np.abs(out["body_acc"][e]).max()  # the difference resolves the derivative


def test_sensor_reading_restates_the_definition(he_model, ref):
    """The reading's pins: a sensor at the joint origin in world axes reads (F_b, sum tau R e_i); the same
    sensor with an offset adds -(R_b p_s) x F_b to the torque; the sensor's own axes are Q^T of the world's.
    With qd_before = qd and no contact the force is the prescribed-base wrench at qdd = 0."""
    s = ref
    n = s.n
    rng = np.random.default_rng(5)
    qd = np.stack([DR.gen_velocity(s.root[e], s.dof[e]) for e in range(n)])
    dq = rng.uniform(-0.2, 0.2, (n, NG))
    dt_step = 1.0 / 30.0
    cf = s.f.copy()
    df = rng.uniform(-50.0, 50.0, (n, ND)).astype(np.float32)
    q = np.array([0.1, -0.3, 0.2, 0.9], np.float32)
    poses = [[0, 0, 0, 0, 0, 0, 1], [0.03, -0.02, 0.05, 0, 0, 0, 1], [0.03, -0.02, 0.05] + list(q / np.linalg.norm(q))]
    got = RR.sensor_reading(he_model, s.root, s.dof, (qd - dq).astype(np.float32), dt_step, cf, df, [7, 7, 7], poses,
                            [True, True, False])
    qdd = (qd - (qd - dq).astype(np.float32).astype(np.float64)) / dt_step
    w = RR.evaluate(he_model, s.root, s.dof, G, qdd[:, 6:].astype(np.float32), qdd[:, :6].astype(np.float32), cf)["wrench"]
    # float32 casts of qdd on the way into evaluate: compare at that rounding
    assert _rel(got[:, 0, :3], w[:, 7, :3]) <= 1e-6
    for e in range(n):
        R = s.R[e, 7]
        F = got[e, 0, :3]
        N0 = sum((df[e, 18 + i] - s.Mo.armature[18 + i] * qdd[e, 6 + 18 + i]) * R[:, i] for i in range(3))
        assert np.abs(got[e, 0, 3:] - N0).max() <= 1e-9 * np.abs(N0).max()
        N1 = N0 - np.cross(R @ np.array(poses[1][:3], np.float32).astype(np.float64), F)
        assert np.abs(got[e, 1, 3:] - N1).max() <= 1e-9 * np.abs(N1).max() and np.array_equal(got[e, 1, :3], F)
        Q = R @ DR._qmat(np.array(poses[2][3:], np.float32).astype(np.float64), np.float64)
        assert np.abs(got[e, 2, :3] - Q.T @ F).max() <= 1e-9 * np.abs(F).max()
        assert np.abs(got[e, 2, 3:] - Q.T @ N1).max() <= 1e-9 * np.abs(N1).max()
    still = RR.sensor_reading(he_model, s.root, s.dof, qd.astype(np.float32), dt_step, None, None, [7], poses[:1], [True])
    w0 = RR.evaluate(he_model, s.root, s.dof, G, None, np.zeros((n, 6), np.float32))["wrench"]
    assert _rel(still[:, 0, :3], w0[:, 7, :3]) <= IDENTITY and np.abs(still[:, 0, 3:]).max() == 0.0
