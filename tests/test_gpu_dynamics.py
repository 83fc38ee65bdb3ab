"""GPU checks of the dynamics-query kernel (include/humanoid_dynamics.h) against the float64 numpy
reference of tests/dynamics_reference.py, which tests/test_dynamics.py pins to finite differences and
to the fp64 oracle.

Tolerance per output: 8 x that output's own float32 floor -- the reference evaluated in float32 against
float64 on the same states, maximum absolute error, for M relative to its largest entry (8 is the
margin of tests/test_gpu_render.py). Floors and the kernel's measured errors on the five states of
this module (MI355X):

    output                      float32 floor    tolerance (8 x)   kernel, measured
    J                           3.55e-07         2.84e-06          2.22e-07
    M / max|M|, armature on     4.73e-08         3.79e-07          4.73e-08
    M / max|M|, armature off    4.73e-08         3.79e-07          4.73e-08
    c with gravity [N, N m]     1.47e-04         1.18e-03          1.47e-04
    c without gravity           1.21e-05         9.68e-05          8.99e-06

(M's and c's largest errors sit in the entries that sum the 24 masses -- the total mass on the root's
linear diagonal, its weight in c -- where the kernel and the float32 reference add in the same order.)
M - M^T is exactly zero; J qd against the engine's own rigid-body velocities after 3 simulate calls:
5.0e-07 m/s against a bound of 7.4e-06.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
import dynamics_reference as DR  # noqa: E402

pytestmark = pytest.mark.gpu
N = 5  # odd: M's 22,500-byte env blocks fall on both 4-byte alignments modulo 8
NB, ND, NG = DR.NB, DR.ND, DR.NG
MARGIN = 8.0
SENTINEL = 12345.0


class _Ctx:
    pass


def _floors(he_model, root, dof, g):
    """Float64 references and float32 floors of the five outputs at these states."""
    out = {}
    J, Ma, c = DR.evaluate(he_model, root, dof, g, np.float64, armature=True)
    J32, Ma32, c32 = DR.evaluate(he_model, root, dof, g, np.float32, armature=True)
    _, M, c0 = DR.evaluate(he_model, root, dof, g, np.float64, armature=False, no_gravity=True)
    _, M32, c032 = DR.evaluate(he_model, root, dof, g, np.float32, armature=False, no_gravity=True)
    out["ref"] = dict(J=J, Ma=Ma, M=M, c=c, c0=c0)
    out["floor"] = dict(J=np.abs(J32 - J).max(), Ma=np.abs(Ma32 - Ma).max() / np.abs(Ma).max(),
                        M=np.abs(M32 - M).max() / np.abs(M).max(), c=np.abs(c32 - c).max(), c0=np.abs(c032 - c0).max())
    return out


def _err(got, ref, relative=False):
    e = np.abs(got.astype(np.float64) - ref).max()
    return e / np.abs(ref).max() if relative else e


@pytest.fixture(scope="module")
def ctx(model, he_model):
    """One engine of five envs in the module's states, one Dynamics, the references and floors (computed
    once, left unchanged), and the outputs of one full refresh."""
    from humanoid_amd import dynamics as D
    from humanoid_amd.engine import Engine
    c = _Ctx()
    c.D = D
    c.eng = Engine(model, N, device=0)
    dev = c.eng.device
    # env 0 stays as he_create_envs left it; 1..3 the random states of test_independent_dynamics.py;
    # env 4 has all-zero dofs (the small-angle branch) with nonzero velocities
    root, dof = cases.random_state(4, np.random.default_rng(11), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
    src_r = np.zeros((N, 13), np.float32)
    src_d = np.zeros((N, ND, 2), np.float32)
    src_r[1:4], src_d[1:4] = root[:3], dof[:3]
    src_r[4], src_d[4] = root[3], dof[3]
    src_d[4, :, 0] = 0.0
    ids = torch.arange(1, N, dtype=torch.int32, device=dev)
    c.eng.set_root_state_indexed(torch.from_numpy(src_r).to(dev), ids)
    c.eng.set_dof_state_indexed(torch.from_numpy(src_d.reshape(N * ND, 2)).to(dev), ids)
    c.dyn = D.Dynamics(c.eng)
    # the kernel reads root and dof state only: right immediately after the indexed writes
    c.dyn.refresh()
    torch.cuda.synchronize()
    c.root = c.eng.root_states.cpu().numpy().copy()
    c.dof = c.eng.dof_state.cpu().numpy().reshape(N, ND, 2).copy()
    assert np.array_equal(c.root[1:], src_r[1:]) and np.array_equal(c.dof[1:], src_d[1:])
    assert c.root[0, 6] == 1.0 and abs(c.root[0, 2] - 0.89) < 1e-6 and not c.dof[0].any()
    c.g = tuple(c.eng.params.gravity)
    f = _floors(he_model, c.root, c.dof, c.g)
    c.ref, c.floor = f["ref"], f["floor"]
    c.tol = {k: MARGIN * v for k, v in c.floor.items()}
    c.J = c.dyn.jacobian.cpu().numpy().copy()
    c.Ma = c.dyn.mass_matrix.cpu().numpy().copy()
    c.c = c.dyn.bias.cpu().numpy().copy()
    print("float32 floors:", c.floor)
    yield c
    del c.dyn, c.eng


def test_outputs_match_the_float64_reference(ctx):
    """J, M (armature on and off) and c (with and without gravity), each within 8 x its own float32
    floor; the module docstring holds the figures."""
    c = ctx
    c.dyn.armature, c.dyn.gravity = False, False
    c.dyn.refresh(jacobian=False)
    torch.cuda.synchronize()
    M = c.dyn.mass_matrix.cpu().numpy().copy()
    c0 = c.dyn.bias.cpu().numpy().copy()
    c.dyn.armature, c.dyn.gravity = True, True
    c.dyn.refresh()
    torch.cuda.synchronize()
    err = dict(J=_err(c.J, c.ref["J"]), Ma=_err(c.Ma, c.ref["Ma"], True), M=_err(M, c.ref["M"], True),
               c=_err(c.c, c.ref["c"]), c0=_err(c0, c.ref["c0"]))
    for k in err:
        print(f"{k}: floor {c.floor[k]:.3e}  tolerance {c.tol[k]:.3e}  kernel {err[k]:.3e}")
    assert np.abs(c.ref["c0"]).max() > 1.0 and np.abs(c.ref["c"] - c.ref["c0"]).max() > 100.0  # both parts matter
    for k in err:
        assert err[k] <= c.tol[k], (k, err[k], c.tol[k])
    # armature: exactly the model's diagonal, nothing else moves
    d = c.Ma.astype(np.float64) - M
    off = d.copy()
    off[:, np.arange(6, NG), np.arange(6, NG)] = 0.0
    assert not off.any()
    arm = np.array(c.eng.he_model.armature[:ND], np.float64)
    assert arm.max() > 0
    np.testing.assert_allclose(d[:, np.arange(6, NG), np.arange(6, NG)], np.broadcast_to(arm, (N, ND)), rtol=0,
                               atol=c.tol["Ma"] * np.abs(c.ref["Ma"]).max())
    # the refresh above restored the default outputs bit for bit
    assert np.array_equal(c.dyn.mass_matrix.cpu().numpy(), c.Ma) and np.array_equal(c.dyn.bias.cpu().numpy(), c.c)


def test_exact_zeros_outside_the_tree_pattern(ctx, he_model):
    parents = np.array(he_model.parents[:NB])
    jm = DR.jacobian_mask(parents)
    assert not ((ctx.J != 0.0) & ~jm[None, :, None, :]).any()
    mm = DR.mass_mask(parents)
    assert not ((ctx.Ma != 0.0) & ~mm[None]).any()
    # and inside the pattern the angular rows are there (unit vectors)
    ang = (ctx.J[:, :, 3:6, 3:] != 0.0).any(axis=2)
    assert np.array_equal(ang, np.broadcast_to(jm[:, 3:], ang.shape))
    assert np.isfinite(ctx.J).all() and np.isfinite(ctx.Ma).all() and np.isfinite(ctx.c).all()


def test_mass_matrix_is_symmetric(ctx):
    asym = np.abs(ctx.Ma - ctx.Ma.transpose(0, 2, 1)).max() / np.abs(ctx.ref["Ma"]).max()
    print("asymmetry / max|M|:", asym)
    assert asym <= ctx.tol["Ma"]


def test_single_outputs_equal_the_joint_launch_bit_for_bit(ctx):
    c = ctx
    for which in ("jacobian", "mass_matrix", "bias"):
        for t in (c.dyn.jacobian, c.dyn.mass_matrix, c.dyn.bias):
            t.fill_(SENTINEL)
        c.dyn.refresh(**{k: k == which for k in ("jacobian", "mass_matrix", "bias")})
        torch.cuda.synchronize()
        got = dict(jacobian=c.dyn.jacobian.cpu().numpy(), mass_matrix=c.dyn.mass_matrix.cpu().numpy(),
                   bias=c.dyn.bias.cpu().numpy())
        want = dict(jacobian=c.J, mass_matrix=c.Ma, bias=c.c)
        for k in got:
            if k == which:
                assert np.array_equal(got[k], want[k]), k
            else:
                assert (got[k] == SENTINEL).all(), f"{k} written by a launch that asked for {which} only"
    c.dyn.refresh()


def test_second_refresh_is_bit_identical(ctx):
    """Unchanged state, same bits: uninitialised LDS or a stray lane tail would show here."""
    c = ctx
    for t in (c.dyn.jacobian, c.dyn.mass_matrix, c.dyn.bias):
        t.fill_(float("nan"))
    c.dyn.refresh()
    torch.cuda.synchronize()
    assert np.array_equal(c.dyn.jacobian.cpu().numpy(), c.J)
    assert np.array_equal(c.dyn.mass_matrix.cpu().numpy(), c.Ma)
    assert np.array_equal(c.dyn.bias.cpu().numpy(), c.c)


def test_nothing_is_written_past_the_last_env(ctx):
    """Each output allocated with 75 more floats of a sentinel behind the last env: the tail of the last
    row, and of M's odd-aligned last block, stays untouched."""
    c = ctx
    shapes = c.D.output_shapes(N)
    bufs, views = {}, {}
    for k, shp in shapes.items():
        numel = int(np.prod(shp))
        bufs[k] = torch.full((numel + NG,), SENTINEL, dtype=torch.float32, device=c.eng.device)
        views[k] = bufs[k][:numel].view(shp)
    c.dyn.refresh_into(views["jacobian"], views["mass_matrix"], views["bias"])
    torch.cuda.synchronize()
    want = dict(jacobian=c.J, mass_matrix=c.Ma, bias=c.c)
    for k, shp in shapes.items():
        numel = int(np.prod(shp))
        assert (bufs[k][numel:] == SENTINEL).all().item(), k
        assert np.array_equal(views[k].cpu().numpy(), want[k]), k


def test_binding_refuses_bad_tensors_on_the_device(ctx):
    c = ctx
    with pytest.raises(c.D.DynamicsError, match="jacobian"):
        c.dyn.refresh_into(jacobian=torch.zeros(N, NB, 6, NG, device="cpu"))
    with pytest.raises(c.D.DynamicsError, match="mass_matrix"):
        c.dyn.refresh_into(mass_matrix=torch.zeros(N, NG, NG, device=c.eng.device).transpose(1, 2))
    with pytest.raises(c.D.DynamicsError, match="unknown flag"):
        c.dyn.refresh_into(bias=c.dyn.bias, flags=8)
    qdd = torch.zeros(N, NG, device=c.eng.device)
    assert torch.equal(c.dyn.inverse_dynamics(qdd), c.dyn.bias)


def test_jacobian_times_velocity_is_the_engines_rigid_body_velocity(ctx):
    """After 3 simulate calls towards stand-still targets, J qd equals the engine's own rb_state rows
    7:13 within the J tolerance times max|qd|: the product tied to the product. (Runs last in this
    module's engine: it moves the state.)"""
    c = ctx
    c.eng.set_dof_targets(c.eng.dof_state.view(N, ND, 2)[:, :, 0].contiguous())
    for _ in range(3):
        c.eng.simulate(1)
    c.dyn.refresh(mass_matrix=False, bias=False)
    torch.cuda.synchronize()
    J = c.dyn.jacobian.cpu().numpy().astype(np.float64)
    qd = c.dyn.generalized_velocity().cpu().numpy().astype(np.float64)
    rb = c.eng.rb_state.view(N, NB, 13).cpu().numpy().astype(np.float64)
    assert not np.array_equal(c.dyn.jacobian.cpu().numpy(), c.J)  # the state has moved
    v = np.einsum("nbrc,nc->nbr", J, qd)
    err = np.abs(v - rb[:, :, 7:13]).max()
    bound = c.tol["J"] * np.abs(qd).max()
    print(f"J qd - rb_state velocities: {err:.3e}, bound {bound:.3e} (max|qd| {np.abs(qd).max():.3f})")
    assert np.abs(qd).max() > 1.0
    assert err <= bound


def test_facade_dynamics_tensors(he_model):
    """The gym facade, driven as tests/test_facade_env.py drives it (4 envs): the acquired tensors
    alias sim.dynamics' memory, a refresh flushes the pending simulate calls first and refreshes its own
    tensor only."""
    from humanoid_amd.isaacgym import gymtorch
    from test_facade_env import _facade_sim
    n = 4
    gym, sim = _facade_sim(n)
    assert gym.refresh_jacobian_tensors(sim) is True and sim.dynamics is None  # before the acquire: a no-op
    with pytest.raises(ValueError, match="no env has an actor"):
        gym.acquire_jacobian_tensor(sim, "nobody")
    assert sim.dynamics is None
    jac = gymtorch.wrap_tensor(gym.acquire_jacobian_tensor(sim, "humanoid_0"))
    mass = gymtorch.wrap_tensor(gym.acquire_mass_matrix_tensor(sim, "humanoid_3"))
    assert jac.shape == (n, NB, 6, NG) and mass.shape == (n, NG, NG)
    assert jac.data_ptr() == sim.dynamics.jacobian.data_ptr() and mass.data_ptr() == sim.dynamics.mass_matrix.data_ptr()
    assert sim.dynamics.engine is sim.engine
    assert gym.refresh_bias_force_tensors(sim) is True and not sim.dynamics.bias.any().item()  # not acquired: no-op
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    r0, d0 = cases.random_state(n, np.random.default_rng(7), height=(1.0, 1.5))
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    src_r, src_d = torch.from_numpy(r0).cuda(), torch.from_numpy(d0.reshape(n * ND, 2)).cuda()
    gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_r), gymtorch.unwrap_tensor(ids), n)
    gym.set_dof_state_tensor_indexed(sim, gymtorch.unwrap_tensor(src_d), gymtorch.unwrap_tensor(ids), n)
    g = tuple(sim.engine.params.gravity)

    def reference():
        r, d = root.cpu().numpy(), dof.cpu().numpy().reshape(n, ND, 2)
        f = _floors(he_model, r, d, g)
        return f["ref"], {k: MARGIN * v for k, v in f["floor"].items()}

    assert gym.refresh_jacobian_tensors(sim) is True
    torch.cuda.synchronize()
    ref0, tol0 = reference()
    J0 = jac.cpu().numpy().copy()
    assert _err(J0, ref0["J"]) <= tol0["J"]
    assert not mass.any().item()  # refresh_jacobian_tensors refreshes the Jacobian only
    gym.simulate(sim)
    gym.simulate(sim)
    assert sim.pending_substeps == 2
    gym.refresh_jacobian_tensors(sim)  # flushes the two substeps, then refreshes
    assert sim.pending_substeps == 0
    torch.cuda.synchronize()
    ref1, tol1 = reference()
    J1 = jac.cpu().numpy().copy()
    assert _err(J1, ref0["J"]) > 100 * tol0["J"]  # the state has moved
    assert _err(J1, ref1["J"]) <= tol1["J"]
    gym.refresh_mass_matrix_tensors(sim)
    torch.cuda.synchronize()
    assert np.array_equal(jac.cpu().numpy(), J1)  # untouched
    assert _err(mass.cpu().numpy(), ref1["Ma"], True) <= tol1["Ma"]  # the facade's M carries the armature
    bias = gymtorch.wrap_tensor(gym.acquire_bias_force_tensor(sim, "humanoid_1"))
    assert bias.shape == (n, NG) and bias.data_ptr() == sim.dynamics.bias.data_ptr()
    gym.refresh_bias_force_tensors(sim)
    torch.cuda.synchronize()
    assert _err(bias.cpu().numpy(), ref1["c"]) <= tol1["c"]
