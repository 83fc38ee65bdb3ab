"""Save, restore and clone env state on the GPU (include/humanoid_engine.h "env state"). The
criterion is torch.equal throughout: the step is deterministic and counter-seeded, so a restored state must
continue on the same trajectory bit for bit, in the same env, in a fresh one after torch.save / torch.load, in
a clone beside its source, and through the gym facade.

One module-scoped HumanoidPHC on the synthetic motions, the default TGS solver, N = 7 (an odd count: the last
env's rows end off any vector boundary). The actions are drawn once with numpy from a fixed seed. The engine
does not read EnvConfig.max_episode_length: its time-out is the end of the env's motion (the imitation step's
pass_time), so the clips are 13 frames long and a time-out falls into every window of a few policy steps.
Every test first loads the state saved after 4 policy steps, so the tests do not depend on their order."""
import ctypes as C
import os

import numpy as np
import pytest

from humanoid_amd import _abi

import cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, ND, NB = 7, 69, 24
WARM, WINDOW = 4, 6
PUBLIC = ("root_states", "dof_state", "rb_state", "contact_forces", "dof_force", "dof_targets", "num_contacts",
          "dropped_contacts", "contact_cache", "initial_root_states")
# the state's fields by the Engine properties of the public buffers they pack
FIELD_OF = dict(zip(PUBLIC, ("root", "dof_state", "rb", "cf", "dof_force", "targets", "num_contacts", "dropped",
                             "cache", "init_root")))


def _clips(model):
    from humanoid_amd import synthetic
    return {f"clip{i}": synthetic.make_clip(model, np.random.default_rng(300 + i), num_frames=13) for i in range(4)}


def _make_env(model):
    from humanoid_amd.env import EnvConfig, HumanoidPHC
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return HumanoidPHC(EnvConfig(num_envs=N, motion_file=_clips(model), seed=4))


def _public(eng):
    return {name: getattr(eng, name).clone() for name in PUBLIC}


def _policy_step(env, a, host_reset=True):
    """One policy step and, as a trainer does, the reset of the envs it flagged. Returns the tensors kept."""
    obs, rew, reset, extras = env.step(a)
    kept = {"obs": obs.clone(), "rew": rew.clone(), "reset": reset.clone(), "terminate": extras["terminate"].clone()}
    if host_reset:
        ids = env.reset_buf.nonzero().flatten()
        if len(ids):
            env.reset(ids)
        kept["obs_after_reset"] = env.obs_buf.clone()
    e = env.engine
    kept.update(root=e.root_states.clone(), dof=e.dof_state.clone(), rb=e.rb_state.clone(),
                cf=e.contact_forces.clone(), dof_force=e.dof_force.clone())
    return kept


def _run(env, actions, **kw):
    return [_policy_step(env, a, **kw) for a in actions]


def _assert_same(run_a, run_b, rows=None):
    assert len(run_a) == len(run_b)
    for step, (a, b) in enumerate(zip(run_a, run_b)):
        assert a.keys() == b.keys()
        for name in a:
            x, y = a[name], b[name]
            if rows is not None:
                x, y = x.view(N, -1)[rows], y.view(N, -1)[rows]
            assert torch.equal(x, y), f"step {step}: {name} differs"


@pytest.fixture(scope="module")
def world(model):
    """The env after a full reset and 4 policy steps, its saved state, and the actions of every test."""
    env = _make_env(model)
    rng = np.random.default_rng(11)
    actions = torch.as_tensor(rng.uniform(-0.3, 0.3, (WARM + WINDOW, N, ND)).astype(np.float32), device="cuda:0")
    env.reset()
    _run(env, actions[:WARM])
    torch.cuda.synchronize()
    return {"env": env, "saved": env.save_state(), "actions": actions, "model": model}


@pytest.fixture(scope="module")
def twin(world):
    """A second env object of the same configuration, which has taken no step of its own."""
    return _make_env(world["model"])


# ------------------------------------------------------------------ 1. the layout
def test_layout_is_the_sum_of_the_included_rows(world):
    eng = world["env"].engine
    words, fields = eng.state_layout
    assert eng.state_layout is eng.state_layout  # cached
    want, offset = [], 0
    for name in PUBLIC:  # what he_get_buffer says of the ten public buffers, in he_buf_kind order
        t = getattr(eng, name)
        want.append((FIELD_OF[name], t.numel() // N, _abi.DTYPE_F32 if t.dtype == torch.float32 else _abi.DTYPE_I32))
    want += [("wrench", NB * 6, _abi.DTYPE_F32), ("dof_act", ND, _abi.DTYPE_F32)]  # the internal rows in the state
    assert list(fields) == [name for name, _, _ in want]
    for name, n, dtype in want:  # contiguous, in table order
        assert fields[name] == (offset, n, dtype), name
        offset += n
    assert words == offset == sum(n for _, n, _ in want)
    layout = _abi.HeStateLayout()
    assert eng.lib.he_state_layout_get(eng.h, C.byref(layout)) == 0
    kinds = [f.kind for f in layout.fields[:layout.num_fields]]
    assert kinds == list(range(10)) + [-1, -1]
    assert _abi.BUF_PHYS_ORDER not in kinds and _abi.BUF_PHYS_COST not in kinds


def test_refusals_behind_the_env_count_come_in_the_stated_order(world):
    """Refusals 3 to 6 of the header's order, each with everything after it wrong as well; none launches."""
    eng = world["env"].engine
    lib, h = eng.lib, eng.h
    before = _public(eng)

    def reason(rc):
        assert rc != 0
        return lib.he_last_error().decode()

    ids = torch.zeros(N, dtype=torch.int32, device="cuda:0")
    buf = torch.zeros(N * eng.state_layout[0] + 1, dtype=torch.int32, device="cuda:0")
    p_ids, p_buf = C.c_void_p(ids.data_ptr()), C.c_void_p(buf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 2)
    assert "he_save_envs: null state buffer" in reason(lib.he_save_envs(h, odd, N + 1, None, None))
    assert "he_load_envs: null state buffer" in reason(lib.he_load_envs(h, odd, -1, None, None))
    assert "he_save_envs: null ids" in reason(lib.he_save_envs(h, None, N - 1, odd, None))
    assert "he_clone_envs: null id array" in reason(lib.he_clone_envs(h, None, odd, N + 1, None))
    assert "he_clone_envs: null id array" in reason(lib.he_clone_envs(h, odd, None, -1, None))
    for k in (-1, N + 1):
        assert f"he_save_envs: k = {k} outside 0..{N}" in reason(lib.he_save_envs(h, odd, k, odd, None))
        assert f"he_load_envs: k = {k} outside 0..{N}" in reason(lib.he_load_envs(h, odd, k, odd, None))
        assert f"he_clone_envs: k = {k} outside 0..{N}" in reason(lib.he_clone_envs(h, odd, odd, k, None))
    assert "he_save_envs: every buffer must be 4-byte aligned" in reason(lib.he_save_envs(h, p_ids, 1, odd, None))
    assert "he_load_envs: every buffer must be 4-byte aligned" in reason(lib.he_load_envs(h, odd, 1, p_buf, None))
    assert "he_clone_envs: every buffer must be 4-byte aligned" in reason(lib.he_clone_envs(h, p_ids, odd, 1, None))
    assert "he_get_sim_state: null sim state" in reason(lib.he_get_sim_state(h, None))
    assert "he_set_sim_state: null sim state" in reason(lib.he_set_sim_state(h, None))
    was = eng.sim_state_dict()
    bad = _abi.HeSimState(version=_abi.STATE_VERSION + 1, wrench_hold=-1, act_set=1, launches=5)
    assert "he_set_sim_state: version 2" in reason(lib.he_set_sim_state(h, C.byref(bad)))
    bad.version = _abi.STATE_VERSION
    assert "he_set_sim_state: negative" in reason(lib.he_set_sim_state(h, C.byref(bad)))
    assert eng.sim_state_dict() == was
    # k == 0 succeeds without a launch, whatever else is handed over
    assert lib.he_save_envs(h, p_ids, 0, p_buf, None) == 0 and lib.he_clone_envs(h, p_ids, p_ids, 0, None) == 0
    torch.cuda.synchronize()
    after = _public(eng)
    assert all(torch.equal(before[k], after[k]) for k in before) and not buf.any()


# ------------------------------------------------------------------ 2. round trip
def test_save_then_load_leaves_every_buffer_and_rows_follow_ids(world):
    env = world["env"]
    env.load_state(world["saved"])
    eng = env.engine
    before = _public(eng)
    state = eng.save_envs()
    assert state.shape == (N, eng.state_layout[0]) and state.dtype == torch.int32
    for name in PUBLIC:  # the saved fields are the live buffers
        assert torch.equal(eng.state_field(state, FIELD_OF[name]), before[name].view(N, -1)), name
    eng.load_envs(state)
    after = _public(eng)
    for name in PUBLIC:
        assert torch.equal(before[name], after[name]), name
    # unsorted ids, k < N: row i belongs to ids[i]
    ids = torch.tensor([5, 0, 3], dtype=torch.int32, device="cuda:0")
    some = eng.save_envs(ids)
    assert torch.equal(some, state[ids.long()])
    out = torch.full_like(some, -1)
    assert eng.save_envs(ids, out=out) is out and torch.equal(out, some)
    # the rows go back where the ids say: scramble the three envs first, leave the others alone
    for name in ("root_states", "contact_cache", "num_contacts"):
        getattr(eng, name)[ids.long()] = 7
    eng.load_envs(some, ids)
    after = _public(eng)
    for name in PUBLIC:
        assert torch.equal(before[name], after[name]), name
    # another env's rows: env 1 takes env 5's state, and nothing else moves
    eng.load_envs(some[:1].contiguous(), torch.tensor([1], dtype=torch.int32, device="cuda:0"))
    moved = eng.save_envs()
    assert torch.equal(moved[1], state[5]) and torch.equal(moved[[0, 2, 3, 4, 5, 6]], state[[0, 2, 3, 4, 5, 6]])


# ------------------------------------------------------------------ 3. bit-exact replay
def test_replay_is_bit_exact(world):
    env, actions = world["env"], world["actions"]
    env.load_state(world["saved"])
    eng = env.engine
    # the hidden state is in play: contacts, and a warm-start cache that holds rows
    assert ((eng.num_contacts > 0) & (eng.contact_cache != 0).any(1)).any()
    first = _run(env, actions[WARM:])
    # the window holds a reset that is a time-out (the motion's end), not a fall
    assert any((k["reset"] & ~k["terminate"]).any() for k in first)
    env.load_state(world["saved"])
    again = _run(env, actions[WARM:])
    _assert_same(first, again)
    world["window"] = first


# ------------------------------------------------------------------ 4. resume in a fresh engine
def test_resume_in_a_fresh_engine(world, twin, tmp_path):
    env, actions = world["env"], world["actions"]
    if "window" not in world:
        env.load_state(world["saved"])
        world["window"] = _run(env, actions[WARM:])
    path = os.path.join(tmp_path, "state.pt")
    torch.save(world["saved"], path)
    twin.load_state(torch.load(path))
    _assert_same(world["window"], _run(twin, actions[WARM:]))


# ------------------------------------------------------------------ 5. clone
def test_clone_is_the_same_state_and_leaves_the_others(world, twin):
    """No host resets here: a reset draws one phase per flagged env, so clones would part at their first one."""
    env = world["env"]
    env.load_state(world["saved"])
    twin.load_state(world["saved"])
    env.clone_envs([2, 2], [4, 6])
    eng = env.engine
    state = eng.save_envs()
    assert torch.equal(state[4], state[2]) and torch.equal(state[6], state[2])
    assert torch.equal(eng.root_states[4, :2], eng.root_states[2, :2])  # the same state, not a translated one
    actions = world["actions"][:5].clone()
    actions[:, 4] = actions[:, 2]
    actions[:, 6] = actions[:, 2]
    cloned = _run(env, actions, host_reset=False)
    plain = _run(twin, actions, host_reset=False)
    for step, k in enumerate(cloned):
        for name, t in k.items():
            rows = t.view(N, -1)
            assert torch.equal(rows[4], rows[2]) and torch.equal(rows[6], rows[2]), f"step {step}: {name}"
    others = torch.tensor([0, 1, 3, 5], device="cuda:0")
    _assert_same(cloned, plain, rows=others)
    assert not torch.equal(cloned[-1]["root"][4], plain[-1]["root"][4])
    assert torch.equal(eng.physics_order.sort().values, torch.arange(N, dtype=torch.int32, device="cuda:0"))
    # a src == dst entry is a no-op
    before = eng.save_envs()
    env.clone_envs([3], [3])
    assert torch.equal(eng.save_envs(), before)


# ------------------------------------------------------------------ 6. pending wrench, torque control
def test_pending_wrench_and_actuation_survive(he_model):
    from humanoid_amd.engine import Engine
    eng = Engine(he_model, N, device=0, sim_params=_abi.default_sim_params())
    rng = np.random.default_rng(21)
    r0, d0 = cases.random_state(N, rng, height=(0.9, 1.0))
    eng.root_states.copy_(torch.from_numpy(r0).cuda())
    eng.dof_state.copy_(torch.from_numpy(d0.reshape(N * ND, 2)).cuda())
    modes = np.full(ND, _abi.DOF_MODE_POS, np.int32)
    modes[[3, 40]] = _abi.DOF_MODE_EFFORT
    eng.set_dof_drive_modes(modes)
    eng.simulate(2)
    tau = torch.as_tensor(rng.uniform(-30, 30, (N, ND)).astype(np.float32), device="cuda:0")
    force = torch.as_tensor(rng.uniform(-200, 200, (N, NB, 3)).astype(np.float32), device="cuda:0")
    eng.set_dof_actuation_forces(tau)
    eng.apply_body_forces(force=force, hold=3)
    state, sim = eng.save_envs(), eng.sim_state_dict()
    assert sim["wrench_hold"] == 3 and sim["act_set"] == 1 and sim["version"] == _abi.STATE_VERSION

    def two_steps():
        out = []
        for _ in range(2):
            eng.simulate(1)
            out.append(_public(eng))
        return out

    first = two_steps()
    assert eng.sim_state().wrench_hold == 1
    # what the load must undo: the wrench rows replaced and its hold run down, the actuation cleared
    eng.apply_body_forces(force=-force, hold=1)
    eng.clear_dof_actuation_forces()
    assert eng.sim_state().act_set == 0
    eng.load_envs(state)
    eng.set_sim_state(sim)
    assert eng.sim_state().wrench_hold == 3 and eng.sim_state().act_set == 1
    again = two_steps()
    for a, b in zip(first, again):
        for name in PUBLIC:
            assert torch.equal(a[name], b[name]), name
    # the wrench and the actuation were in play: without them the two steps end elsewhere
    eng.load_envs(state)
    eng.set_sim_state(dict(sim, wrench_hold=0, act_set=0))
    assert not torch.equal(two_steps()[-1]["root_states"], first[-1]["root_states"])


# ------------------------------------------------------------------ 7. the gym facade
def test_facade_save_load_clone_replay():
    from humanoid_amd.isaacgym import gymtorch
    from test_facade_env import _facade_sim
    gym, sim = _facade_sim(N)
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    tensors = {"root": root, "dof": gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim)),
               "rb": gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim)),
               "cf": gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim)),
               "dof_force": gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))}
    rng = np.random.default_rng(31)
    targets = torch.as_tensor(rng.uniform(-0.4, 0.4, (7, N, ND)).astype(np.float32), device="cuda:0")

    def run(tg):
        kept = []
        for t in tg:
            gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(t.contiguous()))
            gym.simulate(sim)
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            kept.append({k: v.clone() for k, v in tensors.items()})
        return kept

    run(targets[:4])
    gym.simulate(sim)  # a batched call still pending: the save flushes it first
    saved = gym.save_env_states(sim)
    assert sim.pending_substeps == 0
    state = gymtorch.wrap_tensor(saved)
    assert state.shape == (N, sim.engine.state_layout[0]) and state.dtype == torch.int32
    assert torch.equal(sim.engine.state_field(state, "root"), root)
    assert (sim.engine.state_field(state, "num_contacts") > 0).any()
    first = run(targets[4:])
    gym.load_env_states(sim, saved)
    again = run(targets[4:])
    for a, b in zip(first, again):
        for name in a:
            assert torch.equal(a[name], b[name]), name
    # rows by ids, then a clone beside its source
    ids = torch.tensor([6, 1], dtype=torch.int32, device="cuda:0")
    some = gymtorch.wrap_tensor(gym.save_env_states(sim, gymtorch.unwrap_tensor(ids)))
    assert torch.equal(some, sim.engine.save_envs()[ids.long()])
    gym.load_env_states(sim, saved)
    gym.load_env_states(sim, gymtorch.unwrap_tensor(some), gymtorch.unwrap_tensor(ids))
    assert torch.equal(sim.engine.save_envs()[ids.long()], some)
    gym.load_env_states(sim, saved)
    src = torch.tensor([2], dtype=torch.int32, device="cuda:0")
    dst = torch.tensor([4], dtype=torch.int32, device="cuda:0")
    gym.clone_env_states(sim, gymtorch.unwrap_tensor(src), gymtorch.unwrap_tensor(dst))
    tg = targets[4:].clone()
    tg[:, 4] = tg[:, 2]
    cloned = run(tg)
    for step, (k, ref) in enumerate(zip(cloned, first)):
        for name, t in k.items():
            rows, want = t.view(N, -1), ref[name].view(N, -1)
            assert torch.equal(rows[4], rows[2]), f"step {step}: {name}"
            assert torch.equal(rows[[0, 1, 2, 3, 5, 6]], want[[0, 1, 2, 3, 5, 6]]), f"step {step}: {name}"
