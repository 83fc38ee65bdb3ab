"""tools/bench_common.py on the CPU: the order in which `alternate` warms, synchronises and times its sides, the
records it writes against the committed ones, its torch rotations and tree walk against the float64 references,
and the seeded states. No device is opened: the timer, the synchronise, the device name and the code ids are
passed in."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dynamics_reference as DR
import ik_reference as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_common as bc  # noqa: E402

EPS4 = 4 * 2.0 ** -23  # four float32 roundings of a magnitude of 1


def test_alternate_order():
    log = []
    sides = {"a": lambda: log.append(("call", "a")) or "a_out", "b": None, "c": lambda: log.append(("call", "c")) or "c_out"}
    ms = iter(range(1, 100))

    def timed(fn, calls):  # records, calls nothing
        name = next(k for k, f in sides.items() if f is fn)
        log.append(("timed", name, calls))
        return {"a": 0.5, "c": 7.0}[name] + next(ms)

    sync = lambda: log.append(("sync",))  # noqa: E731
    times, last = bc.alternate(sides, {"a": 3, "c": 1}, {"a": 20, "c": 2}, 4, timed=timed, sync=sync)
    warm = log[:next(i for i, e in enumerate(log) if e[0] == "timed")]
    assert warm.count(("call", "a")) == 3 and warm.count(("call", "c")) == 1
    assert log.count(("sync",)) == 1 and warm[-1] == ("sync",)
    assert last == {"a": "a_out", "c": "c_out"}
    assert log[len(warm):] == [("timed", "a", 20), ("timed", "c", 2)] * 4
    assert set(times) == {"a", "c"}
    assert times == {"a": [0.5 + i for i in (1, 3, 5, 7)], "c": [7.0 + i for i in (2, 4, 6, 8)]}
    # an int holds for every side; `compare` sees the last warm-up results after the synchronise, before any timing
    del log[:]
    seen = []
    times, compared = bc.alternate(sides, 2, 5, 1, compare=lambda o: seen.append((dict(o), list(log))) or "compared",
                                   timed=timed, sync=sync)
    assert log[:5] == [("call", "a"), ("call", "c"), ("call", "a"), ("call", "c"), ("sync",)]
    assert seen == [({"a": "a_out", "c": "c_out"}, log[:5])] and compared == "compared"
    assert log[5:] == [("timed", "a", 5), ("timed", "c", 5)] and [len(t) for t in times.values()] == [1, 1]


def _results(tool, blocks):
    """The first result of each of the three tools, as the tool puts it together, on made-up blocks."""
    k, t = blocks, [2.0 * x for x in blocks]
    if tool == "reaction":
        return dict(case="x", **bc.side_fields("kernel", k), **bc.side_fields("torch", t),
                    torch_over_kernel=bc.over(t, k, 1), max_abs_difference_over_max=[0.0])
    if tool == "state":
        return dict(case="x", k=1, **bc.side_fields("kernel", k), kernel_bytes=8, kernel_effective_gb_per_s=1.0,
                    **bc.side_fields("replaced", t), replaced_over_kernel=bc.over(t, k, 2),
                    slowest_kernel_over_fastest_replaced=bc.slowest_over_fastest(k, t))
    return dict(case="x", k=6, mode="force", **bc.side_fields("fused", k), **bc.side_fields("recipe", t),
                recipe_over_fused=bc.over(t, k, 2), slowest_fused_over_fastest_recipe=bc.slowest_over_fastest(k, t),
                max_abs_difference_over_max={})


@pytest.mark.parametrize("tool,libraries,extra", [
    ("reaction", ["solve", "engine"], dict(torch="")),
    ("state", ["engine", "engine_phases"], dict(words_per_env=1, replaced_words_per_env=1, note="")),
    ("task", ["task", "solve", "engine"], dict(recipe=""))])
def test_record(tmp_path, tool, libraries, extra):
    committed = json.load(open(os.path.join(ROOT, "profiles", tool, tool + "_bench.json")))
    blocks = [0.123456789, 0.1, 0.3, 0.2, 0.25]
    assert bc.side_fields("kernel", blocks) == dict(kernel_ms=0.2, kernel_blocks_ms=[0.12346, 0.1, 0.3, 0.2, 0.25])
    assert bc.side_fields("kernel", blocks, 3)["kernel_blocks_ms"][0] == 0.123
    assert bc.over([3.0, 1.0, 2.0], [0.3, 0.7, 0.9], 2) == round(2.0 / 0.7, 2)
    assert bc.slowest_over_fastest([3.0, 1.0, 2.0], [0.3, 0.7, 0.9]) == 10.0
    args = SimpleNamespace(envs=128, warmup=1, calls=2, blocks=5, out="unused", body=3)
    path = tmp_path / "deeper" / "record.json"
    rec = bc.write_record(str(path), f"tools/{tool}_bench.py", args, libraries, [_results(tool, blocks)],
                          device="no device", code_id=lambda lib: os.path.basename(lib), **extra)
    text = path.read_text()
    assert text.endswith("}\n") and json.loads(text) == rec
    assert list(rec) == list(committed)
    assert list(rec["results"][0]) == list(committed["results"][0])
    assert (rec["envs"], rec["warmup"], rec["calls_per_block"], rec["blocks"]) == (128, 1, 2, 5)
    assert rec["device"] == "no device" and rec["engine_device_code_id"].endswith(".so")


def _rotation_vectors():
    rng = np.random.default_rng(0)
    mags = np.concatenate([[0, 1e-8, 1e-5, 9.9e-4, 1e-3, 1.01e-3, 5e-3], rng.uniform(0, 3.1, 200)])
    d = rng.normal(size=(mags.size, 3))
    return (mags[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_quaternion_helpers():
    """float32 on the CPU against ik_reference in float64 on the same float32 inputs: 207 rotation vectors, both
    sides of the small-angle switch and up to 3.1 rad. Bound: four float32 roundings of the largest magnitude, 1
    for a quaternion's components, pi for a rotation vector's."""
    v = _rotation_vectors()
    assert v.shape == (207, 3)
    q = bc.quat_exp(torch.from_numpy(v))
    assert q.dtype == torch.float32
    q64 = np.stack([KR.quat_exp(x.astype(np.float64), np.float64) for x in v])
    e_exp = np.abs(q.numpy() - q64).max()
    qa, qb = q.numpy().astype(np.float64), np.roll(q.numpy(), 1, axis=0).astype(np.float64)
    prod = bc.quat_mul(q, torch.roll(q, 1, 0))
    e_mul = np.abs(prod.numpy() - np.stack([KR.quat_mul(a, b) for a, b in zip(qa, qb)])).max()
    both = torch.cat([q, -q, prod])  # either sign of w
    rv64 = np.stack([KR.quat_rotvec(x) for x in both.numpy().astype(np.float64)])
    e_rv = np.abs(bc.quat_rotvec(both).numpy() - rv64).max()
    print(f"quat_exp {e_exp:.2e} quat_mul {e_mul:.2e} quat_rotvec {e_rv:.2e}")
    assert e_exp <= EPS4 and e_mul <= EPS4 and e_rv <= EPS4 * np.pi


def test_rotation_matrices():
    """rodrigues and quat_matrix in float32 against dynamics_reference._exp and _qmat in float64 on the same 207
    vectors and on their quaternions scaled by 0.5 to 2 (_qmat normalises). Measured on the CPU against the float64
    reference: 2.884e-7 (rodrigues) and 4.226e-7 (quat_matrix), the largest entry differences. Each bound is twice
    its measured value: the run is deterministic, the factor leaves room for another torch build's sin and cos."""
    v = _rotation_vectors()
    R64 = np.stack([DR._exp(x.astype(np.float64), np.float64) for x in v])
    e_rod = np.abs(bc.rodrigues(torch.from_numpy(v)).numpy() - R64).max()
    q = bc.quat_exp(torch.from_numpy(v)) * torch.linspace(0.5, 2.0, v.shape[0])[:, None]  # not unit: _qmat normalises
    Q64 = np.stack([DR._qmat(x, np.float64) for x in q.numpy().astype(np.float64)])
    e_qm = np.abs(bc.quat_matrix(q).numpy() - Q64).max()
    K = bc.skew(torch.from_numpy(v))
    assert torch.equal(bc.mv(K, torch.from_numpy(v)), torch.zeros(207, 3)) and torch.equal(K, -K.transpose(1, 2))
    print(f"rodrigues {e_rod:.3e} quat_matrix {e_qm:.3e}")
    assert e_rod <= 2 * 2.884e-7 and e_qm <= 2 * 4.226e-7


def test_tree_and_forward_kinematics(model, he_model):
    """The level-wise forward kinematics in float32, in both forms (quaternions as ik_bench.py runs it, matrices as
    reaction_bench.py does), against dynamics_reference.fk in float64 on the six states of test_states. Measured on
    the CPU: positions 2.879e-7 m and rotation entries 4.142e-7 in the quaternion form, 3.375e-7 m and 2.794e-7 in
    the matrix form. Each of the four bounds is twice its own measured value: the run is deterministic, the factor
    leaves room for another torch build's sin and cos."""
    Mo = DR.Model(he_model)
    root, dof = DR.test_states(he_model)
    ref = [DR.fk(Mo, r, d) for r, d in zip(root, dof)]
    R64, p64 = np.stack([x[0] for x in ref]), np.stack([x[1] for x in ref])
    tr = bc.tree(model, "cpu")
    assert np.array_equal(tr.sub.numpy().astype(bool), Mo.sub) and sorted(int(b) for bs, _ in tr.levels for b in bs) == \
        list(range(1, bc.NB))
    assert all(tr.parents[int(b)] == int(p) for bs, ps in tr.levels for b, p in zip(bs, ps))
    for name, ref64 in (("local_pos", Mo.local_pos), ("mass", Mo.mass), ("com", Mo.com), ("armature", Mo.armature)):
        assert np.array_equal(getattr(tr, name).numpy().astype(np.float64), ref64), name
    assert tr.inertia.shape == (bc.NB, 3, 3)
    r, th = torch.from_numpy(root), torch.from_numpy(dof[:, :, 0].reshape(-1, bc.NB - 1, 3).copy())
    seen = []
    pos_q, quat = bc.forward_kinematics(tr, r[:, :3], r[:, 3:7], bc.quat_exp(th))
    pos_m, rot = bc.forward_kinematics(tr, r[:, :3], bc.quat_matrix(r[:, 3:7]), bc.rodrigues(th),
                                       lambda bs, ps, ra, rb, d: seen.append((bs, ps, ra.shape, rb.shape, d.shape)))
    assert len(seen) == len(tr.levels) and seen[0][2:] == ((6, 3, 3, 3), (6, 3, 3, 3), (6, 3, 3))
    e = dict(pos_q=np.abs(pos_q.numpy() - p64).max(), rot_q=np.abs(bc.quat_matrix(quat.reshape(-1, 4)).numpy()
                                                                   - R64.reshape(-1, 3, 3)).max(),
             pos_m=np.abs(pos_m.numpy() - p64).max(), rot_m=np.abs(rot.numpy() - R64).max())
    print({k: f"{x:.3e}" for k, x in e.items()})
    assert e["pos_q"] <= 2 * 2.879e-7 and e["rot_q"] <= 2 * 4.142e-7
    assert e["pos_m"] <= 2 * 3.375e-7 and e["rot_m"] <= 2 * 2.794e-7


def test_random_state():
    """The seeded states are the ones tools/dynamics_bench.py drew before the function moved: the float64 sums of
    both arrays at n = 4 from default_rng(0), and the digest of their bytes."""
    import hashlib
    root, dof = bc.random_state(4, np.random.default_rng(0))
    assert root.dtype == dof.dtype == np.float32 and root.shape == (4, 13) and dof.shape == (4, 69, 2)
    assert root.astype(np.float64).sum() == 13.22513273358345 and dof.astype(np.float64).sum() == 15.752724203051912
    assert hashlib.sha256(root.tobytes() + dof.tobytes()).hexdigest() == \
        "12d601a6c3368199e04d05b1fca5324d94467a6f2b518bb2dc1112d14d5b830c"
