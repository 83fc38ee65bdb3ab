"""The joint-space vector solves y <- L^-T y and y <- L^-1 y (humanoid_amd/csrc/he_regla.h) with their
lane-masked updates run under EXEC, against the FMA + select form of the same solves and against a
float64 substitution, through the probe entry point he_probe_masked_solves (one wave per vector).

The factor is a random unit-lower L with the SMPL dof tree's sparsity (L[K][j] != 0 only for the
proper ancestors j of K), off-diagonal entries U(-0.3, 0.3), packed as the physics kernel packs it:
row K at kPackStart[K], the entry of the ancestor at tree depth d at offset d (the tables of
tools/gen_topo.py, read from he_smpl_topo.h).

Checks: the EXEC form equals the select form to the bit (same FMAs in the same order on every
register), and both lie within the componentwise forward-error bound of substitution in float32,
n * eps32 * (|T^-1| |T| |x|)_i with T = L^T or L, x the float64 solution, n = 75 and eps32 = 2^-23
(Higham, Accuracy and Stability of Numerical Algorithms, Theorem 8.5: the computed solution solves
(T + dT) x^ = y with |dT| <= gamma_n |T|, the float32 inputs are exact in float64). The bound is
evaluated from the float64 factor for the vectors used; it is zero where the solution is
structurally zero, and there the result must be exactly zero.

Vectors: one dense random vector in a launch of one workgroup; the 75 unit vectors (each pivot of
L^-T and each level member of L^-1 on its own: dofs 63 / 64 / 74 at the register-set boundary, the
five leaf bodies' dofs with no descendants); three different dense vectors in one launch."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 75
FORMS = ("L^-T exec", "L^-T select", "L^-1 exec", "L^-1 select")


def _table(text, name):
    m = re.search(r"constexpr \w+ " + name + r"(?:\[\d+\])? = \{?([^;]*?)\}?;", text)
    return [int(x, 0) for x in re.findall(r"-?\d+", m.group(1))]


def _topo():
    text = open(os.path.join(ROOT, "humanoid_amd", "csrc", "he_smpl_topo.h")).read()
    parent = _table(text, "kDofParent")
    start = _table(text, "kPackStart")
    npack, = _table(text, "kNpack")
    assert len(parent) == NG and len(start) == NG
    return parent, start, npack


def _factor(rng):
    """(dense float32 L, packed float32 factor)"""
    parent, start, npack = _topo()
    L = np.eye(NG, dtype=np.float32)
    packed = np.zeros(npack, np.float32)
    for k in range(NG):
        chain = []
        j = parent[k]
        while j >= 0:
            chain.append(j)
            j = parent[j]
        chain.reverse()  # root first: the ancestor at depth d is chain[d]
        for d, j in enumerate(chain):
            L[k, j] = np.float32(rng.uniform(-0.3, 0.3))
            packed[start[k] + d] = L[k, j]
    return L, packed


def _substitute(T, y):
    """x with T x = y for a unit triangular float64 T (lower or upper), by substitution"""
    n = len(y)
    x = np.array(y, np.float64)
    lower = np.allclose(T, np.tril(T))
    order = range(n) if lower else range(n - 1, -1, -1)
    for i in order:
        x[i] = y[i] - (T[i] @ x - T[i, i] * x[i])
    return x


@pytest.fixture(scope="module")
def solves():
    """(L float64, {case: (y [n][75], out [4][n][75])}) -- one launch per case, computed once"""
    import torch
    from humanoid_amd import engine
    lib = engine.load_library()
    rng = np.random.default_rng(11)
    L, packed = _factor(rng)
    cases = {
        "dense": rng.uniform(-1.0, 1.0, (1, NG)).astype(np.float32),
        "unit": np.eye(NG, dtype=np.float32),
        "three": rng.uniform(-1.0, 1.0, (3, NG)).astype(np.float32),
    }
    d_factor = torch.from_numpy(packed).cuda()
    out = {}
    for name, y in cases.items():
        n = len(y)
        d_y = torch.from_numpy(y).cuda()
        d_out = torch.full((4, n, NG), float("nan"), dtype=torch.float32, device="cuda")
        engine._check(lib.he_probe_masked_solves(d_factor.data_ptr(), d_y.data_ptr(), n, d_out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        out[name] = (y, d_out.cpu().numpy())
    return L.astype(np.float64), out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dense", "unit", "three"])
def test_exec_form_equals_select_form_to_the_bit(solves, case):
    _, out = solves
    _, o = out[case]
    assert not np.isnan(o).any()
    for a, b in ((0, 1), (2, 3)):
        diff = int((o[a].view(np.uint32) != o[b].view(np.uint32)).sum())
        print(f"{case}: {FORMS[a]} vs {FORMS[b]}: {diff} of {o[a].size} words differ")
        assert diff == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dense", "unit", "three"])
def test_solves_within_the_forward_error_bound(solves, case):
    L, out = solves
    y, o = out[case]
    eps32 = float(np.finfo(np.float32).eps)
    Linv = np.stack([_substitute(L, e) for e in np.eye(NG)], axis=1)  # exact zeros outside the tree's pattern
    for form in range(4):
        T = L.T if form < 2 else L
        Tinv = Linv.T if form < 2 else Linv
        cond = np.abs(Tinv) @ np.abs(T)
        worst = 0.0
        for v in range(len(y)):
            x = _substitute(T, y[v].astype(np.float64))
            bound = NG * eps32 * (cond @ np.abs(x))
            err = np.abs(o[form][v].astype(np.float64) - x)
            zero = bound == 0.0
            assert (o[form][v][zero] == 0.0).all()
            worst = max(worst, float((err[~zero] / bound[~zero]).max()))
            assert (err <= bound).all(), (FORMS[form], v, float((err - bound).max()))
        print(f"{case}: {FORMS[form]}: max error / bound = {worst:.3g}")

