"""numpy restatement of the three solves that ``include/humanoid_solve.h`` defines, written from the
header's text: ``M`` and ``c`` come from ``dynamics_reference.evaluate`` (the yardstick of the dynamics
tensors), the solves are a dense Cholesky written out here so that they run in the dtype asked for.
float64 is the reference the GPU is held to; float32 against float64 on the same states measures the
reference's own rounding, the floor the GPU tolerance is a multiple of. The tree-sparse L^T D L
factorisation (Featherstone, RBDA 6.5) is restated too: it has no fill-in on the dof tree and must
equal the dense result."""
import numpy as np

import dynamics_reference as DR

NB, ND, NG = DR.NB, DR.ND, DR.NG


def terms(he_model, root, dof, gravity, dtype=np.float64, armature=True, no_gravity=False):
    """(M [n,75,75], c [n,75]) of n states in `dtype`."""
    _, M, c = DR.evaluate(he_model, root, dof, gravity, dtype, armature=armature, no_gravity=no_gravity)
    return M, c


# ------------------------------------------------------------------ dense Cholesky in one dtype
def cholesky(A):
    """Lower G with A = G G^T, every operation in A's dtype."""
    n = A.shape[0]
    G = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - G[j, :j] @ G[j, :j]
        G[j, j] = np.sqrt(d)
        if j + 1 < n:
            G[j + 1:, j] = (A[j + 1:, j] - G[j + 1:, :j] @ G[j, :j]) / G[j, j]
    return G


def cho_solve(G, b):
    """x with G G^T x = b; b [n] or [n,k]."""
    n = G.shape[0]
    y = np.array(b, dtype=G.dtype, copy=True)
    for i in range(n):
        y[i] = (y[i] - G[i, :i] @ y[:i]) / G[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - G[i + 1:, i] @ y[i + 1:]) / G[i, i]
    return y


def spd_solve(A, b):
    return cho_solve(cholesky(A), b)


# ------------------------------------------------------------------ the three solves
def forward_dynamics(M, c, gen_force=None):
    """qdd [n,75] = M^-1 (gen_force - c)."""
    f = np.zeros_like(c) if gen_force is None else np.asarray(gen_force).astype(c.dtype)
    return np.stack([spd_solve(M[e], f[e] - c[e]) for e in range(M.shape[0])])


def computed_torque(M, c, qdd_des, gen_force=None):
    """(tau [n,69], a_b [n,6]) with M (a_b; qdd_des) + c - gen_force = (0_6; tau): the base rows give
    a_b, the joint rows tau."""
    dt = c.dtype
    f = np.zeros_like(c) if gen_force is None else np.asarray(gen_force).astype(dt)
    qd = np.asarray(qdd_des).astype(dt)
    n = M.shape[0]
    tau, ab = np.zeros((n, ND), dt), np.zeros((n, 6), dt)
    for e in range(n):
        ab[e] = spd_solve(M[e, :6, :6], f[e, :6] - c[e, :6] - M[e, :6, 6:] @ qd[e])
        tau[e] = M[e, 6:, :6] @ ab[e] + M[e, 6:, 6:] @ qd[e] + c[e, 6:] - f[e, 6:]
    return tau, ab


def solve(M, rhs):
    """out [n,k,75] with out[e,j] = M[e]^-1 rhs[e,j]."""
    r = np.asarray(rhs).astype(M.dtype)
    return np.stack([spd_solve(M[e], r[e].T).T for e in range(M.shape[0])])


# ------------------------------------------------------------------ the tree-sparse L^T D L
def dof_parents(parents):
    """Parent dof of each of the 75 dofs: the root's six in a chain, a joint's three in a chain below the
    last dof of the parent body."""
    lam = np.full(NG, -1, int)
    for i in range(1, 6):
        lam[i] = i - 1
    for b in range(1, NB):
        d0 = 6 + 3 * (b - 1)
        a = int(parents[b])
        lam[d0] = 5 if a == 0 else 6 + 3 * (a - 1) + 2
        lam[d0 + 1], lam[d0 + 2] = d0, d0 + 1
    return lam


def ltdl(M, lam):
    """(L unit lower, D) with M = L^T D L, touching only entries on the ancestor chains (no fill-in)."""
    H = np.array(M, copy=True)
    n = H.shape[0]
    for k in range(n - 1, -1, -1):
        i = lam[k]
        while i >= 0:
            a = H[k, i] / H[k, k]
            j = i
            while j >= 0:
                H[i, j] = H[i, j] - a * H[k, j]
                j = lam[j]
            H[k, i] = a
            i = lam[i]
    L = np.tril(H, -1) + np.eye(n, dtype=H.dtype)
    # off the chains the lower triangle of M is exactly zero and is never touched
    return L, np.diag(H).copy()


def ltdl_solve(M, lam, b):
    """x = M^-1 b through L^-T, D^-1, L^-1 along the chains; b [n]."""
    L, D = ltdl(M, lam)
    n = M.shape[0]
    x = np.array(b, dtype=M.dtype, copy=True)
    for i in range(n - 1, -1, -1):  # x <- L^-T x
        j = lam[i]
        while j >= 0:
            x[j] = x[j] - L[i, j] * x[i]
            j = lam[j]
    x = x / D
    for i in range(n):  # x <- L^-1 x
        j = lam[i]
        while j >= 0:
            x[i] = x[i] - L[i, j] * x[j]
            j = lam[j]
    return x


# ------------------------------------------------------------------ the figures the tests assert
def forward_error(x, x64):
    """max|x - x64| / max|x64| per env (over every trailing axis). An env whose exact answer is all zero
    (no scale to relate to) asks for exact zeros: 0 when x is, else inf."""
    x = np.asarray(x, np.float64).reshape(x64.shape[0], -1)
    r = x64.reshape(x64.shape[0], -1)
    err, scale = np.abs(x - r).max(axis=1), np.abs(r).max(axis=1)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))


def residual(M64, x, b, normwise=None):
    """Backward error per env; x, b [n,75] or [n,k,75]. Componentwise: max_i |M x - b|_i / (|M||x| + |b|)_i
    (a row whose terms all vanish has no residual: 0). For the envs flagged in `normwise` [n] the largest
    residual over the largest scale instead, max_i |M x - b|_i / max_i (|M||x| + |b|)_i: the figure for a
    state of exact equilibrium, where the exact solution is zero in most entries and the componentwise
    quotient in the rows those entries feed is one rounding over another (1 for any perturbation of the
    exact answer, whatever its size)."""
    x = np.asarray(x, np.float64)
    b = np.asarray(b, np.float64)
    if x.ndim == 2:
        x, b = x[:, None], b[:, None]
    n = x.shape[0]
    num = np.abs(np.einsum("eij,ekj->eki", M64, x) - b).reshape(n, -1)
    den = (np.einsum("eij,ekj->eki", np.abs(M64), np.abs(x)) + np.abs(b)).reshape(n, -1)
    comp = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0).max(axis=1)
    if normwise is None:
        return comp
    dmax = den.max(axis=1)
    norm = np.where(dmax > 0, num.max(axis=1) / np.where(dmax > 0, dmax, 1.0), 0.0)
    return np.where(np.asarray(normwise, bool), norm, comp)


def torque_residual(M64, c64, qdd_des, tau, ab, gen_force=None):
    """Componentwise residual of M (a_b; qdd_des) + c - gen_force - (0; tau) = 0 per env, relative to
    |M||qdd| + |c| + |gen_force| + |(0; tau)| (the terms as they stand in the equation: tau is an output,
    so folding it into a right-hand side would hide its cancellation)."""
    n = M64.shape[0]
    qdd = np.concatenate([np.asarray(ab, np.float64), np.asarray(qdd_des, np.float64)], axis=1)
    t = np.concatenate([np.zeros((n, 6)), np.asarray(tau, np.float64)], axis=1)
    f = np.zeros((n, NG)) if gen_force is None else np.asarray(gen_force, np.float64)
    num = np.abs(np.einsum("eij,ej->ei", M64, qdd) + c64 - f - t)
    den = np.einsum("eij,ej->ei", np.abs(M64), np.abs(qdd)) + np.abs(c64) + np.abs(f) + np.abs(t)
    return (num / den).max(axis=1)
