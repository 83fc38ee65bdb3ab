"""numpy restatement of the three tensors that ``include/humanoid_dynamics.h`` defines (written from the
header's text; nothing imported from the product beyond ``_abi`` and the model blob): forward
kinematics, the subtree columns of the body Jacobians, the mass matrix as the kinetic-energy metric
about the bodies' centres of mass, and the bias force by virtual power of the Newton-Euler wrenches.
``evaluate`` takes a dtype: float64 is the reference the GPU is held to, float32 against float64
measures the reference's own rounding (the floor the GPU tolerance is a multiple of)."""
import numpy as np

NB, ND, NG = 24, 69, 75
# generalised-velocity order: the header's (root linear, root angular, dofs) from the oracle's (w, v, dofs)
PERM = np.array([3, 4, 5, 0, 1, 2] + list(range(6, NG)))


class Model:
    """The model blob as arrays of one dtype."""

    def __init__(self, m, dtype=np.float64):
        self.dtype = dtype
        self.parents = np.array(m.parents[:NB])
        self.local_pos = np.array([list(m.local_pos[b]) for b in range(NB)], np.float32).astype(dtype)
        self.mass = np.array(m.mass[:NB], np.float32).astype(dtype)
        self.com = np.array([list(m.com[b]) for b in range(NB)], np.float32).astype(dtype)
        ib = np.array([list(m.inertia[b]) for b in range(NB)], np.float32).astype(dtype)
        self.I = np.array([[[i[0], i[3], i[4]], [i[3], i[1], i[5]], [i[4], i[5], i[2]]] for i in ib], dtype)
        self.armature = np.array(m.armature[:ND], np.float32).astype(dtype)
        # subtree mask: sub[j, b] = j is an ancestor of b or b itself
        self.sub = np.zeros((NB, NB), bool)
        for b in range(NB):
            a = b
            while a >= 0:
                self.sub[a, b] = True
                a = self.parents[a]


def col_joint(c):
    return 0 if c < 6 else 1 + (c - 6) // 3


def jacobian_mask(parents):
    """[24,75] bool: column c may be nonzero in body b's rows (root columns everywhere, a dof column of
    joint j in j's subtree)."""
    sub = np.zeros((NB, NB), bool)
    for b in range(NB):
        a = b
        while a >= 0:
            sub[a, b] = True
            a = parents[a]
    return np.array([[sub[col_joint(c), b] for c in range(NG)] for b in range(NB)])


def mass_mask(parents):
    """[75,75] bool: M[i,k] may be nonzero (one column's joint is an ancestor-or-self of the other's)."""
    jm = jacobian_mask(parents)  # jm[b, c]: joint(c) ancestor-or-self of b
    j = [col_joint(c) for c in range(NG)]
    return np.array([[jm[j[i], k] or jm[j[k], i] for k in range(NG)] for i in range(NG)])


def _skew(v, dtype):
    z = dtype(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype)


def _exp(v, dtype):
    """Rodrigues; below 1e-3 rad the series."""
    t2 = v @ v
    K = _skew(v, dtype)
    if t2 < dtype(1e-6):
        A, B = dtype(1) - t2 / dtype(6), dtype(0.5) - t2 / dtype(24)
    else:
        th = np.sqrt(t2)
        A, B = np.sin(th) / th, (dtype(1) - np.cos(th)) / t2
    return np.eye(3, dtype=dtype) + A * K + B * (K @ K)


def _qmat(q, dtype):
    x, y, z, w = q / np.sqrt(q @ q)
    o, t = dtype(1), dtype(2)
    return np.array([[o - t * (y * y + z * z), t * (x * y - z * w), t * (x * z + y * w)],
                     [t * (x * y + z * w), o - t * (x * x + z * z), t * (y * z - x * w)],
                     [t * (x * z - y * w), t * (y * z + x * w), o - t * (x * x + y * y)]], dtype)


def fk(Mo, root, dof):
    """R [24,3,3], p [24,3] of one env from its root row [13] and dof rows [69,2]."""
    dt = Mo.dtype
    root = np.asarray(root, np.float32).astype(dt)
    th = np.asarray(dof, np.float32)[:, 0].astype(dt)
    R = np.zeros((NB, 3, 3), dt)
    p = np.zeros((NB, 3), dt)
    R[0], p[0] = _qmat(root[3:7], dt), root[:3]
    for b in range(1, NB):
        a = Mo.parents[b]
        R[b] = R[a] @ _exp(th[3 * b - 3:3 * b], dt)
        p[b] = p[a] + R[a] @ Mo.local_pos[b]
    return R, p


def gen_velocity(root, dof, dtype=np.float64):
    """qd [75]: root linear, root angular, the 69 dof velocities (child-frame relative rates)."""
    return np.concatenate([root[7:10], root[10:13], np.asarray(dof)[:, 1]]).astype(np.float32).astype(dtype)


def jacobian(Mo, R, p):
    """J [24,6,75]: rows (origin linear velocity, world angular velocity)."""
    dt = Mo.dtype
    J = np.zeros((NB, 6, NG), dt)
    eye = np.eye(3, dtype=dt)
    for b in range(NB):
        J[b, 0:3, 0:3] = eye
        for i in range(3):
            J[b, 0:3, 3 + i] = np.cross(eye[i], p[b] - p[0])
            J[b, 3:6, 3 + i] = eye[i]
        for j in range(1, NB):
            if not Mo.sub[j, b]:
                continue
            for i in range(3):
                a = R[j][:, i]
                J[b, 0:3, 6 + 3 * (j - 1) + i] = np.cross(a, p[b] - p[j])
                J[b, 3:6, 6 + 3 * (j - 1) + i] = a
    return J


def _com_jacobian(Mo, R, J):
    """Jc [24,3,75] of the centres of mass: v_c = v_origin + w x (R com)."""
    rc = np.einsum("bij,bj->bi", R, Mo.com)
    return J[:, 0:3] + np.cross(J[:, 3:6], rc[:, :, None], axis=1)


def mass_matrix(Mo, R, J, armature):
    """M = sum_b m Jc^T Jc + Jw^T (R I R^T) Jw, plus the armature on the dof diagonal when asked."""
    Jc = _com_jacobian(Mo, R, J)
    M = np.zeros((NG, NG), Mo.dtype)
    for b in range(NB):
        Iw = R[b] @ Mo.I[b] @ R[b].T
        Jw = J[b, 3:6]
        M += Mo.mass[b] * (Jc[b].T @ Jc[b]) + Jw.T @ (Iw @ Jw)
    if armature:
        M[np.arange(6, NG), np.arange(6, NG)] += Mo.armature
    return M


def body_velocities(Mo, R, p, root, dof):
    """World angular velocity, and at qdd = 0 the angular acceleration and the origin acceleration, of
    every body [24,3] each: w_b = w_a + R_b u_b, wd_b = wd_a + w_a x (R_b u_b),
    a_b = a_a + wd_a x d + w_a x (w_a x d) with d = p_b - p_a."""
    dt = Mo.dtype
    qd = gen_velocity(root, dof, dt)
    w, wd, acc = np.zeros((NB, 3), dt), np.zeros((NB, 3), dt), np.zeros((NB, 3), dt)
    w[0] = qd[3:6]
    for b in range(1, NB):
        a = Mo.parents[b]
        wrel = R[b] @ qd[6 + 3 * (b - 1):9 + 3 * (b - 1)]
        d = p[b] - p[a]
        w[b] = w[a] + wrel
        wd[b] = wd[a] + np.cross(w[a], wrel)
        acc[b] = acc[a] + np.cross(wd[a], d) + np.cross(w[a], np.cross(w[a], d))
    return w, wd, acc


def bias_force(Mo, R, p, J, root, dof, gravity):
    """c = sum_b Jc^T m (a_c - g) + Jw^T (I_w wd + w x I_w w): the Newton-Euler wrenches at qdd = 0
    mapped to generalised forces by virtual power."""
    dt = Mo.dtype
    g = np.asarray(gravity, np.float32).astype(dt)
    w, wd, acc = body_velocities(Mo, R, p, root, dof)
    Jc = _com_jacobian(Mo, R, J)
    c = np.zeros(NG, dt)
    for b in range(NB):
        rc = R[b] @ Mo.com[b]
        ac = acc[b] + np.cross(wd[b], rc) + np.cross(w[b], np.cross(w[b], rc))
        Iw = R[b] @ Mo.I[b] @ R[b].T
        F = Mo.mass[b] * (ac - g)
        T = Iw @ wd[b] + np.cross(w[b], Iw @ w[b])
        c += Jc[b].T @ F + J[b, 3:6].T @ T
    return c


def evaluate(he_model, root, dof, gravity=(0.0, 0.0, -9.81), dtype=np.float64, armature=True, no_gravity=False):
    """(J [n,24,6,75], M [n,75,75], c [n,75]) of n states (root [n,13], dof [n,69,2]) in `dtype`."""
    Mo = Model(he_model, dtype)
    n = root.shape[0]
    J = np.zeros((n, NB, 6, NG), dtype)
    M = np.zeros((n, NG, NG), dtype)
    c = np.zeros((n, NG), dtype)
    g = (0.0, 0.0, 0.0) if no_gravity else gravity
    for e in range(n):
        R, p = fk(Mo, root[e], dof[e])
        J[e] = jacobian(Mo, R, p)
        M[e] = mass_matrix(Mo, R, J[e], armature)
        c[e] = bias_force(Mo, R, p, J[e], root[e], dof[e], g)
    return J, M, c


def test_states(he_model):
    """The states the dynamics tests share: the four random ones of tests/test_independent_dynamics.py,
    one with every dof exactly 0 (the small-angle branch) but moving, one with a joint near 2.5 rad."""
    import cases
    root, dof = cases.random_state(4, np.random.default_rng(11), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
    r2, d2 = cases.random_state(2, np.random.default_rng(12), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
    d2[0, :, 0] = 0.0
    ax = np.array([0.6, -0.64, 0.48], np.float32)  # unit
    d2[1, 3 * 4:3 * 4 + 3, 0] = 2.5 * ax   # joint of body 5
    d2[1, 3 * 17:3 * 17 + 3, 0] = -2.45 * ax[::-1]
    return np.concatenate([root, r2]), np.concatenate([dof, d2])


test_states.__test__ = False  # a helper, not a test
