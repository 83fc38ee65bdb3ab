"""numpy restatement of what ``include/humanoid_task.h`` defines, written from the header's text: the task
Jacobian rows and Jdot qd from ``dynamics_reference`` (J, M, c, body_velocities), the solves by the dense
Cholesky of ``solve_reference`` so that everything runs in the dtype asked for. float64 is the reference the
GPU is held to; float32 against float64 on the same states and inputs measures the reference's own
rounding, the floor the GPU tolerance is a multiple of. tests/test_task.py pins it (a finite difference
of J qd, the task equation, the two modes' defining properties)."""
import numpy as np

import dynamics_reference as DR
import solve_reference as SR

NB, ND, NG = DR.NB, DR.ND, DR.NG
MAX_ROWS = 32
MODE_FORCE, MODE_JOINT = 0, 1


# ------------------------------------------------------------------ the row sets the tests share
def row_sets(names):
    """{k: rows} with rows = [(body, axis, point)]. Every set holds R_Hand, whose columns 72..74 are in
    the kernel's 11-column register tail. k = 12 has points a few centimetres off the body origins; k = 31 and
    32 add the pelvis origin's x and y (the pair of pelvis rows that conditions A best: 1.1e4 in force mode,
    3.2e5 in joint mode on five_states(), where its z or its angular x reach 1e5 and 2e6)."""
    b = {n: names.index(n) for n in ("Pelvis", "L_Hand", "R_Hand", "L_Ankle", "R_Ankle", "L_Toe", "R_Toe", "Head")}
    zero = (0.0, 0.0, 0.0)
    six = lambda body: [(body, a, zero) for a in range(6)]  # noqa: E731
    k30 = six(b["L_Hand"]) + six(b["R_Hand"]) + six(b["L_Ankle"]) + six(b["R_Ankle"]) + six(b["Head"])
    offs = {"L_Hand": (0.03, -0.02, 0.01), "R_Hand": (0.03, 0.02, -0.015), "L_Toe": (0.05, 0.01, -0.02),
            "R_Toe": (0.05, -0.01, -0.02)}
    k12 = [(b[n], a, offs[n]) for n in ("L_Hand", "R_Hand", "L_Toe", "R_Toe") for a in range(3)]
    return {1: [(b["R_Hand"], 0, zero)], 6: six(b["R_Hand"]), 12: k12, 30: k30,
            31: k30 + [(b["Pelvis"], 0, zero)], 32: k30 + [(b["Pelvis"], 0, zero), (b["Pelvis"], 1, zero)]}


def five_states():
    """The five states of tests/test_gpu_dynamics.py's ctx, for the tests that run without a GPU: env 0 as
    the engine creates it (standing at the origin, at rest), 1-3 random tumbling, 4 all-zero dof angles
    with nonzero rates."""
    import cases
    root, dof = cases.random_state(4, np.random.default_rng(11), height=(1.0, 2.0), vel=1.0, ang=0.6, tilt=0.8)
    r = np.zeros((5, 13), np.float32)
    d = np.zeros((5, ND, 2), np.float32)
    r[0, 2], r[0, 6] = 0.89, 1.0
    r[1:4], d[1:4] = root[:3], dof[:3]
    r[4], d[4] = root[3], dof[3]
    d[4, :, 0] = 0.0
    return r, d


five_states.__test__ = False


# ------------------------------------------------------------------ the header's definitions
def task_jacobian(Mo, R, J, rows):
    """J_r [k,75] of one env from its body rotations and body Jacobians J [24,6,75]."""
    dt = Mo.dtype
    out = np.zeros((len(rows), NG), dt)
    for r, (body, axis, point) in enumerate(rows):
        if axis >= 3:
            out[r] = J[body, axis]
        else:
            lever = R[body] @ np.asarray(point, np.float32).astype(dt)
            out[r] = J[body, axis] + np.cross(J[body, 3:6].T, lever)[:, axis]
    return out


def bias_acceleration(Mo, R, p, root, dof, rows):
    """b = Jdot qd [k] of one env: the rows' accelerations at qdd = 0."""
    dt = Mo.dtype
    w, wd, acc = DR.body_velocities(Mo, R, p, root, dof)
    out = np.zeros(len(rows), dt)
    for r, (body, axis, point) in enumerate(rows):
        if axis >= 3:
            out[r] = wd[body, axis - 3]
        else:
            lever = R[body] @ np.asarray(point, np.float32).astype(dt)
            out[r] = (acc[body] + np.cross(wd[body], lever) + np.cross(w[body], np.cross(w[body], lever)))[axis]
    return out


def pattern(parents, rows):
    """[k,75] bool: the columns a row may be nonzero in (joints that are ancestor-or-self of its body)."""
    jm = DR.jacobian_mask(parents)
    return np.array([jm[body] for body, _, _ in rows])


class Terms:
    """J [n,k,75], M [n,75,75], c [n,75], b [n,k] of n states in one dtype."""


def body_terms(he_model, root, dof, gravity, dtype=np.float64, armature=True, no_gravity=False):
    """What does not depend on the rows, per env: (R, p, body Jacobians, M, c). evaluate() takes it as
    `bodies`, so that tests with several row sets form M and c once."""
    Mo = DR.Model(he_model, dtype)
    g = (0.0, 0.0, 0.0) if no_gravity else gravity
    out = []
    for e in range(root.shape[0]):
        R, p = DR.fk(Mo, root[e], dof[e])
        Jb = DR.jacobian(Mo, R, p)
        out.append((R, p, Jb, DR.mass_matrix(Mo, R, Jb, armature), DR.bias_force(Mo, R, p, Jb, root[e], dof[e], g)))
    return out


def evaluate(he_model, root, dof, rows, gravity, dtype=np.float64, armature=True, no_gravity=False, bodies=None):
    Mo = DR.Model(he_model, dtype)
    n, k = root.shape[0], len(rows)
    if bodies is None:
        bodies = body_terms(he_model, root, dof, gravity, dtype, armature, no_gravity)
    t = Terms()
    t.dtype, t.rows = dtype, rows
    t.J, t.b = np.zeros((n, k, NG), dtype), np.zeros((n, k), dtype)
    t.M, t.c = np.stack([b[3] for b in bodies]), np.stack([b[4] for b in bodies])
    assert t.M.dtype == dtype
    for e, (R, p, Jb, _, _) in enumerate(bodies):
        t.J[e] = task_jacobian(Mo, R, Jb, rows)
        t.b[e] = bias_acceleration(Mo, R, p, root[e], dof[e], rows)
    return t


def _force(t, gen_force):
    return np.zeros_like(t.c) if gen_force is None else np.asarray(gen_force).astype(t.dtype)


def task_terms(t, gen_force=None):
    """(Y = J M^-1 [n,k,75], Lambda^-1 = Y J^T [n,k,k], xdd_free = Y (f - c) + b [n,k])."""
    f = _force(t, gen_force)
    n = t.M.shape[0]
    Y = np.stack([SR.spd_solve(t.M[e], t.J[e].T).T for e in range(n)])
    Li = np.einsum("eic,ejc->eij", Y, t.J)
    free = np.einsum("eic,ec->ei", Y, f - t.c) + t.b
    return Y, Li, free


def system_matrix(t, Y, Li, mode, damping):
    """A [n,k,k] of the task solve: Lambda^-1 + damping I, or Yj Yj^T + damping I."""
    k = Y.shape[1]
    A = Li if mode == MODE_FORCE else np.einsum("eic,ejc->eij", Y[:, :, 6:], Y[:, :, 6:])
    return A + t.dtype(damping) * np.eye(k, dtype=t.dtype)


def task_control(t, xdd_des, gen_force=None, mode=MODE_FORCE, damping=0.0):
    """(u [n,75], F [n,k], qdd [n,75]) of ht_task_control."""
    f = _force(t, gen_force)
    n = t.M.shape[0]
    Y, Li, free = task_terms(t, gen_force)
    r = np.asarray(xdd_des).astype(t.dtype) - free
    A = system_matrix(t, Y, Li, mode, damping)
    F = np.stack([SR.spd_solve(A[e], r[e]) for e in range(n)])
    if mode == MODE_FORCE:
        u = np.einsum("ekc,ek->ec", t.J, F)
    else:
        u = np.einsum("ekc,ek->ec", Y, F)
        u[:, :6] = 0
    qdd = np.stack([SR.spd_solve(t.M[e], f[e] + u[e] - t.c[e]) for e in range(n)])
    return u, F, qdd


def task_acceleration(t64, qdd):
    """J qdd + b [n,k] with the float64 terms."""
    return np.einsum("ekc,ec->ek", t64.J, np.asarray(qdd, np.float64)) + t64.b
