"""numpy restatement of what ``include/humanoid_ik.h`` defines, written from the header's text: the row
errors on ``dynamics_reference.fk``, an iteration as ``task_reference.task_control`` in force mode at the
resting, gravity-free pose, the integration on the joint manifold, the limits, and the loop with the
iterate rounded to float32 after every iteration, as the output buffers round it. Everything runs in the
dtype asked for: float64 is the reference the GPU is held to, float32 against float64 on the same inputs
measures the reference's own rounding, the floor the GPU tolerance is a multiple of. tests/test_ik.py pins
it. Rotations are composed as unit quaternions (xyzw), from which a rotation vector is read without
cancellation at any angle."""
import numpy as np

import dynamics_reference as DR
import task_reference as TR

NB, ND, NG = DR.NB, DR.ND, DR.NG
MAX_ITERATIONS = 64


# ------------------------------------------------------------------ rotations
def quat_exp(v, dt):
    """quat(exp([v]x)) = (v sin(th / 2) / th, cos(th / 2)); below 1e-3 rad the series, as DR._exp."""
    v = np.asarray(v, dt)
    t2 = v @ v
    if t2 < dt(1e-6):
        s, c = dt(0.5) - t2 / dt(48), dt(1) - t2 / dt(8)
    else:
        th = np.sqrt(t2)
        s, c = np.sin(th / dt(2)) / th, np.cos(th / dt(2))
    return np.array([v[0] * s, v[1] * s, v[2] * s, c], dt)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def quat_unit(q, dt):
    """A stored quaternion, normalised; norm zero stands for the identity."""
    q = np.asarray(q, np.float32).astype(dt)
    n2 = q @ q
    if n2 < dt(1e-24):
        return np.array([0, 0, 0, 1], dt)
    return q / np.sqrt(n2)


def quat_rotvec(q):
    """The rotation vector of a quaternion, angle in [0, pi]: the inverse of quat_exp."""
    dt = q.dtype.type
    if q[3] < 0:
        q = -q
    v, w = q[:3], q[3]
    s2 = v @ v
    if s2 < dt(2.5e-7):
        f = (dt(2) - s2 * dt(2) / dt(3) / (w * w)) / w
    else:
        sn = np.sqrt(s2)
        f = dt(2) * np.arctan2(sn, w) / sn
    return v * f


def matrix_quat(m):
    """A rotation matrix as a quaternion, by the largest of its trace and diagonal (Shepperd)."""
    dt = m.dtype.type
    one, two, q = dt(1), dt(2), dt(0.25)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = two * np.sqrt(tr + one)
        return np.array([(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, q * s], m.dtype)
    if m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = two * np.sqrt(one + m[0, 0] - m[1, 1] - m[2, 2])
        return np.array([q * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s], m.dtype)
    if m[1, 1] > m[2, 2]:
        s = two * np.sqrt(one + m[1, 1] - m[0, 0] - m[2, 2])
        return np.array([(m[0, 1] + m[1, 0]) / s, q * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s], m.dtype)
    s = two * np.sqrt(one + m[2, 2] - m[0, 0] - m[1, 1])
    return np.array([(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, q * s, (m[1, 0] - m[0, 1]) / s], m.dtype)


# ------------------------------------------------------------------ the header's definitions
def fk_pose(Mo, pos, quat, theta):
    """DR.fk on a pose held in the model's dtype (DR.fk rounds its inputs to float32 first): R [24,3,3], p [24,3]."""
    dt = Mo.dtype
    R, p = np.zeros((NB, 3, 3), dt), np.zeros((NB, 3), dt)
    R[0], p[0] = DR._qmat(np.asarray(quat, dt), dt), np.asarray(pos, dt)
    for b in range(1, NB):
        a = Mo.parents[b]
        R[b] = R[a] @ DR._exp(np.asarray(theta, dt)[3 * b - 3:3 * b], dt)
        p[b] = p[a] + R[a] @ Mo.local_pos[b]
    return R, p


def errors_at(Mo, R, p, rows, target, target_rot):
    """e [k] of one env at the bodies' R, p: target [k], target_rot [24,4] or None."""
    dt = Mo.dtype
    e = np.zeros(len(rows), dt)
    for r, (body, axis, point) in enumerate(rows):
        if axis < 3:
            x = p[body] + R[body] @ np.asarray(point, np.float32).astype(dt)
            e[r] = dt(np.float32(target[r])) - x[axis]
        else:
            qb = matrix_quat(R[body])
            qe = quat_mul(quat_unit(target_rot[body], dt), np.array([-qb[0], -qb[1], -qb[2], qb[3]], dt))
            e[r] = quat_rotvec(qe)[axis - 3]
    return e


def row_errors(he_model, root, dof, rows, target, target_rot=None, dtype=np.float64):
    """e [n,k] at the poses root [n,13], dof [n,69,2]."""
    Mo = DR.Model(he_model, dtype)
    out = np.zeros((root.shape[0], len(rows)), dtype)
    for i in range(root.shape[0]):
        R, p = DR.fk(Mo, root[i], dof[i])
        out[i] = errors_at(Mo, R, p, rows, target[i], None if target_rot is None else target_rot[i])
    return out


def step(he_model, root, dof, rows, ebar, damping, dtype=np.float64, armature=True):
    """dq [n,75]: ht_task_control in force mode with xdd_des = ebar and no generalised force, at the poses
    with every velocity zero and without gravity; its qdd. Also the terms it was formed from."""
    root, dof = np.array(root, np.float32), np.array(dof, np.float32)
    root[:, 7:] = 0
    dof[..., 1] = 0
    t = TR.evaluate(he_model, root, dof, rows, (0.0, 0.0, 0.0), dtype, armature=armature, no_gravity=True)
    assert not t.c.any() and not t.b.any()
    _, _, qdd = TR.task_control(t, ebar, None, TR.MODE_FORCE, damping)
    return qdd, t


def limits_of(he_model, dtype=np.float64):
    return (np.array(he_model.dof_lower[:ND], np.float32).astype(dtype),
            np.array(he_model.dof_upper[:ND], np.float32).astype(dtype))


def integrate(root, dof, dq, dtype=np.float64, limits=None):
    """One env's pose (root [13], dof [69,2], any float dtype, taken as they are) moved by dq [75]: the root
    position by dq[0:3], the root quaternion by the world rate dq[3:6] on the left, joint b by its
    child-frame rate on the right, then clamped to limits = (lower, upper) when given. Velocities zero.
    In `dtype`, not rounded."""
    dt = dtype
    root, dof, dq = np.asarray(root).astype(dt), np.asarray(dof).astype(dt), np.asarray(dq).astype(dt)
    r2, d2 = np.zeros(13, dt), np.zeros((ND, 2), dt)
    r2[:3] = root[:3] + dq[:3]
    qr = root[3:7]
    n2 = qr @ qr
    qr = np.array([0, 0, 0, 1], dt) if n2 < dt(1e-24) else qr / np.sqrt(n2)
    q = quat_mul(quat_exp(dq[3:6], dt), qr)
    r2[3:7] = q / np.sqrt(q @ q)
    for b in range(1, NB):
        s = slice(3 * b - 3, 3 * b)
        d2[s, 0] = quat_rotvec(quat_mul(quat_exp(dof[s, 0], dt), quat_exp(dq[6:][s], dt)))
    if limits is not None:
        d2[:, 0] = np.minimum(np.maximum(d2[:, 0], limits[0]), limits[1])
    return r2, d2


def solve(he_model, root, dof, rows, target, target_rot=None, iterations=8, damping=1e-4, step_clip=0.1,
          dtype=np.float64, armature=True, limits=True):
    """hk_solve: (root_out [n,13] float32, dof_out [n,69,2] float32, residual [n,k] in `dtype`). The iterate
    is rounded to float32 after every iteration."""
    assert 1 <= iterations <= MAX_ITERATIONS
    dt = dtype
    r = np.array(root, np.float32)
    d = np.array(dof, np.float32).reshape(-1, ND, 2)
    r[:, 7:] = 0
    d[..., 1] = 0
    lim = limits_of(he_model, dt) if limits else None
    target = np.asarray(target, np.float32)
    for _ in range(iterations):
        e = row_errors(he_model, r, d, rows, target, target_rot, dt)
        ebar = np.clip(e, -dt(np.float32(step_clip)), dt(np.float32(step_clip)))
        dq, _ = step(he_model, r, d, rows, ebar, dt(np.float32(damping)), dt, armature)
        for i in range(r.shape[0]):
            ri, di = integrate(r[i], d[i], dq[i], dt, lim)
            r[i], d[i] = ri.astype(np.float32), di.astype(np.float32)
    return r, d, row_errors(he_model, r, d, rows, target, target_rot, dt)


# ------------------------------------------------------------------ the inputs the tests share
def convergence_rows(names):
    """{k: rows}: k = 6 R_Hand linear and angular; 9 both hands and the head, linear; 12 the offset points of
    task_reference.row_sets; 15 the six of R_Hand plus L_Hand, Head and L_Ankle linear."""
    b = {n: names.index(n) for n in ("L_Hand", "R_Hand", "Head", "L_Ankle")}
    zero = (0.0, 0.0, 0.0)
    lin = lambda body: [(b[body], a, zero) for a in range(3)]  # noqa: E731
    six = [(b["R_Hand"], a, zero) for a in range(6)]
    return {6: six, 9: lin("L_Hand") + lin("R_Hand") + lin("Head"), 12: TR.row_sets(names)[12],
            15: six + lin("L_Hand") + lin("Head") + lin("L_Ankle")}


def convergence_inputs(he_model, n, seed, rest_first=False):
    """(root, dof [n,69,2], goal_root, goal_dof): cases.random_state(ang=0.4) starts with the dofs clamped to
    the limits, and the poses the targets are read from, the starts moved by up to +-0.05 m at the root and
    +-0.15 rad per dof (the root's orientation stays). rest_first: env 0 is as the engine creates it."""
    import cases
    rng = np.random.default_rng(seed)
    root, dof = cases.random_state(n, rng, ang=0.4)
    if rest_first:
        root[0], dof[0] = 0, 0
        root[0, 2], root[0, 6] = 0.89, 1.0
    lo, up = limits_of(he_model, np.float32)
    dof[..., 0] = np.clip(dof[..., 0], lo, up)
    dq = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), np.zeros((n, 3)), rng.uniform(-0.15, 0.15, (n, ND))], axis=1)
    g_root, g_dof = np.zeros_like(root), np.zeros_like(dof)
    for i in range(n):
        ri, di = integrate(root[i], dof[i], dq[i], np.float64)
        g_root[i], g_dof[i] = ri.astype(np.float32), di.astype(np.float32)
    return root, dof, g_root, g_dof


def targets_of(he_model, g_root, g_dof, rows):
    """(target [n,k] float32, target_rot [n,24,4] float32): the rows' places and the bodies' orientations at
    the goal poses."""
    Mo = DR.Model(he_model, np.float64)
    n = g_root.shape[0]
    target, trot = np.zeros((n, len(rows)), np.float32), np.zeros((n, NB, 4), np.float32)
    for i in range(n):
        R, p = DR.fk(Mo, g_root[i], g_dof[i])
        for r, (body, axis, point) in enumerate(rows):
            if axis < 3:
                target[i, r] = (p[body] + R[body] @ np.asarray(point, np.float32).astype(np.float64))[axis]
        trot[i] = np.stack([matrix_quat(R[b]) for b in range(NB)])
    return target, trot
