"""numpy restatement of what ``include/humanoid_derivatives.h`` defines: the derivatives of the inverse
dynamics ``tau(q, qd, a) = M(q) a + c(q, qd)`` with respect to the pose and the generalised velocity, and
from them those of the forward dynamics.

``dynamics_reference.fk`` and ``gen_velocity`` round the state to float32, which a difference quotient
cannot stand, so the kinematics, the body velocities and the bias force are restated here unrounded: the
base point is the float32 state taken exactly, and nothing around it is rounded. Three things are given:

* ``fd_dq`` / ``fd_dv``: the definition itself, Richardson-extrapolated central differences in float64 of
  ``tau`` along ``ik_reference.integrate`` (the header's ``q (+) delta``);
* ``exact``: the exact derivative in the dtype asked for, by propagating the tangent of every body's
  velocity, acceleration and Newton-Euler wrench. float64 is what the GPU is held to; float32 against
  float64 on the same states is the reference's own rounding, the floor the GPU tolerance is a multiple of;
* ``forward``: the derivatives of ``qdd = M^-1 (gen_force - c)`` through ``solve_reference``.
"""
import numpy as np

import dynamics_reference as DR
import ik_reference as IK
import solve_reference as SR

NB, ND, NG = DR.NB, DR.ND, DR.NG
H_Q = (1e-4, 5e-5)  # the two steps of the pose differences
H_V = 1e-2          # tau is quadratic in qd: any step is exact up to rounding


# ------------------------------------------------------------------ the state, unrounded
def split_state(root, dof, dt=np.float64):
    """(pos [3], quat [4], theta [69], qd [75]) of one env: the float32 values exactly, in dt."""
    root = np.asarray(root, np.float32).astype(dt)
    dof = np.asarray(dof, np.float32).astype(dt)
    return root[:3], root[3:7], dof[:, 0], np.concatenate([root[7:10], root[10:13], dof[:, 1]])


def moved(pos, quat, theta, delta, dt=np.float64):
    """The pose q (+) delta (ik_reference.integrate, unrounded)."""
    root = np.concatenate([pos, quat, np.zeros(6, dt)])
    dof = np.stack([theta, np.zeros(ND, dt)], axis=1)
    r2, d2 = IK.integrate(root, dof, delta, dt)
    return r2[:3], r2[3:7], d2[:, 0]


def kinematics(Mo, R, p, qd, acc):
    """Per body [24,3]: the angular velocity, the angular acceleration, the origin's acceleration (both
    with the generalised acceleration acc [75] and the velocity products) and the origin's velocity
    relative to the root origin's."""
    dt = Mo.dtype
    w, wd, A, V = (np.zeros((NB, 3), dt) for _ in range(4))
    w[0], wd[0], A[0] = qd[3:6], acc[3:6], acc[0:3]
    for b in range(1, NB):
        a = Mo.parents[b]
        s = slice(6 + 3 * (b - 1), 9 + 3 * (b - 1))
        wrel = R[b] @ qd[s]
        d = p[b] - p[a]
        w[b] = w[a] + wrel
        wd[b] = wd[a] + np.cross(w[a], wrel) + R[b] @ acc[s]
        A[b] = A[a] + np.cross(wd[a], d) + np.cross(w[a], np.cross(w[a], d))
        V[b] = V[a] + np.cross(w[a], d)
    return w, wd, A, V


def body_wrenches(Mo, R, w, wd, A, g):
    """Per body: rc = R com, I_w, the force m (a_c - g) and the torque about the centre of mass."""
    dt = Mo.dtype
    rc, f, t = (np.zeros((NB, 3), dt) for _ in range(3))
    Iw = np.zeros((NB, 3, 3), dt)
    for b in range(NB):
        rc[b] = R[b] @ Mo.com[b]
        Iw[b] = R[b] @ Mo.I[b] @ R[b].T
        ac = A[b] + np.cross(wd[b], rc[b]) + np.cross(w[b], np.cross(w[b], rc[b]))
        f[b] = Mo.mass[b] * (ac - g)
        t[b] = Iw[b] @ wd[b] + np.cross(w[b], Iw[b] @ w[b])
    return rc, Iw, f, t


def subtree_wrenches(Mo, p, rc, f, t):
    """(N [24,3], F [24,3]): every subtree's wrench about its own joint origin, by explicit sums."""
    dt = Mo.dtype
    N, F = np.zeros((NB, 3), dt), np.zeros((NB, 3), dt)
    c = p + rc
    for j in range(NB):
        s = Mo.sub[j]
        F[j] = f[s].sum(axis=0)
        N[j] = (t[s] + np.cross(c[s] - p[j], f[s])).sum(axis=0)
    return N, F


def tau_of(Mo, R, N, F, acc, armature):
    dt = Mo.dtype
    tau = np.zeros(NG, dt)
    tau[0:3], tau[3:6] = F[0], N[0]
    for j in range(1, NB):
        for i in range(3):
            c = 6 + 3 * (j - 1) + i
            tau[c] = R[j][:, i] @ N[j] + (Mo.armature[c - 6] * acc[c] if armature else dt(0))
    return tau


def tau_at(Mo, pos, quat, theta, qd, acc, g, armature):
    """tau [75] = M a + c at an unrounded pose and velocity, by Newton-Euler."""
    R, p = IK.fk_pose(Mo, pos, quat, theta)
    p = p - p[0]
    w, wd, A, _ = kinematics(Mo, R, p, qd, acc)
    rc, _, f, t = body_wrenches(Mo, R, w, wd, A, g)
    N, F = subtree_wrenches(Mo, p, rc, f, t)
    return tau_of(Mo, R, N, F, acc, armature)


def tau_by_matrices(Mo, pos, quat, theta, qd, acc, g, armature):
    """The same tau as the header writes it, M a + c with dynamics_reference's mass matrix and a bias
    force by virtual power: the check that tau_at restates the definition."""
    dt = Mo.dtype
    R, p = IK.fk_pose(Mo, pos, quat, theta)
    J = DR.jacobian(Mo, R, p)
    M = DR.mass_matrix(Mo, R, J, armature)
    w, wd, A, _ = kinematics(Mo, R, p - p[0], qd, np.zeros(NG, dt))
    rc, _, f, t = body_wrenches(Mo, R, w, wd, A, g)
    Jc = DR._com_jacobian(Mo, R, J)
    c = np.zeros(NG, dt)
    for b in range(NB):
        c += Jc[b].T @ f[b] + J[b, 3:6].T @ t[b]
    return M @ acc + c


# ------------------------------------------------------------------ (a) the definition, by differences
def _central(fun, h):
    cols = []
    for j in range(NG):
        e = np.zeros(NG)
        e[j] = h
        cols.append((fun(e) - fun(-e)) / (2 * h))
    return np.stack(cols, axis=1)


def _richardson(fun, h, h2):
    """Central differences at h and h2 = h / 2, extrapolated: the h^2 term cancels."""
    return (4.0 * _central(fun, h2) - _central(fun, h)) / 3.0


def fd_dq(Mo, state, acc, g, armature, steps=H_Q):
    pos, quat, theta, qd = state
    return _richardson(lambda d: tau_at(Mo, *moved(pos, quat, theta, d), qd, acc, g, armature), *steps)


def fd_dv(Mo, state, acc, g, armature, h=H_V):
    pos, quat, theta, qd = state
    return _central(lambda d: tau_at(Mo, pos, quat, theta, qd + d, acc, g, armature), h)


# ------------------------------------------------------------------ (b) the exact derivative
def _tangents(Mo, R, p, w, wd, A, V, rc, Iw, f, t, N, F, velocity):
    """One [75,75] matrix of d tau_i along direction j, every direction at once (arrays [nj,3]). Direction
    j belongs to joint k = col_joint(j) with the world axis ax through p_k; only the bodies of sub(k) move.
    Per body b of sub(k): phi, the rate at which the subtree's geometry turns (ax for a pose direction, 0
    for a velocity direction), and the tangents dw, dwd, dA of its angular velocity, angular acceleration and
    origin acceleration; from them the tangent of its Newton-Euler wrench. The bodies go deepest first, each
    adds its subtree's tangent wrench about its own origin to its parent's; a row of joint m is then its
    axis on that wrench (plus the turning axis on the wrench itself) inside sub(k), and its axis on subtree
    k's tangent wrench carried, unrotated, to p_m for the ancestors of k."""
    dt = Mo.dtype
    par = Mo.parents
    two = dt(2)
    eye = np.eye(3, dtype=dt)
    cols = np.arange(3, NG)
    K = np.array([DR.col_joint(j) for j in cols])
    ax = np.stack([eye[j - 3] if j < 6 else R[DR.col_joint(j)][:, (j - 6) % 3] for j in cols])
    carrier = np.where(K > 0, par[K], 0)
    # the carrier of k: its parent; for the root its own world rates and accelerations, which are held
    # (a velocity direction of the root has no carrier: its rate is the coordinate itself)
    wa_all = w[carrier] if not velocity else np.where((K > 0)[:, None], w[carrier], dt(0))
    wda_all = wd[carrier]
    dN, dF = np.zeros((NB, NG - 3, 3), dt), np.zeros((NB, NG - 3, 3), dt)
    out = np.zeros((NG, NG), dt)
    cr = np.cross
    for b in range(NB - 1, -1, -1):
        s = Mo.sub[K, b]  # the directions that move body b
        if not s.any():
            continue
        a_, k, wa, wda = ax[s], K[s], wa_all[s], wda_all[s]
        r = p[b] - p[k]
        if not velocity:
            rho = w[b] - wa
            vrel = V[b] - V[k] - cr(wa, r)
            arel = A[b] - A[k] - cr(wda, r) - cr(wa, cr(wa, r)) - two * cr(wa, vrel)
            wr = cr(a_, r)
            phi, dw = a_, cr(a_, rho)
            dwd = cr(wa, dw) + cr(a_, wd[b] - wda - cr(wa, rho))
            dA = cr(wda, wr) + cr(wa, cr(wa, wr)) + two * cr(wa, cr(a_, vrel)) + cr(a_, arel)
        else:
            phi, dw = np.zeros_like(a_), a_
            dwd = cr(wa, a_) + cr(a_, w[b] - w[k])
            dA = cr(cr(wa, a_) - cr(a_, w[k]), r) + two * cr(a_, V[b] - V[k])
        I = Iw[b]
        drc = cr(phi, rc[b])
        dac = (dA + cr(dwd, rc[b]) + cr(wd[b], drc) + cr(dw, cr(w[b], rc[b])) + cr(w[b], cr(dw, rc[b]))
               + cr(w[b], cr(w[b], drc)))
        df = Mo.mass[b] * dac
        Iww = I @ w[b]
        dIwd = cr(phi, I @ wd[b]) - cr(phi, wd[b]) @ I.T
        dIw = cr(phi, Iww) - cr(phi, w[b]) @ I.T
        dtq = dIwd + dwd @ I.T + cr(dw, Iww) + cr(w[b], dIw + dw @ I.T)
        dN[b, s] = dN[b, s] + dtq + cr(drc, f[b]) + cr(rc[b], df)
        dF[b, s] = dF[b, s] + df
        up = s & (K != b)
        if up.any():
            a = par[b]
            lever = p[b] - p[a]
            phi_up = ax[up] if not velocity else np.zeros_like(ax[up])
            dN[a, up] = dN[a, up] + dN[b, up] + cr(cr(phi_up, lever), F[b]) + cr(lever, dF[b, up])
            dF[a, up] = dF[a, up] + dF[b, up]
    idx = np.arange(NG - 3)
    kN, kF = dN[K, idx], dF[K, idx]  # subtree k's tangent wrench about p_k, per direction
    for m in range(NB):
        inside = Mo.sub[K, m]
        above = Mo.sub[m, K] & ~inside
        XN, XF = np.zeros((NG - 3, 3), dt), np.zeros((NG - 3, 3), dt)
        XN[inside], XF[inside] = dN[m, inside], dF[m, inside]
        XN[above], XF[above] = kN[above] + cr(p[K[above]] - p[m], kF[above]), kF[above]
        if m == 0:
            out[0:3, 3:], out[3:6, 3:] = XF.T, XN.T
            continue
        for i in range(3):
            sx = R[m][:, i]
            v = XN @ sx
            if not velocity:
                v = v + np.where(inside, cr(ax, sx) @ N[m], dt(0))
            out[6 + 3 * (m - 1) + i, 3:] = v
    return out


def exact_env(Mo, state, acc, g, armature):
    """(tau [75], dtau_dq [75,75], dtau_dv [75,75]) of one env in Mo.dtype."""
    pos, quat, theta, qd = state
    R, p = IK.fk_pose(Mo, pos, quat, theta)
    p = p - p[0]
    w, wd, A, V = kinematics(Mo, R, p, qd, acc)
    rc, Iw, f, t = body_wrenches(Mo, R, w, wd, A, g)
    N, F = subtree_wrenches(Mo, p, rc, f, t)
    args = (Mo, R, p, w, wd, A, V, rc, Iw, f, t, N, F)
    return tau_of(Mo, R, N, F, acc, armature), _tangents(*args, False), _tangents(*args, True)


def _acc(acc, n, dt):
    return np.zeros((n, NG), dt) if acc is None else np.asarray(acc, np.float32).reshape(n, NG).astype(dt)


def _gravity(gravity, no_gravity, dt):
    return np.zeros(3, dt) if no_gravity else np.asarray(gravity, np.float32).astype(dt)


def exact(he_model, root, dof, acc=None, gravity=(0.0, 0.0, -9.81), dtype=np.float64, armature=True,
          no_gravity=False):
    """dict(tau [n,75], dtau_dq [n,75,75], dtau_dv [n,75,75]) of n states in `dtype`."""
    Mo = DR.Model(he_model, dtype)
    n = root.shape[0]
    a, g = _acc(acc, n, dtype), _gravity(gravity, no_gravity, dtype)
    out = dict(tau=np.zeros((n, NG), dtype), dtau_dq=np.zeros((n, NG, NG), dtype), dtau_dv=np.zeros((n, NG, NG), dtype))
    for e in range(n):
        out["tau"][e], out["dtau_dq"][e], out["dtau_dv"][e] = exact_env(Mo, split_state(root[e], dof[e], dtype), a[e],
                                                                        g, armature)
    return out


def differences(he_model, root, dof, acc=None, gravity=(0.0, 0.0, -9.81), armature=True, no_gravity=False):
    """The same dict by float64 differences of tau (the definition)."""
    Mo = DR.Model(he_model, np.float64)
    n = root.shape[0]
    a, g = _acc(acc, n, np.float64), _gravity(gravity, no_gravity, np.float64)
    out = dict(tau=np.zeros((n, NG)), dtau_dq=np.zeros((n, NG, NG)), dtau_dv=np.zeros((n, NG, NG)))
    for e in range(n):
        st = split_state(root[e], dof[e])
        out["tau"][e] = tau_at(Mo, *st, a[e], g, armature)
        out["dtau_dq"][e] = fd_dq(Mo, st, a[e], g, armature)
        out["dtau_dv"][e] = fd_dv(Mo, st, a[e], g, armature)
    return out


# ------------------------------------------------------------------ (c) the forward form
def mass_and_bias(Mo, state, g, armature):
    pos, quat, theta, qd = state
    R, p = IK.fk_pose(Mo, pos, quat, theta)
    M = DR.mass_matrix(Mo, R, DR.jacobian(Mo, R, p), armature)
    return M, tau_at(Mo, pos, quat, theta, qd, np.zeros(NG, Mo.dtype), g, False)


def forward_env(Mo, state, gen_force, g, armature):
    """(qdd [75], dqdd_dq, dqdd_dv, dqdd_dtau [75,75]) of one env: qdd = M^-1 (gen_force - c), then
    -M^-1 dtau/dq and -M^-1 dtau/dv at a = qdd, and M^-1, all through solve_reference's Cholesky."""
    M, c = mass_and_bias(Mo, state, g, armature)
    G = SR.cholesky(M)
    qdd = SR.cho_solve(G, gen_force - c)
    _, dq, dv = exact_env(Mo, state, qdd, g, armature)
    return qdd, -SR.cho_solve(G, dq), -SR.cho_solve(G, dv), SR.cho_solve(G, np.eye(NG, dtype=Mo.dtype))


def forward(he_model, root, dof, gen_force=None, gravity=(0.0, 0.0, -9.81), dtype=np.float64, armature=True,
            no_gravity=False):
    """dict(qdd [n,75], dqdd_dq, dqdd_dv, dqdd_dtau [n,75,75]) of n states in `dtype`."""
    Mo = DR.Model(he_model, dtype)
    n = root.shape[0]
    f, g = _acc(gen_force, n, dtype), _gravity(gravity, no_gravity, dtype)
    names = ("qdd", "dqdd_dq", "dqdd_dv", "dqdd_dtau")
    rows = [forward_env(Mo, split_state(root[e], dof[e], dtype), f[e], g, armature) for e in range(n)]
    return {name: np.stack([r[i] for r in rows]) for i, name in enumerate(names)}


def forward_differences_env(Mo, state, gen_force, g, armature):
    """(dqdd_dq, dqdd_dv) of one env by float64 differences of solve_reference.forward_dynamics."""
    pos, quat, theta, qd = state

    def qdd_at(st):
        M, c = mass_and_bias(Mo, st, g, armature)
        return SR.forward_dynamics(M[None], c[None], gen_force[None])[0]

    dq = _richardson(lambda d: qdd_at((*moved(pos, quat, theta, d), qd)), *H_Q)
    dv = _central(lambda d: qdd_at((pos, quat, theta, qd + d)), H_V)
    return dq, dv


def error(x, x64):
    """max|x - x64| / max|x64| per env."""
    return SR.forward_error(x, x64)
