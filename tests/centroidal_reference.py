"""numpy restatement of the six outputs that ``include/humanoid_centroidal.h`` defines, written from the
header's text as the textbook sums over the bodies (nothing imported from the product beyond the model
blob): kinematics, the body Jacobians and the bodies' velocities and accelerations at qdd = 0 are
tests/dynamics_reference.py's (``Model``, ``fk``, ``jacobian``, ``body_velocities``). ``evaluate`` takes a
dtype: float64 is the reference the GPU is held to, float32 against float64 measures the reference's own
rounding (the floor each GPU tolerance is a multiple of)."""
import numpy as np

import dynamics_reference as DR

NB, ND, NG = DR.NB, DR.ND, DR.NG
OUTPUTS = ("com", "com_vel", "momentum", "cmm", "cmm_bias", "energy")


def reference_point_shift(rows, r):
    """(linear, angular about o) -> (linear, angular about o + r) for rows [6] or [6,k]: the angular part
    loses r x linear. The header's identities re-reference M's and c's base rows with it."""
    rows = np.asarray(rows)
    out = rows.copy()
    out[3:6] = rows[3:6] - np.cross(r, rows[0:3], axis=0)
    return out


def momentum_of_pose(Mo, R, p, qd):
    """(P, L_G) [6] of the pose (R [24,3,3], p [24,3]) moving with qd [75]: the table's sums, for the
    finite difference of the momentum along the configuration flow."""
    m = Mo.mass
    J = DR.jacobian(Mo, R, p)
    rc = np.einsum("bij,bj->bi", R, Mo.com)
    c = p + rc
    com = (m[:, None] * c).sum(0) / m.sum()
    v = (J[:, 0:3] + np.cross(J[:, 3:6], rc[:, :, None], axis=1)) @ qd
    w = J[:, 3:6] @ qd
    Iww = np.einsum("bij,bjk,blk,bl->bi", R, Mo.I, R, w)
    return np.concatenate([(m[:, None] * v).sum(0), (np.cross(c - com, m[:, None] * v) + Iww).sum(0)])


def one(Mo, root, dof, gravity):
    """The six outputs of one env (root [13], dof [69,2]) in Mo.dtype, as a dict."""
    dt = Mo.dtype
    g = np.asarray(gravity, np.float32).astype(dt)
    R, p = DR.fk(Mo, root, dof)
    J = DR.jacobian(Mo, R, p)
    qd = DR.gen_velocity(np.asarray(root), np.asarray(dof), dt)
    w, wd, acc = DR.body_velocities(Mo, R, p, np.asarray(root), np.asarray(dof))
    m = Mo.mass
    mtot = m.sum()
    rc = np.einsum("bij,bj->bi", R, Mo.com)          # R_b com[b]
    c = p + rc                                       # the bodies' centres of mass
    com = (m[:, None] * c).sum(0) / mtot
    Jw = J[:, 3:6]
    Jc = J[:, 0:3] + np.cross(Jw, rc[:, :, None], axis=1)  # v_c = v_origin + w x (R com)
    v = Jc @ qd
    Iw = np.einsum("bij,bjk,blk->bil", R, Mo.I, R)   # R I R^T
    lever = c - com
    P = (m[:, None] * v).sum(0)
    Iww = np.einsum("bij,bj->bi", Iw, w)
    L = (np.cross(lever, m[:, None] * v) + Iww).sum(0)
    A = np.zeros((6, NG), dt)
    A[0:3] = (m[:, None, None] * Jc).sum(0)
    A[3:6] = (np.cross(lever[:, :, None], m[:, None, None] * Jc, axis=1) + np.einsum("bij,bjk->bik", Iw, Jw)).sum(0)
    ac = acc + np.cross(wd, rc) + np.cross(w, np.cross(w, rc))  # acceleration of c_b at qdd = 0
    bias = np.zeros(6, dt)
    bias[0:3] = (m[:, None] * ac).sum(0)
    bias[3:6] = (np.cross(lever, m[:, None] * ac) + np.einsum("bij,bj->bi", Iw, wd) + np.cross(w, Iww)).sum(0)
    kinetic = dt(0.5) * ((m * (v * v).sum(1)).sum() + (w * Iww).sum())
    potential = -mtot * (g @ com)
    return dict(com=com, com_vel=P / mtot, momentum=np.concatenate([P, L]), cmm=A, cmm_bias=bias,
                energy=np.array([kinetic, potential], dt))


def evaluate(he_model, root, dof, gravity=(0.0, 0.0, -9.81), dtype=np.float64):
    """The six outputs of n states (root [n,13], dof [n,69,2]) in `dtype`: a dict of [n,...] arrays."""
    Mo = DR.Model(he_model, dtype)
    rows = [one(Mo, root[e], dof[e], gravity) for e in range(root.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in OUTPUTS}


# what a tolerance is stated for: the outputs, with the two energies apart (joules of different sizes)
CHECKED = ("com", "com_vel", "momentum", "cmm", "cmm_bias", "kinetic", "potential")


def checked(out):
    """A dict of outputs -> the same with ``energy`` [n,2] split into ``kinetic`` and ``potential`` [n]."""
    d = {k: np.asarray(v) for k, v in out.items() if k != "energy"}
    d["kinetic"], d["potential"] = np.asarray(out["energy"])[..., 0], np.asarray(out["energy"])[..., 1]
    return d


def error(got, ref, relative=False):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    return e / float(np.abs(ref).max()) if relative else e


def errors(got, ref):
    """Largest absolute error of every checked quantity against `ref` (both as `checked` gives them); cmm
    relative to max|A_G|."""
    return {k: error(got[k], ref[k], relative=k == "cmm") for k in CHECKED}


def floors(he_model, root, dof, gravity):
    """(float64 reference, float32 floor per checked quantity) at these states: the error of the
    reference evaluated in float32."""
    ref = checked(evaluate(he_model, root, dof, gravity, np.float64))
    r32 = checked(evaluate(he_model, root, dof, gravity, np.float32))
    return ref, errors(r32, ref)
