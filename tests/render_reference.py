"""numpy restatement of the image that ``include/humanoid_render.h`` defines (written from the header's
text, nothing imported from the product's ``render.py``), the scenes the render tests share, and the
pixel comparison rule. ``render`` takes a dtype: float64 is the reference the GPU is held to, float32
against float64 measures the reference's own rounding (the cap margin and the depth floor)."""
import numpy as np

# the header's constants
AMBIENT, SHADOW, SHADOW_EPS = 0.35, 0.4, 1e-3
LIGHT = (2.0 / 7.0, -3.0 / 7.0, 6.0 / 7.0)
SKY = (0.53, 0.73, 0.92)
GROUND_EVEN, GROUND_ODD = 0.75, 0.55
BODY_RGB = (0.80, 0.68, 0.52)
SEG_MARKER = 1000
FLAG_SHADOWS, FLAG_CHECKER = 1, 2
SPHERE, CAPSULE, BOX = 0, 1, 2
NB = 24


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def rot(q, v):
    """rot(q, v) = (v + w t) + qv x t with t = 2 (qv x v); q xyzw."""
    qv = q[..., :3]
    t = 2 * _cross(qv, v)
    return (v + q[..., 3:4] * t) + _cross(qv, t)


def camera_points(cam, rb, dtype=np.float32):
    """World position and target of a camera (rb [N,24,13]); in float32 this is the header's operation
    order, each product and sum rounded on its own, as the kernel evaluates a following camera."""
    P = np.asarray(cam["pos"], np.float32).astype(dtype)
    T = np.asarray(cam["target"], np.float32).astype(dtype)
    b = cam.get("follow_body", -1)
    if b >= 0:
        row = np.asarray(rb, np.float32)[cam["env"], b].astype(dtype)
        p, q = row[:3], row[3:7]
        mode = cam.get("follow_mode", 0)
        if mode == 1:
            P, T = rot(q, P), rot(q, T)
        if mode == 2:
            P = np.array([p[0] + P[0], p[1] + P[1], P[2]], dtype)
            T = np.array([p[0] + T[0], p[1] + T[1], T[2]], dtype)
        else:
            P, T = p + P, p + T
    return P, T


def _hit_sphere(m, d, r):
    b = _dot(m, d)
    q = m - b[:, None] * d
    h = r * r - _dot(q, q)
    ok = h >= 0
    t = -b - np.sqrt(np.where(ok, h, 0))
    n = (m + t[:, None] * d) / r
    return ok, t, n


def _hit(prim, o, d):
    """Entry hit of one primitive for rays o [P,3], d [P,3]: (hit [P], t [P], normal [P,3])."""
    kind = prim["type"]
    if kind == SPHERE:
        return _hit_sphere(o - prim["C"], d, prim["r"])
    if kind == CAPSULE:
        A, B, w, L, r = prim["A"], prim["B"], prim["w"], prim["L"], prim["r"]
        m = o - A
        hit, t, n = _hit_sphere(m, d, r)
        ok2, t2, n2 = _hit_sphere(o - B, d, r)
        take = ok2 & (~hit | (t2 < t))
        t, n, hit = np.where(take, t2, t), np.where(take[:, None], n2, n), hit | take
        mw, dw = _dot(m, w), _dot(d, w)
        mp, dp = m - mw[:, None] * w, d - dw[:, None] * w
        a = _dot(dp, dp)
        c = _cross(mp, dp)
        h = a * r * r - _dot(c, c)
        ok3 = (a >= 1e-12) & (h >= 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t3 = (-_dot(mp, dp) - np.sqrt(np.where(h >= 0, h, 0))) / a
            s = mw + t3 * dw
            ok3 = ok3 & (s >= 0) & (s <= L)
            take = ok3 & (~hit | (t3 < t))
            n3 = (mp + t3[:, None] * dp) / r
        t, n, hit = np.where(take, t3, t), np.where(take[:, None], n3, n), hit | take
        return hit, t, n
    C, e, R = prim["C"], prim["e"], prim["R"]  # R columns = box axes in the world
    mo = o - C
    ol = np.stack([_dot(R[:, k], mo) for k in range(3)], -1)
    dl = np.stack([_dot(R[:, k][None, :], d) for k in range(3)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-e - ol) / dl, (e - ol) / dl
    lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    tn, tf = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2]), np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    hit = tn <= tf
    k = np.where(lo[:, 0] == tn, 0, np.where(lo[:, 1] == tn, 1, 2))
    ax = R.T[k]  # [P,3]: column k
    dk = np.take_along_axis(dl, k[:, None], 1)[:, 0]
    n = ax * np.where(dk > 0, -1, 1).astype(d.dtype)[:, None]
    return hit, tn, n


def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], q.dtype)


def body_prims(geom_type, geom_params, rows, dtype):
    """The 24 world-space primitives of an env from its rb_state rows [24,13]."""
    prims = []
    gp_all = np.asarray(geom_params, np.float32).astype(dtype)
    rows = np.asarray(rows, np.float32).astype(dtype)
    for b in range(NB):
        p, q, gp = rows[b, :3], rows[b, 3:7], gp_all[b]
        kind = int(geom_type[b])
        if kind == SPHERE:
            prims.append(dict(type=SPHERE, C=p + rot(q, gp[:3]), r=gp[3]))
        elif kind == CAPSULE:
            A, B = p + rot(q, gp[:3]), p + rot(q, gp[3:6])
            L = np.sqrt(_dot(B - A, B - A))
            if L < 1e-9:
                w, L = np.array([0, 0, 1], dtype), dtype(0)
            else:
                w = (B - A) / L
            prims.append(dict(type=CAPSULE, A=A, B=B, w=w, L=L, r=gp[6]))
        else:
            ax, ay, az, aw = q
            bx, by, bz, bw = gp[6:10]
            qq = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                           aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], dtype)
            prims.append(dict(type=BOX, C=p + rot(q, gp[:3]), e=gp[3:6], R=_quat_matrix(qq)))
    return prims


def render(geom_type, geom_params, rb_state, cams, body_rgb=None, body_seg=None, markers=None,
           flags=FLAG_SHADOWS | FLAG_CHECKER, dtype=np.float64):
    """The image of every camera: (color u8 [K,H,W,4], depth float64 [K,H,W], seg i32 [K,H,W]).
    rb_state [N,24,13]; cams: dicts with env, width, height, hfov_deg, near, far, pos, target and optionally
    follow_body / follow_mode; body_rgb [N,24,3], body_seg [N,24]; markers = (pos [N,m,3], rgb [m,3], radius)."""
    dtype = np.dtype(dtype).type
    rb = np.asarray(rb_state, np.float32).reshape(-1, NB, 13)
    K, H, W = len(cams), cams[0]["height"], cams[0]["width"]
    color = np.zeros((K, H, W, 4), np.uint8)
    depth = np.zeros((K, H, W), np.float64)
    seg = np.zeros((K, H, W), np.int32)
    light = np.array(LIGHT, np.float64).astype(dtype)
    for k, cam in enumerate(cams):
        env = cam["env"]
        P, T = camera_points(cam, rb, dtype)
        f = _normalize(T - P)
        r = _cross(f, np.array([0, 0, 1], dtype))
        if np.sqrt(_dot(r, r)) < 1e-6:
            r = _cross(f, np.array([0, 1, 0], dtype))
        r = _normalize(r)
        u = _cross(r, f)
        th = np.tan(dtype(np.float32(cam["hfov_deg"])) * dtype(np.pi) / 360)
        jj, ii = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype))
        x = ((2 * (jj + dtype(0.5)) / W - 1) * th).reshape(-1)
        y = ((1 - 2 * (ii + dtype(0.5)) / H) * (th * H / W)).reshape(-1)
        d = _normalize(f[None, :] + x[:, None] * r[None, :] + y[:, None] * u[None, :])
        o = np.broadcast_to(P, d.shape)
        near, far = dtype(np.float32(cam["near"])), dtype(np.float32(cam["far"]))
        npx = d.shape[0]

        bodies = body_prims(geom_type, geom_params, rb[env], dtype)
        rgb_e = np.asarray(BODY_RGB if body_rgb is None else body_rgb[env], np.float32).astype(dtype)
        rgb_e = np.broadcast_to(rgb_e, (NB, 3))
        seg_e = np.zeros(NB, np.int32) if body_seg is None else np.asarray(body_seg[env], np.int32)
        prims = [(pr, rgb_e[b], int(seg_e[b])) for b, pr in enumerate(bodies)]
        if markers is not None:
            mpos, mrgb, mrad = markers
            mrgb = np.broadcast_to(np.asarray(mrgb, np.float32), (np.asarray(mpos).shape[1], 3)).astype(dtype)
            for j in range(np.asarray(mpos).shape[1]):
                c = np.asarray(mpos, np.float32)[env, j].astype(dtype)
                prims.append((dict(type=SPHERE, C=c, r=dtype(np.float32(mrad))), mrgb[j], SEG_MARKER))

        best = np.full(npx, np.inf, dtype)
        who = np.full(npx, -2, np.int64)  # -2 sky, -1 ground
        nrm = np.tile(np.array([0, 0, 1], dtype), (npx, 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            tg = -o[:, 2] / d[:, 2]
        okg = (d[:, 2] < 0) & (o[:, 2] > 0) & (tg >= near) & (tg <= far)
        best, who = np.where(okg, tg, best), np.where(okg, -1, who)
        for idx, (pr, _, _) in enumerate(prims):
            hit, t, n = _hit(pr, o, d)
            take = hit & (t >= near) & (t <= far) & (t < best)
            best, who, nrm = np.where(take, t, best), np.where(take, idx, who), np.where(take[:, None], n, nrm)

        hitm = who > -2
        tb = np.where(hitm, best, 0)
        hp = o + tb[:, None] * d
        ndl = np.maximum(0, _dot(nrm, light[None, :]))
        s = np.ones(npx, dtype)
        if flags & FLAG_SHADOWS:
            want = hitm & (ndl > 0)
            so = hp + nrm * dtype(SHADOW_EPS)
            ld = np.broadcast_to(light, so.shape)
            shadowed = np.zeros(npx, bool)
            for pr in bodies:
                hit, t, _ = _hit(pr, so, ld)
                shadowed |= hit & (t >= 0)
            s = np.where(want & shadowed, dtype(SHADOW), s)
        par = (np.floor(hp[:, 0]) + np.floor(hp[:, 1])).astype(np.int64) & 1
        grey = np.where((par == 1) & bool(flags & FLAG_CHECKER), dtype(GROUND_ODD), dtype(GROUND_EVEN))
        alb = np.repeat(grey[:, None], 3, 1)
        sid = np.zeros(npx, np.int32)
        for idx, (_, c, sg) in enumerate(prims):
            mine = who == idx
            alb[mine] = c
            sid[mine] = sg
        shade = dtype(AMBIENT) + (1 - dtype(AMBIENT)) * ndl * s
        col = np.where(hitm[:, None], alb * shade[:, None], np.array(SKY, np.float64).astype(dtype)[None, :])
        col = np.clip(col, 0, 1)
        color[k, ..., :3] = np.floor(col * 255 + dtype(0.5)).astype(np.uint8).reshape(H, W, 3)
        color[k, ..., 3] = 255
        dep = np.where(hitm, -best * _dot(d, f[None, :]), -np.inf)
        depth[k] = dep.astype(np.float64).reshape(H, W)
        seg[k] = sid.reshape(H, W)
    return color, depth, seg


# --------------------------------------------------------------------------------- comparison rule
CAP = 0.005  # of an image's pixels


def _agree(ca, da, sa, cb, db, sb, tol):
    col = (np.abs(ca.astype(np.int32) - cb.astype(np.int32)) <= 1).all(-1)
    both_inf = np.isinf(da) & np.isinf(db)
    with np.errstate(invalid="ignore"):
        dep = both_inf | (np.abs(da - db) <= tol)
    return col & dep & (sa == sb)


def compare(image, ref, depth_tol):
    """image / ref: (color [H,W,4], depth [H,W], seg [H,W]) of one camera. Returns (agree [H,W] bool,
    edge [H,W] bool): a pixel agrees when seg is equal, colour within +-1 level per channel and depth
    within depth_tol (both -inf agree) at that pixel; otherwise it is an edge pixel when it agrees with the
    reference at one of its 8 neighbours. A pixel in neither set fails outright."""
    c, d, s = image
    rc, rd, rs = ref
    d = np.asarray(d, np.float64)
    H, W = s.shape
    agree = _agree(c, d, s, rc, rd, rs, depth_tol)
    edge = np.zeros_like(agree)
    pc = np.pad(rc, ((1, 1), (1, 1), (0, 0)), mode="edge")
    pd = np.pad(rd, 1, mode="edge")
    ps = np.pad(rs, 1, mode="edge")
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            sl = (slice(1 + di, 1 + di + H), slice(1 + dj, 1 + dj + W))
            edge |= _agree(c, d, s, pc[sl], pd[sl], ps[sl], depth_tol)
    return agree, edge & ~agree


def check(image, ref, depth_tol, cap=CAP):
    """Apply the rule; returns the number of edge pixels, asserts no outright failure and the cap."""
    agree, edge = compare(image, ref, depth_tol)
    bad = ~(agree | edge)
    assert not bad.any(), f"{int(bad.sum())} pixels agree with no neighbour, first at {np.argwhere(bad)[0]}"
    n = int(edge.sum())
    assert n <= cap * agree.size, f"{n} edge pixels > cap {cap * agree.size:.1f}"
    return n


# --------------------------------------------------------------------------------- shared scenes
N_ENVS = 4
W, H = 70, 45  # partial tiles on both edges of a 16 x 16 tiling
FAR_ENV = 3    # every body 1000 m away: an empty scene around the origin
# The depth tolerance of the GPU tests is measured, not chosen: DEPTH_FLOOR is the largest |float32 - float64|
# of this reference's depth over the agreeing pixels of the scenes below (3.32e-6 m, recomputed and held
# to this constant by test_render.py::test_reference_self_check), and the GPU, which orders operations
# differently and contracts to FMA, gets 8 x that.
DEPTH_FLOOR = 3.5e-6
DEPTH_TOL = 8 * DEPTH_FLOOR


def scene(env0_rows=None, seed=0):
    """rb_state [4,24,13] float32. Env 0: the pose he_create_envs leaves in the rigid-body buffer (all-zero
    rows; pass the engine's own rows to use them); envs 1-2: per-body random rotations, positions scattered
    in a 1 m cube above the ground; env 3: as env 1 with every body moved 1000 m along x."""
    g = np.random.default_rng(seed)
    rb = np.zeros((N_ENVS, NB, 13), np.float32)
    if env0_rows is not None:
        rb[0] = np.asarray(env0_rows, np.float32).reshape(NB, 13)
    for e in (1, 2, 3):
        q = g.standard_normal((NB, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        rb[e, :, 3:7] = q
        rb[e, :, 0:2] = g.uniform(-0.5, 0.5, (NB, 2))
        rb[e, :, 2] = g.uniform(0.3, 1.3, NB)
    rb[FAR_ENV, :, 0] += 1000.0
    return rb


def cam(env, pos, target, hfov_deg=90.0, near=0.01, far=20.0, follow_body=-1, follow_mode=0, width=W, height=H):
    return dict(env=env, width=width, height=height, hfov_deg=hfov_deg, near=near, far=far, follow_body=follow_body,
                follow_mode=follow_mode, pos=tuple(pos), target=tuple(target))


def parity_cameras():
    """K = 3 on envs (2, 0, 2): two cameras in one env, camera order unlike env order, fovs 90 and 40."""
    return [cam(2, (1.4, -1.2, 1.5), (0.0, 0.0, 0.8), 90.0), cam(0, (1.0, -1.5, 0.8), (0.0, 0.0, 0.1), 40.0),
            cam(2, (-0.3, 2.5, 2.5), (0.0, 0.0, 0.6), 40.0)]


def down_camera(h=3.0):
    """Straight down from height h over the empty env (placed so that no pixel centre falls on a line
    of the checker)."""
    return [cam(FAR_ENV, (0.37, 0.21, h), (0.37, 0.21, 0.0), 90.0)]


def distinct_seg():
    """Segmentation ids [4,24], all different and non-zero."""
    return (1 + np.arange(N_ENVS * NB, dtype=np.int32)).reshape(N_ENVS, NB)


def distinct_rgb(seed=1):
    return np.random.default_rng(seed).uniform(0.2, 1.0, (N_ENVS, NB, 3)).astype(np.float32)
