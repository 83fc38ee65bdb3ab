"""numpy restatement of the terrain and of the ray-cast sensor that ``include/humanoid_render.h`` defines
(written from the header's text; nothing imported from the product's ``render.py``). The camera, the body
primitives, their hit tests and the pixel comparison rule are those of ``render_reference.py``; what is
stated here is the ground of an env (plane, slope, steps), the image drawn on it and the sensor's rays.
``render`` and ``cast`` take a dtype: float64 is the reference the GPU is held to, float32 against float64
measures the reference's own rounding (the floors the GPU tolerances are 8 x of)."""
import numpy as np

import render_reference as RR
from render_reference import body_prims, camera_points, _hit  # noqa: F401  (the unchanged pieces)

MAX_STEP_CELLS = 512
MAX_RAYS = 1024
FRAME_POSITION, FRAME_HEADING, FRAME_TRANSFORM = 0, 1, 2
HIT_NOTHING, HIT_TERRAIN = -2, -1


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def terrain(kind=None, slope=np.deg2rad(10.0), step_height=0.05, step_length=0.4):
    """The arguments of hr_set_terrain: kind [N] (None: the plane everywhere) and the three host floats."""
    return dict(kind=None if kind is None else np.asarray(kind, np.int32), slope=np.float32(slope),
                step_height=np.float32(step_height), step_length=np.float32(step_length))


def kind_of(ter, env):
    """Kind 1 is the slope, 2 the steps; any other value, or no array, is the plane (0)."""
    if ter is None or ter["kind"] is None:
        return 0
    k = int(ter["kind"][env])
    return k if k in (1, 2) else 0


def _steps_hit(o, d, L, S, far):
    """The walk over the cells of the steps, every ray at once (an `active` mask plays the walk's exits)."""
    dtype = o.dtype.type
    npx = o.shape[0]
    ox, oz, dx, dz = o[:, 0], o[:, 2], d[:, 0], d[:, 2]
    c = np.maximum(np.floor(ox / L), 0)
    active = oz > S * c  # entry hits only
    hit = np.zeros(npx, bool)
    t = np.full(npx, np.inf, dtype)
    nrm = np.tile(np.array([0, 0, 1], dtype), (npx, 1))
    ckx = ox.copy()
    t0 = np.zeros(npx, dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(MAX_STEP_CELLS):
            if not active.any():
                break
            # 1. the tread
            tt = (S * c - oz) / dz
            xt = ox + tt * dx
            incell = (xt < (c + 1) * L) & ((c == 0) | (xt >= c * L))
            tread = active & (dz < 0) & (tt >= t0) & incell
            hit |= tread
            t = np.where(tread, tt, t)
            ckx = np.where(tread, xt, ckx)
            active = active & ~tread
            # 2. moving up
            up = active & (dx > 0)
            tb = ((c + 1) * L - ox) / dx
            active = active & ~(up & (tb > far))
            up = up & active
            zb = oz + tb * dz
            riser = up & (zb < S * (c + 1))
            hit |= riser
            t = np.where(riser, tb, t)
            nrm = np.where(riser[:, None], np.array([-1, 0, 0], dtype)[None, :], nrm)
            ckx = np.where(riser, (c + dtype(0.5)) * L, ckx)
            active = active & ~riser
            up = up & active
            # 3. moving down
            down = active & (dx < 0)
            active = active & ~(down & (c == 0))
            down = down & active
            tb2 = (c * L - ox) / dx
            active = active & ~(down & (tb2 > far))
            down = down & active
            # 4. d_x = 0
            active = active & ~(dx == 0)
            c = np.where(up, c + 1, np.where(down, c - 1, c))
            t0 = np.where(up, tb, np.where(down, tb2, t0))
    return hit, t, nrm, ckx


def terrain_hit(ter, kind, o, d, far):
    """Entry hit of the ground of kind `kind` for rays o [P,3], d [P,3] (of one dtype):
    (hit [P], t [P], normal [P,3], the x the checker takes [P])."""
    dtype = o.dtype.type
    npx = o.shape[0]
    up = np.tile(np.array([0, 0, 1], dtype), (npx, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == 1:
            sn, cs = dtype(np.sin(np.float32(ter["slope"]))), dtype(np.cos(np.float32(ter["slope"])))  # float32 on the host
            n = np.array([-sn, 0, cs], dtype)
            dn, on = _dot(d, n[None, :]), _dot(o, n[None, :])
            hit = (dn < 0) & (on > 0)
            t = -on / dn
            return hit, t, np.tile(n, (npx, 1)), o[:, 0] + np.where(hit, t, 0) * d[:, 0]
        if kind == 2:
            return _steps_hit(o, d, dtype(ter["step_length"]), dtype(ter["step_height"]), dtype(far))
        hit = (d[:, 2] < 0) & (o[:, 2] > 0)
        t = -o[:, 2] / d[:, 2]
        return hit, t, up, o[:, 0] + np.where(hit, t, 0) * d[:, 0]


def one_ray(ter, kind, o, d, far=np.inf, dtype=np.float64):
    """terrain_hit for a single ray: (hit, t, normal, checker x) as Python values."""
    o, d = np.asarray(o, dtype)[None, :], np.asarray(d, dtype)[None, :]
    hit, t, n, ckx = terrain_hit(ter, kind, o, d / np.sqrt(_dot(d, d))[:, None], far)
    return bool(hit[0]), float(t[0]), tuple(float(x) for x in n[0]), float(ckx[0])


def render(geom_type, geom_params, rb_state, cams, ter=None, body_rgb=None, body_seg=None, markers=None,
           flags=RR.FLAG_SHADOWS | RR.FLAG_CHECKER, dtype=np.float64):
    """The image of every camera on its env's terrain: (color u8 [K,H,W,4], depth float64 [K,H,W], seg i32
    [K,H,W]). Arguments as render_reference.render, plus ter = terrain(...)."""
    dtype = np.dtype(dtype).type
    rb = np.asarray(rb_state, np.float32).reshape(-1, RR.NB, 13)
    K, H, W = len(cams), cams[0]["height"], cams[0]["width"]
    color = np.zeros((K, H, W, 4), np.uint8)
    depth = np.zeros((K, H, W), np.float64)
    seg = np.zeros((K, H, W), np.int32)
    light = np.array(RR.LIGHT, np.float64).astype(dtype)
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
        o = np.ascontiguousarray(np.broadcast_to(P, d.shape))
        near, far = dtype(np.float32(cam["near"])), dtype(np.float32(cam["far"]))
        npx = d.shape[0]

        bodies = body_prims(geom_type, geom_params, rb[env], dtype)
        rgb_e = np.asarray(RR.BODY_RGB if body_rgb is None else body_rgb[env], np.float32).astype(dtype)
        rgb_e = np.broadcast_to(rgb_e, (RR.NB, 3))
        seg_e = np.zeros(RR.NB, np.int32) if body_seg is None else np.asarray(body_seg[env], np.int32)
        prims = [(pr, rgb_e[b], int(seg_e[b])) for b, pr in enumerate(bodies)]
        if markers is not None:
            mpos, mrgb, mrad = markers
            mrgb = np.broadcast_to(np.asarray(mrgb, np.float32), (np.asarray(mpos).shape[1], 3)).astype(dtype)
            for j in range(np.asarray(mpos).shape[1]):
                c = np.asarray(mpos, np.float32)[env, j].astype(dtype)
                prims.append((dict(type=RR.SPHERE, C=c, r=dtype(np.float32(mrad))), mrgb[j], RR.SEG_MARKER))

        # the ground takes the first place, then the bodies and the markers; strictly nearer replaces
        kind = kind_of(ter, env)
        hg, tg, ng, ckx = terrain_hit(ter, kind, o, d, far)
        okg = hg & (tg >= near) & (tg <= far)
        best = np.where(okg, tg, dtype(np.inf))
        who = np.where(okg, -1, -2).astype(np.int64)  # -2 sky, -1 ground
        nrm = np.where(okg[:, None], ng, np.array([0, 0, 1], dtype)[None, :])
        for idx, (pr, _, _) in enumerate(prims):
            hit, t, n = _hit(pr, o, d)
            take = hit & (t >= near) & (t <= far) & (t < best)
            best, who, nrm = np.where(take, t, best), np.where(take, idx, who), np.where(take[:, None], n, nrm)

        hitm = who > -2
        tb = np.where(hitm, best, 0)
        hp = o + tb[:, None] * d
        ndl = np.maximum(0, _dot(nrm, light[None, :]))
        s = np.ones(npx, dtype)
        if flags & RR.FLAG_SHADOWS:  # the terrain casts none; the shadow ray leaves along the hit's normal
            want = hitm & (ndl > 0)
            so = hp + nrm * dtype(RR.SHADOW_EPS)
            ld = np.broadcast_to(light, so.shape)
            shadowed = np.zeros(npx, bool)
            for pr in bodies:
                hit, t, _ = _hit(pr, so, ld)
                shadowed |= hit & (t >= 0)
            s = np.where(want & shadowed, dtype(RR.SHADOW), s)
        gx = np.where((who == -1) & (nrm[:, 0] < 0) & (kind == 2), ckx, hp[:, 0])  # a riser: the tread's middle
        par = (np.floor(gx) + np.floor(hp[:, 1])).astype(np.int64) & 1
        grey = np.where((par == 1) & bool(flags & RR.FLAG_CHECKER), dtype(RR.GROUND_ODD), dtype(RR.GROUND_EVEN))
        alb = np.repeat(grey[:, None], 3, 1)
        sid = np.zeros(npx, np.int32)
        for idx, (_, c, sg) in enumerate(prims):
            mine = who == idx
            alb[mine] = c
            sid[mine] = sg
        shade = dtype(RR.AMBIENT) + (1 - dtype(RR.AMBIENT)) * ndl * s
        col = np.where(hitm[:, None], alb * shade[:, None], np.array(RR.SKY, np.float64).astype(dtype)[None, :])
        col = np.clip(col, 0, 1)
        color[k, ..., :3] = np.floor(col * 255 + dtype(0.5)).astype(np.uint8).reshape(H, W, 3)
        color[k, ..., 3] = 255
        dep = np.where(hitm, -best * _dot(d, f[None, :]), -np.inf)
        depth[k] = dep.astype(np.float64).reshape(H, W)
        seg[k] = sid.reshape(H, W)
    return color, depth, seg


# ------------------------------------------------------------------------------------- the ray-cast sensor
def heading(q):
    """(c, s) of the heading of the rotation q (xyzw)."""
    hx = RR.rot(q, np.array([1, 0, 0], q.dtype))
    l = np.sqrt(hx[0] * hx[0] + hx[1] * hx[1])
    if l < 1e-6:
        return q.dtype.type(1), q.dtype.type(0)
    return hx[0] / l, hx[1] / l


def world_rays(rays, row, mode, dtype):
    """rays [R,6] float32 (origin, unit direction) in the frame of the body whose rb_state row is `row`:
    world origins and directions [R,3] each."""
    a = np.asarray(rays, np.float32).astype(dtype)
    row = np.asarray(row, np.float32).astype(dtype)
    p, q = row[:3], row[3:7]
    org, dr = a[:, :3], a[:, 3:]
    if mode == FRAME_HEADING:
        c, s = heading(q)

        def H(w):
            return np.stack([c * w[:, 0] - s * w[:, 1], s * w[:, 0] + c * w[:, 1], w[:, 2]], -1)
        org, dr = H(org), H(dr)
    elif mode == FRAME_TRANSFORM:
        org, dr = RR.rot(q[None, :], org), RR.rot(q[None, :], dr)
    return p[None, :] + org, dr


def cast(geom_type, geom_params, rb_state, rays, body, mode, ter, max_range, skip_bodies, dtype=np.float64):
    """hr_cast_rays: (dist float64 [N,R], +inf without a hit; hit i32 [N,R]: -2 nothing, -1 terrain, else
    the body index). The hits are the image's with near = 0, far = max_range; markers are never hit."""
    dtype = np.dtype(dtype).type
    rb = np.asarray(rb_state, np.float32).reshape(-1, RR.NB, 13)
    n_env, n_ray = rb.shape[0], np.asarray(rays).shape[0]
    dist = np.full((n_env, n_ray), np.inf)
    who_all = np.full((n_env, n_ray), HIT_NOTHING, np.int32)
    far = dtype(np.float32(max_range))
    for env in range(n_env):
        o, d = world_rays(rays, rb[env, body], mode, dtype)
        o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        hg, tg, _, _ = terrain_hit(ter, kind_of(ter, env), o, d, far)
        okg = hg & (tg >= 0) & (tg <= far)
        best = np.where(okg, tg, dtype(np.inf))
        who = np.where(okg, HIT_TERRAIN, HIT_NOTHING).astype(np.int32)
        if not skip_bodies:
            for b, pr in enumerate(body_prims(geom_type, geom_params, rb[env], dtype)):
                hit, t, _ = _hit(pr, o, d)
                take = hit & (t >= 0) & (t <= far) & (t < best)
                best, who = np.where(take, t, best), np.where(take, b, who)
        dist[env], who_all[env] = best.astype(np.float64), who
    return dist, who_all


# --------------------------------------------------------------------------------- shared scenes and floors
KINDS = (2, 1, 2, 0)  # of the four envs of RR.scene(): steps, slope, steps, plane
SLOPE = np.deg2rad(10.0)
STEP_SETTINGS = ((0.05, 0.4), (0.15, 0.3))  # (step_height, step_length)
MAX_RANGE = 10.0


def settings():
    return [terrain(KINDS, SLOPE, s, l) for s, l in STEP_SETTINGS]


# The six views (position, target, fov). A camera whose image plane holds a checker line, or that looks
# along a riser plane, flips whole rows of pixels between float32 and float64 and fails the rule on its
# own, whatever draws it: (1,-2,1) -> (1,0,0.2) does (x = 1 is both), so none of these does.
VIEWS = (((-1.0, -2.0, 1.5), (2.0, 0.0, 0.1), 90.0), ((4.5, 1.0, 2.6), (1.0, 0.0, 0.1), 90.0),
         ((1.3, -3.0, 0.9), (1.5, 0.0, 0.2), 40.0), ((1.37, 0.21, 3.0), (1.37, 0.21, 0.0), 90.0),
         ((-2.0, 0.3, 0.6), (3.0, 0.0, 0.6), 90.0), ((0.1, -0.2, 0.3), (3.0, 0.5, 0.5), 90.0))
# each view on env 2 (steps under scattered bodies) and env 1 (the slope under scattered bodies); the first
# and the straight-down view also on env 0 (steps under the rest pose)
CAMERA_ENVS = (2, 1)


def cameras():
    cams = [RR.cam(e, p, t, fov) for e in CAMERA_ENVS for p, t, fov in VIEWS]
    return cams + [RR.cam(0, *VIEWS[0][:2], VIEWS[0][2]), RR.cam(0, *VIEWS[3][:2], VIEWS[3][2])]


def sensor_rays():
    """185 rays [R,6] float32: an 11 x 11 grid of straight-down rays 0.1 m apart, offset (0.003, 0.007), from
    1 m above the body, and a fan of 64 rays pitched 0.2 rad down from 0.2 m above it. Directions are
    normalised in float64 before they are rounded."""
    g = (np.arange(11) - 5) * 0.1
    down = np.zeros((11, 11, 6))
    down[..., 0], down[..., 1], down[..., 2], down[..., 5] = g[:, None] + 0.003, g[None, :] + 0.007, 1.0, -1.0
    az = np.arange(64) * (2 * np.pi / 64)
    fan = np.zeros((64, 6))
    fan[:, 2] = 0.2
    fan[:, 3], fan[:, 4], fan[:, 5] = np.cos(az) * np.cos(0.2), np.sin(az) * np.cos(0.2), -np.sin(0.2)
    rays = np.concatenate([down.reshape(-1, 6), fan])
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    return rays.astype(np.float32)


RAY_BODY = 0  # the pelvis

# The GPU tolerances are measured, not chosen: each floor is the largest |float32 - float64| of this
# reference over what agrees between the two, recomputed and held to these constants (within a factor 2)
# by test_terrain_render.py::test_reference_self_check; the GPU, which orders operations differently and
# contracts to FMA, gets 8 x.
TERRAIN_DEPTH_FLOOR = 3.0e-5  # m, images at far = 20 (measured 2.88e-5)
TERRAIN_DEPTH_TOL = 8 * TERRAIN_DEPTH_FLOOR
# ray distances, per env of RR.scene() (env 3 sits at x = 1000 m): terrain only, and with the bodies
RAY_FLOOR_TERRAIN = (4e-6, 5e-6, 2e-6, 4e-6)    # measured 3.45e-6, 4.70e-6, 1.78e-6, 3.67e-6
RAY_FLOOR_BODIES = (4e-6, 5e-6, 1.2e-6, 2.5e-4)  # measured 3.45e-6, 4.70e-6, 1.08e-6, 2.34e-4
HIT_ID_CAP = 0.01  # of the rays may differ from float64 in their hit id (the reference alone: none)
