"""A float64 numpy reference of contact generation, written from the text of DESIGN §4.1 item 5, DESIGN §5
("Patch friction", "Capacity") and include/humanoid_engine.h (the row keys), vectorised over envs. It
shares no code with the kernel's ``gen_contacts`` or the oracle's restatement of it, and the closest
distance of two segments comes from another algorithm than their clamped closed form: the nine
candidate minima of the squared distance over the unit square (the interior stationary point, the four
edges' stationary points, the four corners) are enumerated and the smallest taken.

* Body poses: a numpy forward kinematics of the model blob from the fp32 state taken exactly.
* Terrain points: a sphere's centre, a capsule's two ends (minus the radius), a box's 8 corners; a box
  keeps its 4 deepest corners, ties to the lower corner index. Plane: z. Slope: the signed distance
  along (-sin s, 0, cos s). Steps: z - step_height floor(x / step_length) for x > 0, else z.
* Self pairs: segment proxies (a sphere its centre, a capsule its axis, a box a capsule along its
  longest half-extent with radius geom_radius); gap = distance - radii; normal from the second body's
  point to the first's; point = the second's closest point + n (r_second + gap / 2).
* A point or pair is a candidate when its gap is under ``contact_offset``; slot order is terrain
  (bodies in order, a body's points by index), then pairs in pair-list order.
* Capacity: the limit slots first; of the first ``pool`` candidates (limits not counted) the contacts
  are taken deepest first, ties in slot order, each kept while its rows fit (a self pair or a body's
  first terrain point 3, its second 2, 1 after) within 63 rows and ``max_contacts`` slots; the kept
  ones stay in slot order. Every candidate counts as generated.

The *margin* of an env is how far (m) its result is from changing: the smallest of every point's and
pair's |gap - contact_offset|, a box's 5th-deepest minus 4th-deepest corner gap (when the 5th is a
candidate), and the gap difference of two rank neighbours of the reduction whose exchange changes the
kept set. Envs under ``BORDERLINE`` are left out of fp32 comparisons.
"""
import numpy as np

NB = 24
MAX_SLOTS, MAX_ROWS, POOL = 40, 63, 128  # include/humanoid_engine.h; DESIGN §5 "Capacity"
# fp32 positions of about 1 m carry 1e-7 m and a nine-link FK chain a few 1e-6 m; ten times that
BORDERLINE = 2e-5
SPHERE, CAPSULE, BOX = 0, 1, 2
INTERIOR, EDGE, CORNER = 0, 1, 2  # class of a segment pair's minimiser
CLASS_NAMES = ("interior", "edge", "corner")


class Model:
    """The model blob's kinematic tree and geometry as float64 arrays."""

    def __init__(self, m):
        self.parents = np.array(m.parents[:NB])
        self.local_pos = np.array([list(m.local_pos[b]) for b in range(NB)], np.float64)
        self.gtype = np.array(m.geom_type[:NB])
        gp = np.array([list(m.geom_params[b]) for b in range(NB)], np.float64)
        grad = np.array(m.geom_radius[:NB], np.float64)
        self.pairs = np.array([list(m.pairs[i]) for i in range(m.num_pairs)], np.int64).reshape(-1, 2)
        # terrain points in slot order: body, index on the body, local position, radius
        body, sub, loc, rad = [], [], [], []
        self.seg = np.zeros((NB, 2, 3))  # self-collision segment, body frame
        self.seg_r = np.zeros(NB)
        for b in range(NB):
            g = gp[b]
            if self.gtype[b] == SPHERE:
                pts, r = [g[0:3]], g[3]
                self.seg[b], self.seg_r[b] = [g[0:3], g[0:3]], g[3]
            elif self.gtype[b] == CAPSULE:
                pts, r = [g[0:3], g[3:6]], g[6]
                self.seg[b], self.seg_r[b] = [g[0:3], g[3:6]], g[6]
            else:
                A = _quat_matrix(g[6:10], normalise=False)  # the geom's frame as the blob states it
                pts = [g[0:3] + A @ (np.array([(c & 1) * 2 - 1, (c >> 1 & 1) * 2 - 1, (c >> 2 & 1) * 2 - 1]) * g[3:6])
                       for c in range(8)]
                r = 0.0
                ax = int(np.argmax(g[3:6]))  # the first of equal half-extents
                half = max(g[3 + ax] - grad[b], 0.0)
                self.seg[b], self.seg_r[b] = [g[0:3] - A[:, ax] * half, g[0:3] + A[:, ax] * half], grad[b]
            for i, x in enumerate(pts):
                body.append(b), sub.append(i), loc.append(x), rad.append(r)
        self.pt_body, self.pt_sub = np.array(body), np.array(sub)
        self.pt_local, self.pt_rad = np.array(loc, np.float64), np.array(rad, np.float64)


def _quat_matrix(q, normalise=True):
    q = np.asarray(q, np.float64)
    if normalise:
        q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
        np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
        np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _rodrigues(v):
    """Rotation matrices [...,3,3] of rotation vectors [...,3]."""
    th = np.linalg.norm(v, axis=-1)[..., None, None]
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(ths) / ths)
    b = np.where(small, 0.5, (1.0 - np.cos(ths)) / (ths * ths))
    return np.eye(3) + a * K + b * (K @ K)


def body_poses(M, root, dof_pos):
    """World rotations [N,24,3,3] and origins [N,24,3] from fp32 root rows [N,13] and joint exp-map
    coordinates [N,69], taken exactly (tests/test_independent_dynamics.py's FK, over envs)."""
    root = np.asarray(root, np.float64)
    q = np.asarray(dof_pos, np.float64).reshape(root.shape[0], NB - 1, 3)
    Rl = _rodrigues(q)
    R = np.zeros((root.shape[0], NB, 3, 3))
    p = np.zeros((root.shape[0], NB, 3))
    R[:, 0], p[:, 0] = _quat_matrix(root[:, 3:7]), root[:, :3]
    for b in range(1, NB):
        a = M.parents[b]
        R[:, b] = R[:, a] @ Rl[:, b - 1]
        p[:, b] = p[:, a] + np.einsum("nij,j->ni", R[:, a], M.local_pos[b])
    return R, p


def terrain_distance(x, kind, slope, step_height, step_length):
    """Signed distance [N,K] and normal [N,K,3] of world points x [N,K,3] to each env's terrain (kind
    [N]: 0 plane, 1 slope, 2 steps)."""
    kind = np.asarray(kind)[:, None]
    n = np.zeros(x.shape)
    n[..., 2] = 1.0
    ns = np.array([-np.sin(slope), 0.0, np.cos(slope)])
    n = np.where((kind == 1)[..., None], ns, n)
    h = np.where(x[..., 0] > 0, step_height * np.floor(x[..., 0] / step_length), 0.0)
    d = np.where(kind == 1, x @ ns, np.where(kind == 2, x[..., 2] - h, x[..., 2]))
    return d, n


def segment_distance(p1, q1, p2, q2):
    """Closest points of segments p1q1 and p2q2 [...,3] by enumeration: the squared distance over
    (s, t) in the unit square is a convex quadratic, so its minimum is the interior stationary point
    when that lies inside, else a stationary point of one of the four edges when inside the edge, else
    a corner. Returns (distance, c1, c2, class, parallel): the closest points on each segment, the
    minimiser's class (INTERIOR, EDGE, CORNER; ties go to the lower class) and whether two proper
    segments are exactly parallel (then the closest points are not unique)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e = (d1 * d1).sum(-1), (d2 * d2).sum(-1)
    b, c, f = (d1 * d2).sum(-1), (d1 * r).sum(-1), (d2 * r).sum(-1)
    shape = a.shape
    S, T, ok, cls = [], [], [], []

    def add(s, t, valid, k):
        S.append(np.broadcast_to(s, shape)), T.append(np.broadcast_to(t, shape))
        ok.append(np.broadcast_to(valid, shape)), cls.append(k)

    with np.errstate(divide="ignore", invalid="ignore"):
        # interior: grad = 0 -> [a -b; -b e] (s, t) = (-c, f)
        den = a * e - b * b
        proper = den > 1e-14 * a * e
        s0, t0 = (b * f - c * e) / den, (a * f - b * c) / den
        add(s0, t0, proper & (a > 0) & (e > 0) & (s0 > 0) & (s0 < 1) & (t0 > 0) & (t0 < 1), INTERIOR)
        for sv in (0.0, 1.0):  # edges s = 0, 1: t = (f + b s) / e
            t1 = (f + b * sv) / e
            add(sv, t1, (e > 0) & (t1 > 0) & (t1 < 1), EDGE)
        for tv in (0.0, 1.0):  # edges t = 0, 1: s = (b t - c) / a
            s1 = (b * tv - c) / a
            add(s1, tv, (a > 0) & (s1 > 0) & (s1 < 1), EDGE)
    for sv in (0.0, 1.0):
        for tv in (0.0, 1.0):
            add(sv, tv, True, CORNER)
    S, T, ok = np.stack(S), np.stack(T), np.stack(ok)
    S, T = np.where(ok, S, 0.0), np.where(ok, T, 0.0)
    c1 = p1 + S[..., None] * d1
    c2 = p2 + T[..., None] * d2
    dist2 = np.where(ok, ((c1 - c2) ** 2).sum(-1), np.inf)
    best = np.argmin(dist2, 0)  # the first of equal minima
    c1 = np.take_along_axis(c1, best[None, ..., None], 0)[0]
    c2 = np.take_along_axis(c2, best[None, ..., None], 0)[0]
    parallel = (a > 0) & (e > 0) & ~proper
    return np.sqrt(np.take_along_axis(dist2, best[None], 0)[0]), c1, c2, np.array(cls)[best], parallel


def _greedy(order, valid, body, nlim, maxc):
    """The deepest-first pass over candidates in the given rank order [N,T] (valid [N,T] in that
    order, body [N,T] by candidate index, -1 a self pair): kept flags by candidate index [N,T]."""
    N, T = order.shape
    ar = np.arange(N)
    klim = np.minimum(nlim, maxc)
    rows, slots = klim.copy(), klim.copy()
    pc = np.zeros((N, NB), np.int64)
    kept = np.zeros((N, T), bool)
    for q in range(T):
        k = order[:, q]
        b = body[ar, k]
        bi = np.maximum(b, 0)
        n_b = pc[ar, bi]
        cost = np.where(b < 0, 3, np.where(n_b == 0, 3, np.where(n_b == 1, 2, 1)))
        take = valid[:, q] & (slots < maxc) & (rows + cost <= MAX_ROWS)
        rows += np.where(take, cost, 0)
        slots += take
        pc[ar, bi] += take & (b >= 0)
        kept[ar, k] |= take
    return kept


def generate(M, root, dof_pos, contact_offset=0.02, terrain_kind=None, terrain_slope=0.0, step_height=0.0,
             step_length=1.0, max_contacts=MAX_SLOTS, nlim=None, self_collision=True, pool=POOL, swap_window=1e-4,
             count_only=False):
    """Contact generation of N envs. nlim [N]: the joint-limit slots in front of the contacts (default
    none). Returns a dict:
      key, gap, x, n, b0, b1, cls [N, MAX_SLOTS(,3)]: the kept contacts in slot order (key -1 past the
        count; b1 -1 terrain; cls the pair's minimiser class, -1 for a terrain point; parallel likewise;
        sep the distance of the pair's closest points, inf for a terrain point)
      kept, generated, dropped [N]: slot count, contacts generated and contacts dropped, limits included
      candidates [N]: terrain and self candidates; survivors [N]: pairs passing the bounding-sphere cull
      point_gap [N,P], pair_gap [N,pairs]: every gap, the near misses included
      margin [N] and its parts margin_offset, margin_box, margin_swap (rank neighbours closer than
        swap_window are exchanged and the reduction run again).
    pool: the candidates the reduction ranks, limits not counted. count_only: the counts and gaps alone."""
    root = np.asarray(root)
    N = root.shape[0]
    off = float(contact_offset)
    kind = np.zeros(N, np.int64) if terrain_kind is None else np.asarray(terrain_kind, np.int64)
    nlim = np.zeros(N, np.int64) if nlim is None else np.asarray(nlim, np.int64)
    maxc = min(int(max_contacts), MAX_SLOTS)
    R, p = body_poses(M, root, dof_pos)
    ar = np.arange(N)[:, None]

    # terrain points
    xw = p[:, M.pt_body] + np.einsum("npij,pj->npi", R[:, M.pt_body], M.pt_local)
    d, tn = terrain_distance(xw, kind, terrain_slope, step_height, step_length)
    pgap = d - M.pt_rad
    px = xw - M.pt_rad[:, None] * tn
    pcand = pgap < off
    margin_box = np.full(N, np.inf)
    for b in np.flatnonzero(M.gtype == BOX):
        cols = np.flatnonzero(M.pt_body == b)
        g = np.where(pcand[:, cols], pgap[:, cols], np.inf)
        rank = np.argsort(np.argsort(g, 1, kind="stable"), 1, kind="stable")
        pcand[:, cols] &= rank < 4
        gs = np.sort(g, 1)
        with np.errstate(invalid="ignore"):
            margin_box = np.minimum(margin_box, np.where(np.isfinite(gs[:, 4]), gs[:, 4] - gs[:, 3], np.inf))
    margin_off = np.abs(pgap - off).min(1)

    # self pairs
    P = M.pairs
    npair = len(P) if self_collision else 0
    P = P[:npair]
    sa = p[:, :, None] + np.einsum("nbij,bkj->nbki", R, M.seg)  # [N,24,2,3]
    I, J = P[:, 0], P[:, 1]
    dist, ci, cj, cls, par = segment_distance(sa[:, I, 0], sa[:, I, 1], sa[:, J, 0], sa[:, J, 1])
    sgap = dist - M.seg_r[I] - M.seg_r[J]
    with np.errstate(invalid="ignore", divide="ignore"):
        sn = np.where(dist[..., None] > 1e-9, (ci - cj) / dist[..., None], np.array([0.0, 0.0, 1.0]))
    sx = cj + sn * (M.seg_r[J] + 0.5 * sgap)[..., None]
    scand = sgap < off
    if npair:
        margin_off = np.minimum(margin_off, np.abs(sgap - off).min(1))
        margin_off = np.where((scand & (dist <= 1e-9)).any(1), 0.0, margin_off)  # coincident axes: no normal
    mid = 0.5 * (sa[:, :, 0] + sa[:, :, 1])
    brad = 0.5 * np.linalg.norm(sa[:, :, 1] - sa[:, :, 0], axis=-1) + M.seg_r
    survivors = (np.linalg.norm(mid[:, I] - mid[:, J], axis=-1) < brad[:, I] + brad[:, J] + off + 1e-3).sum(1)

    # the candidates in slot order, compacted to the front
    cand = np.concatenate([pcand, scand], 1)
    allgap = np.concatenate([pgap, sgap], 1)
    pos = np.argsort(~cand, 1, kind="stable")  # candidate columns first, in slot order
    ncand = cand.sum(1)
    if count_only:  # for choosing inputs: the counts and gaps without the reduction
        return dict(candidates=ncand, survivors=survivors, point_gap=pgap, pair_gap=sgap)
    T = int(min(max(ncand.max(), 1), pool))
    col = pos[:, :T]
    inpool = np.arange(T)[None, :] < np.minimum(ncand, pool)[:, None]
    cgap = np.where(inpool, allgap[ar, col], np.inf)
    cbody = np.where(col < len(M.pt_body), M.pt_body[np.minimum(col, len(M.pt_body) - 1)], -1)
    order = np.argsort(cgap, 1, kind="stable")  # deepest first, ties in slot order
    valid = np.take_along_axis(inpool, order, 1)
    kept = _greedy(order, valid, cbody, nlim, maxc)

    # the rank neighbours whose exchange changes the kept set
    margin_swap = np.full(N, np.inf)
    sg = np.take_along_axis(cgap, order, 1)
    with np.errstate(invalid="ignore"):
        close = valid[:, 1:] & (sg[:, 1:] - sg[:, :-1] < swap_window)
    over = kept.sum(1) < np.minimum(ncand, pool)  # something in the pool was dropped
    close &= over[:, None]
    for r in range(int(close.sum(1).max()) if N else 0):
        has = close.sum(1) > r
        j = np.argmax(np.cumsum(close, 1) == r + 1, 1)  # the r-th close neighbour pair (j, j + 1)
        o2 = order.copy()
        e = np.flatnonzero(has)
        o2[e, j[e]], o2[e, j[e] + 1] = order[e, j[e] + 1], order[e, j[e]]
        k2 = _greedy(o2[e], valid[e], cbody[e], nlim[e], maxc)
        diff = (k2 != kept[e]).any(1)
        dg = sg[e, j[e] + 1] - sg[e, j[e]]
        margin_swap[e] = np.minimum(margin_swap[e], np.where(diff, dg, np.inf))

    # the kept contacts in slot order
    nk = kept.sum(1)
    klim = np.minimum(nlim, maxc)
    out = dict(key=np.full((N, MAX_SLOTS), -1, np.int64), gap=np.zeros((N, MAX_SLOTS)), x=np.zeros((N, MAX_SLOTS, 3)),
               n=np.zeros((N, MAX_SLOTS, 3)), b0=np.full((N, MAX_SLOTS), -1, np.int64),
               b1=np.full((N, MAX_SLOTS), -1, np.int64), cls=np.full((N, MAX_SLOTS), -1, np.int64),
               parallel=np.zeros((N, MAX_SLOTS), bool), sep=np.full((N, MAX_SLOTS), np.inf))
    npt = len(M.pt_body)
    allx = np.concatenate([px, sx], 1) if npair else px
    alln = np.concatenate([tn, sn], 1) if npair else tn
    b0 = np.concatenate([M.pt_body, I])
    b1 = np.concatenate([np.full(npt, -1), J])
    sub = np.concatenate([M.pt_sub, np.zeros(npair, np.int64)])
    keyc = b0 | ((b1 + 2) << 5) | (sub << 10)
    clsc = np.concatenate([np.full((N, npt), -1), cls], 1) if npair else np.full((N, npt), -1)
    parc = np.concatenate([np.zeros((N, npt), bool), par], 1) if npair else np.zeros((N, npt), bool)
    kpos = np.argsort(~kept, 1, kind="stable")[:, :MAX_SLOTS]
    W = kpos.shape[1]
    kc = col[ar, kpos]  # the kept candidates' columns, slot order
    on = np.arange(W)[None, :] < nk[:, None]
    out["key"][:, :W] = np.where(on, keyc[kc], -1)
    out["gap"][:, :W] = np.where(on, allgap[ar, kc], 0.0)
    out["x"][:, :W] = np.where(on[..., None], allx[ar, kc], 0.0)
    out["n"][:, :W] = np.where(on[..., None], alln[ar, kc], 0.0)
    out["b0"][:, :W] = np.where(on, b0[kc], -1)
    out["b1"][:, :W] = np.where(on, b1[kc], -1)
    out["cls"][:, :W] = np.where(on, clsc[ar, kc], -1)
    out["parallel"][:, :W] = np.where(on, parc[ar, kc], False)
    sepc = np.concatenate([np.full((N, npt), np.inf), dist], 1) if npair else np.full((N, npt), np.inf)
    out["sep"][:, :W] = np.where(on, sepc[ar, kc], np.inf)
    out.update(kept=klim + nk, generated=nlim + ncand, candidates=ncand, survivors=survivors,
               point_gap=pgap, pair_gap=sgap, pair_class=cls, margin_offset=margin_off, margin_box=margin_box,
               margin_swap=margin_swap, margin=np.minimum(np.minimum(margin_off, margin_box), margin_swap))
    out["dropped"] = out["generated"] - out["kept"]
    return out


def sorted_keys(ref, e):
    """The kept contacts' normal-row keys of env e, sorted."""
    k = ref["key"][e]
    return tuple(sorted(int(v) for v in k[k >= 0]))
