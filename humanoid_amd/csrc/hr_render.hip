// libhumanoid_render.so: the camera-sensor ray caster (include/humanoid_render.h defines the image).
// One launch draws every camera: grid (ceil(W/16), ceil(H/16), K), 256 threads, one pixel per thread.
//   prologue   lanes 0..47 of wave 0 put the env's primitives (24 body geoms, then the markers) into
//              LDS in world space, lane 48 the camera (resolved from its body when it follows one);
//   culling    each wave (a 16 x 4 pixel strip) tests its rays against every primitive's bounding
//              sphere and keeps the primitives any lane may hit as a 64-bit wave-uniform mask; the
//              pixel loop walks the set bits, so the trip count is the same in all lanes and only the
//              hit tests diverge. The shadow rays get a second mask over the 24 bodies;
//   stores     masked (partial tiles run every barrier), one packed 32-bit colour store per pixel.
// The ground every ray tests first is the env's terrain (hr_set_terrain): its kind is one wave-uniform
// load in the prologue of render_kernel<true>. A renderer without a kind array launches
// render_kernel<false>, the same body with the plane fixed at compile time: an unset terrain costs nothing.
// A second kernel, rays_kernel, is the ray-cast sensor (hr_cast_rays) on the same scene: one 64-lane
// wave per env, lanes 0..23 build the env's body primitives into LDS, the rays are lane-strided.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/humanoid_render.h"
#include "he_host.h"
#include "he_topo.h"

namespace {

constexpr int NB = HE_NUM_BODIES;
constexpr int kMaxPrims = NB + HR_MAX_MARKERS;  // 48: one bit each of the wave's 64-bit mask
constexpr int kTile = 16;
constexpr int kGeomWords = 11;  // per body on the device: geom_type bits, geom_params[10]

// device copy of a camera (hr_set_cameras): the tangent of the half fov is taken on the host
struct DCam {
    int32_t env, follow_body, follow_mode;
    float th, nearp, farp;
    float pos[3], target[3];
};

struct Params {
    const float* rb;        // [N*24,13]
    const float* geom;      // [24][kGeomWords]
    const DCam* cams;       // [K]
    const float* body_rgb;  // [N,24,3] or null
    const int32_t* body_seg;  // [N,24] or null
    const float* mpos;      // [N,m,3]
    const float* mrgb;      // [m,3]
    uint32_t* color;        // [K,H,W] packed RGBA8, or null
    float* depth;           // [K,H,W] or null
    int32_t* seg;           // [K,H,W] or null
    int32_t W, H, m;
    uint32_t flags;
    float mradius;
    const int32_t* terrain_kind;  // [N] or null: the plane everywhere
    float sn, cs, step_h, step_l;  // the slope's sine and cosine, the steps' height and length
};

// the ray-cast sensor's own arguments (the scene is a Params)
struct RayParams {
    const hr_ray* rays;  // [R], in the frame of `body`
    float* dist;         // [N,R] or null
    int32_t* hit;        // [N,R] or null
    int32_t R, body, mode;
    float max_range;
};

struct f3 {
    float x, y, z;
};
__device__ inline f3 operator+(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline f3 operator-(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline f3 operator*(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
__device__ inline float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline f3 cross(f3 a, f3 b) { return f3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline f3 normalize(f3 a) { return a * (1.f / sqrtf(dot(a, a))); }
__device__ inline f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }

// rot(q, v) = (v + w t) + qv x t, t = 2 (qv x v)
__device__ inline f3 rot(const float* q, f3 v) {
    const f3 qv{q[0], q[1], q[2]};
    const f3 t = cross(qv, v) * 2.f;
    return (v + t * q[3]) + cross(qv, t);
}

// The following camera's world points, each product and sum rounded on its own (the header's promise
// that a fixed camera at host-computed points draws the same bits): no contraction in here.
__device__ inline void camera_points(const DCam& c, const float* rb, f3& P, f3& T) {
#pragma clang fp contract(off)
    P = ld3(c.pos);
    T = ld3(c.target);
    if (c.follow_body >= 0) {
        const float* row = rb + ((size_t)c.env * NB + c.follow_body) * 13;
        const f3 p = ld3(row);
        if (c.follow_mode == HR_FOLLOW_TRANSFORM) {
            const float qx = row[3], qy = row[4], qz = row[5], qw = row[6];
            f3 v[2] = {P, T};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const f3 a = v[i];
                const float tx = 2.f * (qy * a.z - qz * a.y);
                const float ty = 2.f * (qz * a.x - qx * a.z);
                const float tz = 2.f * (qx * a.y - qy * a.x);
                const float cx = qy * tz - qz * ty;
                const float cy = qz * tx - qx * tz;
                const float cz = qx * ty - qy * tx;
                v[i] = f3{(a.x + qw * tx) + cx, (a.y + qw * ty) + cy, (a.z + qw * tz) + cz};
            }
            P = v[0];
            T = v[1];
        }
        const bool xy = c.follow_mode == HR_FOLLOW_POSITION_XY;  // the heights stay absolute
        P = f3{p.x + P.x, p.y + P.y, xy ? P.z : p.z + P.z};
        T = f3{p.x + T.x, p.y + T.y, xy ? T.z : p.z + T.z};
    }
}

// a primitive in LDS (24 words)
struct Prim {
    int32_t type;  // HE_GEOM_*
    float bc[3];   // bounding sphere
    float br;
    float g[15];   // sphere: C3 r | capsule: A3 w3 L r B3 | box: C3 e3 R9 (columns)
    float rgb[3];
    int32_t seg;
};
struct Cam {
    float o[3], f[3], r[3], u[3];
    float tx, ty, nearp, farp;
};

// entry hit of a sphere, m = o - C
__device__ inline bool hit_sphere(f3 m, f3 d, float r, float& t, f3& n) {
    const float b = dot(m, d);
    const f3 q = m - d * b;
    const float h = r * r - dot(q, q);
    if (h < 0.f) return false;
    t = -b - sqrtf(h);
    n = (m + d * t) * (1.f / r);
    return true;
}

__device__ inline bool intersect(const Prim& p, f3 o, f3 d, float& t, f3& n) {
    const float* g = p.g;
    const int type = p.type;
    if (type == HE_GEOM_SPHERE) return hit_sphere(o - ld3(g), d, g[3], t, n);
    if (type == HE_GEOM_CAPSULE) {
        const f3 m = o - ld3(g), w = ld3(g + 3);
        const float L = g[6], r = g[7];
        bool hit = hit_sphere(m, d, r, t, n);
        float t2;
        f3 n2;
        if (hit_sphere(o - ld3(g + 8), d, r, t2, n2) && (!hit || t2 < t)) {
            t = t2;
            n = n2;
            hit = true;
        }
        const float mw = dot(m, w), dw = dot(d, w);
        const f3 mp = m - w * mw, dp = d - w * dw;
        const float a = dot(dp, dp);
        const f3 c = cross(mp, dp);
        const float h = a * r * r - dot(c, c);
        if (a >= 1e-12f && h >= 0.f) {
            t2 = (-dot(mp, dp) - sqrtf(h)) / a;
            const float s = mw + t2 * dw;
            if (s >= 0.f && s <= L && (!hit || t2 < t)) {
                t = t2;
                n = (mp + dp * t2) * (1.f / r);
                hit = true;
            }
        }
        return hit;
    }
    // box: slabs in the box frame
    const f3 mo = o - ld3(g);
    const f3 c0 = ld3(g + 6), c1 = ld3(g + 9), c2 = ld3(g + 12);
    const float ol[3] = {dot(c0, mo), dot(c1, mo), dot(c2, mo)};
    const float dl[3] = {dot(c0, d), dot(c1, d), dot(c2, d)};
    float lo[3], tn = -INFINITY, tf = INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t1 = (-g[3 + k] - ol[k]) / dl[k], t2 = (g[3 + k] - ol[k]) / dl[k];
        lo[k] = fminf(t1, t2);
        tn = fmaxf(tn, lo[k]);
        tf = fminf(tf, fmaxf(t1, t2));
    }
    if (!(tn <= tf)) return false;
    t = tn;
    const int k = lo[0] == tn ? 0 : (lo[1] == tn ? 1 : 2);
    const f3 ax = k == 0 ? c0 : (k == 1 ? c1 : c2);
    const float dk = k == 0 ? dl[0] : (k == 1 ? dl[1] : dl[2]);
    n = ax * (dk > 0.f ? -1.f : 1.f);
    return true;
}

// ground: the plane z = 0
__device__ inline bool hit_plane(f3 o, f3 d, float& t) {
    if (!(d.z < 0.f && o.z > 0.f)) return false;
    t = -o.z / d.z;
    return true;
}

// The box steps along +x: cell c(x) = max(floor(x / L), 0) of height S c. The walk over the cells is
// the header's, HR_MAX_STEP_CELLS cells at most. Two kinds of ray leave before it because no step of
// it can give them a hit: one that does not descend and does not move up the stairs (treads need
// d.z < 0, risers d.x > 0), and, inside the walk, a ray that does not descend once it has cleared a
// riser while climbing faster than the stairs do (every later riser is cleared by more).
// The walk does not begin at the ray's own cell when the ray starts well above the line z = S x / L
// (from x < 0: the line through (o.x, 0) of that slope), which no tread or riser on the ray's way
// reaches: the cells it crosses while it is more than m above that
// line cannot give a hit, so the walk lands one cell before the first that might (they count towards
// the HR_MAX_STEP_CELLS all the same, and t0 is the boundary's, as the walk would have left it). m is
// 1e-4 of the heights involved, a thousand times the rounding of the walk's own z_b.
// ckx: the x the steps' checker takes (a riser's is the middle of the tread below it).
__device__ inline bool hit_steps(float L, float S, f3 o, f3 d, float farp, float& t, f3& n, float& ckx) {
    float c = fmaxf(floorf(o.x / L), 0.f);
    if (o.z <= S * c) return false;  // inside the solid: entry hits only
    if (d.z >= 0.f && d.x <= 0.f) return false;
    const bool outruns = d.z >= 0.f && d.z * L >= 1.01f * S * d.x;
    float t0 = 0.f;
    int it = 0;
    {
        const float k = S / L, xo = fmaxf(o.x, 0.f);
        const float g0 = o.z - k * xo, g1 = d.z - k * d.x;  // height over the line, and its rate
        const float m = 1e-4f * (fabsf(o.z) + k * xo + (float)HR_MAX_STEP_CELLS * S);
        if (g0 > m && d.x > 0.f) {
            if (g1 >= 0.f) return false;  // never comes down to it
            const float cs = floorf((o.x + ((g0 - m) / -g1) * d.x) / L) - 1.f;
            if (cs > c) {
                if (cs - c >= (float)HR_MAX_STEP_CELLS) return false;
                it = (int)(cs - c);
                c = cs;
                t0 = (c * L - o.x) / d.x;
                if (t0 > farp) return false;
            }
        } else if (g0 > m && d.x < 0.f) {  // down the stairs, as far as cell 1 (cell 0 is all of x < L)
            const float xs = g1 < 0.f ? o.x + ((g0 - m) / -g1) * d.x : -INFINITY;
            const float cs = fmaxf(floorf(xs / L) + 1.f, 1.f);
            if (cs < c) {
                if (c - cs >= (float)HR_MAX_STEP_CELLS) return false;
                it = (int)(c - cs);
                t0 = ((cs + 1.f) * L - o.x) / d.x;
                c = cs;
                if (t0 > farp) return false;
            }
        }
    }
    for (; it < HR_MAX_STEP_CELLS; ++it) {
        if (d.z < 0.f) {  // the tread
            const float tt = (S * c - o.z) / d.z;
            const float xt = o.x + tt * d.x;
            if (tt >= t0 && xt < (c + 1.f) * L && (c == 0.f || xt >= c * L)) {
                t = tt;
                n = f3{0.f, 0.f, 1.f};
                ckx = xt;
                return true;
            }
        }
        if (d.x > 0.f) {  // up the stairs: the riser of the next cell
            const float tb = ((c + 1.f) * L - o.x) / d.x;
            if (tb > farp) return false;
            const float zb = o.z + tb * d.z, hn = S * (c + 1.f);
            if (zb < hn) {
                t = tb;
                n = f3{-1.f, 0.f, 0.f};
                ckx = (c + 0.5f) * L;
                return true;
            }
            if (outruns && zb - hn >= 1e-4f * fabsf(zb)) return false;
            c += 1.f;
            t0 = tb;
        } else if (d.x < 0.f) {  // down the stairs: a riser faces -x and is never entered from above
            if (c == 0.f) return false;
            const float tb = (c * L - o.x) / d.x;
            if (tb > farp) return false;
            c -= 1.f;
            t0 = tb;
        } else {
            return false;
        }
    }
    return false;
}

// entry hit of the env's terrain (kind 1 the slope, 2 the steps, anything else the plane)
__device__ inline bool hit_terrain(const Params& P, int kind, f3 o, f3 d, float farp, float& t, f3& n, float& ckx) {
    if (kind == 1) {
        n = f3{-P.sn, 0.f, P.cs};
        const float dn = dot(d, n), on = dot(o, n);
        if (!(dn < 0.f && on > 0.f)) return false;
        t = -on / dn;
        return true;
    }
    if (kind == 2) return hit_steps(P.step_l, P.step_h, o, d, farp, t, n, ckx);
    n = f3{0.f, 0.f, 1.f};
    return hit_plane(o, d, t);
}

// may the ray touch the primitive's bounding sphere? Conservative: the slack covers the rounding of
// the test itself (|q| carries about 4e-7 |m|), so culling never changes a pixel.
__device__ inline bool may_hit(const Prim& p, f3 o, f3 d) {
    const f3 m = o - ld3(p.bc);
    const float b = dot(m, d), mm = dot(m, m);
    const f3 q = m - d * b;
    const float slack = 1e-5f * mm + 1e-4f;
    return dot(q, q) <= p.br * p.br + slack && b <= p.br + slack;
}

__device__ void build_prim(const Params& P, int env, int i, Prim& out) {
    if (i < NB) {
        const float* row = P.rb + ((size_t)env * NB + i) * 13;
        const float* q = row + 3;
        const f3 p = ld3(row);
        const float* g = P.geom + i * kGeomWords;
        const int type = __float_as_int(g[0]);
        const float* gp = g + 1;
        out.type = type;
        f3 bc;
        float br;
        if (type == HE_GEOM_SPHERE) {
            bc = p + rot(q, ld3(gp));
            br = gp[3];
            out.g[0] = bc.x, out.g[1] = bc.y, out.g[2] = bc.z, out.g[3] = gp[3];
        } else if (type == HE_GEOM_CAPSULE) {
            const f3 A = p + rot(q, ld3(gp)), B = p + rot(q, ld3(gp + 3));
            const f3 ab = B - A;
            float L = sqrtf(dot(ab, ab));
            f3 w{0.f, 0.f, 1.f};
            if (L < 1e-9f) L = 0.f;
            else w = ab * (1.f / L);
            out.g[0] = A.x, out.g[1] = A.y, out.g[2] = A.z;
            out.g[3] = w.x, out.g[4] = w.y, out.g[5] = w.z;
            out.g[6] = L, out.g[7] = gp[6];
            out.g[8] = B.x, out.g[9] = B.y, out.g[10] = B.z;
            bc = (A + B) * 0.5f;
            br = 0.5f * L + gp[6];
        } else {
            bc = p + rot(q, ld3(gp));
            // Hamilton product q * qb
            const float ax = q[0], ay = q[1], az = q[2], aw = q[3];
            const float bx = gp[6], by = gp[7], bz = gp[8], bw = gp[9];
            const float x = aw * bx + ax * bw + ay * bz - az * by;
            const float y = aw * by - ax * bz + ay * bw + az * bx;
            const float z = aw * bz + ax * by - ay * bx + az * bw;
            const float w = aw * bw - ax * bx - ay * by - az * bz;
            out.g[0] = bc.x, out.g[1] = bc.y, out.g[2] = bc.z;
            out.g[3] = gp[3], out.g[4] = gp[4], out.g[5] = gp[5];
            out.g[6] = 1.f - 2.f * (y * y + z * z), out.g[7] = 2.f * (x * y + w * z), out.g[8] = 2.f * (x * z - w * y);
            out.g[9] = 2.f * (x * y - w * z), out.g[10] = 1.f - 2.f * (x * x + z * z), out.g[11] = 2.f * (y * z + w * x);
            out.g[12] = 2.f * (x * z + w * y), out.g[13] = 2.f * (y * z - w * x), out.g[14] = 1.f - 2.f * (x * x + y * y);
            br = sqrtf(gp[3] * gp[3] + gp[4] * gp[4] + gp[5] * gp[5]);
        }
        out.bc[0] = bc.x, out.bc[1] = bc.y, out.bc[2] = bc.z;
        out.br = br * 1.001f + 1e-4f;
        const size_t a = (size_t)env * NB + i;
        out.rgb[0] = P.body_rgb ? P.body_rgb[a * 3 + 0] : HR_BODY_R;
        out.rgb[1] = P.body_rgb ? P.body_rgb[a * 3 + 1] : HR_BODY_G;
        out.rgb[2] = P.body_rgb ? P.body_rgb[a * 3 + 2] : HR_BODY_B;
        out.seg = P.body_seg ? P.body_seg[a] : 0;
    } else {
        const int k = i - NB;
        const float* c = P.mpos + ((size_t)env * P.m + k) * 3;
        out.type = HE_GEOM_SPHERE;
        out.g[0] = out.bc[0] = c[0], out.g[1] = out.bc[1] = c[1], out.g[2] = out.bc[2] = c[2];
        out.g[3] = P.mradius;
        out.br = P.mradius * 1.001f + 1e-4f;
        out.rgb[0] = P.mrgb[k * 3], out.rgb[1] = P.mrgb[k * 3 + 1], out.rgb[2] = P.mrgb[k * 3 + 2];
        out.seg = HR_SEG_MARKER;
    }
}

__device__ void build_camera(const Params& P, const DCam& c, Cam& out) {
    f3 o, T;
    camera_points(c, P.rb, o, T);
    const f3 f = normalize(T - o);
    f3 r = cross(f, f3{0.f, 0.f, 1.f});
    if (dot(r, r) < 1e-12f) r = cross(f, f3{0.f, 1.f, 0.f});  // |f x z| < 1e-6
    r = normalize(r);
    const f3 u = cross(r, f);
    out.o[0] = o.x, out.o[1] = o.y, out.o[2] = o.z;
    out.f[0] = f.x, out.f[1] = f.y, out.f[2] = f.z;
    out.r[0] = r.x, out.r[1] = r.y, out.r[2] = r.z;
    out.u[0] = u.x, out.u[1] = u.y, out.u[2] = u.z;
    out.tx = c.th;
    out.ty = c.th * (float)P.H / (float)P.W;
    out.nearp = c.nearp;
    out.farp = c.farp;
}

__device__ inline uint32_t channel(float c) {
    c = fminf(fmaxf(c, 0.f), 1.f);
    return (uint32_t)(int)(c * 255.f + 0.5f);
}

// TERRAIN = false is the kernel of a renderer without a kind array: the ground is the plane at compile
// time, and nothing of the terrain is in its code.
template <bool TERRAIN>
__global__ __launch_bounds__(256) void render_kernel(const Params P) {
    __shared__ Prim prims[kMaxPrims];
    __shared__ Cam cam;
    const int tid = threadIdx.y * kTile + threadIdx.x;
    const int k = blockIdx.z;
    const DCam& dc = P.cams[k];
    const int env = dc.env;
    const int tk = TERRAIN ? P.terrain_kind[env] : 0;  // wave-uniform: a scalar load
    const int nprim = NB + P.m;
    if (tid < nprim) build_prim(P, env, tid, prims[tid]);
    if (tid == kMaxPrims) build_camera(P, dc, cam);
    __syncthreads();  // every thread of the workgroup, partial tiles included

    const int j = blockIdx.x * kTile + threadIdx.x, i = blockIdx.y * kTile + threadIdx.y;
    const bool valid = j < P.W && i < P.H;
    const f3 o = ld3(cam.o), f = ld3(cam.f);
    const float x = (2.f * ((float)j + 0.5f) / (float)P.W - 1.f) * cam.tx;
    const float y = (1.f - 2.f * ((float)i + 0.5f) / (float)P.H) * cam.ty;
    const f3 d = normalize(f + ld3(cam.r) * x + ld3(cam.u) * y);
    const float nearp = cam.nearp, farp = cam.farp;

    // the primitives any ray of this wave may hit
    const bool cull = !(P.flags & HR_FLAG_NO_CULL);
    unsigned long long mask = nprim >= 64 ? ~0ull : ((1ull << nprim) - 1ull);
    if (cull) {
        mask = 0ull;
        for (int p = 0; p < nprim; ++p)
            if (__ballot(valid && may_hit(prims[p], o, d)) != 0ull) mask |= 1ull << p;
    }

    float best = INFINITY;
    int who = -2;  // -2 sky, -1 ground (the env's terrain), else the primitive
    f3 n{0.f, 0.f, 1.f};
    float ckx = 0.f;
    if constexpr (TERRAIN) {
        float t;
        f3 nn;
        if (hit_terrain(P, tk, o, d, farp, t, nn, ckx) && t >= nearp && t <= farp) {
            best = t;
            who = -1;
            n = nn;
        }
    } else {
        float t;
        if (hit_plane(o, d, t) && t >= nearp && t <= farp) {
            best = t;
            who = -1;
        }
    }
    for (unsigned long long mm = mask; mm != 0ull; mm &= mm - 1ull) {
        const int p = __builtin_ctzll(mm);
        float t;
        f3 nn;
        if (intersect(prims[p], o, d, t, nn) && t >= nearp && t <= farp && t < best) {
            best = t;
            who = p;
            n = nn;
        }
    }

    float cr = HR_SKY_R, cg = HR_SKY_G, cb = HR_SKY_B;
    int sid = 0;
    const bool hit = who > -2;
    const f3 hp = o + d * best;
    const f3 l{HR_LIGHT_X, HR_LIGHT_Y, HR_LIGHT_Z};
    const float ndl = fmaxf(0.f, dot(n, l));
    // shadow rays: a second wave-uniform mask over the body geoms
    float s = 1.f;
    if (P.flags & HR_FLAG_SHADOWS) {
        const bool want = valid && hit && ndl > 0.f;
        const f3 so = hp + n * HR_SHADOW_EPS;
        unsigned long long smask = 0ull;
        if (cull) {
            for (int p = 0; p < NB; ++p)
                if (__ballot(want && may_hit(prims[p], so, l)) != 0ull) smask |= 1ull << p;
        } else if (__ballot(want) != 0ull) {
            smask = (1ull << NB) - 1ull;
        }
        for (unsigned long long mm = smask; mm != 0ull; mm &= mm - 1ull) {
            const int p = __builtin_ctzll(mm);
            float t;
            f3 nn;
            if (want && intersect(prims[p], so, l, t, nn) && t >= 0.f) s = HR_SHADOW;
        }
    }
    if (hit) {
        float ar, ag, ab;
        if (who < 0) {
            const int par = (int)floorf(tk == 2 ? ckx : hp.x) + (int)floorf(hp.y);
            ar = ag = ab = ((P.flags & HR_FLAG_CHECKER) && (par & 1)) ? HR_GROUND_ODD : HR_GROUND_EVEN;
        } else {
            ar = prims[who].rgb[0], ag = prims[who].rgb[1], ab = prims[who].rgb[2];
            sid = prims[who].seg;
        }
        const float shade = HR_AMBIENT + (1.f - HR_AMBIENT) * ndl * s;
        cr = ar * shade, cg = ag * shade, cb = ab * shade;
    }
    if (valid) {
        const size_t px = ((size_t)k * P.H + i) * P.W + j;
        if (P.color) P.color[px] = channel(cr) | channel(cg) << 8 | channel(cb) << 16 | 0xff000000u;
        if (P.depth) P.depth[px] = hit ? -best * dot(d, f) : -INFINITY;
        if (P.seg) P.seg[px] = sid;
    }
}

// The ray-cast sensor: block = env, one wave. The hits are the image's with near = 0, far = max_range:
// terrain first, then bodies 0..23, a strictly nearer one replaces; markers are never hit.
__global__ __launch_bounds__(64) void rays_kernel(const Params P, const RayParams A) {
    __shared__ Prim prims[NB];
    const int env = blockIdx.x, lane = threadIdx.x;
    const int tk = P.terrain_kind ? P.terrain_kind[env] : 0;
    const bool bodies = !(P.flags & HR_RAYS_SKIP_BODIES);
    if (bodies && lane < NB) build_prim(P, env, lane, prims[lane]);
    __syncthreads();
    const float* row = P.rb + ((size_t)env * NB + A.body) * 13;
    const f3 p = ld3(row);
    const float* q = row + 3;
    float hc = 1.f, hs = 0.f;  // the heading
    if (A.mode == HR_RAY_FRAME_HEADING) {
        const f3 hx = rot(q, f3{1.f, 0.f, 0.f});
        const float l = sqrtf(hx.x * hx.x + hx.y * hx.y);
        if (!(l < 1e-6f)) hc = hx.x / l, hs = hx.y / l;
    }
    for (int r = lane; r < A.R; r += 64) {
        f3 ro = ld3(A.rays[r].origin), d = ld3(A.rays[r].dir);
        if (A.mode == HR_RAY_FRAME_HEADING) {
            ro = f3{hc * ro.x - hs * ro.y, hs * ro.x + hc * ro.y, ro.z};
            d = f3{hc * d.x - hs * d.y, hs * d.x + hc * d.y, d.z};
        } else if (A.mode == HR_RAY_FRAME_TRANSFORM) {
            ro = rot(q, ro);
            d = rot(q, d);
        }
        const f3 o = p + ro;
        float best = INFINITY, t, ckx;
        int who = -2;
        f3 nn;
        if (hit_terrain(P, tk, o, d, A.max_range, t, nn, ckx) && t >= 0.f && t <= A.max_range) {
            best = t;
            who = -1;
        }
        if (bodies) {
            for (int b = 0; b < NB; ++b)
                if (intersect(prims[b], o, d, t, nn) && t >= 0.f && t <= A.max_range && t < best) {
                    best = t;
                    who = b;
                }
        }
        const size_t at = (size_t)env * A.R + r;
        if (A.dist) A.dist[at] = best;
        if (A.hit) A.hit[at] = who;
    }
}

}  // namespace

struct hr_renderer {
    int device = 0;
    int num_envs = 0;
    DeviceArray<float> d_geom;
    DeviceArray<float> d_mrgb;  // [HR_MAX_MARKERS,3]
    DeviceArray<DCam> d_cams;
    int cam_cap = 0;
    int k = 0, W = 0, H = 0;
    // borrowed from the caller (hr_set_appearance, hr_set_markers), who keeps them alive
    const float* body_rgb = nullptr;
    const int32_t* body_seg = nullptr;
    const float* mpos = nullptr;
    int m = 0;
    float mradius = 0.f;
    // hr_set_terrain: the borrowed kind array and the host's floats
    const int32_t* terrain_kind = nullptr;
    float sn = 0.f, cs = 1.f, step_h = 0.f, step_l = 1.f;
    // hr_set_rays
    DeviceArray<hr_ray> d_rays;
    int ray_cap = 0;
    int R = 0, ray_body = 0, ray_mode = 0;
};

namespace {

// the scene both kernels read
Params scene_params(const hr_renderer* h, const float* rb_state, uint32_t flags) {
    Params P{};
    P.rb = rb_state;
    P.geom = h->d_geom;
    P.body_rgb = h->body_rgb;
    P.body_seg = h->body_seg;
    P.flags = flags;
    P.terrain_kind = h->terrain_kind;
    P.sn = h->sn;
    P.cs = h->cs;
    P.step_h = h->step_h;
    P.step_l = h->step_l;
    return P;
}

}  // namespace

extern "C" {

const char* hr_last_error(void) { return last_error(); }
int hr_version(void) { return 1; }

int hr_create(int device, const he_model* model, int num_envs, hr_renderer** out) {
    if (!out) return fail("hr_create: null output pointer");
    *out = nullptr;
    if (check_model(model, "hr_create", HE_MAX_BOXES)) return 1;
    if (num_envs < 1) return fail("hr_create: num_envs %d < 1", num_envs);
    float geom[NB * kGeomWords];
    for (int b = 0; b < NB; ++b) {
        memcpy(&geom[b * kGeomWords], &model->geom_type[b], sizeof(int32_t));
        memcpy(&geom[b * kGeomWords + 1], model->geom_params[b], 10 * sizeof(float));
    }
    if (select_device(device, "hr_create")) return 1;
    std::unique_ptr<hr_renderer> h(new hr_renderer);  // a failed step below frees it and its arrays
    h->device = device;
    h->num_envs = num_envs;
    HE_CHECK(h->d_geom.assign(geom, NB * kGeomWords));
    HE_CHECK(h->d_mrgb.alloc(HR_MAX_MARKERS * 3));
    *out = h.release();
    return 0;
}

int hr_destroy(hr_renderer* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;
    return 0;
}

int hr_validate_cameras(const hr_camera* c, int k, int num_envs) {
    if (k < 1) return fail("camera set: k = %d < 1", k);
    if (!c) return fail("camera set: null camera array");
    for (int i = 0; i < k; ++i) {
        if (c[i].width < 1 || c[i].height < 1) return fail("camera %d: size %d x %d is not positive", i, c[i].width, c[i].height);
        if (c[i].width != c[0].width || c[i].height != c[0].height)
            return fail("camera %d is %d x %d, camera 0 is %d x %d: the cameras of one renderer share one size", i,
                        c[i].width, c[i].height, c[0].width, c[0].height);
        if (!(c[i].hfov_deg > 0.f && c[i].hfov_deg < 180.f)) return fail("camera %d: horizontal fov %g not in (0, 180)", i, c[i].hfov_deg);
        if (!(c[i].near > 0.f)) return fail("camera %d: near plane %g is not positive", i, c[i].near);
        if (!(c[i].far >= c[i].near)) return fail("camera %d: far plane %g before the near plane %g", i, c[i].far, c[i].near);
        if (c[i].env < 0 || c[i].env >= num_envs) return fail("camera %d: env %d outside [0, %d)", i, c[i].env, num_envs);
        if (c[i].follow_body < -1 || c[i].follow_body >= NB) return fail("camera %d: follow_body %d outside [-1, %d)", i, c[i].follow_body, NB);
        if (c[i].follow_mode < HR_FOLLOW_POSITION || c[i].follow_mode > HR_FOLLOW_POSITION_XY)
            return fail("camera %d: follow_mode %d is not 0 (position), 1 (transform) or 2 (position xy)", i, c[i].follow_mode);
    }
    return 0;
}

int hr_set_cameras(hr_renderer* h, const hr_camera* c, int k) {
    if (!h) return fail("hr_set_cameras: null handle");
    if (hr_validate_cameras(c, k, h->num_envs)) return 1;
    if ((long long)k > 65535) return fail("hr_set_cameras: %d cameras, at most 65535 in one launch", k);
    std::vector<DCam> dc(k);
    for (int i = 0; i < k; ++i) {
        dc[i].env = c[i].env;
        dc[i].follow_body = c[i].follow_body;
        dc[i].follow_mode = c[i].follow_mode;
        dc[i].th = (float)tan((double)c[i].hfov_deg * (M_PI / 360.0));
        dc[i].nearp = c[i].near;
        dc[i].farp = c[i].far;
        for (int a = 0; a < 3; ++a) dc[i].pos[a] = c[i].pos[a], dc[i].target[a] = c[i].target[a];
    }
    HE_CHECK(hipSetDevice(h->device));
    if (k > h->cam_cap) {
        DeviceArray<DCam> p;
        HE_CHECK(p.assign(dc.data(), k));
        h->d_cams = std::move(p);
        h->cam_cap = k;
    } else {
        HE_CHECK(h->d_cams.upload(dc.data(), k));
    }
    h->k = k;
    h->W = c[0].width;
    h->H = c[0].height;
    return 0;
}

int hr_set_appearance(hr_renderer* h, const float* body_rgb, const int32_t* body_seg) {
    if (!h) return fail("hr_set_appearance: null handle");
    h->body_rgb = body_rgb;
    h->body_seg = body_seg;
    return 0;
}

int hr_set_markers(hr_renderer* h, const float* pos, int m, const float* host_rgb, float radius) {
    if (!h) return fail("hr_set_markers: null handle");
    if (m < 0 || m > HR_MAX_MARKERS) return fail("hr_set_markers: %d markers, 0..%d per env", m, HR_MAX_MARKERS);
    if (m == 0) {
        h->m = 0;
        h->mpos = nullptr;
        return 0;
    }
    if (!pos || !host_rgb) return fail("hr_set_markers: null positions or colours");
    if (!(radius > 0.f)) return fail("hr_set_markers: radius %g is not positive", radius);
    HE_CHECK(hipSetDevice(h->device));
    HE_CHECK(h->d_mrgb.upload(host_rgb, (size_t)m * 3));
    h->mpos = pos;
    h->m = m;
    h->mradius = radius;
    return 0;
}

int hr_set_terrain(hr_renderer* h, const int32_t* terrain_kind, float slope, float step_height, float step_length) {
    if (!h) return fail("hr_set_terrain: null handle");
    if (!std::isfinite(slope)) return fail("hr_set_terrain: slope %g is not finite", slope);
    if (!(std::isfinite(step_height) && step_height >= 0.f)) return fail("hr_set_terrain: step_height %g is not finite and >= 0", step_height);
    if (!(std::isfinite(step_length) && step_length > 0.f)) return fail("hr_set_terrain: step_length %g is not finite and > 0", step_length);
    h->terrain_kind = terrain_kind;
    h->sn = sinf(slope);
    h->cs = cosf(slope);
    h->step_h = step_height;
    h->step_l = step_length;
    return 0;
}

int hr_set_rays(hr_renderer* h, const hr_ray* rays, int R, int body, int frame_mode) {
    if (!h) return fail("hr_set_rays: null handle");
    if (!rays) return fail("hr_set_rays: null ray array");
    if (R < 1 || R > HR_MAX_RAYS) return fail("hr_set_rays: %d rays, 1..%d", R, HR_MAX_RAYS);
    if (body < 0 || body >= NB) return fail("hr_set_rays: body %d outside [0, %d)", body, NB);
    if (frame_mode < HR_RAY_FRAME_POSITION || frame_mode > HR_RAY_FRAME_TRANSFORM)
        return fail("hr_set_rays: frame_mode %d is not 0 (position), 1 (heading) or 2 (transform)", frame_mode);
    for (int i = 0; i < R; ++i) {
        double dd = 0.0;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(rays[i].origin[a]) || !std::isfinite(rays[i].dir[a]))
                return fail("hr_set_rays: ray %d has a component that is not finite", i);
            dd += (double)rays[i].dir[a] * (double)rays[i].dir[a];
        }
        if (!(fabs(sqrt(dd) - 1.0) <= 1e-3)) return fail("hr_set_rays: ray %d: |dir| = %g is not of unit length", i, sqrt(dd));
    }
    HE_CHECK(hipSetDevice(h->device));
    if (R > h->ray_cap) {
        DeviceArray<hr_ray> p;
        HE_CHECK(p.assign(rays, R));
        h->d_rays = std::move(p);
        h->ray_cap = R;
    } else {
        HE_CHECK(h->d_rays.upload(rays, R));
    }
    h->R = R;
    h->ray_body = body;
    h->ray_mode = frame_mode;
    return 0;
}

int hr_cast_rays(hr_renderer* h, const float* rb_state, float max_range, float* dist_out, int32_t* hit_out, uint32_t flags,
                 void* stream) {
    if (!h) return fail("hr_cast_rays: null handle");
    if (!rb_state) return fail("hr_cast_rays: null rb_state");
    if (!dist_out && !hit_out) return fail("hr_cast_rays: no output buffer");
    if (flags & ~HR_RAYS_SKIP_BODIES) return fail("hr_cast_rays: unknown flag bits 0x%x", flags & ~HR_RAYS_SKIP_BODIES);
    if (!(std::isfinite(max_range) && max_range > 0.f)) return fail("hr_cast_rays: max_range %g is not finite and > 0", max_range);
    if (h->R < 1) return fail("hr_cast_rays: no rays set (hr_set_rays)");
    const Params P = scene_params(h, rb_state, flags);
    RayParams A{};
    A.rays = h->d_rays;
    A.dist = dist_out;
    A.hit = hit_out;
    A.R = h->R;
    A.body = h->ray_body;
    A.mode = h->ray_mode;
    A.max_range = max_range;
    hipLaunchKernelGGL(rays_kernel, dim3(h->num_envs), dim3(64), 0, static_cast<hipStream_t>(stream), P, A);
    HE_CHECK(hipGetLastError());
    return 0;
}

int hr_render(hr_renderer* h, const float* rb_state, uint8_t* color, float* depth, int32_t* seg, uint32_t flags,
              void* stream) {
    if (!h) return fail("hr_render: null handle");
    if (h->k < 1) return fail("hr_render: no cameras (hr_set_cameras)");
    if (!rb_state) return fail("hr_render: null rb_state");
    if (!color && !depth && !seg) return fail("hr_render: no output buffer");
    if (reinterpret_cast<uintptr_t>(color) & 3u) return fail("hr_render: the colour buffer must be 4-byte aligned");
    Params P = scene_params(h, rb_state, flags);
    P.cams = h->d_cams;
    P.mpos = h->mpos;
    P.mrgb = h->d_mrgb;
    P.color = reinterpret_cast<uint32_t*>(color);
    P.depth = depth;
    P.seg = seg;
    P.W = h->W;
    P.H = h->H;
    P.m = h->m;
    P.mradius = h->mradius;
    const dim3 grid((h->W + kTile - 1) / kTile, (h->H + kTile - 1) / kTile, h->k);
    if (grid.y > 65535u) return fail("hr_render: image height %d too large for one launch", h->H);
    hipLaunchKernelGGL(h->terrain_kind ? render_kernel<true> : render_kernel<false>, grid, dim3(kTile, kTile, 1), 0,
                       static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
