// libhumanoid_dynamics.so: body Jacobians, joint-space inertia and bias force of every env
// (include/humanoid_dynamics.h defines the three). One launch, one 64-lane wave (= one block) per env:
//   load       root row and the 69 (pos, vel) pairs into LDS;
//   kinematics lanes 0..23 take one body each: the joint's Rodrigues matrix in registers, then one
//              pass per tree level composes rotation, origin (relative to the root origin o = p_0, the
//              reference point of all spatial quantities: levers stay below a body length), angular
//              velocity and, at qdd = 0, angular acceleration and origin acceleration into LDS;
//   bodies     lanes 0..23: spatial inertia about o (m, m c, I_o) and the Newton-Euler wrench about o;
//              lanes 0..74 (64 + 11): the column's motion vector S = (w, v_o);
//   subtrees   composite inertias and wrenches, one (body, component) per lane over the subtree mask;
//   columns    F = I^c S per column; the bias S . wrench^c goes out as one 75-dword row;
//   stores     a lane owns a COLUMN (lanes 0..63, then the 11-column tail in lanes 0..10) with the
//              column's constants in registers, and the loop walks the rows: one store instruction
//              covers 64 (or the last 11) consecutive dwords of one row. Plain dword stores, so no
//              alignment beyond 4 bytes is assumed: M's 22,500-byte env blocks and the 300-byte rows
//              are not 16-byte aligned. M[i,k] = S_anc . F_desc (CRBA), J from R and the relative
//              origins; both are exact zeros off the tree's pattern.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/humanoid_dynamics.h"
#include "he_host.h"
#include "he_topo.h"

namespace {

constexpr int NB = HE_NUM_BODIES;
constexpr int ND = HE_NUM_DOF;
constexpr int NG = HE_NUM_GEN;
constexpr int kWave = 64;
constexpr int kJacEnv = NB * HD_JAC_ROWS * NG;  // 10800 dwords per env
constexpr int kJacBody = HD_JAC_ROWS * NG;      // 450
constexpr int kMassEnv = NG * NG;               // 5625
constexpr int kMaxDepth = 8;                    // joints on the longest chain (he_topo.h body_chain)

// what the kernel reads of the model (hd_create)
struct DModel {
    int32_t parent[NB];
    int32_t depth[NB];
    uint32_t anc[NB];  // bit a: a is ancestor-or-self of b
    uint32_t sub[NB];  // bit d: d in subtree(b)
    float local_pos[NB][3];
    float mass[NB];
    float com[NB][3];
    float inertia[NB][6];  // xx yy zz xy xz yz
    float armature[ND];
    float gravity[3];
    int32_t max_depth;
};

struct Params {
    const DModel* model;
    const float* root;  // [N,13]
    const float* dof;   // [N*69,2]
    float* jac;         // [N,24,6,75] or null
    float* mass;        // [N,75,75] or null
    float* bias;        // [N,75] or null
    uint32_t flags;
};

struct v3 {
    float x, y, z;
};
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ v3 cross(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// S . F = w . n + v . p in one fixed order of fused multiply-adds
__device__ __forceinline__ float dot6(v3 w, v3 v, v3 n, v3 p) {
    return fmaf(v.z, p.z, fmaf(v.y, p.y, fmaf(v.x, p.x, fmaf(w.z, n.z, fmaf(w.y, n.y, w.x * n.x)))));
}
__device__ __forceinline__ v3 ld3(const float* p) { return v3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, v3 a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

// a 3x3 matrix in named registers (row-major): no indexed register arrays, so nothing goes to scratch
struct m3 {
    float a00, a01, a02, a10, a11, a12, a20, a21, a22;
};
__device__ __forceinline__ v3 mul(const m3& m, v3 v) {
    return v3{m.a00 * v.x + m.a01 * v.y + m.a02 * v.z, m.a10 * v.x + m.a11 * v.y + m.a12 * v.z,
              m.a20 * v.x + m.a21 * v.y + m.a22 * v.z};
}
__device__ __forceinline__ m3 mul(const m3& a, const m3& b) {
    return m3{a.a00 * b.a00 + a.a01 * b.a10 + a.a02 * b.a20, a.a00 * b.a01 + a.a01 * b.a11 + a.a02 * b.a21,
              a.a00 * b.a02 + a.a01 * b.a12 + a.a02 * b.a22, a.a10 * b.a00 + a.a11 * b.a10 + a.a12 * b.a20,
              a.a10 * b.a01 + a.a11 * b.a11 + a.a12 * b.a21, a.a10 * b.a02 + a.a11 * b.a12 + a.a12 * b.a22,
              a.a20 * b.a00 + a.a21 * b.a10 + a.a22 * b.a20, a.a20 * b.a01 + a.a21 * b.a11 + a.a22 * b.a21,
              a.a20 * b.a02 + a.a21 * b.a12 + a.a22 * b.a22};
}
__device__ __forceinline__ m3 ldm(const float* p) { return m3{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }
__device__ __forceinline__ void stm(float* p, const m3& m) {
    p[0] = m.a00, p[1] = m.a01, p[2] = m.a02, p[3] = m.a10, p[4] = m.a11, p[5] = m.a12, p[6] = m.a20, p[7] = m.a21,
    p[8] = m.a22;
}

// exp([v]x) = 1 + A K + B K^2, A = sin(th) / th, B = (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2 (no
// cancellation); below 1e-3 rad the series (the next terms are under 1e-14)
__device__ __forceinline__ m3 rodrigues(v3 v) {
    const float t2 = dot(v, v);
    float A, B;
    if (t2 < 1e-6f) {
        A = 1.f - t2 * (1.f / 6.f);
        B = 0.5f - t2 * (1.f / 24.f);
    } else {
        const float th = sqrtf(t2);
        const float sh = sinf(0.5f * th);
        A = sinf(th) / th;
        B = 2.f * sh * sh / t2;
    }
    const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z;
    const float xy = B * v.x * v.y, xz = B * v.x * v.z, yz = B * v.y * v.z;
    return m3{1.f - B * (yy + zz), xy - A * v.z, xz + A * v.y, xy + A * v.z, 1.f - B * (xx + zz), yz - A * v.x,
              xz - A * v.y, yz + A * v.x, 1.f - B * (xx + yy)};
}

__device__ __forceinline__ m3 quat_matrix(float x, float y, float z, float w) {
    const float n2 = x * x + y * y + z * z + w * w;
    if (n2 < 1e-24f) return m3{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    const float s = 2.f / n2;
    return m3{1.f - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w), s * (x * y + z * w),
              1.f - s * (x * x + z * z), s * (y * z - x * w), s * (x * z - y * w), s * (y * z + x * w),
              1.f - s * (x * x + y * y)};
}

__device__ __forceinline__ int col_joint(int c) { return c < 6 ? 0 : 1 + (c - 6) / 3; }

// a column of the mass matrix: S = (w, v), F = I^c S = (n, p), its joint and the joint's ancestor mask
struct Col {
    v3 Sw, Sv, Fn, Fp;
    uint32_t anc;
    int j;
    float arm;
};
__device__ __forceinline__ Col load_col(const float* sf, const uint32_t* anc, int c, bool arm, const float* armature) {
    const float4* q = reinterpret_cast<const float4*>(sf);  // 48-byte records, 16-byte aligned
    const float4 a = q[0], b = q[1], d = q[2];
    const int j = col_joint(c);
    return Col{v3{a.x, a.y, a.z}, v3{a.w, b.x, b.y}, v3{b.z, b.w, d.x}, v3{d.y, d.z, d.w}, anc[j], j,
               arm && c >= 6 ? armature[c - 6] : 0.f};
}
// M[i,k] = S_anc . F_desc when one column's joint is an ancestor-or-self of the other's, else 0. Bodies
// are in DFS order, so the ancestor is the column with the smaller index: one operand order for both
// triangles, M == M^T bit for bit. MODE 1: k <= i in every lane, 2: k > i in every lane, 0: either.
template <int MODE>
__device__ __forceinline__ float mass_entry(int i, int k, const Col& ci, const Col& ck) {
    float lo = 0.f, hi = 0.f;
    if (MODE != 2) lo = (ci.anc >> ck.j & 1u) ? dot6(ck.Sw, ck.Sv, ci.Fn, ci.Fp) : 0.f;  // k <= i
    if (MODE != 1) hi = (ck.anc >> ci.j & 1u) ? dot6(ci.Sw, ci.Sv, ck.Fn, ck.Fp) : 0.f;  // k > i
    float val = MODE == 1 ? lo : (MODE == 2 ? hi : (k <= i ? lo : hi));
    if (MODE != 2 && i == k) val += ck.arm;
    return val;
}

__global__ __launch_bounds__(kWave) void dynamics_kernel(const Params P) {
    __shared__ float sQ[ND], sU[ND];
    __shared__ float sR[NB][9];   // world rotation, row-major
    __shared__ float sP[NB][3];   // origin relative to the root origin o
    __shared__ float sW[NB][3];   // world angular velocity
    __shared__ float sWd[NB][3];  // world angular acceleration at qdd = 0
    __shared__ float sA[NB][3];   // origin acceleration at qdd = 0
    __shared__ float sBody[NB][16];  // about o: m, h3 = m c, I_o (xx yy zz xy xz yz), wrench (n3, f3)
    __shared__ float sComp[NB][16];  // the same summed over the body's subtree
    __shared__ __align__(16) float sSF[NG][12];  // per column: motion vector S (w, v_o), then F = I^c S (n_o, p)
    __shared__ uint32_t sAnc[NB];

    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const DModel& M = *P.model;

    for (int d = lane; d < ND; d += kWave) {
        const float* row = P.dof + (env * ND + d) * 2;
        sQ[d] = row[0];
        sU[d] = row[1];
    }
    const float* root = P.root + env * 13;
    m3 Rl{};  // body b >= 1: the joint's rotation; filled after the barrier below
    int depth = -1, parent = 0;
    if (lane < NB) {
        depth = M.depth[lane];
        parent = M.parent[lane];
        sAnc[lane] = M.anc[lane];
        if (lane == 0) {
            stm(sR[0], quat_matrix(root[3], root[4], root[5], root[6]));
            st3(sP[0], v3{0.f, 0.f, 0.f});
            st3(sW[0], ld3(root + 10));
            st3(sWd[0], v3{0.f, 0.f, 0.f});
            st3(sA[0], v3{0.f, 0.f, 0.f});
        }
    }
    __syncthreads();
    if (lane >= 1 && lane < NB) Rl = rodrigues(ld3(&sQ[3 * (lane - 1)]));

    // one pass per tree level (max_depth is the model's: the same in every lane)
    const int levels = M.max_depth;
    for (int lvl = 1; lvl <= levels; ++lvl) {
        if (depth == lvl) {
            const int b = lane, a = parent;
            const m3 Ra = ldm(sR[a]);
            const v3 wa = ld3(sW[a]), wda = ld3(sWd[a]);
            const m3 Rb = mul(Ra, Rl);
            const v3 d = mul(Ra, ld3(M.local_pos[b]));
            const v3 wrel = mul(Rb, ld3(&sU[3 * (b - 1)]));
            stm(sR[b], Rb);
            st3(sP[b], ld3(sP[a]) + d);
            st3(sW[b], wa + wrel);
            st3(sWd[b], wda + cross(wa, wrel));
            st3(sA[b], ld3(sA[a]) + cross(wda, d) + cross(wa, cross(wa, d)));
        }
        __syncthreads();
    }

    if (lane < NB) {
        const int b = lane;
        const m3 R = ldm(sR[b]);
        const float m = M.mass[b];
        const v3 rc = mul(R, ld3(M.com[b]));
        const v3 c = ld3(sP[b]) + rc;
        // I_w = R I R^T
        const float* ib = M.inertia[b];
        const m3 I{ib[0], ib[3], ib[4], ib[3], ib[1], ib[5], ib[4], ib[5], ib[2]};
        const m3 RI = mul(R, I);
        const float wxx = RI.a00 * R.a00 + RI.a01 * R.a01 + RI.a02 * R.a02;
        const float wyy = RI.a10 * R.a10 + RI.a11 * R.a11 + RI.a12 * R.a12;
        const float wzz = RI.a20 * R.a20 + RI.a21 * R.a21 + RI.a22 * R.a22;
        const float wxy = RI.a00 * R.a10 + RI.a01 * R.a11 + RI.a02 * R.a12;
        const float wxz = RI.a00 * R.a20 + RI.a01 * R.a21 + RI.a02 * R.a22;
        const float wyz = RI.a10 * R.a20 + RI.a11 * R.a21 + RI.a12 * R.a22;
        const m3 Iw{wxx, wxy, wxz, wxy, wyy, wyz, wxz, wyz, wzz};
        float* o = sBody[b];
        o[0] = m;
        st3(o + 1, c * m);
        // parallel axes: I_o = I_w + m (|c|^2 1 - c c^T)
        o[4] = wxx + m * (c.y * c.y + c.z * c.z);
        o[5] = wyy + m * (c.x * c.x + c.z * c.z);
        o[6] = wzz + m * (c.x * c.x + c.y * c.y);
        o[7] = wxy - m * c.x * c.y;
        o[8] = wxz - m * c.x * c.z;
        o[9] = wyz - m * c.y * c.z;
        // Newton-Euler at qdd = 0: f = m (a_c - g), t_c = I_w wd + w x I_w w, about o: n = t_c + c x f
        const v3 w = ld3(sW[b]), wd = ld3(sWd[b]);
        const v3 ac = ld3(sA[b]) + cross(wd, rc) + cross(w, cross(w, rc));
        const v3 g = (P.flags & HD_FLAG_NO_GRAVITY) ? v3{0.f, 0.f, 0.f} : ld3(M.gravity);
        const v3 f = (ac - g) * m;
        const v3 n = mul(Iw, wd) + cross(w, mul(Iw, w)) + cross(c, f);
        st3(o + 10, n);
        st3(o + 13, f);
    }
    for (int c = lane; c < NG; c += kWave) {
        v3 w{0.f, 0.f, 0.f}, v{0.f, 0.f, 0.f};
        if (c < 3) {
            v = v3{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        } else if (c < 6) {
            w = v3{c == 3 ? 1.f : 0.f, c == 4 ? 1.f : 0.f, c == 5 ? 1.f : 0.f};  // about o itself: v_o = 0
        } else {
            const int j = 1 + (c - 6) / 3, i = (c - 6) % 3;
            w = v3{sR[j][i], sR[j][3 + i], sR[j][6 + i]};  // a = R_j e_i
            v = cross(ld3(sP[j]), w);                      // a x (o - p_j)
        }
        st3(sSF[c], w);
        st3(sSF[c] + 3, v);
    }
    __syncthreads();

    // subtree sums: 24 x 16 (body, component) items
    for (int it = lane; it < NB * 16; it += kWave) {
        const int j = it >> 4, k = it & 15;
        const uint32_t sub = M.sub[j];
        float s = 0.f;
        for (int b = j; b < NB; ++b)  // DFS order: a subtree lies at and after its root
            if (sub >> b & 1u) s += sBody[b][k];
        sComp[j][k] = s;
    }
    __syncthreads();

    for (int c = lane; c < NG; c += kWave) {
        const float* I = sComp[col_joint(c)];
        const v3 w = ld3(sSF[c]), v = ld3(sSF[c] + 3);
        const v3 h = ld3(I + 1);
        const v3 n{I[4] * w.x + I[7] * w.y + I[8] * w.z, I[7] * w.x + I[5] * w.y + I[9] * w.z,
                   I[8] * w.x + I[9] * w.y + I[6] * w.z};
        st3(sSF[c] + 6, n + cross(h, v));              // angular momentum about o
        st3(sSF[c] + 9, v * I[0] + cross(w, h));       // linear momentum
        if (P.bias) P.bias[env * NG + c] = dot(w, ld3(I + 10)) + dot(v, ld3(I + 13));
    }
    __syncthreads();

    // Stores. A lane owns a column (slot 0: columns 0..63, slot 1: the 11-column tail) and keeps the
    // column's constants in registers; the loop walks the rows, so one store instruction covers 64 (or
    // the last 11) consecutive dwords of one row and a row costs a handful of instructions.
    if (P.mass) {
        float* out = P.mass + env * kMassEnv;
        const bool arm = (P.flags & HD_FLAG_ARMATURE) != 0;
        const bool tail = lane < NG - kWave;
        const int k0 = lane, k1 = tail ? lane + kWave : NG - 1;  // idle tail lanes compute column 74, store nothing
        const Col c0 = load_col(sSF[k0], sAnc, k0, arm, M.armature);
        const Col c1 = load_col(sSF[k1], sAnc, k1, arm, M.armature);
        // rows 0..63: every tail column lies right of the diagonal; rows 64..74: every slot-0 column left of it
        for (int i = 0; i < kWave; ++i) {
            const Col ci = load_col(sSF[i], sAnc, i, false, M.armature);
            out[i * NG + k0] = mass_entry<0>(i, k0, ci, c0);
            if (tail) out[i * NG + k1] = mass_entry<2>(i, k1, ci, c1);
        }
        for (int i = kWave; i < NG; ++i) {
            const Col ci = load_col(sSF[i], sAnc, i, false, M.armature);
            out[i * NG + k0] = mass_entry<1>(i, k0, ci, c0);
            if (tail) out[i * NG + k1] = mass_entry<0>(i, k1, ci, c1);
        }
    }

    if (P.jac) {
        float* out = P.jac + env * kJacEnv;
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            const int c = lane + slot * kWave;
            if (c < NG) {
                // the column's joint j, axis a and pivot p_j: root linear (e_i, 0) everywhere, root angular
                // (e_i x (p_b - p_0), e_i), dof i of joint j (a x (p_b - p_j), a) with a = R_j e_i
                const int j = col_joint(c);
                const bool lin = c < 3;
                const int i = c < 3 ? c : (c < 6 ? c - 3 : (c - 6) % 3);
                v3 a{i == 0 ? 1.f : 0.f, i == 1 ? 1.f : 0.f, i == 2 ? 1.f : 0.f};
                v3 pj{0.f, 0.f, 0.f};
                if (c >= 6) {
                    a = v3{sR[j][i], sR[j][3 + i], sR[j][6 + i]};
                    pj = ld3(sP[j]);
                }
                const v3 zero{0.f, 0.f, 0.f};
                for (int b = 0; b < NB; ++b) {
                    const bool in = (sAnc[b] >> j & 1u) != 0;  // exact zeros outside j's subtree
                    v3 l = lin ? a : cross(a, ld3(sP[b]) - pj);
                    v3 w = lin ? zero : a;
                    if (!in) l = zero, w = zero;
                    float* row = out + b * kJacBody + c;
                    row[0] = l.x, row[NG] = l.y, row[2 * NG] = l.z;
                    row[3 * NG] = w.x, row[4 * NG] = w.y, row[5 * NG] = w.z;
                }
            }
        }
    }
}

}  // namespace

struct hd_dynamics {
    int device = 0;
    int num_envs = 0;
    DeviceArray<DModel> d_model;
};

extern "C" {

const char* hd_last_error(void) { return last_error(); }
int hd_version(void) { return 1; }

int hd_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    int depth[NB] = {0};  // this kernel's own bound: one pass per tree level
    for (int b = 1; b < NB; ++b) {
        depth[b] = depth[model->parents[b]] + 1;
        if (depth[b] > kMaxDepth) return fail("model: body %d is %d joints from the root, at most %d", b, depth[b], kMaxDepth);
    }
    return 0;
}

int hd_create(int device, const he_model* model, const float gravity[3], int num_envs, hd_dynamics** out) {
    if (!out) return fail("hd_create: null output pointer");
    *out = nullptr;
    if (num_envs < 1) return fail("hd_create: num_envs %d < 1", num_envs);
    if (!gravity) return fail("hd_create: null gravity vector");
    if (hd_validate_model(model)) return 1;
    DModel dm{};
    for (int b = 0; b < NB; ++b) {
        const int a = model->parents[b];
        dm.parent[b] = a;
        dm.depth[b] = b == 0 ? 0 : dm.depth[a] + 1;
        dm.anc[b] = (b == 0 ? 0u : dm.anc[a]) | 1u << b;
        if (dm.depth[b] > dm.max_depth) dm.max_depth = dm.depth[b];
        dm.mass[b] = model->mass[b];
        for (int c = 0; c < 3; ++c) dm.local_pos[b][c] = model->local_pos[b][c], dm.com[b][c] = model->com[b][c];
        for (int c = 0; c < 6; ++c) dm.inertia[b][c] = model->inertia[b][c];
    }
    for (int b = 0; b < NB; ++b)
        for (int d = 0; d < NB; ++d)
            if (dm.anc[d] >> b & 1u) dm.sub[b] |= 1u << d;
    for (int d = 0; d < ND; ++d) dm.armature[d] = model->armature[d];
    for (int c = 0; c < 3; ++c) dm.gravity[c] = gravity[c];
    if (select_device(device, "hd_create")) return 1;
    std::unique_ptr<hd_dynamics> h(new hd_dynamics);  // a failed step below frees it and its array
    h->device = device;
    h->num_envs = num_envs;
    HE_CHECK(h->d_model.assign(&dm, 1));
    *out = h.release();
    return 0;
}

int hd_destroy(hd_dynamics* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;
    return 0;
}

int hd_compute(hd_dynamics* h, const float* root_state, const float* dof_state, float* jac_out, float* mass_out,
               float* bias_out, uint32_t flags, void* stream) {
    if (!h) return fail("hd_compute: null handle");
    if (!root_state || !dof_state) return fail("hd_compute: null state pointer");
    if (!jac_out && !mass_out && !bias_out) return fail("hd_compute: no output buffer");
    if (flags & ~HD_FLAGS_ALL) return fail("hd_compute: unknown flag bits 0x%x", flags & ~HD_FLAGS_ALL);
    const uintptr_t al = reinterpret_cast<uintptr_t>(root_state) | reinterpret_cast<uintptr_t>(dof_state) |
                         reinterpret_cast<uintptr_t>(jac_out) | reinterpret_cast<uintptr_t>(mass_out) |
                         reinterpret_cast<uintptr_t>(bias_out);
    if (al & 3u) return fail("hd_compute: every buffer must be 4-byte aligned");
    Params P{};
    P.model = h->d_model;
    P.root = root_state;
    P.dof = dof_state;
    P.jac = jac_out;
    P.mass = mass_out;
    P.bias = bias_out;
    P.flags = flags;
    hipLaunchKernelGGL(dynamics_kernel, dim3(h->num_envs), dim3(kWave), 0, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
