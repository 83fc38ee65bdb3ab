// libhumanoid_dynamics.so: body Jacobians, joint-space inertia and bias force of every env
// (include/humanoid_dynamics.h defines the three). One launch, one 64-lane wave (= one block) per env:
// (load and kinematics are he_tree_state.h's tree_kinematics, shared with hs_solve.hip)
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

#include <cstring>

#include "../../include/humanoid_dynamics.h"
#include "he_host.h"
#include "he_topo.h"
#include "he_tree_state.h"

namespace {

constexpr int kJacEnv = NB * HD_JAC_ROWS * NG;  // 10800 dwords per env
constexpr int kJacBody = HD_JAC_ROWS * NG;      // 450
constexpr int kMassEnv = NG * NG;               // 5625

struct Params {
    const TreeModel* model;
    const float* root;  // [N,13]
    const float* dof;   // [N*69,2]
    float* jac;         // [N,24,6,75] or null
    float* mass;        // [N,75,75] or null
    float* bias;        // [N,75] or null
    uint32_t flags;
};

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

// 4 waves per SIMD is what a grid of 4096 envs fills (16 blocks per CU); saying so gives the register
// allocator 128 VGPRs to schedule the serial prologue with
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4, 4))) void dynamics_kernel(const Params P) {
    // the kinematic state at qdd = 0, one array each (he_tree_state.h names them and says why)
    __shared__ float sQ[ND], sU[ND], sR[NB][9], sP[NB][3], sW[NB][3], sWd[NB][3], sA[NB][3];
    __shared__ float sBody[NB][16];  // about o: m, h3 = m c, I_o (xx yy zz xy xz yz), wrench (n3, f3)
    __shared__ float sComp[NB][16];  // the same summed over the body's subtree
    __shared__ __align__(16) float sSF[NG][12];  // per column: motion vector S (w, v_o), then F = I^c S (n_o, p)
    __shared__ uint32_t sAnc[NB];

    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    const TreeState S{sQ, sU, nullptr, sR, sP, sW, sWd, sA};

    tree_kinematics<false>(S, P.model, P.root, P.dof, nullptr, env, lane);  // ends on a barrier

    if (lane < NB) {
        const int b = lane;
        sAnc[b] = M.anc[b];  // read after the barriers below
        const BodyWorld B = body_world(S, P.model, b);
        const float m = B.m;
        const v3 c = B.c;
        float* o = sBody[b];
        o[0] = m;
        st3(o + 1, c * m);
        // parallel axes: I_o = I_w + m (|c|^2 1 - c c^T)
        o[4] = B.wxx + m * (c.y * c.y + c.z * c.z);
        o[5] = B.wyy + m * (c.x * c.x + c.z * c.z);
        o[6] = B.wzz + m * (c.x * c.x + c.y * c.y);
        o[7] = B.wxy - m * c.x * c.y;
        o[8] = B.wxz - m * c.x * c.z;
        o[9] = B.wyz - m * c.y * c.z;
        // Newton-Euler at qdd = 0: f = m (a_c - g), t_c = I_w wd + w x I_w w, about o: n = t_c + c x f.
        // Inline, not a shared function: called as one, a_c's sums move behind the gravity branch, this
        // translation unit's SLP pairing follows, and c changes in its last bits.
        const m3 Iw{B.wxx, B.wxy, B.wxz, B.wxy, B.wyy, B.wyz, B.wxz, B.wyz, B.wzz};
        const v3 w = ld3(sW[b]), wd = ld3(sWd[b]);
        const v3 ac = ld3(sA[b]) + cross(wd, B.rc) + cross(w, cross(w, B.rc));
        const v3 g = (P.flags & HD_FLAG_NO_GRAVITY) ? v3{0.f, 0.f, 0.f} : ld3(M.gravity);
        const v3 f = (ac - g) * m;
        st3(o + 10, mul(Iw, wd) + cross(w, mul(Iw, w)) + cross(c, f));
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
            w = v3{S.R[j][i], S.R[j][3 + i], S.R[j][6 + i]};  // a = R_j e_i
            v = cross(ld3(S.P[j]), w);                      // a x (o - p_j)
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
                    a = v3{S.R[j][i], S.R[j][3 + i], S.R[j][6 + i]};
                    pj = ld3(S.P[j]);
                }
                const v3 zero{0.f, 0.f, 0.f};
                for (int b = 0; b < NB; ++b) {
                    const bool in = (sAnc[b] >> j & 1u) != 0;  // exact zeros outside j's subtree
                    v3 l = lin ? a : cross(a, ld3(S.P[b]) - pj);
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

struct hd_dynamics : QueryHandle<TreeModel> {};

extern "C" {

const char* hd_last_error(void) { return last_error(); }
int hd_version(void) { return 1; }

int hd_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    return check_tree_depth(model);
}

int hd_create(int device, const he_model* model, const float gravity[3], int num_envs, hd_dynamics** out) {
    return query_create("hd_create", device, model, gravity, num_envs, out, hd_validate_model, fill_tree_model);
}

int hd_destroy(hd_dynamics* h) { return query_destroy(h); }

int hd_compute(hd_dynamics* h, const float* root_state, const float* dof_state, float* jac_out, float* mass_out,
               float* bias_out, uint32_t flags, void* stream) {
    if (check_call("hd_compute", h, root_state, dof_state)) return 1;
    if (!jac_out && !mass_out && !bias_out) return fail("hd_compute: no output buffer");
    if (check_flags("hd_compute", flags, HD_FLAGS_ALL)) return 1;
    if (check_aligned("hd_compute", {root_state, dof_state, jac_out, mass_out, bias_out})) return 1;
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

// the centroidal queries (include/humanoid_centroidal.h, the hc_ entry points): a second kernel and entry-point
// family of this library, kept in a header of their own and included last
#include "hd_centroidal.h"
