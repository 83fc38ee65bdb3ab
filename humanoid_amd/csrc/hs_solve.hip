// libhumanoid_solve.so: the solves with the joint-space inertia M a controller calls each step
// (include/humanoid_solve.h defines them). One launch, one 64-lane wave (= one block) per env, M never
// leaves the wave:
//   state      root row and the 69 (pos, vel) pairs into LDS; forward kinematics by tree level
//              (he_tree_state.h, the routine hd_dynamics.hip runs too, with the joints' accelerations
//              carried when the entry has any), the bodies' inertias and Newton-Euler wrenches about their
//              centres of mass,
//              their subtree sums about each joint's own origin, and per column the axis, the pivot and
//              F = I^c S;
//   solve_kernel (hs_forward_dynamics, hs_solve)
//              CRBA straight into regla::RegMat (lane j owns column j, H[i][j] = S_j . F_i on the
//              dof tree's pattern), the sparse L^T D L in registers (he_regla.h, deepest dof first, no
//              fill-in), the packed factor in LDS; then every right-hand side through
//              L^-T (solve_LT_vec_pipelined), D^-1 and L^-1 (solve_L_streamed), lane = dof. The k
//              vectors of hs_solve share the factor and take the same instructions one after another;
//   torque_kernel (hs_computed_torque)
//              no factorisation: w = RNEA at qdd = (0; qdd_des), the base block of M is the composite
//              inertia of the whole body (the root columns' F), a_b = M_bb^-1 (f_b - w_b) by a 6 x 6
//              L D L^T in every lane, tau = w - f + M_jb a_b with M_jb a_b = F_j . (a_b as a motion vector).
// Spatial quantities of a subtree are referred to its own joint origin, never to a common far point: an
// entry of M is then exact to float32 of the descendant's own inertia (see columns()).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

#include "../../include/humanoid_solve.h"
#include "he_host.h"
#include "he_regla.h"
#include "he_topo.h"
#include "he_tree_state.h"

namespace {

constexpr int NH = NG - kWave;  // the 11-column tail: second register set of lanes 0..10
static_assert(NB == smpl::kNB && NG == smpl::kNG, "he_regla.h is unrolled for this tree");

struct Params {
    const TreeModel* model;
    const float* root;       // [N,13]
    const float* dof;        // [N*69,2]
    const float* gen_force;  // [N,75] or null
    const float* qdd_des;    // [N,69] (torque_kernel)
    const float* rhs;        // [N,k,75] (solve_kernel, k > 0)
    float* out;              // [N,75] qdd, or [N,k,75]; torque_kernel: tau [N,69] or null
    float* base_acc;         // [N,6] or null
    int k;                   // 0: forward dynamics
    uint32_t flags;
};

// one env's working set (9.8 KB of LDS; solve_kernel adds the factor's 5.3 KB)
struct Lds {
    float q[ND], u[ND], qdd[ND], R[NB][9], P[NB][3], W[NB][3], Wd[NB][3], A[NB][3];  // what TreeState views
    float body[NB][16];           // m, centre of mass c3 (relative to o), I_w about it (xx yy zz xy xz yz), t_c3, f3
    float comp[NB][16];           // subtree j about its joint origin p_j: m, first moment h3, inertia 6, wrench (n3, f3)
    alignas(16) float SF[NG][12];  // per column: axis w, pivot (relative to o), then F = I^c S about the pivot (n, p)
    float bias[NG];                // S . wrench^c: c, or the RNEA force at (0; qdd_des)
};
// the factor, solve_kernel only
struct Factor {
    alignas(16) float Lp[smpl::kNpack + 4];  // packed unit-lower factor (he_regla.h: row K at kPackStart[K])
    int16_t pack_start[NG];
    int8_t dof_depth[NG];
};

// state -> S, F per column and the RNEA force per column. QDD: the joints' accelerations P.qdd_des enter
// the bodies' accelerations (tree_kinematics).
template <bool QDD>
__device__ __forceinline__ void columns(Lds& L, const TreeModel& M, const Params& P, size_t env, int lane) {
    const TreeState S{L.q, L.u, L.qdd, L.R, L.P, L.W, L.Wd, L.A};
    tree_kinematics<QDD>(S, &M, P.root, P.dof, P.qdd_des, env, lane);  // ends on a barrier

    if (lane < NB) {
        const int b = lane;
        const m3 R = ldm(L.R[b]);
        const float m = M.mass[b];
        const v3 rc = mul(R, ld3(M.com[b]));
        const v3 c = ld3(L.P[b]) + rc;
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
        // the body about its own centre of mass: nothing here is referred to a far point yet
        float* o = L.body[b];
        o[0] = m;
        st3(o + 1, c);
        o[4] = wxx, o[5] = wyy, o[6] = wzz, o[7] = wxy, o[8] = wxz, o[9] = wyz;
        // Newton-Euler: f = m (a_c - g), t_c = I_w wd + w x I_w w
        const v3 w = ld3(L.W[b]), wd = ld3(L.Wd[b]);
        const v3 ac = ld3(L.A[b]) + cross(wd, rc) + cross(w, cross(w, rc));
        const v3 g = (P.flags & HS_FLAG_NO_GRAVITY) ? v3{0.f, 0.f, 0.f} : ld3(M.gravity);
        st3(o + 10, mul(Iw, wd) + cross(w, mul(Iw, w)));
        st3(o + 13, (ac - g) * m);
    }
    for (int c = lane; c < NG; c += kWave) {
        v3 w{0.f, 0.f, 0.f}, pv{0.f, 0.f, 0.f};
        if (c >= 3 && c < 6) {
            w = v3{c == 3 ? 1.f : 0.f, c == 4 ? 1.f : 0.f, c == 5 ? 1.f : 0.f};
        } else if (c >= 6) {
            const int j = 1 + (c - 6) / 3, i = (c - 6) % 3;
            w = v3{L.R[j][i], L.R[j][3 + i], L.R[j][6 + i]};  // a = R_j e_i
            pv = ld3(L.P[j]);
        }
        st3(L.SF[c], w);
        st3(L.SF[c] + 3, pv);
    }
    __syncthreads();

    // Subtree sums about each joint's OWN origin p_j (lanes 0..23: mass, first moment, inertia; lanes
    // 24..47: wrench). Referred to the root origin instead, a hand's inertia about its joint would be the
    // difference of two m r^2 of a metre's lever: exact to float32 of the whole body's inertia, and wrong
    // in the fifth digit of its own, which is the scale its row of the solve is read at.
    if (lane < 2 * NB) {
        const bool wrench = lane >= NB;
        const int j = wrench ? lane - NB : lane;
        const v3 pj = ld3(L.P[j]);
        const uint32_t sub = M.sub[j];
        float ms = 0.f, ixx = 0.f, iyy = 0.f, izz = 0.f, ixy = 0.f, ixz = 0.f, iyz = 0.f;
        v3 h{0.f, 0.f, 0.f}, n{0.f, 0.f, 0.f}, fs{0.f, 0.f, 0.f};
        for (int b = j; b < NB; ++b) {  // DFS order: a subtree lies at and after its root
            if (!(sub >> b & 1u)) continue;
            const float* o = L.body[b];
            const v3 r = ld3(o + 1) - pj;
            if (!wrench) {
                const float m = o[0];
                ms += m;
                h = h + r * m;
                ixx += o[4] + m * (r.y * r.y + r.z * r.z);  // parallel axes: I_w + m (|r|^2 1 - r r^T)
                iyy += o[5] + m * (r.x * r.x + r.z * r.z);
                izz += o[6] + m * (r.x * r.x + r.y * r.y);
                ixy += o[7] - m * r.x * r.y;
                ixz += o[8] - m * r.x * r.z;
                iyz += o[9] - m * r.y * r.z;
            } else {
                const v3 f = ld3(o + 13);
                n = n + ld3(o + 10) + cross(r, f);
                fs = fs + f;
            }
        }
        float* o = L.comp[j];
        if (!wrench) {
            o[0] = ms;
            st3(o + 1, h);
            o[4] = ixx, o[5] = iyy, o[6] = izz, o[7] = ixy, o[8] = ixz, o[9] = iyz;
        } else {
            st3(o + 10, n);
            st3(o + 13, fs);
        }
    }
    __syncthreads();

    // F = I^c S about the column's own pivot, where S = (w, v) with v = e_c for a root linear column and 0
    // for every other (a joint's axis passes through its pivot); the RNEA force S . wrench^c
    for (int c = lane; c < NG; c += kWave) {
        const float* I = L.comp[col_joint(c)];
        const v3 w = ld3(L.SF[c]);
        const v3 v{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        const v3 h = ld3(I + 1);
        const v3 n{I[4] * w.x + I[7] * w.y + I[8] * w.z, I[7] * w.x + I[5] * w.y + I[9] * w.z,
                   I[8] * w.x + I[9] * w.y + I[6] * w.z};
        st3(L.SF[c] + 6, n + cross(h, v));         // angular momentum about the pivot
        st3(L.SF[c] + 9, v * I[0] + cross(w, h));  // linear momentum
        L.bias[c] = dot(w, ld3(I + 10)) + dot(v, ld3(I + 13));
    }
    __syncthreads();
}

// a column's motion vector as a lane holds it: the axis w, its pivot and the constant linear part v0
// (root linear columns: e_c), so that about any point x it is (w, v0 + w x (x - pivot))
struct ColS {
    v3 w, pv, v0;
};
__device__ __forceinline__ ColS load_S(const float* sf, int c) {
    const float4* q = reinterpret_cast<const float4*>(sf);  // 48-byte records, 16-byte aligned
    const float4 a = q[0], b = q[1];
    return ColS{v3{a.x, a.y, a.z}, v3{a.w, b.x, b.y}, v3{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f}};
}

// row I of H into the registers: lane j takes H[I][j] = S_j . F_I where dof j is on dof I's chain (the
// ancestor's S, the descendant's F), both about dof I's own pivot, so that the entry is exact to float32
// of the descendant's inertia; exact zero off the chain; the armature on the diagonal. F_I and its pivot
// are one LDS broadcast.
template <int I>
__device__ __forceinline__ void crba_row(regla::RegMat& H, const Lds& L, const ColS& s1, const ColS& s2, float arm1,
                                         float arm2, int lane) {
    const float4* q = reinterpret_cast<const float4*>(L.SF[I]);
    const float4 a = q[0], b = q[1], d = q[2];
    const v3 x{a.w, b.x, b.y}, Fn{b.z, b.w, d.x}, Fp{d.y, d.z, d.w};
    float v = dot6(s1.w, s1.v0 + cross(s1.w, x - s1.pv), Fn, Fp);
    if constexpr (I < kWave) v += lane == I ? arm1 : 0.f;
    v = regla::lanes<smpl::kAncLo[I]>() ? v : 0.f;
    asm volatile("" : "+v"(v));  // the entry is formed here: sunk to its first use, the row's F stays live instead
    regla::mc_set<I>(H, v);
    if constexpr (I >= kWave) {
        float v2 = dot6(s2.w, s2.v0 + cross(s2.w, x - s2.pv), Fn, Fp);
        v2 += lane == I - kWave ? arm2 : 0.f;
        v2 = regla::lanes<(uint64_t)smpl::kAncHi[I]>() ? v2 : 0.f;
        asm volatile("" : "+v"(v2));
        regla::mc2_set<I - kWave>(H, v2);
    }
    __builtin_amdgcn_sched_barrier(0);  // row by row: hoisting all 75 broadcasts costs 450 registers
}

__global__ __launch_bounds__(kWave, 2) void solve_kernel(const Params P) {
    __shared__ Lds L;
    __shared__ Factor Fc;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    const bool hi = lane < NH;

    for (int i = lane; i < smpl::kNpack + 4; i += kWave) Fc.Lp[i] = 0.f;
    for (int i = lane; i < NG; i += kWave) {
        Fc.pack_start[i] = (int16_t)smpl::kPackStart[i];
        Fc.dof_depth[i] = (int8_t)(smpl::kDofNanc[i] - 1);
    }
    columns<false>(L, M, P, env, lane);  // ends on a barrier

    const int dj = Fc.dof_depth[lane], dj2 = hi ? Fc.dof_depth[kWave + lane] : 0;
    float D1 = 1.f, D2 = 1.f;
    {
        regla::RegMat H;
        H.cp[(NG + 1) / 2 - 1] = regla::f2v{0.f, 0.f};  // the pairs' unused halves
        H.cp2[(NH + 1) / 2 - 1] = regla::f2v{0.f, 0.f};
        const bool arm = (P.flags & HS_FLAG_ARMATURE) != 0;
        const float arm1 = arm && lane >= 6 ? M.armature[lane >= 6 ? lane - 6 : 0] : 0.f;
        const float arm2 = arm && hi ? M.armature[hi ? kWave - 6 + lane : 0] : 0.f;
        const ColS s1 = load_S(L.SF[lane], lane);
        const ColS s2 = load_S(L.SF[hi ? kWave + lane : NG - 1], NG - 1);
        regla::static_for<0, NG, 1>([&](auto i) { crba_row<decltype(i)::value>(H, L, s1, s2, arm1, arm2, lane); });
        // the factorisation carries one right-hand side along; the solves below replay it from the
        // stored factor instead, so that every vector of a call takes the same instructions
        float z1 = 0.f, z2 = 0.f;
        regla::factor_pipelined(H, D1, D2, Fc.Lp, dj, dj2, z1, z2);
    }
    __syncthreads();
    const float dinv1 = 1.f / D1, dinv2 = 1.f / D2;
    const float* row1 = Fc.Lp + Fc.pack_start[lane];
    const float* row2 = Fc.Lp + Fc.pack_start[hi ? kWave + lane : 0];

    const int k = P.k > 0 ? P.k : 1;
    for (int j = 0; j < k; ++j) {  // wave-uniform trip count
        float y1, y2 = 0.f;
        if (P.k > 0) {
            const float* b = P.rhs + (env * k + j) * NG;
            y1 = b[lane];
            if (hi) y2 = b[kWave + lane];
        } else {
            const float* f = P.gen_force ? P.gen_force + env * NG : nullptr;
            y1 = (f ? f[lane] : 0.f) - L.bias[lane];
            if (hi) y2 = (f ? f[kWave + lane] : 0.f) - L.bias[kWave + lane];
        }
        regla::solve_LT_vec_pipelined(Fc.Lp, dj, dj2, y1, y2);
        y1 *= dinv1;
        y2 *= dinv2;
        regla::solve_L_streamed(row1, row2, y1, y2);
        float* o = P.out + (env * k + j) * NG;
        o[lane] = y1;
        if (hi) o[kWave + lane] = y2;
    }
}

__global__ __launch_bounds__(kWave) void torque_kernel(const Params P) {
    __shared__ Lds L;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    columns<true>(L, M, P, env, lane);  // L.bias = w, the RNEA force at qdd = (0; qdd_des); ends on a barrier

    // the base block of M: row i = (F_i's linear part, F_i's angular part) of root column i, the
    // composite inertia of the whole body about o. The same small solve in every lane.
    const float* f = P.gen_force ? P.gen_force + env * NG : nullptr;
    float A[6][6], y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const v3 n = ld3(L.SF[i] + 6), p = ld3(L.SF[i] + 9);
        A[i][0] = p.x, A[i][1] = p.y, A[i][2] = p.z, A[i][3] = n.x, A[i][4] = n.y, A[i][5] = n.z;
        y[i] = (f ? f[i] : 0.f) - L.bias[i];
    }
    // A = Lb D Lb^T in place (lower triangle), then the two substitutions
    float dinv[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float d = A[j][j];
#pragma unroll
        for (int s = 0; s < j; ++s) d -= A[j][s] * A[j][s] * A[s][s];
        A[j][j] = d;
        dinv[j] = 1.f / d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float v = A[i][j];
#pragma unroll
            for (int s = 0; s < j; ++s) v -= A[i][s] * A[j][s] * A[s][s];
            A[i][j] = v * dinv[j];
        }
    }
#pragma unroll
    for (int i = 1; i < 6; ++i)
#pragma unroll
        for (int s = 0; s < i; ++s) y[i] -= A[i][s] * y[s];
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] *= dinv[i];
#pragma unroll
    for (int i = 4; i >= 0; --i)
#pragma unroll
        for (int s = i + 1; s < 6; ++s) y[i] -= A[s][i] * y[s];

    if (P.base_acc && lane < 6) {
        float v = y[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) v = lane == i ? y[i] : v;
        P.base_acc[env * 6 + lane] = v;
    }
    if (P.out) {
        const bool arm = (P.flags & HS_FLAG_ARMATURE) != 0;
        const v3 al{y[0], y[1], y[2]}, aw{y[3], y[4], y[5]};
        for (int d = lane; d < ND; d += kWave) {
            const int c = 6 + d;
            float t = L.bias[c] - (f ? f[c] : 0.f);
            if (arm) t += M.armature[d] * L.qdd[d];
            // M_jb a_b = F_c . (a_b as a motion vector about the column's pivot: (aw, al + aw x pivot))
            t += dot(ld3(L.SF[c] + 9), al + cross(aw, ld3(L.SF[c] + 3))) + dot(ld3(L.SF[c] + 6), aw);
            P.out[env * ND + d] = t;
        }
    }
}

}  // namespace

struct hs_solver {
    int device = 0;
    int num_envs = 0;
    DeviceArray<TreeModel> d_model;
};

extern "C" {

const char* hs_last_error(void) { return last_error(); }
int hs_version(void) { return 1; }

int hs_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    if (check_tree_depth(model)) return 1;
    for (int b = 0; b < NB; ++b)  // the factorisation's register indices are this tree's
        if (model->parents[b] != smpl::kParentBody[b])
            return fail("model: body %d hangs on body %d; the factorisation is unrolled for a tree where it hangs on %d", b,
                        model->parents[b], smpl::kParentBody[b]);
    return 0;
}

int hs_create(int device, const he_model* model, const float gravity[3], int num_envs, hs_solver** out) {
    if (!out) return fail("hs_create: null output pointer");
    *out = nullptr;
    if (num_envs < 1) return fail("hs_create: num_envs %d < 1", num_envs);
    if (!gravity) return fail("hs_create: null gravity vector");
    if (hs_validate_model(model)) return 1;
    TreeModel dm;
    fill_tree_model(model, gravity, dm);
    if (select_device(device, "hs_create")) return 1;
    std::unique_ptr<hs_solver> h(new hs_solver);  // a failed step below frees it and its array
    h->device = device;
    h->num_envs = num_envs;
    HE_CHECK(h->d_model.assign(&dm, 1));
    *out = h.release();
    return 0;
}

int hs_destroy(hs_solver* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;
    return 0;
}

int hs_forward_dynamics(hs_solver* h, const float* root_state, const float* dof_state, const float* gen_force,
                        float* qdd_out, uint32_t flags, void* stream) {
    if (!h) return fail("hs_forward_dynamics: null handle");
    if (!root_state || !dof_state) return fail("hs_forward_dynamics: null state pointer");
    if (!qdd_out) return fail("hs_forward_dynamics: null output buffer");
    if (flags & ~HS_FLAGS_ALL) return fail("hs_forward_dynamics: unknown flag bits 0x%x", flags & ~HS_FLAGS_ALL);
    if (misaligned({root_state, dof_state, gen_force, qdd_out}))
        return fail("hs_forward_dynamics: every buffer must be 4-byte aligned");
    Params P{};
    P.model = h->d_model;
    P.root = root_state;
    P.dof = dof_state;
    P.gen_force = gen_force;
    P.out = qdd_out;
    P.k = 0;
    P.flags = flags;
    hipLaunchKernelGGL(solve_kernel, dim3(h->num_envs), dim3(kWave), 0, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

int hs_computed_torque(hs_solver* h, const float* root_state, const float* dof_state, const float* qdd_des,
                       const float* gen_force, float* tau_out, float* base_acc_out, uint32_t flags, void* stream) {
    if (!h) return fail("hs_computed_torque: null handle");
    if (!root_state || !dof_state) return fail("hs_computed_torque: null state pointer");
    if (!qdd_des) return fail("hs_computed_torque: null desired acceleration");
    if (!tau_out && !base_acc_out) return fail("hs_computed_torque: no output buffer");
    if (flags & ~HS_FLAGS_ALL) return fail("hs_computed_torque: unknown flag bits 0x%x", flags & ~HS_FLAGS_ALL);
    if (misaligned({root_state, dof_state, qdd_des, gen_force, tau_out, base_acc_out}))
        return fail("hs_computed_torque: every buffer must be 4-byte aligned");
    Params P{};
    P.model = h->d_model;
    P.root = root_state;
    P.dof = dof_state;
    P.qdd_des = qdd_des;
    P.gen_force = gen_force;
    P.out = tau_out;
    P.base_acc = base_acc_out;
    P.flags = flags;
    hipLaunchKernelGGL(torque_kernel, dim3(h->num_envs), dim3(kWave), 0, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

int hs_solve(hs_solver* h, const float* root_state, const float* dof_state, const float* rhs, float* out, int k,
             uint32_t flags, void* stream) {
    if (!h) return fail("hs_solve: null handle");
    if (!root_state || !dof_state) return fail("hs_solve: null state pointer");
    if (!rhs) return fail("hs_solve: null right-hand side");
    if (!out) return fail("hs_solve: null output buffer");
    if (rhs == out) return fail("hs_solve: rhs and out are the same buffer (the solve is not in place)");
    if (k < 1 || k > HS_MAX_RHS) return fail("hs_solve: k = %d outside 1..%d", k, HS_MAX_RHS);
    if (flags & ~HS_FLAGS_ALL) return fail("hs_solve: unknown flag bits 0x%x", flags & ~HS_FLAGS_ALL);
    if (misaligned({root_state, dof_state, rhs, out})) return fail("hs_solve: every buffer must be 4-byte aligned");
    Params P{};
    P.model = h->d_model;
    P.root = root_state;
    P.dof = dof_state;
    P.rhs = rhs;
    P.out = out;
    P.k = k;
    P.flags = flags;
    hipLaunchKernelGGL(solve_kernel, dim3(h->num_envs), dim3(kWave), 0, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
