// he_joint_space.h -- from an env's state to the columns of its joint-space inertia: what the two
// libraries that factor M in registers (hs_solve.hip, ht_task.hip) share. One env's working set in LDS,
// per column the motion axis S and the force F = I^c S (columns()), and the row of H = S . F a lane takes
// into regla::RegMat (crba_row). Spatial quantities of a subtree are referred to its own joint origin,
// never to a common far point: an entry of M is then exact to float32 of the descendant's own inertia.
// Nothing of the engine includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "he_regla.h"
#include "he_tree_state.h"

// internal linkage, as he_tree_state.h: each library carries its own copy
namespace {

constexpr int NH = NG - kWave;  // the 11-column tail: second register set of lanes 0..10
static_assert(NB == smpl::kNB && NG == smpl::kNG, "he_regla.h is unrolled for this tree");
// bit 1 of every library's flags (HD_ / HS_ / HT_FLAG_NO_GRAVITY): the bias force without gravity
constexpr uint32_t kFlagNoGravity = 2u;

// one env's working set (9.8 KB of LDS; the kernels that factor M add the factor's 5.3 KB)
struct Lds {
    float q[ND], u[ND], qdd[ND], R[NB][9], P[NB][3], W[NB][3], Wd[NB][3], A[NB][3];  // what TreeState views
    float body[NB][16];           // m, centre of mass c3 (relative to o), I_w about it (xx yy zz xy xz yz), t_c3, f3
    float comp[NB][16];           // subtree j about its joint origin p_j: m, first moment h3, inertia 6, wrench (n3, f3)
    alignas(16) float SF[NG][12];  // per column: axis w, pivot (relative to o), then F = I^c S about the pivot (n, p)
    float bias[NG];                // S . wrench^c: c, or the RNEA force at (0; qdd_des)
};
// the factor of the kernels that factor M
struct Factor {
    alignas(16) float Lp[smpl::kNpack + 4];  // packed unit-lower factor (he_regla.h: row K at kPackStart[K])
    int16_t pack_start[NG];
    int8_t dof_depth[NG];
};

// state -> S, F per column and the RNEA force per column. Params: the kernel's own argument block, of
// which root [N,13], dof [N*69,2], qdd_des [N,69] (read when QDD) and flags are read. QDD: the joints'
// accelerations P.qdd_des enter the bodies' accelerations (tree_kinematics). Without QDD, L.qdd is neither
// read nor written here or in tree_kinematics: ht_task.hip's inverse kinematics keeps the root's world
// position in L.qdd[0..2] across the call, so a change that touches L.qdd under !QDD has to move that.
template <bool QDD, class Params>
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
        const v3 g = (P.flags & kFlagNoGravity) ? v3{0.f, 0.f, 0.f} : ld3(M.gravity);
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

// the factorisation's own demand on a model that passed check_tree_depth: its register indices are this tree's
int check_factored_tree(const he_model* model) {
    for (int b = 0; b < NB; ++b)
        if (model->parents[b] != smpl::kParentBody[b])
            return fail("model: body %d hangs on body %d; the factorisation is unrolled for a tree where it hangs on %d", b,
                        model->parents[b], smpl::kParentBody[b]);
    return 0;
}

}  // namespace
