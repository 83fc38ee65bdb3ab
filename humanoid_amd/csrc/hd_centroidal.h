// hd_centroidal.h -- the centroidal queries of libhumanoid_dynamics.so (include/humanoid_centroidal.h, the
// hc_ entry points): centre of mass, momentum, the centroidal momentum matrix A_G, its rate term and the
// energies of every env. hd_dynamics.hip includes this file last: one translation unit, one library, two
// public headers. dynamics_kernel is not touched (its Newton-Euler lines stay inline there, and are
// restated here: moved into a shared function they round differently in that kernel).
// One launch, one 64-lane wave (= one block) per env:
//   kinematics he_tree_state.h's tree_kinematics<false>, origins relative to the root origin o = p_0;
//   bodies     lanes 0..23: the body's spatial inertia about o (m, m c, I_o), its Newton-Euler wrench
//              about o at qdd = 0 without gravity, and its momentum about o and kinetic energy, from the
//              body's own velocity (the root's plus w_a x (p_k - p_a) up the chain: no further pass);
//   subtrees   composite inertias and wrenches (24 x 16 items over the subtree masks), and the 7 sums
//              over all bodies (P, L_o, kinetic) in body order, accumulated in double and rounded once;
//   columns    lane = column (lanes 0..63, then the 11-column tail in lanes 0..10): S = (w, v_o) and
//              F = I^c S = (n_o, p) in registers, shifted from o to the centre of mass with
//              r = h_root / m: n_G = n_o - r x p; six row stores of 64 + 11 consecutive dwords;
//   root       com = p_0 + r (the one place the world position enters), com_vel = P / m,
//              L_G = L_o - r x P, cmm_bias = (f, n_o - r x f) of the root's composite wrench, the energies.
// Everything but the column stage is computed in every launch, and every store sits behind a
// wave-uniform branch on its pointer, so an output's bits do not depend on which others are asked for.
#pragma once
#include "../../include/humanoid_centroidal.h"
#include "he_host.h"
#include "he_tree_state.h"

namespace {

constexpr int kCmmEnv = HC_MOMENTUM_ROWS * NG;  // 450 dwords per env
constexpr int kBodyWords = 24;  // m, h3, I_o 6, wrench (n3, f3), then P3, L_o 3, kinetic, one unused
constexpr int kTotals = 7;      // P, L_o, kinetic over all bodies

struct CentroidalParams {
    const TreeModel* model;
    const float* root;  // [N,13]
    const float* dof;   // [N*69,2]
    hc_outputs out;
};

// dynamics_kernel's occupancy: 4 waves per SIMD is what a grid of 4096 envs fills
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4, 4))) void centroidal_kernel(
    const CentroidalParams P) {
    __shared__ float sQ[ND], sU[ND], sR[NB][9], sP[NB][3], sW[NB][3], sWd[NB][3], sA[NB][3];
    __shared__ float sBody[NB][kBodyWords];
    __shared__ float sComp[NB][16];  // m, h3, I_o, wrench summed over the body's subtree
    __shared__ float sTot[8];

    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    const TreeState S{sQ, sU, nullptr, sR, sP, sW, sWd, sA};
    const float* root = P.root + env * 13;

    tree_kinematics<false>(S, P.model, P.root, P.dof, nullptr, env, lane);  // ends on a barrier

    if (lane < NB) {
        const int b = lane;
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
        // Newton-Euler at qdd = 0, no gravity: f = m a_c, t_c = I_w wd + w x I_w w, about o: n = t_c + c x f
        const m3 Iw{B.wxx, B.wxy, B.wxz, B.wxy, B.wyy, B.wyz, B.wxz, B.wyz, B.wzz};
        const v3 w = ld3(sW[b]), wd = ld3(sWd[b]);
        const v3 ac = ld3(sA[b]) + cross(wd, B.rc) + cross(w, cross(w, B.rc));
        const v3 f = ac * m;
        const v3 Iww = mul(Iw, w);
        st3(o + 10, mul(Iw, wd) + cross(w, Iww) + cross(c, f));
        st3(o + 13, f);
        // the body's own velocity: the root origin's, plus w_a x (p_k - p_a) up the chain (at most 8 joints)
        v3 v = ld3(root + 7);
        for (int k = b; k != 0;) {
            const int a = M.parent[k];
            v = v + cross(ld3(sW[a]), ld3(sP[k]) - ld3(sP[a]));
            k = a;
        }
        const v3 vc = v + cross(w, B.rc);
        const v3 p = vc * m;
        st3(o + 16, p);
        st3(o + 19, cross(c, p) + Iww);  // angular momentum about o
        o[22] = 0.5f * (m * dot(vc, vc) + dot(w, Iww));
    }
    __syncthreads();

    // subtree sums (24 x 16 items), then the 7 sums over all bodies, each in body order
    for (int it = lane; it < NB * 16 + kTotals; it += kWave) {
        float s = 0.f;
        if (it < NB * 16) {
            const int j = it >> 4, k = it & 15;
            const uint32_t sub = M.sub[j];
            for (int b = j; b < NB; ++b)  // DFS order: a subtree lies at and after its root
                if (sub >> b & 1u) s += sBody[b][k];
            sComp[j][k] = s;
        } else {
            // in double, rounded once: 24 float32 additions of like-signed terms (the kinetic energy) cost
            // 2 to 3 ulp of the sum, which is more than the float32 reference of the tests loses
            const int k = it - NB * 16;
            double t = 0.0;
            for (int b = 0; b < NB; ++b) t += static_cast<double>(sBody[b][16 + k]);
            sTot[k] = static_cast<float>(t);
        }
    }
    __syncthreads();

    // the root's composite: total mass, r = com - o (the same in every lane)
    const float* I0 = sComp[0];
    const float m = I0[0];
    const float inv_m = 1.f / m;
    const v3 r = ld3(I0 + 1) * inv_m;

    if (P.out.cmm) {
        float* out = P.out.cmm + env * kCmmEnv;
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            const int c = lane + slot * kWave;
            if (c < NG) {
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
                const float* I = sComp[col_joint(c)];
                const v3 h = ld3(I + 1);
                const v3 n{I[4] * w.x + I[7] * w.y + I[8] * w.z, I[7] * w.x + I[5] * w.y + I[9] * w.z,
                           I[8] * w.x + I[9] * w.y + I[6] * w.z};
                const v3 p = v * I[0] + cross(w, h);  // linear momentum per unit rate
                v3 nG = n + cross(h, v) - cross(r, p);  // angular momentum about the centre of mass
                // a translation of the whole body carries no angular momentum about its centre of mass:
                // h x e_i - r x (m e_i) is zero by r = h / m, and is written as the zero it is
                if (c < 3) nG = v3{0.f, 0.f, 0.f};
                float* col = out + c;
                col[0] = p.x, col[NG] = p.y, col[2 * NG] = p.z;
                col[3 * NG] = nG.x, col[4 * NG] = nG.y, col[5 * NG] = nG.z;
            }
        }
    }

    if (lane == 0) {
        const v3 Pl = ld3(sTot), Lo = ld3(sTot + 3);
        const v3 com = ld3(root) + r;
        if (P.out.com) st3(P.out.com + env * 3, com);
        if (P.out.com_vel) st3(P.out.com_vel + env * 3, Pl * inv_m);
        if (P.out.momentum) {
            st3(P.out.momentum + env * 6, Pl);
            st3(P.out.momentum + env * 6 + 3, Lo - cross(r, Pl));
        }
        if (P.out.cmm_bias) {
            const v3 n = ld3(I0 + 10), f = ld3(I0 + 13);
            st3(P.out.cmm_bias + env * 6, f);
            st3(P.out.cmm_bias + env * 6 + 3, n - cross(r, f));
        }
        if (P.out.energy) {
            P.out.energy[env * 2] = sTot[6];
            P.out.energy[env * 2 + 1] = -m * dot(ld3(M.gravity), com);
        }
    }
}

}  // namespace

struct hc_centroidal : QueryHandle<TreeModel> {};

extern "C" {

// the translation unit has one error text: hc_last_error and hd_last_error read the same one
const char* hc_last_error(void) { return last_error(); }
int hc_version(void) { return 1; }

int hc_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    return check_tree_depth(model);
}

int hc_create(int device, const he_model* model, const float gravity[3], int num_envs, hc_centroidal** out) {
    return query_create("hc_create", device, model, gravity, num_envs, out, hc_validate_model, fill_tree_model);
}

int hc_destroy(hc_centroidal* h) { return query_destroy(h); }

int hc_compute(hc_centroidal* h, const float* root_state, const float* dof_state, const hc_outputs* out, void* stream) {
    if (check_call("hc_compute", h, root_state, dof_state)) return 1;
    if (!out) return fail("hc_compute: null output struct");
    if (!out->com && !out->com_vel && !out->momentum && !out->cmm && !out->cmm_bias && !out->energy)
        return fail("hc_compute: no output buffer");
    if (check_aligned("hc_compute", {root_state, dof_state, out->com, out->com_vel, out->momentum, out->cmm,
                                     out->cmm_bias, out->energy}))
        return 1;
    CentroidalParams P{};
    P.model = h->d_model;
    P.root = root_state;
    P.dof = dof_state;
    P.out = *out;
    hipLaunchKernelGGL(centroidal_kernel, dim3(h->num_envs), dim3(kWave), 0, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
