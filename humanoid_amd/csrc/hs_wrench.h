// hs_wrench.h -- the joint-reaction queries (include/humanoid_wrench.h, the hw_ entry points): the device
// code that extends hs_solve.hip's torque_kernel at run time. columns<true>() leaves in L.comp[j] every
// subtree's composite inertia (0..9) and Newton-Euler wrench at a_b = 0 (10..15), both about the joint's
// OWN origin p_j, and in L.A / L.Wd the bodies' accelerations at a_b = 0. What is here
//   reaction_external  subtracts the external wrenches' subtree sums E_j from L.comp[j]'s wrench and forms
//                      the RNEA force L.bias again from it, so that everything after it (the base solve,
//                      the tau loop, the wrenches) sees the external wrench without a term of its own;
//   reaction_outputs   W_j = wrench_j + I^c_j a_b referred to p_j, the bodies' accelerations at the base
//                      acceleration a_b, both staged in LDS and written as contiguous dwords.
// A wrench never leaves its own joint origin: a hand's is exact to float32 of the hand (columns()), and a
// root 1 km from the world origin changes nothing, since every lever is relative to the root origin o.
// Every branch on a Params pointer is wave-uniform. hs_computed_torque leaves the pointers null and calls
// neither function.
#pragma once
#include "../../include/humanoid_wrench.h"
#include "he_joint_space.h"

namespace {

constexpr int kReactRow = 6;                 // force 3 + torque 3; origin acceleration 3 + angular 3
constexpr int kReactEnv = NB * kReactRow;    // 144 floats per env and output
static_assert(2 * kReactEnv <= NB * 16, "the two outputs are staged in L.body");

// External wrenches (P.body_force, P.body_torque [N*24,3], world axes, the force at the centre of mass;
// either may be null): L.comp[j][10..15] -= E_j with
//   E_j = (sum t_b + (c_b - p_j) x f_b, sum f_b) over sub(j),
// then L.bias = S . wrench^c from the corrected wrench. Stages (t_b, f_b) in L.body[b][10..15], whose
// Newton-Euler wrench is dead once columns() has summed it. Ends on a barrier.
template <class Params>
__device__ __forceinline__ void reaction_external(Lds& L, const TreeModel& M, const Params& P, size_t env, int lane) {
    if (lane < NB) {
        const size_t row = (env * NB + lane) * 3;
        const v3 z{0.f, 0.f, 0.f};
        st3(L.body[lane] + 10, P.body_torque ? ld3(P.body_torque + row) : z);
        st3(L.body[lane] + 13, P.body_force ? ld3(P.body_force + row) : z);
    }
    __syncthreads();
    if (lane < NB) {
        const int j = lane;
        const v3 pj = ld3(L.P[j]);
        const uint32_t sub = M.sub[j];
        v3 n{0.f, 0.f, 0.f}, fs{0.f, 0.f, 0.f};
        for (int b = j; b < NB; ++b) {  // DFS order: a subtree lies at and after its root
            if (!(sub >> b & 1u)) continue;
            const float* o = L.body[b];
            const v3 f = ld3(o + 13);
            n = n + ld3(o + 10) + cross(ld3(o + 1) - pj, f);
            fs = fs + f;
        }
        float* o = L.comp[j];
        st3(o + 10, ld3(o + 10) - n);
        st3(o + 13, ld3(o + 13) - fs);
    }
    __syncthreads();
    for (int c = lane; c < NG; c += kWave) {
        const float* I = L.comp[col_joint(c)];
        const v3 v{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        L.bias[c] = dot(ld3(L.SF[c]), ld3(I + 10)) + dot(v, ld3(I + 13));
    }
    __syncthreads();
}

// P.wrench [N,24,6] and P.body_acc [N,24,6] at the base acceleration (al, aw), either may be null.
// With al_j = al + aw x (p_j - o) the origin acceleration of joint j that the base's adds, subtree j takes
// the force m_s al_j + aw x h and the torque I^c aw + h x al_j about p_j on top of its wrench at a_b = 0.
// L.body is dead by now (its last reader is reaction_external, which ends on a barrier) and stages the
// 144 + 144 floats, so that the stores are contiguous dwords and not 6-float rows from 24 lanes.
template <class Params>
__device__ __forceinline__ void reaction_outputs(Lds& L, const Params& P, size_t env, int lane, v3 al, v3 aw) {
    float* stage = &L.body[0][0];
    if (lane < NB) {
        const int j = lane;
        const v3 pj = ld3(L.P[j]);
        const v3 alj = al + cross(aw, pj);
        if (P.wrench) {
            const float* I = L.comp[j];
            const v3 h = ld3(I + 1);
            const v3 Iaw{I[4] * aw.x + I[7] * aw.y + I[8] * aw.z, I[7] * aw.x + I[5] * aw.y + I[9] * aw.z,
                         I[8] * aw.x + I[9] * aw.y + I[6] * aw.z};
            v3 F = ld3(I + 13) + alj * I[0] + cross(aw, h);
            v3 Nq = ld3(I + 10) + Iaw + cross(h, alj);
            if (P.frame == HW_FRAME_BODY) {  // R_j^T: the columns of the row-major R_j
                const float* R = L.R[j];
                const v3 c0{R[0], R[3], R[6]}, c1{R[1], R[4], R[7]}, c2{R[2], R[5], R[8]};
                F = v3{dot(c0, F), dot(c1, F), dot(c2, F)};
                Nq = v3{dot(c0, Nq), dot(c1, Nq), dot(c2, Nq)};
            }
            st3(stage + j * kReactRow, F);
            st3(stage + j * kReactRow + 3, Nq);
        }
        if (P.body_acc) {
            st3(stage + kReactEnv + j * kReactRow, ld3(L.A[j]) + alj);
            st3(stage + kReactEnv + j * kReactRow + 3, ld3(L.Wd[j]) + aw);
        }
    }
    __syncthreads();
    if (P.wrench)
        for (int i = lane; i < kReactEnv; i += kWave) P.wrench[env * kReactEnv + i] = stage[i];
    if (P.body_acc)
        for (int i = lane; i < kReactEnv; i += kWave) P.body_acc[env * kReactEnv + i] = stage[kReactEnv + i];
}

}  // namespace
