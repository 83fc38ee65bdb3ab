// hs_derivs.h -- the dynamics derivatives (include/humanoid_derivatives.h, the hg_ entry points): the
// device code that extends hs_solve.hip's torque_kernel at run time, as hs_wrench.h does. One env per
// wave; a lane owns one DIRECTION j (a column of the two matrices), in two passes: 64 directions, then 11.
//
// The derivative is the exact one, by tangent propagation. Direction j belongs to joint k = col_joint(j)
// with the world axis ax = R_k e_i through p_k (a root angular direction: e_i through o). Only the bodies
// of sub(k) move, and their tangents have closed forms in the body's own state and that of k's carrier
// (k's parent; for the root its own world rates and accelerations, which the definition holds):
//   pose direction      sub(k) turns rigidly about p_k at rate ax while the carrier keeps its motion.
//                       With rho = w_b - w_a, r = p_b - p_k, vrel and arel the origin's velocity and
//                       acceleration relative to the carrier's frame (both turn with the subtree),
//                         dw = ax x rho,  dwd = w_a x dw + ax x (wd_b - wd_a - w_a x rho),
//                         dA = wd_a x (ax x r) + w_a x (w_a x (ax x r)) + 2 w_a x (ax x vrel) + ax x arel,
//                       and the geometry (R com, I_w, the levers, the row axes of sub(k)) turns at ax;
//   velocity direction  sub(k) gains the angular velocity ax on a fixed geometry:
//                         dw = ax,  dwd = w_a x ax + ax x (w_b - w_k),
//                         dA = (w_a x ax - ax x w_k) x r + 2 ax x (V_b - V_k).
// From (dw, dwd, dA) the tangent of the body's Newton-Euler wrench; the bodies go deepest first (DFS order
// backwards), each adds its subtree's tangent wrench about its own origin to its parent's, and row i of
// joint m is S_i . dW_m (+ (ax x S_i) . N_m under a pose direction) inside sub(k), S_i . (dW_k carried to
// p_m) for the ancestors of k, and exactly zero elsewhere: never computed, written as 0.
// Per lane the subtrees' tangent wrenches live in dynamic LDS ([24][6][64] floats, kDerivLds bytes, which
// only hg_compute's launch asks for); everything about a body is an LDS broadcast. A lane touches only its
// own column of that block, so the passes need no barrier.
// Every branch on a Params pointer is wave-uniform. The other entries leave the pointers null.
#pragma once
#include "../../include/humanoid_derivatives.h"
#include "he_joint_space.h"

namespace {

constexpr int kDerivRow = 6;                                          // dN 3, dF 3
constexpr size_t kDerivLds = size_t(NB) * kDerivRow * kWave * sizeof(float);  // 36 KB, dynamic

__device__ __forceinline__ v3 mulsym(const float* o, v3 v) {  // I_w (xx yy zz xy xz yz at o[4..9]) v
    return v3{o[4] * v.x + o[7] * v.y + o[8] * v.z, o[7] * v.x + o[5] * v.y + o[9] * v.z,
              o[8] * v.x + o[9] * v.y + o[6] * v.z};
}
__device__ __forceinline__ v3 rcol(const float* R, int i) { return v3{R[i], R[3 + i], R[6 + i]}; }

// The state with the whole generalised acceleration (P.acc [N,75] or null = 0): L.R, L.P, L.W by
// tree_kinematics, then by tree level L.Wd, L.A with the base and joint accelerations and the origins'
// velocities relative to the root origin's in L.comp[b][0..2]; the bodies' Newton-Euler wrenches in
// L.body and their subtree sums about each joint's own origin in L.comp[j][10..15], as columns() leaves
// them. Ends on a barrier.
template <class Params>
__device__ __forceinline__ void derivative_state(Lds& L, const TreeModel& M, const Params& P, size_t env, int lane) {
    const float* acc = P.acc ? P.acc + env * NG : nullptr;
    for (int d = lane; d < ND; d += kWave) L.qdd[d] = acc ? acc[6 + d] : 0.f;
    const TreeState S{L.q, L.u, L.qdd, L.R, L.P, L.W, L.Wd, L.A};
    tree_kinematics<false>(S, &M, P.root, P.dof, nullptr, env, lane);  // ends on a barrier

    int depth = -1, parent = 0;
    if (lane < NB) {
        depth = M.depth[lane];
        parent = M.parent[lane];
        if (lane == 0) {
            const v3 z{0.f, 0.f, 0.f};
            st3(L.A[0], acc ? ld3(acc) : z);
            st3(L.Wd[0], acc ? ld3(acc + 3) : z);
            st3(L.comp[0], z);
        }
    }
    __syncthreads();
    const int levels = M.max_depth;
    for (int lvl = 1; lvl <= levels; ++lvl) {
        if (depth == lvl) {
            const int b = lane, a = parent;
            const m3 Rb = ldm(L.R[b]);
            const v3 wa = ld3(L.W[a]), wda = ld3(L.Wd[a]);
            const v3 d = ld3(L.P[b]) - ld3(L.P[a]);
            const v3 wrel = mul(Rb, ld3(&L.u[3 * (b - 1)]));
            const v3 wad = cross(wa, d);
            st3(L.Wd[b], wda + cross(wa, wrel) + mul(Rb, ld3(&L.qdd[3 * (b - 1)])));
            st3(L.A[b], ld3(L.A[a]) + cross(wda, d) + cross(wa, wad));
            st3(L.comp[b], ld3(L.comp[a]) + wad);
        }
        __syncthreads();
    }

    if (lane < NB) {  // the body about its own centre of mass (columns()' lines, at the full acceleration)
        const int b = lane;
        const m3 R = ldm(L.R[b]);
        const float m = M.mass[b];
        const v3 rc = mul(R, ld3(M.com[b]));
        const float* ib = M.inertia[b];
        const m3 I{ib[0], ib[3], ib[4], ib[3], ib[1], ib[5], ib[4], ib[5], ib[2]};
        const m3 RI = mul(R, I);
        float* o = L.body[b];
        o[0] = m;
        st3(o + 1, ld3(L.P[b]) + rc);
        o[4] = RI.a00 * R.a00 + RI.a01 * R.a01 + RI.a02 * R.a02;
        o[5] = RI.a10 * R.a10 + RI.a11 * R.a11 + RI.a12 * R.a12;
        o[6] = RI.a20 * R.a20 + RI.a21 * R.a21 + RI.a22 * R.a22;
        o[7] = RI.a00 * R.a10 + RI.a01 * R.a11 + RI.a02 * R.a12;
        o[8] = RI.a00 * R.a20 + RI.a01 * R.a21 + RI.a02 * R.a22;
        o[9] = RI.a10 * R.a20 + RI.a11 * R.a21 + RI.a12 * R.a22;
        const v3 w = ld3(L.W[b]), wd = ld3(L.Wd[b]);
        const v3 ac = ld3(L.A[b]) + cross(wd, rc) + cross(w, cross(w, rc));
        const v3 g = (P.flags & kFlagNoGravity) ? v3{0.f, 0.f, 0.f} : ld3(M.gravity);
        st3(o + 10, mulsym(o, wd) + cross(w, mulsym(o, w)));
        st3(o + 13, (ac - g) * m);
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
        st3(L.comp[j] + 10, n);
        st3(L.comp[j] + 13, fs);
    }
    __syncthreads();
}

// tau [N,75] = M a + c: the base rows are the whole body's wrench about o, a joint's rows its axes on its
// subtree's torque about its own origin, the armature on top under the flag.
template <class Params>
__device__ __forceinline__ void derivative_tau(const Lds& L, const TreeModel& M, const Params& P, size_t env, int lane) {
    const bool arm = (P.flags & HG_FLAG_ARMATURE) != 0;
    for (int c = lane; c < NG; c += kWave) {
        const int j = col_joint(c);
        const float* I = L.comp[j];
        float t;
        if (c < 3) {
            t = I[13 + c];
        } else if (c < 6) {
            t = I[10 + c - 3];
        } else {
            t = dot(rcol(L.R[j], (c - 6) % 3), ld3(I + 10));
            if (arm) t += M.armature[c - 6] * L.qdd[c - 6];
        }
        P.tau_full[env * NG + c] = t;
    }
}

// One matrix, one pass of lanes: lane's direction is j (j >= NG: no direction, nothing written).
// out[e][i][j], or out[e][j][i] when by_direction. D: the wave's dynamic LDS.
template <bool VELOCITY>
__device__ __forceinline__ void derivative_pass(const Lds& L, const TreeModel& M, float* D, float* out, bool by_direction,
                                                size_t env, int lane, int j) {
    const bool writes = j < NG;
    const bool live = writes && j >= 3;  // a root linear direction changes nothing: gravity is uniform
    const int k = live ? col_joint(j) : 0;
    const uint32_t kmask = M.sub[k], amask = M.anc[k];
    const int ca = k ? M.parent[k] : 0;
    v3 ax{j == 3 ? 1.f : 0.f, j == 4 ? 1.f : 0.f, j == 5 ? 1.f : 0.f};
    if (k) ax = rcol(L.R[k], (j - 6) % 3);
    const v3 z{0.f, 0.f, 0.f};
    // the carrier's rates; a velocity direction of the root has none
    const v3 wa = (VELOCITY && !k) ? z : ld3(L.W[ca]);
    const v3 wda = ld3(L.Wd[ca]);
    const v3 pk = ld3(L.P[k]), wk = ld3(L.W[k]), Ak = ld3(L.A[k]), Vk = ld3(L.comp[k]);

    float* Dl = D + lane;
    for (int i = 0; i < NB * kDerivRow; ++i) Dl[i * kWave] = 0.f;
    v3 kN = z, kF = z;  // subtree k's tangent wrench about p_k, once body k is through

    const size_t base = env * NG * NG;
    const size_t si = by_direction ? 1 : NG, sj = by_direction ? NG : 1;
    for (int b = NB - 1; b >= 0; --b) {  // wave-uniform: body b's state is a broadcast
        v3 r0 = z, r1 = z;  // the rows of joint b: r0 (and r1 for the root's angular rows)
        const float* Rb = L.R[b];
        if (live && (kmask >> b & 1u)) {
            const float* o = L.body[b];
            const v3 pb = ld3(L.P[b]), wb = ld3(L.W[b]), wdb = ld3(L.Wd[b]);
            const v3 rc = ld3(o + 1) - pb, rr = pb - pk;
            const v3 Vb = ld3(L.comp[b]);
            v3 dw, dwd, dA;
            if (!VELOCITY) {
                const v3 rho = wb - wa;
                const v3 vrel = Vb - Vk - cross(wa, rr);
                const v3 arel = ld3(L.A[b]) - Ak - cross(wda, rr) - cross(wa, cross(wa, rr)) - cross(wa, vrel) * 2.f;
                const v3 wr = cross(ax, rr);
                dw = cross(ax, rho);
                dwd = cross(wa, dw) + cross(ax, wdb - wda - cross(wa, rho));
                dA = cross(wda, wr) + cross(wa, cross(wa, wr)) + cross(wa, cross(ax, vrel)) * 2.f + cross(ax, arel);
            } else {
                dw = ax;
                dwd = cross(wa, ax) + cross(ax, wb - wk);
                dA = cross(cross(wa, ax) - cross(ax, wk), rr) + cross(ax, Vb - Vk) * 2.f;
            }
            // the body's own wrench tangent, about its origin
            const v3 Iww = mulsym(o, wb);
            v3 dac = dA + cross(dwd, rc) + cross(dw, cross(wb, rc)) + cross(wb, cross(dw, rc));
            v3 dt = mulsym(o, dwd) + cross(dw, Iww) + cross(wb, mulsym(o, dw));
            v3 own = z;  // what the turning geometry adds to the torque about the origin
            if (!VELOCITY) {
                const v3 drc = cross(ax, rc);
                dac = dac + cross(wdb, drc) + cross(wb, cross(wb, drc));
                dt = dt + cross(ax, mulsym(o, wdb)) - mulsym(o, cross(ax, wdb)) +
                     cross(wb, cross(ax, Iww) - mulsym(o, cross(ax, wb)));
                own = cross(drc, ld3(o + 13));
            }
            const v3 df = dac * o[0];
            float* Db = Dl + b * kDerivRow * kWave;
            const v3 dN = v3{Db[0], Db[kWave], Db[2 * kWave]} + dt + own + cross(rc, df);
            const v3 dF = v3{Db[3 * kWave], Db[4 * kWave], Db[5 * kWave]} + df;
            if (b != k) {  // to the parent's origin; the lever turns with the subtree
                const int a = M.parent[b];
                const v3 lever = pb - ld3(L.P[a]);
                v3 up = dN + cross(lever, dF);
                if (!VELOCITY) up = up + cross(cross(ax, lever), ld3(L.comp[b] + 13));
                float* Da = Dl + a * kDerivRow * kWave;
                Da[0] += up.x, Da[kWave] += up.y, Da[2 * kWave] += up.z;
                Da[3 * kWave] += dF.x, Da[4 * kWave] += dF.y, Da[5 * kWave] += dF.z;
            } else {
                kN = dN, kF = dF;
            }
            if (b == 0) {
                r0 = dF, r1 = dN;
            } else {  // the row axes turn with the subtree
                const v3 s0 = rcol(Rb, 0), s1 = rcol(Rb, 1), s2 = rcol(Rb, 2);
                r0 = v3{dot(s0, dN), dot(s1, dN), dot(s2, dN)};
                if (!VELOCITY) {
                    const v3 Nb = ld3(L.comp[b] + 10);
                    r0 = r0 + v3{dot(cross(ax, s0), Nb), dot(cross(ax, s1), Nb), dot(cross(ax, s2), Nb)};
                }
            }
        } else if (live && b != k && (amask >> b & 1u)) {  // an ancestor of k: the geometry above k stands
            const v3 X = kN + cross(pk - ld3(L.P[b]), kF);
            if (b == 0)
                r0 = kF, r1 = X;
            else
                r0 = v3{dot(rcol(Rb, 0), X), dot(rcol(Rb, 1), X), dot(rcol(Rb, 2), X)};
        }
        if (writes) {
            float* o = out + base + size_t(j) * sj;
            if (b == 0) {
                o[0 * si] = r0.x, o[1 * si] = r0.y, o[2 * si] = r0.z;
                o[3 * si] = r1.x, o[4 * si] = r1.y, o[5 * si] = r1.z;
            } else {
                const size_t i = 6 + 3 * (b - 1);
                o[i * si] = r0.x, o[(i + 1) * si] = r0.y, o[(i + 2) * si] = r0.z;
            }
        }
    }
}

// hg_compute's body of torque_kernel
template <class Params>
__device__ __forceinline__ void derivatives(Lds& L, const TreeModel& M, const Params& P, float* D, size_t env, int lane) {
    derivative_state(L, M, P, env, lane);
    if (P.tau_full) derivative_tau(L, M, P, env, lane);
    const bool by_direction = (P.flags & HG_FLAG_BY_DIRECTION) != 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int j = pass * kWave + lane;
        if (P.dtau_dq) derivative_pass<false>(L, M, D, P.dtau_dq, by_direction, env, lane, j);
        if (P.dtau_dv) derivative_pass<true>(L, M, D, P.dtau_dv, by_direction, env, lane, j);
    }
}

}  // namespace
