// he_phys_tree.h -- the phases that walk the body tree: the subtree sums by body levels (pick_body,
// subtree_level_flat, subtree_levels), the pointer-jumping tables and prefix (JumpTable, Jump4,
// jump_of, chain_prefix6), the kinematics, the joint-angle limits (angle_row, limit_clamp,
// limit_detect) and the integration (integrate_bodies).
// LDS: kinematics reads root_q, u0, q or qloc, T and writes qloc, qw, pw, V, Acc (ACC), S;
// subtree_levels sums the rows it is given in place (F and Ic, or Acc); integrate_bodies reads its
// src velocity, qw, qloc, root_q, T and writes u0 (write_out), q, qloc, root_pos, root_q, limmask;
// limit_detect writes limmask. On entry: load_tables has filled L.T, and the state words (root_pos,
// root_q, q, u0) are set.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/humanoid_engine.h"
#include "he_math.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_phys_spatial.h"
#include "he_regla.h"
#include "he_smpl_topo.h"

namespace {

// one level with every parent at once: lane (group g = lane / NC, component x) takes its parent and
// children from compile-time selects, reads them (a missing child reads the parent and adds 0:
// the sum order of subtree_parent, bit-identical) and writes back; no exec-mask branch per parent
template <int J, int JE>
HE_DEV int pick_body(int g, int j0, int k) {  // k = -1: the parent, else child slot k (-1 = none)
    if constexpr (J < JE) {
        constexpr int p = smpl::kParentLevelBodies[J];
        const int v = k < 0 ? p : (k == 0 ? smpl::kChildren[p][0] : (k == 1 ? smpl::kChildren[p][1] : smpl::kChildren[p][2]));
        return g == J - j0 ? v : pick_body<J + 1, JE>(g, j0, k);
    } else {
        return -1;
    }
}
template <int NC, int D>
HE_DEV void subtree_level_flat(float* F, float* I, int lane) {
    constexpr int j0 = smpl::kParentLevelStart[D], j1 = smpl::kParentLevelStart[D + 1];
    static_assert((j1 - j0) * NC <= W, "one level's parents fit one wave");
    const int g = lane / NC, x = lane - g * NC;
    const int p = pick_body<j0, j1>(g, j0, -1);
    const int c0 = pick_body<j0, j1>(g, j0, 0), c1 = pick_body<j0, j1>(g, j0, 1), c2 = pick_body<j0, j1>(g, j0, 2);
    if (lane < (j1 - j0) * NC) {
        float* X = x < 6 ? F : I;
        const int st = x < 6 ? 6 : 10, xx = x < 6 ? x : x - 6;
        float v = X[p * st + xx];
        const float v0 = X[(c0 >= 0 ? c0 : p) * st + xx];
        const float v1 = X[(c1 >= 0 ? c1 : p) * st + xx];
        const float v2 = X[(c2 >= 0 ? c2 : p) * st + xx];
        v += c0 >= 0 ? v0 : 0.f;
        v += c1 >= 0 ? v1 : 0.f;
        v += c2 >= 0 ? v2 : 0.f;
        X[p * st + xx] = v;
    }
}
template <int NC, int D>
HE_DEV void subtree_levels(float* F, float* I, int lane) {
    if constexpr (D >= 0) {
        constexpr int j0 = smpl::kParentLevelStart[D], j1 = smpl::kParentLevelStart[D + 1];
        if constexpr (j1 > j0) {
            subtree_level_flat<NC, D>(F, I, lane);
            sync();
        }
        subtree_levels<NC, D - 1>(F, I, lane);
    }
}

// ---------------------------------------------------------------------------------- kinematics
// 2^k-th ancestor of every body (-1: none), for pointer jumping over the body tree
struct JumpTable {
    int j[4][NB];
    constexpr JumpTable() : j() {
        for (int b = 0; b < NB; ++b)
            j[0][b] = smpl::kParentBody[b] == 0 ? -1 : smpl::kParentBody[b];  // stops below the root
        for (int k = 1; k < 4; ++k)
            for (int b = 0; b < NB; ++b) j[k][b] = j[k - 1][b] < 0 ? -1 : j[k - 1][j[k - 1][b]];
    }
};
constexpr JumpTable kJumpT{};
static_assert(smpl::kNumBodyLevels <= 16, "four pointer-jumping rounds cover chains of 16 bodies");
static_assert(smpl::kNumBodyLevels - 1 <= 8, "three rounds cover the root's subtrees of depth 8");
constexpr int kKinRounds = 3;

struct Jump4 {  // the four jump targets of each body packed as bytes (LDS table BodyTopo::jump4)
    uint32_t v[NB];
    constexpr Jump4() : v() {
        for (int b = 0; b < NB; ++b)
            for (int k = 0; k < 4; ++k) v[b] |= (uint32_t)(kJumpT.j[k][b] & 0xFF) << (8 * k);
    }
};
constexpr Jump4 kJump4{};
template <int K>
HE_DEV int jump_of(uint32_t jp) {  // byte K of the lane's packed entry, sign-extended (v_bfe_i32)
    return (int)(int8_t)(jp >> (8 * K));
}
// y_b <- the sum of y over body b's chain below the root (lane = body; jp: the lane's packed jump
// entry, 0xFFFFFFFF for none), by pointer jumping; the root's own term is added by the caller
HE_DEV void chain_prefix6(uint32_t jp, int lane, float (&y)[6]) {
    regla::static_for<0, kKinRounds, 1>([&](auto kc) {
        const int j = jump_of<decltype(kc)::value>(jp);
        const int src = j < 0 ? lane : j;
        float ya[6];
#pragma unroll
        for (int x = 0; x < 6; ++x) ya[x] = __shfl(y[x], src, W);
        if (j >= 0)
#pragma unroll
            for (int x = 0; x < 6; ++x) y[x] += ya[x];
    });
}

// World poses and spatial velocities, lane = body, by pointer jumping: X_b <- X_{J_k(b)} o X_b and
// V_b <- V_b + V_{J_k(b)} with J_k the 2^k-th ancestor, four rounds for chains of up to 16 bodies
// (log depth instead of a chain walk per body). X = (q, p): (qa, pa) o (qb, pb) = (qa qb, pa + Ra pb).
// The table stops below the root, so three rounds compose each chain in the root's
// frame (SMPL subtrees are 8 deep) and the root's pose / velocity / base acceleration, uniform LDS
// reads, are applied once at the end -- one dependent ds_bpermute round fewer per prefix.
// Joint axes S (lane = dof) follow from the world poses.
template <bool ACC>
HE_DEV void kinematics(Lds& L, const he_model& m, int lane, const he_sim_params& sp, bool cached) {
    const BodyTopo& T = L.T;
    const bool act = lane < NB;
    const int b = act ? lane : 0;
    const uint32_t jp = act ? T.jump4[b] : 0xFFFFFFFFu;
    f4 q;
    f3 p;
    float u[3];
    // the root's pose, read by every lane (uniform LDS addresses: broadcast)
    const f4 qr = qnormalize(f4{L.root_q[0], L.root_q[1], L.root_q[2], L.root_q[3]});
    if (b == 0) {
        q = qr;
        p = f3{0.f, 0.f, 0.f};  // origins about o
        u[0] = L.u0[0]; u[1] = L.u0[1]; u[2] = L.u0[2];
    } else {
        const int d = 3 * (b - 1);
        if (cached) {  // the previous substep's integrated rotation (pre-log)
            q = f4{L.qloc[b][0], L.qloc[b][1], L.qloc[b][2], L.qloc[b][3]};
        } else {
            q = pqexp(f3{L.q[d], L.q[d + 1], L.q[d + 2]});
            L.qloc[b][0] = q.x; L.qloc[b][1] = q.y; L.qloc[b][2] = q.z; L.qloc[b][3] = q.w;
        }
        p = f3{T.local_pos[b][0], T.local_pos[b][1], T.local_pos[b][2]};
        u[0] = L.u0[6 + d]; u[1] = L.u0[7 + d]; u[2] = L.u0[8 + d];
    }
    auto jump = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        const int j = jump_of<K>(jp);
        const int src = j < 0 ? lane : j;
        const f4 qa = f4{__shfl(q.x, src, W), __shfl(q.y, src, W), __shfl(q.z, src, W), __shfl(q.w, src, W)};
        const f3 pa = f3{__shfl(p.x, src, W), __shfl(p.y, src, W), __shfl(p.z, src, W)};
        if (j >= 0) {
            p = pa + qapply(qa, p);
            q = qmul(qa, q);
        }
    };
    regla::static_for<0, kKinRounds, 1>(jump);
    if (b != 0) {  // root-frame pose of the chain -> world axes, origin about o
        p = qapply(qr, p);
        q = qmul(qr, q);
    }
    // own joint's velocity contribution: root (w0, v0 at o); joint b: (w, (p_b - o) x w), w = R_b u_b
    float V[6];
    if (b == 0) {
        V[0] = u[0]; V[1] = u[1]; V[2] = u[2]; V[3] = L.u0[3]; V[4] = L.u0[4]; V[5] = L.u0[5];
    } else {
        const f3 w = qapply(q, f3{u[0], u[1], u[2]});
        const f3 l = cross3(p, w);
        V[0] = w.x; V[1] = w.y; V[2] = w.z; V[3] = l.x; V[4] = l.y; V[5] = l.z;
    }
    float vj[6];  // the joint's own velocity S_b u_b (RNEA velocity-product term below)
#pragma unroll
    for (int x = 0; x < 6; ++x) vj[x] = V[x];
    chain_prefix6(jp, lane, V);
    if (b != 0) {  // plus the root's own velocity
#pragma unroll
        for (int x = 0; x < 6; ++x) V[x] += L.u0[x];
    }
    if (act) {
        L.qw[b][0] = q.x; L.qw[b][1] = q.y; L.qw[b][2] = q.z; L.qw[b][3] = q.w;
        L.pw[b][0] = p.x; L.pw[b][1] = p.y; L.pw[b][2] = p.z;
        for (int x = 0; x < 6; ++x) L.V[b][x] = V[x];
    }
    if constexpr (ACC) {
        // RNEA bias acceleration (gravity as base acceleration): a_b = a_0 + sum over the chain's
        // joints j of V_j x (S_j u_j), the same prefix over the tree by pointer jumping. The base:
        // (0, v0 x w0 - g) for the free root (u = [w0, v0 at o]).
        float A[6];
        const f3 vxw = cross3(f3{L.u0[3], L.u0[4], L.u0[5]}, f3{L.u0[0], L.u0[1], L.u0[2]});
        const float A0[6] = {0.f, 0.f, 0.f, vxw.x - sp.gravity[0], vxw.y - sp.gravity[1], vxw.z - sp.gravity[2]};
        if (b == 0) {
#pragma unroll
            for (int x = 0; x < 6; ++x) A[x] = A0[x];
        } else {
            crm(V, vj, A);
        }
        chain_prefix6(jp, lane, A);
        if (b != 0) {  // plus the base acceleration
#pragma unroll
            for (int x = 0; x < 6; ++x) A[x] += A0[x];
        }
        if (act)
            for (int x = 0; x < 6; ++x) L.Acc[b][x] = A[x];
    }
    sync();
    // lane = dof: dofs 0..63 with the root's six unit axes selected in, then dofs 64..74 (ball
    // joints only); no loop and no root branch
    auto axis = [&](int i, bool may_root) {
        const bool rd = may_root && i < 6;
        const int k = rd ? 0 : i - 6;
        const int kb = k / 3, c = k - 3 * kb, bb = kb + 1;
        const f4 qb = f4{L.qw[bb][0], L.qw[bb][1], L.qw[bb][2], L.qw[bb][3]};
        const f3 e = f3{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        const f3 ax = qapply(qb, e);
        const f3 l = cross3(f3{L.pw[bb][0], L.pw[bb][1], L.pw[bb][2]}, ax);
        const float g[6] = {ax.x, ax.y, ax.z, l.x, l.y, l.z};
        float* S = L.S[i];
#pragma unroll
        for (int x = 0; x < 6; ++x) S[x] = rd ? (x == i ? 1.f : 0.f) : g[x];
    };
    axis(lane, true);
    static_assert(NG - W <= W && NG - W > 0, "a second set of lanes covers dofs 64..NG-1");
    if (lane < NG - W) axis(W + lane, false);
    sync();
}

// Joint-angle limit of joint b (oracle/he_oracle_physics.c angle_row): the exp-map coordinate
// wraps at |q_b| = pi, so the MJCF's +-180 / +-720 deg ranges hold the rotation angle at
// pi - kLimitGuard; the speculative row is emitted within limit_margin + dt * (closing rate).
constexpr float kLimitGuard = 0.02f;
HE_DEV bool angle_row(f3 th, f3 u, const he_sim_params& p, float& gap, f3& dir) {
    const float t = __builtin_amdgcn_sqrtf(dot3(th, th));
    dir = th * __builtin_amdgcn_rcpf(fmaxf(t, 1e-30f));
    gap = (3.14159265358979f - kLimitGuard) - t;
    const float closing = dot3(dir, u);
    return t >= 1e-6f && gap < p.limit_margin + p.dt * fmaxf(closing, 0.f);
}

// the scalar part of a joint rotation at limit_clamp's cap, cos((pi - kLimitGuard / 2) / 2): its first test,
// which integrate_bodies makes once for the wave in front of the call
constexpr float kWcap = 0.00499997917f;
// Backstop when the limit rows lose (oracle/he_oracle_physics.c limit_clamp): a limit against a
// deep self contact has no solution, and a joint near 100 rad/s can cross the margin in one
// substep. nq = exp(q_old) (x) exp(dt w) before the log (exp(q_old) has w >= 0: the kinematics'
// and this function's qloc): its scalar part is negative when the rotation went past pi this
// substep, and the log then comes back on the far side with the axis flipped, which would reverse
// the joint's PD error and spin it. The angle is continued past pi instead, then held at
// pi - kLimitGuard / 2 on the joint's side with the outward rate q^ . w removed. Returns whether it
// acted (nv and w changed).
HE_DEV bool limit_clamp(f4 nq, f3& nv, float (&w)[3]) {
    constexpr float kTwoPi = 6.28318530717959f;
    constexpr float cap = 3.14159265358979f - 0.5f * kLimitGuard;
    if (nq.w >= kWcap) return false;         // inside the cap, not crossed: the common case
    const float t0 = sqrtf(dot3(nv, nv));
    if (!(t0 >= 1e-12f)) return false;
    f3 dir = nv * (1.0f / t0);
    float t = t0;
    if (nq.w < 0.f) {
        t = kTwoPi - t0;
        dir = dir * -1.f;
    }
    if (t <= cap) return false;
    nv = dir * cap;
    const float out = dir.x * w[0] + dir.y * w[1] + dir.z * w[2];
    if (out > 0.f) { w[0] -= out * dir.x; w[1] -= out * dir.y; w[2] -= out * dir.z; }
    return true;
}

// Which joints emit their limit row in the next substep, from joint b's exp map th and velocity u
// (lane = body b; every lane calls, the root and lanes >= NB with on = false), read by the drive
// terms (a joint on its limit cannot give way). Evaluated where q and u are set -- the state load,
// then each integration but the last; the contact phase re-evaluates the rows themselves from the
// same L.q / L.u0 (bit-identical inputs, the same decision).
HE_DEV void limit_detect(Lds& L, int lane, bool joint, f3 th, f3 u, const he_sim_params& sp) {
    float lg = 0.f;
    f3 ld = f3{0.f, 0.f, 0.f};
    const bool on = joint && angle_row(th, u, sp, lg, ld);
    const uint64_t bm = __ballot(on);
    if (lane == 0) L.limmask = (uint32_t)bm;
}

// ---------------------------------------------------------------------------------- integration
// Damping, the angular-velocity clamps and the semi-implicit position update over hs in one pass per
// body (lane = body). src: the solved generalized velocity (PGS: L.uf; TGS: the working velocity
// L.u0). write_out: the damped, clamped velocity becomes the state's (PGS always; TGS the last
// position iteration only: the solver's own velocity is not clamped, oracle substep_tgs). detect: the
// next substep's limit rows from the new state.
HE_DEV void integrate_bodies(Lds& L, const BodyTopo& T, int lane, const he_sim_params& p, float hs, float damp,
                             const float* src, bool write_out, bool detect) {
    // damping, the angular-velocity clamps and the semi-implicit position update in one pass per
    // body: the root composes exp(dt w) (x) q, a ball joint log(exp(q) (x) exp(dt u)); both as
    // normalize(e1 (x) e2) with the operands selected, so the two cases share one code path
    f3 lim_th = f3{0.f, 0.f, 0.f}, lim_u = f3{0.f, 0.f, 0.f};  // the joint's new q and u
    const bool bl = lanes_body();
    const bool root = regla::lanes<1ull>();
    const int d0 = root ? 0 : 6 + 3 * ((bl ? lane : 1) - 1);
    float w[3] = {src[d0] * damp, src[d0 + 1] * damp, src[d0 + 2] * damp};
    {
        // the joint's relative rate: PhysX articulation joint maxJointVelocity
        const float n2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];  // squared: the norm only where it acts
        // rare: one test for the wave (a lane >= NB carries body 1's rates)
        const bool fast = n2 > p.max_joint_velocity * p.max_joint_velocity;
        if (__builtin_expect((__ballot(fast) & ~1ull) != 0ull, 0)) {
            if (!root && fast) {
                const float s = p.max_joint_velocity / sqrtf(n2);
                w[0] *= s; w[1] *= s; w[2] *= s;
            }
        }
        // the link's WORLD angular velocity (asset max_angular_velocity, PxRigidBody): w_b = w_parent +
        // R_b u_b summed along the chain (Acc is scratch here), clamped link by link; the joint rates
        // are then re-derived, u_b = R_b^T (w'_b - w'_parent) (oracle: the same pass)
        // no link can be over when |w_root| + (joints on the longest chain) x max_j |u_j| stays under
        // the cap (triangle inequality; a 1 % margin covers the prefix's rounding): the prefix and
        // the clamp are then skipped (wave-uniform), with the result they would give
        const float un = __builtin_amdgcn_sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);  // a skip test with a 1 % margin
        const float wroot = regla::rdlane(un, 0);
        // every lane compares (no short-circuit region); the joints' lanes picked from the ballot
        const uint64_t may = __ballot(un * (float)(smpl::kNumBodyLevels - 1) > 0.99f * p.max_angular_velocity - wroot) &
                             (((1ull << NB) - 1ull) & ~1ull);
        if (__builtin_expect(may != 0ull, 0)) {
        const f4 qb = bl ? f4{L.qw[lane][0], L.qw[lane][1], L.qw[lane][2], L.qw[lane][3]} : f4{0.f, 0.f, 0.f, 1.f};
        const f3 wr = root ? f3{w[0], w[1], w[2]} : qapply(qb, f3{w[0], w[1], w[2]});
        // chain prefix by pointer jumping (the table stops below the root: its rate is added last)
        f3 wo = bl ? wr : f3{0.f, 0.f, 0.f};
        {
            const uint32_t jp = bl ? T.jump4[lane] : 0xFFFFFFFFu;
            auto round = [&](auto kc) {
                constexpr int K = decltype(kc)::value;
                const int j = jump_of<K>(jp);
                const int src = j < 0 ? lane : j;
                const f3 wa = f3{__shfl(wo.x, src, W), __shfl(wo.y, src, W), __shfl(wo.z, src, W)};
                if (j >= 0) wo = wo + wa;
            };
            round(std::integral_constant<int, 0>{});
            round(std::integral_constant<int, 1>{});
            round(std::integral_constant<int, 2>{});
            if constexpr (kKinRounds == 4) round(std::integral_constant<int, 3>{});
            const f3 w0 = f3{__shfl(wr.x, 0, W), __shfl(wr.y, 0, W), __shfl(wr.z, 0, W)};
            if (bl && !root) wo = wo + w0;
        }
        const float wmax = p.max_angular_velocity;
        const float wn2 = dot3(wo, wo);
        const bool over = bl && wn2 > wmax * wmax;
        if (__builtin_expect(__ballot(over) != 0ull, 0)) {  // rare (wave-uniform branch)
            const f3 wc = over ? wo * (wmax * __builtin_amdgcn_rsqf(wn2)) : wo;
            const int pb = bl && !root ? T.chain[lane][T.depth[lane] - 1] : 0;
            const f3 wp = f3{__shfl(wc.x, pb, W), __shfl(wc.y, pb, W), __shfl(wc.z, pb, W)};
            if (bl) {
                const f3 rel = root ? wc : wc - wp;
                const f3 ub = root ? rel : qapply(qconj(qb), rel);
                w[0] = ub.x; w[1] = ub.y; w[2] = ub.z;
            }
        }
        }
    }
    if (bl) {
        if (write_out) { L.u0[d0] = w[0]; L.u0[d0 + 1] = w[1]; L.u0[d0 + 2] = w[2]; }
        const int d = root ? 0 : 3 * (lane - 1);
        const f3 dtw = f3{hs * w[0], hs * w[1], hs * w[2]};
        const f4 ed = pqexp(dtw);  // exp(q_b) itself: the kinematics' qloc (L.q is unchanged since)
        const f4 e1 = root ? ed : f4{L.qloc[lane][0], L.qloc[lane][1], L.qloc[lane][2], L.qloc[lane][3]};
        const f4 e2 = root ? f4{L.root_q[0], L.root_q[1], L.root_q[2], L.root_q[3]} : ed;
        const f4 nq = qnormalize(qmul(e1, e2));
        if (root) {
            if (write_out) { L.u0[3] = src[3]; L.u0[4] = src[4]; L.u0[5] = src[5]; }
            for (int c = 0; c < 3; ++c) L.root_pos[c] += hs * src[3 + c];
            L.root_q[0] = nq.x; L.root_q[1] = nq.y; L.root_q[2] = nq.z; L.root_q[3] = nq.w;
        } else {
            f3 nv = pqlog(nq);
            f4 nql = nq;
            // rare: the limit rows lost. limit_clamp's own first test, once for the wave's joints
            if (p.joint_limits && __builtin_expect(__ballot(!(nq.w >= kWcap)) != 0ull, 0) && limit_clamp(nq, nv, w)) {
                if (write_out) { L.u0[d0] = w[0]; L.u0[d0 + 1] = w[1]; L.u0[d0 + 2] = w[2]; }
                nql = pqexp(nv);
            }
            L.q[d] = nv.x; L.q[d + 1] = nv.y; L.q[d + 2] = nv.z;
            // the next substep's kinematics starts from this rotation instead of exp(log(.))
            L.qloc[lane][0] = nql.x; L.qloc[lane][1] = nql.y; L.qloc[lane][2] = nql.z; L.qloc[lane][3] = nql.w;
            lim_th = nv;
            lim_u = f3{w[0], w[1], w[2]};
        }
    }
    if (p.joint_limits && detect) limit_detect(L, lane, lane >= 1 && lane < NB, lim_th, lim_u, p);
    sync();
}

}  // namespace
