// he_phys_dynamics.h -- from the kinematics to the free motion: body inertias and RNEA forces
// (body_forces), the external wrench and actuation terms of the EXT kernels (ext_*), the implicit PD
// drives (drive_terms), the CRBA on the matrix cores and the factorisation (crba_*, factor_free),
// the packed factor's rows (load_rows), the midpoint bias (mid_lt, joint_velocity, bias_midpoint)
// and what a TGS position iteration runs between its sweeps (tgs_bias_at, tgs_rhs, tgs_velocity,
// tgs_drive_acc).
// LDS: reads qw, pw, V, Acc, S, q, tgt, u0, limmask, T; writes Ic, Ib, F, Q, IS, dforce, uf, rhs,
// coef, Lp, sDinv, yh (factor_free), then yh, uf, u0 and the V / F / Acc scratch (the midpoint and the
// TGS helpers). On entry: the kinematics of this substep has run; the tgs_* helpers need the step's
// factor (Lp, sDinv), its S and Ib, and kp parked in dforce.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/humanoid_engine.h"
#include "he_kernels.h"
#include "he_math.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_phys_spatial.h"
#include "he_phys_tree.h"
#include "he_regla.h"
#include "he_smpl_topo.h"

namespace {

// body spatial inertias about o + RNEA body forces, gravity as base acceleration (oracle
// body_inertia and the force pass of rnea), lane = body. Reads qw, pw, V, Acc of the kinematics;
// writes Ic (own inertia: the subtree sums accumulate in place), Ib (the same, for the midpoint's and
// the TGS iterations' second RNEA) and F (body force).
HE_DEV void body_forces(Lds& L, const he_model& m, const he_sim_params& p, int lane, const float* mass_scale) {
    if (lane < NB) {
        int b = lane;
        float ms = mass_scale ? mass_scale[b] : 1.f;
        float mass = m.mass[b] * ms;
        f4 q = f4{L.qw[b][0], L.qw[b][1], L.qw[b][2], L.qw[b][3]};
        f3 c0, c1, c2;
        qcols(q, c0, c1, c2);
        f3 cw = qapply(q, f3{m.com[b][0], m.com[b][1], m.com[b][2]});
        f3 s = f3{L.pw[b][0], L.pw[b][1], L.pw[b][2]} + cw;  // CoM about o
        const float* in = m.inertia[b];
        float Ib[3][3] = {{in[0], in[3], in[4]}, {in[3], in[1], in[5]}, {in[4], in[5], in[2]}};
        float R[3][3] = {{c0.x, c1.x, c2.x}, {c0.y, c1.y, c2.y}, {c0.z, c1.z, c2.z}};
        float T1[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) T1[r][c] = R[r][0] * Ib[0][c] + R[r][1] * Ib[1][c] + R[r][2] * Ib[2][c];
        float I[3][3];
        float ss = dot3(s, s);
        float sv[3] = {s.x, s.y, s.z};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                I[r][c] = (T1[r][0] * R[c][0] + T1[r][1] * R[c][1] + T1[r][2] * R[c][2]) * ms +
                          mass * ((r == c ? ss : 0.f) - sv[r] * sv[c]);
        float* o10 = L.Ic[b];  // own inertia; the subtree sums accumulate in place
        o10[0] = mass; o10[1] = mass * s.x; o10[2] = mass * s.y; o10[3] = mass * s.z;
        o10[4] = I[0][0]; o10[5] = I[1][1]; o10[6] = I[2][2]; o10[7] = I[0][1]; o10[8] = I[0][2]; o10[9] = I[1][2];
        if (p.bias_midpoint)  // the body's own inertia for the midpoint's second RNEA (Ib is free until
            for (int x = 0; x < 10; ++x) L.Ib[b][x] = o10[x];  // the contact phase's segments)
        body_force(o10, L.Acc[b], L.V[b], L.F[b]);  // body force f_b (accumulated in place)
    }
    sync();
}

// External wrenches (he_apply_body_forces; the EXT kernels only), after the subtree sums: body b's
// (torque, force at the CoM) row becomes the spatial wrench about o, W_b = (tau_b + s_b x f_b, f_b) with
// s_b the CoM about o as body_forces forms it, so the force follows the body from step to step; the
// subtree sums by body levels; Q_i = S_i . sum_subtree(body(i)) W into L.Q. Acc is scratch (dead from
// body_forces to the midpoint bias / the contact phase). on == false (the launch's physics steps past
// the wrench's hold): Q = 0, and the step computes what the kernels without the wrench code compute.
// The dof actuation forces (he_set_dof_actuation_forces; PhysArgs.dof_act non-null) then add the env's
// clamped joint torques to Q[6..75), in every physics step of the launch: the row is loaded from
// global memory here (lane i adds dof i - 6 to Q[i], then lanes 0..10 dofs 58..68 to Q[64..74]), nothing
// is kept between phases.
HE_DEV void ext_actuation_terms(Lds& L, const PhysArgs& a, int lane) {
    if (a.dof_act) {  // wave-uniform (a launch argument)
        const float* row = a.dof_act + (size_t)L.sch_e * ND;  // the env from LDS: no register held
        if (lane >= 6) L.Q[lane] += row[lane >= 6 ? lane - 6 : 0];
        if (lane < NG - W) L.Q[W + lane] += row[W - 6 + lane];
        sync();
    }
}
HE_DEV void ext_wrench_terms(Lds& L, const he_model& m, const PhysArgs& a, int lane, bool on) {
    if (!on || !a.ext_wrench) {  // wave-uniform; an actuation alone runs without a wrench array
        L.Q[lane] = 0.f;
        if (lane < NG - W) L.Q[W + lane] = 0.f;
        sync();
        ext_actuation_terms(L, a, lane);
        return;
    }
    if (lane < NB) {
        const int b = lane;
        const float* w = a.ext_wrench + ((size_t)L.sch_e * NB + b) * 6;  // the env from LDS: no register held
        const f3 tq = f3{w[0], w[1], w[2]}, f = f3{w[3], w[4], w[5]};
        const f4 q = f4{L.qw[b][0], L.qw[b][1], L.qw[b][2], L.qw[b][3]};
        const f3 s = f3{L.pw[b][0], L.pw[b][1], L.pw[b][2]} + qapply(q, f3{m.com[b][0], m.com[b][1], m.com[b][2]});
        const f3 n = tq + cross3(s, f);
        L.Acc[b][0] = n.x; L.Acc[b][1] = n.y; L.Acc[b][2] = n.z;
        L.Acc[b][3] = f.x; L.Acc[b][4] = f.y; L.Acc[b][5] = f.z;
    }
    sync();
    subtree_levels<6, smpl::kNumBodyLevels - 2>(&L.Acc[0][0], nullptr, lane);
    L.Q[lane] = dot6(L.S[lane], L.Acc[dof_body(lane)]);
    if (lane < NG - W) L.Q[W + lane] = dot6(L.S[W + lane], L.Acc[(W + lane - 6) / 3 + 1]);
    sync();
    ext_actuation_terms(L, a, lane);
}
// HE_BUF_DOF_FORCE includes the applied actuation (the EXT kernels, after the solver's drive and limit
// forces are final): dforce[d] += the env's row, re-read from global memory. Ends on a sync.
HE_DEV void ext_actuation_out(Lds& L, const PhysArgs& a, int lane) {
    if (a.dof_act) {  // wave-uniform
        const float* row = a.dof_act + (size_t)L.sch_e * ND;
        L.dforce[lane] += row[lane];
        if (lane < ND - W) L.dforce[W + lane] += row[W + lane];
        sync();
    }
}

// Bias forces, IS_i = Ic S_i and the implicit PD drives (oracle: the drive block), lane = dof, then
// dofs 64..74 on lanes 0..10. Writes IS, dforce (PGS: the drive torque; TGS: the scaled stiffness),
// uf (TGS: the bias at u0), rhs, coef. The per-dof body stays a lambda that captures by reference:
// as a function taking hs and limmask by value, the PGS kernel came out with one v_fma and one v_mul
// fewer and one v_sub more (a product contracted another way), and its results left the parent's bits.
template <bool TGS, bool EXT>
HE_DEV void drive_terms(Lds& L, const he_model& m, const he_sim_params& p, int lane, float hs) {
    const uint32_t limmask = p.joint_limits ? (uint32_t)__builtin_amdgcn_readfirstlane((int)L.limmask) : 0u;
    // lane = dof (then dofs 64..74 on lanes 0..10), the root's six dofs selected out: no loop,
    // no root branch, saturation by selects
    auto dof_terms = [&](int i, bool may_root) {
        const int b = may_root ? dof_body(i) : (i - 6) / 3 + 1;
        float bias = dot6(L.S[i], L.F[b]);
        if constexpr (EXT) bias -= L.Q[i];  // an external wrench enters as a bias of the opposite sign
        si_apply(L.Ic[b], L.S[i], L.IS[i]);
        const bool jd = !may_root || i >= 6;
        const int d = jd ? i - 6 : 0;
        float kp = m.stiffness[d] * p.kp_scale, kd = m.damping[d] * p.kd_scale;
        const float err = L.tgt[d] - L.q[d];
        const float u = L.u0[i];
        float tau = kp * (err - hs * u) - kd * u;
        const float lim = m.effort[d];
        // effort limit: the implicit step's drive torque, estimated with the dof's own joint-space
        // inertia H_ii = S_i . IS_i (+ armature) as tau - c dt (tau - bias) / (H_ii + dt c), scales
        // the whole drive down to the limit (oracle/he_oracle_physics.c, the drive block)
        // A joint held at its angle limit cannot give way: its check takes the torque at rest.
        const float c = hs * kp + kd;
        const float hii = dot6(L.S[i], L.IS[i]) + m.armature[d];
        const bool blocked = p.joint_limits && jd && ((limmask >> b) & 1u);
        const float tau_i = blocked ? tau : tau - c * hs * (tau - bias) * __builtin_amdgcn_rcpf(hii + hs * c);
        const float sc = fabsf(tau_i) > lim ? lim / fabsf(tau_i) : 1.f;
        tau *= sc;
        kp *= sc;
        kd *= sc;
        if (jd) L.dforce[d] = TGS ? kp : tau;  // TGS: the scaled stiffness, for the iterations' drives
        if constexpr (TGS) L.uf[i] = bias;       // TGS: the bias at u0, until an iteration re-evaluates it
        L.rhs[i] = hs * (jd ? tau - bias : -bias);
        L.coef[i] = jd ? hs * kp + kd : 0.f;
    };
    dof_terms(lane, true);
    if (lane < NG - W) dof_terms(W + lane, false);
    sync();
}

// CRBA on the matrix cores: H = IS^T S as v_mfma_f32_32x32x2_f32 tiles (rows i, columns j, K = the
// six spatial components in three steps), lower block triangle only: 6 tiles, 18 MFMAs. Operands
// come straight from LDS (lane l: IS_{32R + l%32}[2s + l/32] and S_{32C + l%32}[2s + l/32]). One
// v_permlane32_swap per register pair of a row block's column-tile pair lands "lane j holds column
// j" (RegMat), then the diagonal addends (armature + implicit drive).
template <int RB>
HE_DEV void crba_tile_rows(regla::RegMat& M, const f32x16& ta, const f32x16& tb) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = RB + (v & 3) + 8 * (v >> 2);
        float a = ta[v], b = tb[v];
        swap32(a, b);  // a: row r of columns (lane), b: row r + 4
        if (r < NG) M.cp[r >> 1][r & 1] = a;
        if (r + 4 < NG) M.cp[(r + 4 < NG ? r + 4 : 0) >> 1][(r + 4) & 1] = b;
    }
}
// Entries off the ancestor chains are left as the dense product. The elimination
// reads only chain entries (an update of row I on lane j uses row K on lane j, and j in chain(I),
// I in chain(K) gives j in chain(K)), stores only chain lanes, and the pivots are diagonal, so
// those entries never reach L, D or the right-hand side; only the diagonal addends remain.
template <int I>
HE_DEV void crba_mask_rows(regla::RegMat& M, float dadd, float dadd2) {
    using namespace regla;
    if constexpr (I < NG) {
        float h = mc<I>(M);
        if constexpr (I < 64) h = lanes<1ull << I>() ? h + dadd : h;  // armature + implicit drive
        asm volatile("" : "+v"(h));
        mc_set<I>(M, h);
        if constexpr (I >= 64) {
            float h2 = mc2<I - 64>(M);
            h2 = lanes<1ull << (I - 64)>() ? h2 + dadd2 : h2;
            asm volatile("" : "+v"(h2));
            mc2_set<I - 64>(M, h2);
        }
        crba_mask_rows<I + 1>(M, dadd, dadd2);
    }
}
HE_DEV void crba_mfma(regla::RegMat& M, const Lds& L, int lane, float dadd, float dadd2) {
    const int l31 = lane & 31, kh = lane >> 5;
    float bS[3][3], aI[3][3];  // [block][k step]
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int j = 32 * c + l31;
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            bS[c][st] = j < NG ? L.S[j < NG ? j : 0][2 * st + kh] : 0.f;
            aI[c][st] = j < NG ? L.IS[j < NG ? j : 0][2 * st + kh] : 0.f;
        }
    }
    const f32x16 zero = {};
    {
        f32x16 t0 = {};
#pragma unroll
        for (int st = 0; st < 3; ++st) t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[0][st], bS[0][st], t0, 0, 0, 0);
        crba_tile_rows<0>(M, t0, zero);  // rows 0-31 are above the diagonal for columns 32-63
    }
    {
        f32x16 t0 = {}, t1 = {};
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[1][st], bS[0][st], t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[1][st], bS[1][st], t1, 0, 0, 0);
        }
        crba_tile_rows<32>(M, t0, t1);
    }
    {
        f32x16 t0 = {}, t1 = {}, t2 = {};
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[2][st], bS[0][st], t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[2][st], bS[1][st], t1, 0, 0, 0);
            t2 = __builtin_amdgcn_mfma_f32_32x32x2f32(aI[2][st], bS[2][st], t2, 0, 0, 0);
        }
        crba_tile_rows<64>(M, t0, t1);
        // columns 64-74 (second register set, lanes 0-10): rows r from the low half, r + 4 from
        // the high half of the same tile
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = 64 + (v & 3) + 8 * (v >> 2);
            float a = t2[v], b = t2[v];
            swap32(a, b);
            if (r < NG) M.cp2[(r - 64) >> 1][(r - 64) & 1] = a;
            if (r + 4 < NG) M.cp2[(r + 4 < NG ? r - 60 : 0) >> 1][(r - 60) & 1] = b;
        }
    }
    crba_mask_rows<0>(M, dadd, dadd2);
}

// CRBA straight into registers (lane j owns column j, H[i][j] = S_j . IS_i), the sparse LTDL in
// registers (RBDA 6.5, deepest dof first) with the free-velocity right-hand side y = L^-T (dt rhs)
// carried through the elimination. Leaves Lp (the packed factor), sDinv and yh in LDS; the mass
// matrix never leaves the registers of this function. IS is dead after it.
HE_DEV void factor_free(Lds& L, const he_model& m, int lane, float hs, Stamps& st) {
    using namespace regla;
    RegMat M;
    {
        // per-lane diagonal addend (dof = lane, and 64 + lane on lanes < 11), loaded once
        const float dadd = lane >= 6 ? m.armature[lane >= 6 ? lane - 6 : 0] + hs * L.coef[lane] : 0.f;
        const float dadd2 = lane < NH ? m.armature[lane < NH ? 58 + lane : 0] + hs * L.coef[64 + lane] : 0.f;
        crba_mfma(M, L, lane, dadd, dadd2);
    }
    STAMP(PH_CRBA);
    float yl = L.rhs[lane], y2 = lane < NH ? L.rhs[64 + lane] : 0.f;
    float Dl = 1.f, D2 = 1.f;
    __builtin_amdgcn_s_setprio(kPrioSerial);
    factor_pipelined(M, Dl, D2, L.Lp, L.T.dof_depth[lane], lane < NH ? L.T.dof_depth[64 + lane] : 0, yl, y2);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.sDinv[lane] = 1.0f / sqrtf(Dl);
    if (lane < NH) L.sDinv[64 + lane] = 1.0f / sqrtf(D2);
    // the free velocity is not formed here: the contact bias takes z.u0 + zh.yh, and one L^-1
    // sweep after the solver gives uf = u0 + L^-1 D^-1/2 (yh + Zh^T lambda)
    L.yh[lane] = yl * (1.0f / sqrtf(Dl));
    if (lane < NH) L.yh[64 + lane] = y2 * (1.0f / sqrtf(D2));
    sync();
}

// lane i's packed row of L (dof i) and the row of dof 64 + i (lanes >= NH read row 64 and never
// use it: an exec-masked second load measured slower than the unmasked one, A/B r01)
HE_DEV void load_rows(const Lds& L, const BodyTopo& T, int lane, float (&r1)[regla::kRowRegs],
                      float (&r2)[regla::kRowRegs]) {
    const float4* p1 = reinterpret_cast<const float4*>(L.Lp + T.pack_start[lane]);
    const float4* p2 = reinterpret_cast<const float4*>(L.Lp + T.pack_start[lane < regla::NH ? 64 + lane : 0]);
#pragma unroll
    for (int q = 0; q < regla::kRowRegs / 4; ++q) {
        const float4 a1 = p1[q], a2 = p2[q];
        r1[4 * q] = a1.x; r1[4 * q + 1] = a1.y; r1[4 * q + 2] = a1.z; r1[4 * q + 3] = a1.w;
        r2[4 * q] = a2.x; r2[4 * q + 1] = a2.y; r2[4 * q + 2] = a2.z; r2[4 * q + 3] = a2.w;
    }
}

// ---------------------------------------------------------------------------------- midpoint bias
// he_sim_params.bias_midpoint (oracle/he_oracle_physics.c: substep, bias_at): the velocity-dependent
// bias (Coriolis, gyroscopic; gravity cancels) again at the midpoint velocity um = (u0 + uf) / 2 of
// the explicit step, and the free velocity corrected through the same factor:
// yh += D^-1/2 L^-T dt (bias(u0) - bias(um)). Runs between the factorisation and the contact phase,
// with the factor in Lp and the first bias's subtree forces in F. Scratch: uf (holds um), V (the
// final kinematics rewrites it), Acc (the contact phase's scratch after), Ib (own inertias, stored
// by the force pass).
// yh += D^-1/2 L^-T dc (lane = dof, then dofs 64..74 on lanes 0..10): the midpoint correction's
// forward substitution replayed from the stored factor
HE_DEV void mid_lt(Lds& L, const BodyTopo& T, int lane, float c1, float c2) {
    using regla::NH;
    __builtin_amdgcn_s_setprio(kPrioSerial);  // a serial chain: -1.2 % physics launch by A/B (r04)
    regla::solve_LT_vec_pipelined(L.Lp, T.dof_depth[lane], lane < NH ? T.dof_depth[64 + lane] : 0, c1, c2);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.yh[lane] += c1 * L.sDinv[lane];
    if (lane < NH) L.yh[64 + lane] += c2 * L.sDinv[64 + lane];
    sync();
}

// joint b's own velocity S_b u_b at the generalized velocity vel (the root's S are the unit axes)
HE_DEV void joint_velocity(const Lds& L, const BodyTopo& T, int b, const float* vel, float (&vj)[6]) {
    if (b == 0) {
        for (int x = 0; x < 6; ++x) vj[x] = vel[x];
    } else {
        const int d0 = T.dof0[b];
        const float u0_ = vel[d0], u1_ = vel[d0 + 1], u2_ = vel[d0 + 2];
        for (int x = 0; x < 6; ++x) vj[x] = L.S[d0][x] * u0_ + L.S[d0 + 1][x] * u1_ + L.S[d0 + 2][x] * u2_;
    }
}
HE_DEV void bias_midpoint(Lds& L, const BodyTopo& T, int lane, const he_sim_params& p, Stamps& st) {
    using namespace regla;
    const float dt = p.dt;
    {  // um = u0 + (L^-1 D^-1/2 yh) / 2, the midpoint of u0 and the explicit free velocity
        float r1[regla::kRowRegs], r2[regla::kRowRegs];
        load_rows(L, T, lane, r1, r2);
        float t1 = L.yh[lane] * L.sDinv[lane];
        float t2 = lane < NH ? L.yh[64 + lane] * L.sDinv[64 + lane] : 0.f;
        __builtin_amdgcn_s_setprio(kPrioSerial);  // a serial chain (level sweep)
        regla::solve_L_rows<0>(r1, r2, t1, t2);  // y <- L^-1 y for the lane's rows
        __builtin_amdgcn_s_setprio(kPrioDefault);
        L.uf[lane] = L.u0[lane] + 0.5f * t1;
        if (lane < NH) L.uf[64 + lane] = L.u0[64 + lane] + 0.5f * t2;
    }
    sync();
    STAMP(PH_MID_UM);
    const bool bl = lane < NB;
    const int b = bl ? lane : 0;
    // velocities and bias accelerations at um by pointer jumping over the chain, as the kinematics
    // does at u0 (the jump table stops below the root; the root's velocity and base acceleration are
    // added once at the end): no LDS chain walks
    float Fb[6];
    {
        const uint32_t jp = bl ? T.jump4[b] : 0xFFFFFFFFu;
        float vj[6];
        joint_velocity(L, T, b, L.uf, vj);
        float V[6];
        for (int x = 0; x < 6; ++x) V[x] = vj[x];
        chain_prefix6(jp, lane, V);
        const float um6[6] = {L.uf[0], L.uf[1], L.uf[2], L.uf[3], L.uf[4], L.uf[5]};
        if (b != 0)
            for (int x = 0; x < 6; ++x) V[x] += um6[x];
        const f3 vxw = cross3(f3{um6[3], um6[4], um6[5]}, f3{um6[0], um6[1], um6[2]});
        const float A0[6] = {0.f, 0.f, 0.f, vxw.x - p.gravity[0], vxw.y - p.gravity[1], vxw.z - p.gravity[2]};
        float A[6];
        if (b == 0) {
            for (int x = 0; x < 6; ++x) A[x] = A0[x];
        } else {
            crm(V, vj, A);  // joint b's velocity-product term V_b x S_b um_b
        }
        chain_prefix6(jp, lane, A);
        if (b != 0)
            for (int x = 0; x < 6; ++x) A[x] += A0[x];
        body_force(L.Ib[b], A, V, Fb);
    }
    sync();
    if (bl)
        for (int x = 0; x < 6; ++x) L.Acc[b][x] = Fb[x];
    sync();
    STAMP(PH_MID_RNEA);
    // subtree sums of the new body forces, in place by body levels (as the first bias's): +4.8 %
    // against the per-dof-lane sums below (r03 A/B, profiles/r03/ab_pred_levels.txt, under the
    // two-wave bound that lets it fit)
    subtree_levels<6, smpl::kNumBodyLevels - 2>(&L.Acc[0][0], nullptr, lane);
    auto corr = [&](int i) {
        const int bi = i < 6 ? 0 : (i - 6) / 3 + 1;
        return dt * (dot6(L.S[i], L.F[bi]) - dot6(L.S[i], L.Acc[bi]));
    };
    float c1 = corr(lane);
    float c2 = lane < NH ? corr(64 + lane) : 0.f;
    STAMP(PH_MID_SUBTREE);
    mid_lt(L, T, lane, c1, c2);
    STAMP(PH_MID_LT);
}

// ---------------------------------------------------------------------------------- TGS iterations
// he_sim_params.solver_type 1 (oracle/he_oracle_physics.c substep_tgs): the velocity-dependent bias of
// the next position iteration at the working velocity `vel` (L.u0), with the step's kinematics (S, V
// frames, own inertias Ib) -- bias_midpoint's second RNEA: the bodies' velocities and bias
// accelerations by pointer jumping, their forces, the subtree sums by body levels (L.Acc scratch: the
// contact phase's bounding spheres and patch radii are dead after the row set-up). Returns b_i = S_i . F
// for dof lane and dof 64 + lane (lanes < NH).
HE_DEV void tgs_bias_at(Lds& L, const BodyTopo& T, int lane, const he_sim_params& p, const float* vel, float& c1,
                        float& c2) {
    // in short phases through LDS (the body velocities V and joint velocities vj in the V / F words, dead
    // from the row set-up to the next kinematics), so that each phase's temporaries fit beside the
    // iterations' long-lived rows and columns
    const bool bl = lanes_body();
    const int b = bl ? lane : 0;
    const uint32_t jp = bl ? T.jump4[b] : 0xFFFFFFFFu;
    {  // joint velocities vj = S_b u_b and body velocities V = prefix of vj (+ the root's)
        float vj[6];
        joint_velocity(L, T, b, vel, vj);
        if (bl)
            for (int x = 0; x < 6; ++x) L.F[b][x] = vj[x];
        float V[6];
        for (int x = 0; x < 6; ++x) V[x] = vj[x];
        chain_prefix6(jp, lane, V);
        if (b != 0)
            for (int x = 0; x < 6; ++x) V[x] += vel[x];
        if (bl)
            for (int x = 0; x < 6; ++x) L.V[b][x] = V[x];
    }
    sync();
    __builtin_amdgcn_sched_barrier(0);
    {  // bias accelerations A = prefix of V x vj (+ the base's), then the body forces
        float A[6];
        {
            const f3 vxw = cross3(f3{vel[3], vel[4], vel[5]}, f3{vel[0], vel[1], vel[2]});
            if (b == 0) {
                A[0] = 0.f; A[1] = 0.f; A[2] = 0.f;
                A[3] = vxw.x - p.gravity[0]; A[4] = vxw.y - p.gravity[1]; A[5] = vxw.z - p.gravity[2];
            } else {
                crm(L.V[b], L.F[b], A);  // joint b's velocity-product term V_b x S_b u_b
            }
        }
        chain_prefix6(jp, lane, A);
        if (b != 0) {
            const f3 vxw = cross3(f3{vel[3], vel[4], vel[5]}, f3{vel[0], vel[1], vel[2]});
            A[3] += vxw.x - p.gravity[0]; A[4] += vxw.y - p.gravity[1]; A[5] += vxw.z - p.gravity[2];
        }
        float IA[6], IV[6], X[6], Vb[6];
        for (int x = 0; x < 6; ++x) Vb[x] = L.V[b][x];
        si_apply(L.Ib[b], A, IA);
        si_apply(L.Ib[b], Vb, IV);
        crf(Vb, IV, X);
        sync();
        if (bl)
            for (int x = 0; x < 6; ++x) L.Acc[b][x] = IA[x] + X[x];
    }
    sync();
    __builtin_amdgcn_sched_barrier(0);
    subtree_levels<6, smpl::kNumBodyLevels - 2>(&L.Acc[0][0], nullptr, lane);
    // the dofs' S and Acc rows through the phase's own view: their six addresses are invariant over
    // the iterations, and carried across them each came back from scratch in front of its read
    const Lds& Lt = phase_lds();
    const int ln = phase_lane();
    c1 = dot6(Lt.S[ln], Lt.Acc[dof_body(ln)]);
    c2 = lanes_hi() ? dot6(Lt.S[64 + ln], Lt.Acc[(64 + ln - 6) / 3 + 1]) : 0.f;
}

// the next position iteration's free motion: yh = D^-1/2 L^-T hs (kp (tgt - q) - c u - b) per dof (lane,
// then 64 + lane), forward substituted from the stored factor (kp parked in L.dforce during the step,
// c = hs kp + kd in L.coef, u the working velocity L.u0, b from tgs_bias_at)
HE_DEV void tgs_rhs(Lds& L, const BodyTopo& T, int lane, float hs, float c1, float c2) {
    using regla::NH;
    auto rhs = [&](int i, float b) {
        const bool jd = i >= 6;
        const int d = jd ? i - 6 : 0;
        const float drive = jd ? L.dforce[d] * (L.tgt[d] - L.q[d]) - L.coef[i] * L.u0[i] : 0.f;
        return hs * (drive - b);
    };
    float y1 = rhs(lane, c1);
    float y2 = lanes_hi() ? rhs(64 + lane, c2) : 0.f;
    __builtin_amdgcn_s_setprio(kPrioSerial);
    regla::solve_LT_vec_pipelined(L.Lp, T.dof_depth[lane], lanes_hi() ? T.dof_depth[64 + lane] : 0, y1, y2);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.yh[lane] = y1 * L.sDinv[lane];
    if (lanes_hi()) L.yh[64 + lane] = y2 * L.sDinv[64 + lane];
    sync();
}

// the working velocity's update by one iteration: u += L^-1 D^-1/2 (yh + extra), extra = Zh^T (the
// iteration's impulse change) reduced into lane = dof (0 without contact rows)
HE_DEV void tgs_velocity(Lds& L, const BodyTopo& T, int lane, float e1, float e2) {
    using regla::NH;
    float yl = (e1 + L.yh[lane]) * L.sDinv[lane];
    float y2 = lanes_hi() ? (e2 + L.yh[64 + lane]) * L.sDinv[64 + lane] : 0.f;
    __builtin_amdgcn_s_setprio(kPrioSerial);
    regla::solve_L_streamed(L.Lp + T.pack_start[lane], L.Lp + T.pack_start[lanes_hi() ? 64 + lane : 0], yl, y2);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.u0[lane] += yl;
    if (lanes_hi()) L.u0[64 + lane] += y2;
    sync();
}

// the iteration's implicit drive torque kp (tgt - q) - c u at its end velocity, accumulated per dof
// (lane, then 64 + lane): the reported drive force is the iterations' mean
HE_DEV void tgs_drive_acc(const Lds& L, int, float& f1, float& f2) {
    // the lane afresh: max(lane, 6) below is the drive terms' own index at the step's start, and shared
    // with it was parked in scratch through the rows' peak for this read
    const int lane = phase_lane();
    auto tq = [&](int i) {
        const int d = i - 6;
        return L.dforce[d] * (L.tgt[d] - L.q[d]) - L.coef[i] * L.u0[i];
    };
    if (lanes_joint_dof()) f1 += tq(lane >= 6 ? lane : 6);
    if (lanes_hi()) f2 += tq(64 + lane);
}

}  // namespace
