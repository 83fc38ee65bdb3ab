// he_phys_solve.h -- the solves and what follows them: the Gauss-Seidel sweeps (pgs_sweep_fix,
// pgs_sweep_tgs), Zh^T x into lane = dof (reduce_scatter_z, reduce_scatter_z_legs), what PGS and TGS
// share (ax_rows, warm_residual, PatchMask, patch_mask, patch_bound, Columns, prep_block,
// prep_columns, add_limit_force), the TGS position iterations (TgsStep, tgs_advance, tgs_drive_out,
// solve_tgs, solve_tgs_rows, tgs_free_iterations), the PGS solve and its velocity (solve_pgs,
// pgs_velocity, free_velocity, pgs_drive_out) and contact_forces_out.
// LDS: reads lam (the bound weights row_setup parked), cgap, rslot, tcnt, nlim, cbb, cx, yh, sDinv, Lp,
// u0, coef, uf, Q; writes lam (the impulses), nwc, u0 or uf, dforce, row_dirs (scaled), cf, and through
// tgs_advance everything integrate_bodies and the tgs_* helpers write. On entry: RowDesc and RowSystem
// of this substep in registers (row_setup, row_system) when there are rows; the step's factor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/humanoid_engine.h"
#include "he_math.h"
#include "he_phys_dynamics.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_phys_rows.h"
#include "he_phys_tree.h"
#include "he_regla.h"

namespace {

// One Gauss-Seidel sweep, branch-free: every row up to a compile-time class bound N (16, 32, 48,
// 63) by the row count, with no per-row row-count branch (a row-count exit every 4 rows); rows nr..N-1 are empty rows (zero columns and
// bound weights in every lane, zero cd and bounds in their own lanes: a +-0 change).
template <int R, int N, int M = MAXR>
HE_DEV void pgs_sweep_fix(regla::f2v& ch, float& dvec, float& lo, const regla::f2v (&ak)[M], int nr) {
    if constexpr (R < N) {
        if constexpr (R > 0 && R % 4 == 0) {  // a row-count exit every 4 rows
            if (R >= nr) return;
        }
        const float d = regla::rdlane(__builtin_amdgcn_fmed3f(ch.x, lo, ch.y), R);
        ch = __builtin_elementwise_fma(ak[R], regla::f2v{d, d}, ch);
        lo = fmaf(-ak[R].y, d, lo);
        dvec = regla::wrlane<R>(d, dvec);
        pgs_sweep_fix<R + 1, N, M>(ch, dvec, lo, ak, nr);
    }
}

// TGS (solver_type 1): the same sweep with the friction bound weights rebuilt per row from the lane's
// patch mask (2 VALU off the dependent chain) instead of a second register per row: the scaled
// columns, the rows' Zh and the sweep state stay in registers through the position iterations'
// triangular solves, bias passes and integrations
template <int R, int N, int M>
HE_DEV void pgs_sweep_tgs(regla::f2v& ch, float& dvec, float& lo, const float (&ap)[M], uint32_t mlo, uint32_t mhi,
                          float muw, int nr) {
    static_assert(N <= M, "the sweep's rows within the columns held");
    if constexpr (R < N) {
        if constexpr (R > 0 && R % 4 == 0) {  // a row-count exit every 4 rows
            if (R >= nr) return;
        }
        const float d = regla::rdlane(__builtin_amdgcn_fmed3f(ch.x, lo, ch.y), R);
        const int sel = __builtin_amdgcn_sbfe((int)(R < 32 ? mlo : mhi), R & 31, 1);
        const float wr = __int_as_float(sel & __float_as_int(muw));
        // scalar FMAs: a packed pair built from ap[R] makes the compiler load ap as overlapping
        // two-float vectors, which keeps the whole column array in scratch
        ch.x = fmaf(ap[R], d, ch.x);
        ch.y = fmaf(wr, d, ch.y);
        lo = fmaf(-wr, d, lo);
        dvec = regla::wrlane<R>(d, dvec);
        pgs_sweep_tgs<R + 1, N, M>(ch, dvec, lo, ap, mlo, mhi, muw, nr);
    }
}

// Zh^T x into lane = dof (lane i: sum over rows r of z_r[i] x_r; lanes < 11 also dof 64 + lane in e2): the
// same butterfly as reduce_scatter with the products formed as the first stage consumes them, so at
// most 32 + 8 of them are live at once (the TGS iterations run it beside the rows' Zh and columns)
// The products and the first two stages' sums run on the register pairs (v_pk_mul / v_pk_add: half the
// VALU of the scalar forms, the same IEEE results)
HE_DEV void reduce_scatter_z(const regla::ZVec& z, float x, int lane, float& e1, float& e2) {
    using regla::f2v;
    const f2v xx = f2v{x, x};
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; j += 2) {
        const f2v pa = z.p[j >> 1] * xx, pb = z.p[(j + 32) >> 1] * xx;
        float a0 = pa.x, b0 = pb.x, a1 = pa.y, b1 = pb.y;
        swap32(a0, b0);
        swap32(a1, b1);
        const f2v s = f2v{a0, a1} + f2v{b0, b1};
        v[j] = s.x;
        v[j + 1] = s.y;
    }
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        swap16(v[j], v[j + 16]);
        swap16(v[j + 1], v[j + 17]);
        const f2v s = f2v{v[j], v[j + 1]} + f2v{v[j + 16], v[j + 17]};
        v[j] = s.x;
        v[j + 1] = s.y;
    }
    rs_dpp<8, 0x140, 0xFF00FF00FF00FF00ull>(v);
    rs_dpp<4, 0x141, 0xF0F0F0F0F0F0F0F0ull>(v);
    rs_dpp<2, 0x4E, 0xCCCCCCCCCCCCCCCCull>(v);
    rs_dpp<1, 0xB1, 0xAAAAAAAAAAAAAAAAull>(v);
    e1 = v[0];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float a = 64 + j < NG ? ZV(z, 64 + j < NG ? 64 + j : 0) * x : 0.f;
        float b = 72 + j < NG ? ZV(z, 72 + j < NG ? 72 + j : 0) * x : 0.f;
        swap32(a, b);
        w[j] = a + b;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { swap16(w[j], w[j + 4]); w[j] += w[j + 4]; }
    rs_dpp<2, 0x140, 0xFF00FF00FF00FF00ull>(w);
    rs_dpp<1, 0x141, 0xF0F0F0F0F0F0F0F0ull>(w);
    w[0] += dpp<0x4E>(w[0]);
    w[0] += dpp<0xB1>(w[0]);
    e2 = __shfl(w[0], 4 * (lane & 15), W);
}
// Zh^T x over dofs 0..KZ-1 into lane = dof: the butterfly's stages inside each 32-lane half (lane bits
// 4 .. 0: the 32 values to one per lane), then the two halves' partial sums added (lane bit 5). Lanes
// >= KZ return 0 (e2 = 0: no dof past 63 is on the support). The same sum as reduce_scatter_z's in
// another association order: equal to the bit only under solve_tgs' leg-class precondition (at most
// 32 rows, and rows >= nr with x == 0 and a finite z, so that lanes 32..63 add exact zeros).
HE_DEV float reduce_scatter_z_legs(const regla::ZVec& z, float x) {
    using regla::f2v;
    const f2v xx = f2v{x, x};
    float v[KZ];
#pragma unroll
    for (int j = 0; j < KZ / 2; j += 2) {
        const f2v pa = z.p[j >> 1] * xx, pb = z.p[(j + KZ / 2) >> 1] * xx;
        float a0 = pa.x, b0 = pb.x, a1 = pa.y, b1 = pb.y;
        swap16(a0, b0);
        swap16(a1, b1);
        const f2v s = f2v{a0, a1} + f2v{b0, b1};
        v[j] = s.x;
        v[j + 1] = s.y;
    }
    rs_dpp<8, 0x140, 0xFF00FF00FF00FF00ull>(v);
    rs_dpp<4, 0x141, 0xF0F0F0F0F0F0F0F0ull>(v);
    rs_dpp<2, 0x4E, 0xCCCCCCCCCCCCCCCCull>(v);
    rs_dpp<1, 0xB1, 0xAAAAAAAAAAAAAAAAull>(v);
    float a = v[0], b = v[0];
    swap32(a, b);  // a: lanes < 32 their own half's sum, b: the other half's (lanes >= 32: swapped roles)
    const float e = a + b;
    return regla::lanes<0xFFFFFFFFull>() ? e : 0.f;
}

// ---------------------------------------------------------------------------------- the solves
// What the PGS and the TGS solve share. Each helper takes the values its caller has (TGS passes a
// readfirstlane'd row count, PGS the plain one); it chooses none.

// A x over the first NRW rows (lane c of acol holds A[r][c] = A[c][r]; x_r broadcast from lane r):
// four independent accumulation chains, broadcasts in blocks of 4
template <int NRW>
HE_DEV float ax_rows(const float (&acol)[MAXR], float x) {
    float wa[4] = {0.f, 0.f, 0.f, 0.f};
    regla::static_for<0, NRW, 4>([&](auto rc) {
        constexpr int r0 = decltype(rc)::value;
        float sv[4];
        regla::rdlane4<r0>(x, sv);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (r0 + q < NRW) wa[(r0 + q) & 3] = fmaf(acol[r0 + q < NRW ? r0 + q : 0], sv[q], wa[(r0 + q) & 3]);
    });
    return (wa[0] + wa[1]) + (wa[2] + wa[3]);
}
// the warm start's residual share A x by row-count class (wave-uniform; rows >= nrows hold no impulse)
HE_DEV float warm_residual(const float (&acol)[MAXR], float x, int nrows) {
    if (nrows <= 16) return ax_rows<16>(acol, x);
    else if (nrows <= 32) return ax_rows<32>(acol, x);
    else if (nrows <= 48) return ax_rows<48>(acol, x);
    else return ax_rows<MAXR>(acol, x);
}

// a friction row's patch: its normal rows n0 .. n0 + pc - 1 as a 64-bit lane mask (other rows: 0)
struct PatchMask { uint32_t mlo, mhi; int n0; };
HE_DEV PatchMask patch_mask(const Lds& L, const RowDesc& r, int lane) {
    PatchMask m{0u, 0u, 0};
    const bool isn = r.kind == 0;
    if (r.act && !isn) {
        const int pc = r.rb1 == -1 ? L.tcnt[r.rb0] : 1;
        const uint64_t pm = ((1ull << pc) - 1ull) << (lane - (r.kind - 1) - pc);
        m.mlo = (uint32_t)pm;
        m.mhi = (uint32_t)(pm >> 32);
    }
    m.n0 = r.act && !isn ? (int)__builtin_ctzll(((uint64_t)m.mhi << 32) | m.mlo) : 0;
    return m;
}
// a friction row's bound: muw x the patch's normal impulses lv (<= 4 rows)
HE_DEV float patch_bound(float lv, const PatchMask& m, float muw) {
    float bnd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = __shfl(lv, (m.n0 + j) & (W - 1), W);
        const int bit = m.n0 + j;
        const bool in = bit < 32 ? ((m.mlo >> (bit & 31)) & 1u) : ((m.mhi >> (bit & 31)) & 1u);
        bnd += in ? v : 0.f;
    }
    return bnd * muw;
}

// The sweep's columns -A[r][lane] / A[lane][lane] of a row-count class of NC rows. PACK: each with
// its row's bound weight as a register pair (pgs_sweep_fix); else the columns alone, the weights
// rebuilt per row (pgs_sweep_tgs: NC registers fewer).
template <int NC, bool PACK>
struct Columns {
    float ap[PACK ? 1 : NC];
    regla::f2v ak[PACK ? NC : 1];
};
template <int R0, int NC, bool PACK>
HE_DEV void prep_block(Columns<NC, PACK>& c, const float (&acol)[MAXR], float ninvd, const PatchMask& m, float muw) {
#pragma unroll
    for (int r = R0; r < (R0 + 16 < NC ? R0 + 16 : NC); ++r) {
        if constexpr (PACK) {
            const int sel = __builtin_amdgcn_sbfe((int)(r < 32 ? m.mlo : m.mhi), r & 31, 1);
            c.ak[r] = regla::f2v{acol[r] * ninvd, __int_as_float(sel & __float_as_int(muw))};
        } else {
            c.ap[r] = acol[r] * ninvd;
        }
    }
}
// the columns of the row-count class's rows only (the branch-free sweep reads no row past its
// class): blocks of 16 rows, each behind a wave-uniform row-count test
template <int NC, bool PACK>
HE_DEV void prep_columns(Columns<NC, PACK>& c, const float (&acol)[MAXR], float ninvd, const PatchMask& m, float muw,
                         int nrb) {
    prep_block<0>(c, acol, ninvd, m, muw);
    if (nrb > 16) prep_block<16>(c, acol, ninvd, m, muw);
    if constexpr (NC > 32) {
        if (nrb > 32) prep_block<32>(c, acol, ninvd, m, muw);
        if (nrb > 48) prep_block<48>(c, acol, ninvd, m, muw);
    }
}

// The joint-limit force added to dof_force (the joint's solver force, drive and limit together;
// oracle/he_oracle_physics.c): limit slot c (one per joint, row c) adds g lambda / dt over its
// joint's dofs, g = its row (kept in the contact-position words). lam: the lane's row impulse.
HE_DEV void add_limit_force(Lds& L, int lane, float lam, float dt) {
    const int nl = __builtin_amdgcn_readfirstlane(L.nlim);
    if (lane < nl) {
        const int d0 = 3 * ((L.cbb[lane < MAXC ? lane : 0] & 0xFF) - 1);
        const float lf = lam / dt;
        L.dforce[d0] += L.cx[lane < MAXC ? lane : 0][0] * lf;
        L.dforce[d0 + 1] += L.cx[lane < MAXC ? lane : 0][1] * lf;
        L.dforce[d0 + 2] += L.cx[lane < MAXC ? lane : 0][2] * lf;
    }
}

// The TGS position iterations' constants and running sums (oracle substep_tgs): K iterations of
// hs = dt / K on this step's factor and contact set
struct TgsStep {
    int K;
    float hs, damp;
    bool last;       // the policy step's last substep
    float tf1, tf2;  // the iterations' drive torques, summed per dof (lane, 64 + lane): the last substep only
};
// What follows a position iteration's velocity update: its drive torques, the positions by hs (the
// last iteration: the step's output velocity), then (not the last) the next iteration's bias and
// free motion
// WIDE (the 63-row class, whose columns leave no register for an address held over the iterations):
// the phases' lane and LDS view taken afresh per iteration, so that the integration's, the bias
// RNEA's and its subtree levels' per-lane addresses are rebuilt instead of fetched from scratch one
// by one; the <= 32-row class and the free iterations keep theirs in registers.
template <bool EXT, bool WIDE = false>
HE_DEV void tgs_advance(Lds& L0, const BodyTopo& T0, const he_sim_params& p, int lane0, int it, TgsStep& ts, Stamps& st) {
    Lds& L = WIDE ? phase_lds() : L0;
    const BodyTopo& T = WIDE ? L.T : T0;
    const int lane = WIDE ? phase_lane() : lane0;
    const bool lastit = it + 1 == ts.K;
    // the drive sums feed tgs_drive_out alone, which only a reporting step runs (wave-uniform)
    if (reports(ts.last)) tgs_drive_acc(L, lane, ts.tf1, ts.tf2);
    integrate_bodies(L, T, lane, p, ts.hs, ts.damp, L.u0, lastit, lastit && !ts.last);
    __builtin_amdgcn_sched_barrier(0);
    STAMP(PH_INTEGRATE);
    if (!lastit) {
        // the velocity-dependent bias: re-evaluated at the start of every second iteration (oracle
        // g_bias_every: as stable as every iteration at half the passes), else the one in L.uf
        if (p.bias_midpoint && ((it + 1) % kTgsBiasEvery) == 0) {
            float b1, b2;
            tgs_bias_at(L, T, lane, p, L.u0, b1, b2);
            if constexpr (EXT) {  // the step's kinematics are frozen: Q holds over the iterations
                b1 -= L.Q[lane];
                if (lane < regla::NH) b2 -= L.Q[64 + lane];
            }
            L.uf[lane] = b1;
            if (lane < regla::NH) L.uf[64 + lane] = b2;
        }
        const float c1 = L.uf[lane];
        const float c2 = lane < regla::NH ? L.uf[64 + lane] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
        STAMP(PH_TGS_BIAS);
        tgs_rhs(L, T, lane, ts.hs, c1, c2);
        __builtin_amdgcn_sched_barrier(0);
        STAMP(PH_TGS_RHS);
    }
}
// the reported drive force, the iterations' mean (the joint-limit force is added by the caller)
HE_DEV void tgs_drive_out(Lds& L, int lane, const TgsStep& ts) {
    // the iteration count converted here, from its SGPR: (float)K held in a VGPR since the step's start
    // was parked in scratch across the iterations and fetched back in front of each division
    const float kf = (float)opaque_s(ts.K);
    if (lane >= 6) L.dforce[lane >= 6 ? lane - 6 : 0] = ts.tf1 / kf;
    if (lane < regla::NH) L.dforce[58 + lane] = ts.tf2 / kf;
    sync();
}

// The TGS position iterations for one row-count class of columns held in registers (<= 32 rows: a
// standing body's 28; more: the 63-row form), so that the common case keeps 31 registers free for
// the phases between the sweeps. Each iteration is one Gauss-Seidel sweep on the accumulated
// impulses, started from them plus the previous iteration's change (the first: the cached change of
// the previous step, g0 with residual w0), against J u of the iteration's free velocity and the bias
// of the row's separation, advanced by hs J_r u after each iteration. nrb: the row count as a
// scalar, from the caller (a second readfirstlane here: +11 VGPR spills). Reads lam (the bound
// weights row_setup parked). Returns the step's accumulated impulse of the lane's row.
//
// The leg class (legs_it): the iterations' Zh products over dofs 0..KZ-1 when every row's support is
// in the legs, a wave-uniform branch inside the one instantiation (its own instantiation, with Zh's
// other 44 registers dead, ran the standing body as fast but every other env 1-2 % slower: the
// second copy of the loop body; profiles/r06/ab_tgs_legs.txt). reduce_scatter_z_legs sums in another
// association order than reduce_scatter_z; the two agree to the bit (which
// test_leg_class_leaves_the_step_unchanged asserts) only because the terms the leg form leaves out
// are exact zeros. Precondition: NC == 32 (no row sits on lanes 32..63), and every lane >= nr
// carries dl == 0 (its `act` is false) with a finite z, so that its products are +-0 and not NaN.
// A change to how the inactive lanes are handled has to keep both.
// Under legs_it the iterations read ZV(s.z, i) for i < KZ only (reduce_scatter_z_legs, zdot_lanes<KZ>):
// RowSystem::zshort leaves the registers past them unwritten, so nothing here may read them without
// excluding legs_it first (the wide instantiation never sees zshort set: it implies nr <= 32).
template <int NC, bool EXT>
HE_DEV float solve_tgs(Lds& L, const BodyTopo& T, const he_sim_params& p, int lane, int nr, const RowDesc& r,
                       const RowSystem& s, int nrb, float g0, float w0, TgsStep& ts, Stamps& st) {
    using regla::NH;
    const bool act = r.act;
    const float hs = ts.hs, dt = p.dt;
    const float invd = 1.0f / (act ? s.diag + 1e-12f : 1.f);
    const float ninvd = -invd;
    const bool legs_it = NC == 32 && s.legs;
    // up to 32 rows packed with their bound weights as the PGS sweep's, past 32 the weights rebuilt
    // per row (63 registers fewer)
    constexpr bool PACK = NC <= 32;
    Columns<NC, PACK> col;
    const bool isn = r.kind == 0;
    const float muw = L.lam[lane];  // the friction bound weight parked by the row set-up
    const PatchMask pm = patch_mask(L, r, lane);
    prep_columns(col, s.acol, ninvd, pm, muw, nrb);
    auto gbias = [&](float g) {
        return g >= 0.f ? g / hs : fmaxf(p.baumgarte * g / dt, -p.max_depenetration_velocity);
    };
    const float kInf = __builtin_inff();
    float sep = act && isn ? L.cgap[row_slot_again(act)] : 0.f;  // the row's separation (a limit row: its angle gap)
    float bb = act && isn ? gbias(sep) : 0.f;     // its bias (brow holds it)
    float applied = 0.f;                           // the impulse already in the working velocity
    float lamv = g0;
    float dl = 0.f;
    float cd = act ? -w0 * invd : 0.f;
    float bnd = patch_bound(lamv, pm, muw);
    float lo = isn ? -lamv : -bnd - lamv;
    float hi = isn ? kInf : bnd - lamv;
    const int nru = __builtin_amdgcn_readfirstlane(nr);
    for (int it = 0; it < ts.K; ++it) {
        float dvec = 0.f;
        // the row count through an opaque copy per sweep (see solve_pgs)
        int nrs = nru;
        asm volatile("" : "+s"(nrs));
        regla::f2v ch = {cd, hi};
        __builtin_amdgcn_s_setprio(kPrioSerial);
        if constexpr (PACK) {
            if (nrs <= 16) pgs_sweep_fix<0, 16, NC>(ch, dvec, lo, col.ak, nrs);
            else pgs_sweep_fix<0, 32, NC>(ch, dvec, lo, col.ak, nrs);
        } else {
            if (nrs <= 48) pgs_sweep_tgs<0, 48, NC>(ch, dvec, lo, col.ap, pm.mlo, pm.mhi, muw, nrs);
            else pgs_sweep_tgs<0, MAXR, NC>(ch, dvec, lo, col.ap, pm.mlo, pm.mhi, muw, nrs);
        }
        __builtin_amdgcn_s_setprio(kPrioDefault);
        STAMP(PH_PGS);
        cd = ch.x;
        lamv += dvec;
        dl = act ? lamv - applied : 0.f;  // this iteration's impulse change
        applied = lamv;
        const float v = act ? -cd * (s.diag + 1e-12f) - bb : 0.f;  // J_r u after the sweep
        float e1, e2;  // Zh^T dl, lane = dof (and 64 + lane): also the next start's A dl = Zh (Zh^T dl)
        __builtin_amdgcn_sched_barrier(0);  // phase fences: each phase's temporaries beside the
        if (legs_it) {                          // loop's long-lived rows and columns, not several
            e1 = reduce_scatter_z_legs(s.z, dl);
            e2 = 0.f;
        } else {
            reduce_scatter_z(s.z, dl, lane, e1, e2);
        }
        __builtin_amdgcn_sched_barrier(0);
        e2 = lane < NH ? e2 : 0.f;
        tgs_velocity(L, T, lane, e1, e2);  // the working velocity: u += L^-1 D^-1/2 (yh + Zh^T dl)
        __builtin_amdgcn_sched_barrier(0);
        STAMP(PH_DU_SOLVE);
        if (isn) sep += hs * v;
        const bool lastit = it + 1 == ts.K;
        tgs_advance<EXT, (NC > 32)>(L, T, p, lane, it, ts, st);
        __builtin_amdgcn_sched_barrier(0);
        if (!lastit) {
            // the next sweep's start about lambda = applied + dl: w = J u + zh . yh + bias(sep) + A dl,
            // with zh . yh + A dl = zh . (yh + Zh^T dl), one dot product
            const float yhl = L.yh[lane] + e1;
            float zy;
            if (legs_it) {
                zy = zdot_lanes<KZ>(s.z, yhl, 0.f);
            } else {
                const float yh2 = lane < NH ? L.yh[64 + lane] + e2 : 0.f;
                zy = zdot_lanes(s.z, yhl, yh2);
            }
            bb = act && isn ? gbias(sep) : 0.f;
            lamv = applied + dl;
            cd = act ? -(v + zy + bb) * invd : 0.f;
            bnd = patch_bound(lamv, pm, muw);
            lo = isn ? -lamv : -bnd - lamv;
            hi = isn ? kInf : bnd - lamv;
            STAMP(PH_TGS_NEXT);
        }
    }
    return lamv;
}
// The TGS solve with contact rows: the first iteration starts from the cached (previous step's)
// impulses' per-iteration share g0, its residual w = brow + A g0; then the iterations by row-count
// class; the cache and the reported forces take the step's accumulated impulses. Writes lam, nwc,
// dforce (drive and joint-limit force).
template <bool EXT>
HE_DEV float solve_tgs_rows(Lds& L, const BodyTopo& T, const he_sim_params& p, int lane, int nr, const RowDesc& r,
                            const RowSystem& s, TgsStep& ts, Stamps& st) {
    const int nrb = __builtin_amdgcn_readfirstlane(nr);
    const float g0 = r.lam0 * (1.0f / (float)opaque_s(ts.K));  // K from its SGPR (tgs_drive_out)
    float w0 = s.brow;
    if (__ballot(g0 != 0.f)) w0 += warm_residual(s.acol, g0, nrb);  // wave-uniform
    float lamv;
    if (__builtin_expect(nrb <= 32, 1)) lamv = solve_tgs<32, EXT>(L, T, p, lane, nr, r, s, nrb, g0, w0, ts, st);
    else lamv = solve_tgs<MAXR, EXT>(L, T, p, lane, nr, r, s, nrb, g0, w0, ts, st);
    L.lam[lane] = r.act ? lamv : 0.f;
    if (lane == 0) L.nwc = p.warm_start ? nr : 0;
    // dforce is stored from the launch's last step alone; the next step's drive_terms overwrites it
    if (reports(ts.last)) {
        tgs_drive_out(L, lane, ts);
        add_limit_force(L, lane, lamv, p.dt);  // limit row c = slot c
    }
    sync();
    return lamv;
}
// TGS without contact rows: the iterations' drives and bias only
template <bool EXT>
HE_DEV void tgs_free_iterations(Lds& L, const BodyTopo& T, const he_sim_params& p, int lane, TgsStep& ts, Stamps& st) {
    for (int it = 0; it < ts.K; ++it) {
        tgs_velocity(L, T, lane, 0.f, 0.f);
        STAMP(PH_DU_SOLVE);
        tgs_advance<EXT>(L, T, p, lane, it, ts, st);
    }
    if (reports(ts.last)) tgs_drive_out(L, lane, ts);
    else sync();  // the ordering point tgs_drive_out ends on
}

// Projected Gauss-Seidel over the rows (pgs_sweep_fix): lane r keeps its unconstrained change, its
// impulse and its bounds. Reads lam (the bound weights row_setup parked), then writes the solve's
// impulses there with nwc: the next solve's warm start and the reported forces. Returns the lane's
// row impulse.
HE_DEV float solve_pgs(Lds& L, const he_sim_params& p, int lane, int nr, const RowDesc& r, const RowSystem& s, Stamps& st) {
    const bool act = r.act;
    const float lam0 = r.lam0;
    const float invd = 1.0f / (act ? s.diag + 1e-12f : 1.f);
    // residual at the warm start: w = brow + A lambda0
    float w0 = s.brow;
    if (__ballot(lam0 != 0.f)) w0 += warm_residual(s.acol, lam0, nr);  // wave-uniform
    float lamv = lam0;
    float cd = act ? -w0 * invd : 0.f;
    const float ninvd = -invd;
    const bool isn = r.kind == 0;
    const float muw = L.lam[lane];
    const PatchMask pm = patch_mask(L, r, lane);
    // a friction row's bound at the warm start
    float bnd = 0.f;
    if (__ballot(lam0 != 0.f)) bnd = patch_bound(lam0, pm, muw);
    Columns<MAXR, true> col;
    prep_columns(col, s.acol, ninvd, pm, muw, __builtin_amdgcn_readfirstlane(nr));
    const float kInf = __builtin_inff();
    float lo = isn ? -lamv : -bnd - lamv;
    float hi = isn ? kInf : bnd - lamv;
    const int nru = __builtin_amdgcn_readfirstlane(nr);
    STAMP(PH_PGS_SETUP);  // the solve's set-up (warm-start residual, bounds, scaled columns) apart from its sweeps
    __builtin_amdgcn_s_setprio(kPrioSerial);
    const float tol = p.solver_tolerance;
    for (int it = 0; it < p.solver_iterations; ++it) {
        float dvec = 0.f;
        // the row count through an opaque copy per sweep: the 63 early-exit compares stay
        // scalar compares in the sweep instead of being hoisted out of the loop as 63
        // lane-mask pairs (SGPR spills)
        int nrs = nru;
        asm volatile("" : "+s"(nrs));
        regla::f2v ch = {cd, hi};
        if (nrs <= 16) pgs_sweep_fix<0, 16>(ch, dvec, lo, col.ak, nrs);
        else if (nrs <= 32) pgs_sweep_fix<0, 32>(ch, dvec, lo, col.ak, nrs);
        else if (nrs <= 48) pgs_sweep_fix<0, 48>(ch, dvec, lo, col.ak, nrs);
        else pgs_sweep_fix<0, MAXR>(ch, dvec, lo, col.ak, nrs);
        cd = ch.x;
        hi = ch.y;
        // the bound at the sweep's end: B = hi + lambda(start); then the bounds about the new impulse
        const float bn = hi + lamv;
        lamv += dvec;
        lo = isn ? -lamv : -bn - lamv;
        hi = isn ? kInf : bn - lamv;
        // converged (optional, solver_tolerance > 0): no row's velocity moved by more than
        // the tolerance in this sweep, |d lambda_r| A_rr (oracle: the same test)
        if (tol > 0.f && __ballot(act && fabsf(dvec) * s.diag > tol) == 0ull) break;
    }
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.lam[lane] = act ? lamv : 0.f;
    if (lane == 0) L.nwc = p.warm_start ? nr : 0;  // warm_start 0: every substep's solve is cold
    sync();
    STAMP(PH_PGS);
    return lamv;
}

// PGS: uf = u0 + L^-1 D^-1/2 (yh + Zh^T lambda). Lane r scales its row by lambda_r, a wave
// reduce-scatter sums the 75 columns into lane = dof, then one L^-1 sweep. No sync at its end (the
// next reader follows one).
HE_DEV void pgs_velocity(Lds& L, const BodyTopo& T, int lane, const regla::ZVec& z, float lamv) {
    using regla::NH;
    __builtin_amdgcn_s_setprio(kPrioDefault);
    float v64[64], v16[16];
#pragma unroll
    for (int i = 0; i < 64; ++i) v64[i] = ZV(z, i) * lamv;
#pragma unroll
    for (int i = 0; i < 16; ++i) v16[i] = 64 + i < NG ? ZV(z, 64 + i < NG ? 64 + i : 0) * lamv : 0.f;
    float yl = reduce_scatter<64>(v64);
    float y2 = __shfl(reduce_scatter<16>(v16), 4 * (lane & 15), W);
    yl = (yl + L.yh[lane]) * L.sDinv[lane];
    y2 = lane < NH ? (y2 + L.yh[64 + lane]) * L.sDinv[64 + lane] : 0.f;
    float r1[regla::kRowRegs], r2[regla::kRowRegs];
    load_rows(L, T, lane, r1, r2);
    regla::solve_L_rows<0>(r1, r2, yl, y2);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    L.uf[lane] = L.u0[lane] + yl;
    if (lane < NH) L.uf[64 + lane] = L.u0[64 + lane] + y2;
}
// PGS without contact rows: uf = u0 + L^-1 D^-1/2 yh
HE_DEV void free_velocity(Lds& L, const BodyTopo& T, int lane) {
    using regla::NH;
    float yl = L.yh[lane] * L.sDinv[lane];
    float y2 = lane < NH ? L.yh[64 + lane] * L.sDinv[64 + lane] : 0.f;
    float r1[regla::kRowRegs], r2[regla::kRowRegs];
    load_rows(L, T, lane, r1, r2);
    regla::solve_L_rows<0>(r1, r2, yl, y2);
    L.uf[lane] = L.u0[lane] + yl;
    if (lane < NH) L.uf[64 + lane] = L.u0[64 + lane] + y2;
    sync();
}
// PGS: the drive force actually applied (the reported one is the last substep's), plus the
// joint-limit force
HE_DEV void pgs_drive_out(Lds& L, int lane, int nr, float dt) {
    for (int i = lane; i < NG; i += W)
        if (i >= 6) L.dforce[i - 6] -= L.coef[i] * (L.uf[i] - L.u0[i]);
    sync();
    if (nr > 0) add_limit_force(L, lane, L.lam[lane], dt);
    sync();
}

// Reported contact forces (net linear contact impulse per body / dt), lane = body: the output is the
// last substep's, so the earlier substeps skip them (gen_contacts zeroes cf, and row_setup writes
// row_dirs, in that substep alone). Turns row_dirs into the per-row linear impulses (the stored directions x lambda).
HE_DEV void contact_forces_out(Lds&, int lane, int nc, bool act, float lamv, float dt) {
    Lds& L = phase_lds();  // the step's LDS base does not survive the iterations in a register
    float* fr = row_dirs(L);
    if (act) {
        fr[3 * lane] *= lamv;
        fr[3 * lane + 1] *= lamv;
        fr[3 * lane + 2] *= lamv;
    }
    sync();
    if (lane < NB) {
        // the body's own terrain rows (its patch: a contiguous row range, in row order), then
        // the self-pair rows with their sign; the same summation order as over all rows
        float F3[3] = {0.f, 0.f, 0.f};
        const int tn = L.tcnt[lane];
        const int r0 = tn > 0 ? L.srow0[L.tbase[lane]] : 0;
        const int rn = tn == 0 ? 0 : tn + (tn >= 2 ? 3 : 2);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            if (k < rn) {
                const int r = r0 + k;
                for (int x = 0; x < 3; ++x) F3[x] += fr[3 * r + x];
            }
        }
        const int nterr = __builtin_amdgcn_readfirstlane(L.nterr);
        for (int c = nterr; c < nc; ++c) {  // wave-uniform bounds
            const int cb = L.cbb[c];
            const float sg = ((cb & 0xFF) == lane ? 1.f : 0.f) - ((cb >> 8) - 2 == lane ? 1.f : 0.f);
            const int r = L.srow0[c];
            for (int k = 0; k < 3; ++k)
                for (int x = 0; x < 3; ++x) F3[x] += sg * fr[3 * (r + k) + x];
        }
        L.cf[lane][0] = F3[0] / dt; L.cf[lane][1] = F3[1] / dt; L.cf[lane][2] = F3[2] / dt;
    }
    sync();
}

}  // namespace
