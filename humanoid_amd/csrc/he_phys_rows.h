// he_phys_rows.h -- from the contact slots to the rows' system in registers: the tangent basis
// (friction_basis), J^T on the matrix cores (GroupBodies, block_bodies, zrows_block, zrows_mfma), the
// rows' scalings and dot products (scale_rows, zdot_lds, znorm2, zdot_lanes) with the leg class's
// constants, the Delassus tiles (delassus_mfma48, delassus_mfma), then build_rows, RowDesc,
// row_slot_again, row_setup, RowSystem and row_system.
// LDS: reads the slots (cx, cn, cgap, cbb, ckey), tbase, tcnt, S, u0, yh, sDinv, Lp, wckey, nwc,
// T.anc_mask; writes srow0, rslot, rkind, F and patch_radius (the patches), wckey, lam (the bound
// weights) and row_dirs. On entry: gen_contacts' slots, the step's factor (Lp, sDinv, yh), and the
// previous solve's impulse of the lane in a register (lam_prev).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/humanoid_engine.h"
#include "he_math.h"
#include "he_phys_contacts.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_regla.h"
#include "he_smpl_topo.h"

namespace {

HE_DEV void friction_basis(f3 n, f3& t1, f3& t2) {
    f3 a = fabsf(n.x) > 0.9f ? f3{0.f, 1.f, 0.f} : f3{1.f, 0.f, 0.f};
    float d = dot3(a, n);
    t1 = a - n * d;
    t1 = t1 * (1.0f / norm3(t1));
    t2 = cross3(n, t1);
}

// ---- contact-row helpers (rows phase)
// bodies touched by dof group g (4 dofs), as a mask over bodies
struct GroupBodies {
    uint32_t m[(NG + 3) / 4];
    constexpr GroupBodies() : m() {
        for (int g = 0; g < (NG + 3) / 4; ++g) {
            m[g] = 0u;
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < NG) m[g] |= 1u << smpl::kDofBody[4 * g + k];
        }
    }
};
constexpr GroupBodies kGroupBodiesT{};
constexpr const uint32_t* kGroupBodies = kGroupBodiesT.m;

// z = J_r^T on the matrix cores: C[i][r] = S_i . u_r with u_r = (rho, dd) of row r (lane r), as
// v_mfma_f32_32x32x2_f32 tiles over the dof blocks of 32 that hold a live body (A = S from LDS, B =
// the rows' 6-vectors redistributed by one permlane32 swap per k step). The two row tiles of a
// block are paired by v_permlane32_swap into "lane r holds z[r][i]" (ZVec); then each dof takes its
// body's sign for the row (+1 on the first contact body's chain, -1 on the second's, 0 elsewhere).
constexpr uint32_t block_bodies(int D) {
    uint32_t m = 0;
    for (int i = 32 * D; i < 32 * D + 32 && i < NG; ++i) m |= 1u << (i < 6 ? 0 : (i - 6) / 3 + 1);
    return m;
}
template <int D, int DN = (NG + 31) / 32>  // dof blocks D .. DN - 1
HE_DEV void zrows_block(regla::ZVec& z, uint32_t lb, const float (&b0)[3], const float (&b1)[3], const Lds& L, int l31,
                        int kh, bool rows32) {
    if constexpr (D < DN && 32 * D < NG) {
        if (lb & block_bodies(D)) {
            float aS[3];
            const int j = 32 * D + l31;
#pragma unroll
            for (int st = 0; st < 3; ++st) aS[st] = j < NG ? L.S[j < NG ? j : 0][2 * st + kh] : 0.f;
            f32x16 t0 = {}, t1 = {};
#pragma unroll
            for (int st = 0; st < 3; ++st) t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aS[st], b0[st], t0, 0, 0, 0);
            if (!rows32) {  // rows 32-63 exist (wave-uniform)
#pragma unroll
                for (int st = 0; st < 3; ++st) t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aS[st], b1[st], t1, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = 32 * D + (v & 3) + 8 * (v >> 2);
                float a = t0[v], b = t1[v];
                swap32(a, b);  // a: z[lane][i], b: z[lane][i + 4]
                if (i < NG) ZV(z, i < NG ? i : 0) = a;
                if (i + 4 < NG) ZV(z, i + 4 < NG ? i + 4 : 0) = b;
            }
        } else {
#pragma unroll
            for (int i = 32 * D; i < 32 * D + 32 && i < NG; ++i) ZV(z, i) = 0.f;
        }
        zrows_block<D + 1, DN>(z, lb, b0, b1, L, l31, kh, rows32);
    }
}
// zshort (wave-uniform, RowSystem::zshort): only dofs 0..KZ-1 are written, the block of the legs' dofs
// with the signs of its bodies; z past them stays unwritten, for a solve that reads none of it. The
// registers that are written get the full form's instructions on the full form's operands.
constexpr int KZ = 32;  // the leg class's dofs (below: kLegBodies)
HE_DEV void zrows_mfma(regla::ZVec& z, uint32_t lb, uint32_t anc0, uint32_t anc1, f3 rho, f3 dd, const Lds& L,
                       int lane, bool rows32, bool zshort) {
    const int l31 = lane & 31, kh = lane >> 5;
    float b0[3], b1[3];
    {
        const float u[6] = {rho.x, rho.y, rho.z, dd.x, dd.y, dd.z};
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            float x = u[2 * st], y = u[2 * st + 1];
            swap32(x, y);  // x: B operand of rows 0-31, y: of rows 32-63
            b0[st] = x;
            b1[st] = y;
        }
    }
    auto sign = [&](int B) { return (float)((anc0 >> B) & 1u) - (float)((anc1 >> B) & 1u); };
    constexpr int BZ = (KZ - 1 - 6) / 3 + 2;  // the bodies of dofs 0..KZ-1
    static_assert(KZ % 32 == 0 && KZ > 6 && BZ <= NB, "the short form is whole dof blocks");
    zrows_block<0, KZ / 32>(z, lb, b0, b1, L, l31, kh, rows32);
    float sg[NB];
#pragma unroll
    for (int B = 0; B < BZ; ++B) sg[B] = sign(B);
#pragma unroll
    for (int i = 0; i < KZ; ++i) ZV(z, i) *= sg[i < 6 ? 0 : (i - 6) / 3 + 1];
    if (!zshort) {
        zrows_block<KZ / 32>(z, lb, b0, b1, L, l31, kh, rows32);
#pragma unroll
        for (int B = BZ; B < NB; ++B) sg[B] = sign(B);
#pragma unroll
        for (int i = KZ; i < NG; ++i) ZV(z, i) *= sg[i < 6 ? 0 : (i - 6) / 3 + 1];
    }
}

template <int I, int N = NG>
HE_DEV void scale_rows(regla::ZVec& z, float sdl, float sdl2) {
    if constexpr (I < N) {
        ZV(z, I) *= I < 64 ? regla::rdlane(sdl, I < 64 ? I : 0) : regla::rdlane(sdl2, I >= 64 ? I - 64 : 0);
        scale_rows<I + 1, N>(z, sdl, sdl2);
    }
}
// the rows' dot products over the register pairs (dof i into partial sum i mod 4) over dofs 0..N-1:
// sum_i a_r[i] u_i with u read from LDS (J_r u0), and |zh_r|^2
template <int N>
HE_DEV float zdot_lds(const regla::ZVec& z, const float* u) {
    float bacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const regla::f2v uk = *reinterpret_cast<const regla::f2v*>(&u[2 * k]);
        regla::f2v acc = regla::f2v{bacc[(2 * k) & 3], bacc[(2 * k + 1) & 3]};
        acc = __builtin_elementwise_fma(z.p[k], uk, acc);
        bacc[(2 * k) & 3] = acc.x;
        bacc[(2 * k + 1) & 3] = acc.y;
    }
    if constexpr (N & 1) bacc[(N - 1) & 3] = fmaf(ZV(z, N - 1), u[N - 1], bacc[(N - 1) & 3]);
    return (bacc[0] + bacc[1]) + (bacc[2] + bacc[3]);
}
template <int N>
HE_DEV float znorm2(const regla::ZVec& z) {
    float dacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        regla::f2v acc = regla::f2v{dacc[(2 * k) & 3], dacc[(2 * k + 1) & 3]};
        acc = __builtin_elementwise_fma(z.p[k], z.p[k], acc);
        dacc[(2 * k) & 3] = acc.x;
        dacc[(2 * k + 1) & 3] = acc.y;
    }
    if constexpr (N & 1) dacc[(N - 1) & 3] = fmaf(ZV(z, N - 1), ZV(z, N - 1), dacc[(N - 1) & 3]);
    return (dacc[0] + dacc[1]) + (dacc[2] + dacc[3]);
}

// zh_r . y with y_i broadcast from lane i (yl: dofs 0..63, y2: dofs 64..74 on lanes 0..10): the
// readlanes in blocks of four SGPRs (one hazard nop per block), the products on the register pairs
// (v_pk_fma: half the VALU), the four partial sums of the scalar form (dof i into sum i mod 4),
// so the result is that form's to the bit
// over dofs 0..N-1: N = NG, or the leg class's KZ (below), bit for bit the full form when Zh is zero
// past them (its dropped terms are fma(0, y, s) = s)
template <int N = NG>
HE_DEV float zdot_lanes(const regla::ZVec& z, float yl, float y2) {
    using regla::f2v;
    f2v a = f2v{0.f, 0.f}, b = f2v{0.f, 0.f};
    regla::static_for<0, N, 4>([&](auto ic) {
        constexpr int i0 = decltype(ic)::value;
        float sv[4];
        if constexpr (i0 < 64) regla::rdlane4<i0>(yl, sv);
        else regla::rdlane4<i0 - 64>(y2, sv);
        a = __builtin_elementwise_fma(z.p[i0 >> 1], f2v{sv[0], sv[1]}, a);
        if constexpr (i0 + 3 < N) b = __builtin_elementwise_fma(z.p[(i0 >> 1) + 1], f2v{sv[2], sv[3]}, b);
        else if constexpr (i0 + 2 < N) b.x = fmaf(ZV(z, i0 + 2), sv[2], b.x);
    });
    return (a.x + a.y) + (b.x + b.y);
}
// The rows' support inside the root and the two legs (bodies 0..8: dofs 0..29, the DFS prefix; a body
// standing or walking on its feet): Zh is zero past dof 29, so the iterations' products run over the
// first KZ = 32 dofs (dofs 30, 31 exact zeros) with Zh's other 44 registers dead. PhysArgs.full_dofs
// (HE_TGS_LEGS=0 in the environment) turns the class off at run time.
constexpr uint32_t kLegBodies = 0x1FFu;  // KZ: above zrows_mfma
static_assert(smpl::kNB > 9, "the leg prefix is bodies 0..8");

// Delassus operator on the matrix cores: A = Zh Zh^T as four 32x32 tiles of
// v_mfma_f32_32x32x2_f32 (exact f32, k-ordered fma chain), K = live dofs two at a time. Lane r
// holds row r of Zh; one v_permlane32_swap per dof pair turns (z[k], z[k+1]) into the A/B operand
// of rows 0-31 (p0) and of rows 32-63 (p1). A second round of swaps moves the C tiles
// (col = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)) into "lane c holds column c".
constexpr int NGRP = (NG + 3) / 4;  // dof groups of four
// 33-48 rows (11-16 contacts): 16x16x4 tiles over three row blocks instead of four 32x32 tiles
// (9 x 32 cycles per four dofs instead of 8 x 64). Operands: a 4x4 transpose of (register,
// 16-lane group) by two permlane32 and two permlane16 swaps turns z[k0..k0+3] into the A/B
// operand of each row block; results: the same transpose moves each tile's 4 row quads into the
// column's lane group (lane c holds A[r][c]).
HE_DEV void delassus_mfma48(const regla::ZVec& z, float (&acol)[MAXR], uint32_t live) {
    f32x4 c[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
        if ((live >> g) & 1u) {
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = 4 * g + k < NG ? ZV(z, 4 * g + k < NG ? 4 * g + k : 0) : 0.f;
            xpose4(r);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) c[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(r[i], r[j], c[i][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float x[4] = {c[i][0][v], c[i][1][v], c[i][2][v], 0.f};
            xpose4(x);  // x[g] on lane c: A[16 i + 4 g + v][c]
#pragma unroll
            for (int g = 0; g < 4; ++g) acol[16 * i + 4 * g + v] = x[g];
        }
#pragma unroll
    for (int r = 48; r < MAXR; ++r) acol[r] = 0.f;
}
// The four 32x32 tiles; WIDE = false (at most 32 rows, <= 10 contacts): only the rows-0-31 x
// columns-0-31 tile (one MFMA per dof pair instead of four), rows >= 32 of acol zero
template <bool WIDE>
HE_DEV void delassus_mfma(const regla::ZVec& z, float (&acol)[MAXR], uint32_t live) {
    f32x16 t00 = {}, t01 = {}, t10 = {}, t11 = {};
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
        if ((live >> g) & 1u) {
#pragma unroll
            for (int h = 0; h < 4; h += 2) {
                const int k0 = 4 * g + h;
                if (k0 < NG) {
                    float p0 = ZV(z, k0), p1 = k0 + 1 < NG ? ZV(z, k0 + 1 < NG ? k0 + 1 : 0) : 0.f;
                    swap32(p0, p1);
                    t00 = __builtin_amdgcn_mfma_f32_32x32x2f32(p0, p0, t00, 0, 0, 0);
                    if constexpr (WIDE) {
                        t01 = __builtin_amdgcn_mfma_f32_32x32x2f32(p0, p1, t01, 0, 0, 0);
                        t10 = __builtin_amdgcn_mfma_f32_32x32x2f32(p1, p0, t10, 0, 0, 0);
                        t11 = __builtin_amdgcn_mfma_f32_32x32x2f32(p1, p1, t11, 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = (v & 3) + 8 * (v >> 2);
        float a = t00[v], b = t01[v], c = t10[v], d = t11[v];
        swap32(a, b);  // a: A[r][lane], b: A[r + 4][lane] (narrow: lanes >= 32 zero)
        if constexpr (WIDE) swap32(c, d);  // c: A[32 + r][lane], d: A[36 + r][lane]
        acol[r] = a;
        acol[r + 4] = b;
        if (32 + r < MAXR) acol[32 + r < MAXR ? 32 + r : 0] = c;
        if (36 + r < MAXR) acol[36 + r < MAXR ? 36 + r : 0] = d;
    }
}

// ---------------------------------------------------------------------------------- solver rows
// Solver rows (patch friction, oracle build_rows), lane = slot: a joint limit 1 row, a point its
// normal row, the last point of a body's terrain patch then the patch's 2 tangential rows (+ 1
// torsional from 2 points on), a self pair its normal and 2 tangential rows; the row table (srow0,
// rslot, rkind) by the slots' exclusive prefix. Then each body's terrain patch (lane = body, tcnt >
// 0): normal = the normalised sum of its points' normals, the points' centroid (about o) and the
// torsion radius (mean tangential distance of the points from the centroid), into the RNEA force
// scratch F (dead from the midpoint bias to the next substep's force pass) and patch_radius.
// Returns the number of rows.
HE_DEV int build_rows(Lds& L, int lane, int nc) {
    int nr = 0;
    {
        const bool on = lane < nc;
        const int bb = on ? L.cbb[lane < MAXC ? lane : 0] : 0;
        const int b0 = bb & 0xFF, b1 = (bb >> 8) - 2;
        int cost = 0;
        if (on) {
            if (b1 == -2) cost = 1;
            else if (b1 >= 0) cost = 3;
            else {
                const int tn = L.tcnt[b0];
                cost = lane == L.tbase[b0] + tn - 1 ? 1 + (tn >= 2 ? 3 : 2) : 1;
            }
        }
        const int start = wave_prefix3(cost, nr);
        if (on) {
            L.srow0[lane < MAXC ? lane : 0] = (int8_t)start;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cost) { L.rslot[start + k] = (int8_t)lane; L.rkind[start + k] = (int8_t)k; }
        }
    }
    if (lane < NB && L.tcnt[lane] > 0) {
        const int p0 = L.tbase[lane], pc = L.tcnt[lane];
        f3 px[4];
        f3 np = f3{0.f, 0.f, 0.f}, xp = f3{0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sj = j < pc ? p0 + j : p0;
            px[j] = f3{L.cx[sj][0], L.cx[sj][1], L.cx[sj][2]};
            if (j < pc) {
                np = np + f3{L.cn[sj][0], L.cn[sj][1], L.cn[sj][2]};
                xp = xp + px[j];
            }
        }
        np = np * (1.0f / norm3(np));
        xp = xp * (1.0f / (float)pc);
        float rp = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f3 d = px[j] - xp;
            const f3 tg = d - np * dot3(d, np);
            if (j < pc) rp += norm3(tg);
        }
        float* pf = L.F[lane];
        pf[0] = np.x; pf[1] = np.y; pf[2] = np.z; pf[3] = xp.x; pf[4] = xp.y; pf[5] = xp.z;
        patch_radius(L)[lane] = rp * (1.0f / (float)pc);
    }
    sync();
    return nr;
}

// The lane's solver row (lane = row), from row_setup to the end of the substep
struct RowDesc {
    bool act;      // lane < nr
    int rs_;       // its slot
    int kind;      // 0 normal / limit, 1 2 tangential, 3 torsional
    int rb0, rb1;  // its bodies (rb1: -1 terrain, -2 a joint limit)
    int rkey;      // its 16-bit key
    f3 dd, rho;    // the row's linear direction, and its moment about o (a torsional row: the normal)
    float lam0;    // the previous solve's impulse of the row's key
};
// The row's slot read again where a late phase needs it (row_setup's own read of rslot, which
// build_rows wrote and nothing overwrites within the step): the slot's address held from the row
// set-up through the rows' register peak came back from scratch in front of the gap's read.
HE_DEV int row_slot_again(bool act) {
    const Lds& L = phase_lds();
    const int ln = phase_lane();
    return act ? L.rslot[ln] : 0;
}
// Each row's Jacobian data: slot, kind, bodies; a friction row's patch (a body's terrain points
// [tbase, tbase + tcnt), or the self pair alone) gives its tangent basis, centroid and torsion
// radius. The warm start: the previous solve's impulse of each row's key (lane r matches its key
// against the old keys by readlane and fetches the impulse from lam_prev). Writes wckey (this solve's
// keys), lam (the friction bound weight muw: mu, or mu r for the torsional row, parked in the impulse
// words until the solve's set-up: a short live range through the rows' register peak) and row_dirs
// (the row's linear direction for the reported forces; a joint limit's and a torsional row's: none;
// written in the launch's last physics step only, `last`: no other step reports forces).
// No sync at its end: the next phases read these words in the writing lane only.
HE_DEV void row_setup(Lds& L, int lane, int nr, float mu, float lam_prev, bool last, RowDesc& r) {
    r.act = lane < nr;
    r.rs_ = r.act ? L.rslot[lane] : 0;
    r.kind = r.act ? L.rkind[lane] : 0;
    const int rbb = L.cbb[r.rs_];
    r.rb0 = rbb & 0xFF;
    r.rb1 = (rbb >> 8) - 2;
    // the row's 16-bit key: a normal row its slot's, a friction row its patch's (terrain: the body's
    // patch, HE_KEY_PATCH) with the kind
    r.rkey = r.kind == 0 ? L.ckey[r.rs_]
                         : ((r.rb1 == -1 ? row_key(r.rb0, -1, HE_KEY_PATCH, 0) : L.ckey[r.rs_]) | (r.kind << 14));
    r.lam0 = 0.f;
    {
        const int nw = __builtin_amdgcn_readfirstlane(L.nwc);
        if (nw > 0 && nr > 0) {
            const int wk = lane < nw ? L.wckey[lane] : -1;
            const int ck = r.act ? r.rkey : -2;
            if (nw == nr && __ballot(r.act && wk != ck) == 0ull) {
                r.lam0 = r.act ? lam_prev : 0.f;  // the same rows in the same order (at rest)
            } else {
                int src = -1;
                for (int j = 0; j < nw; ++j) {
                    const int kj = __builtin_amdgcn_readlane(wk, j);
                    src = (src < 0 && kj == ck) ? j : src;
                }
                const float v = __shfl(lam_prev, src >= 0 ? src : 0, W);
                r.lam0 = (r.act && src >= 0) ? v : 0.f;
            }
        }
        // the old keys are matched: this solve's row keys replace them (the next solve's warm start)
        L.wckey[lane] = r.act ? r.rkey : -1;
    }
    const f3 xs = f3{L.cx[r.rs_][0], L.cx[r.rs_][1], L.cx[r.rs_][2]};
    const f3 ns = f3{L.cn[r.rs_][0], L.cn[r.rs_][1], L.cn[r.rs_][2]};
    // a friction row's patch: the body's terrain patch (build_rows), or a self pair's own point
    const bool terr = r.rb1 == -1;
    const float* pf = L.F[r.rb0];
    const f3 np = terr ? f3{pf[0], pf[1], pf[2]} : ns;
    const f3 xp = terr ? f3{pf[3], pf[4], pf[5]} : xs;
    const float rp = terr ? patch_radius(L)[r.rb0] : 0.f;
    f3 t1, t2;
    friction_basis(np, t1, t2);
    r.dd = r.kind == 0 ? ns : (r.kind == 1 ? t1 : (r.kind == 2 ? t2 : f3{0.f, 0.f, 0.f}));
    r.rho = r.kind == 3 ? np : cross3(r.kind == 0 ? xs : xp, r.dd);  // contact points about o
    L.lam[lane] = r.act && r.kind > 0 ? (r.kind == 3 ? mu * rp : mu) : 0.f;
    if (r.act && reports(last)) {  // contact_forces_out, the only reader, runs in the launch's last step
        float* fr = row_dirs(L);
        const bool none = r.rb1 == -2;
        fr[3 * lane] = none ? 0.f : r.dd.x;
        fr[3 * lane + 1] = none ? 0.f : r.dd.y;
        fr[3 * lane + 2] = none ? 0.f : r.dd.z;
    }
}

// The rows' system, in registers from row_system to the solve: lane r holds row r of Zh = D^-1/2
// L^-T J^T (kept for du = L^-1 D^-1/2 Zh^T lambda), lane c column c of the Delassus operator
struct RowSystem {
    regla::ZVec z;
    float acol[MAXR];  // lane c: A[r][c]
    float brow;        // J_r uf + bias
    float diag;        // |zh_r|^2 = A[r][r]
    bool legs;         // every row's support inside the root and the legs (wave-uniform)
    // legs, in a TGS kernel, with at most 32 rows (wave-uniform): z holds dofs 0..KZ-1 only, and
    // ZV(z, i >= KZ) is unwritten (in every other case it holds all NG dofs, exact zeros outside the
    // support). Whoever reads z past KZ has to exclude zshort first: row_system's limit rows and
    // reductions, zbs (skips bodies outside lb), delassus_mfma<false> (dof groups of lb: none past dof 31)
    // and solve_tgs<32> (legs_it) do; the wide solves, the wide Delassus forms, full_dofs and the PGS
    // kernel's pgs_velocity read every dof and never see it set.
    bool zshort;
};
// Contact rows, one per lane (oracle row_jacobian, contact_bias): z = J_r^T, brow = J_r uf + bias,
// then z <- D^-1/2 L^-T z (dofs outside every row's support stay zero and are skipped
// wave-uniformly), so that the Delassus operator A = Zh Zh^T is a plain Gram matrix of the lanes'
// registers. Reads S, u0, yh, sDinv, Lp and the slots; writes no LDS.
template <bool TGS>
HE_DEV void row_system(Lds& L, const BodyTopo& T, const he_sim_params& p, bool full_dofs, int lane, int nr, float hs,
                       const RowDesc& r, RowSystem& s, Stamps& st) {
    using namespace regla;
    const float dt = p.dt;
    const uint32_t anc0 = r.act ? T.anc_mask[r.rb0] : 0u;
    const uint32_t anc1 = (r.act && r.rb1 >= 0) ? T.anc_mask[r.rb1] : 0u;
    // bodies on some row's support (wave-uniform): the only ones whose dofs can be nonzero
    const uint32_t lb = wave_or(anc0 | anc1);
    s.legs = (lb & ~kLegBodies) == 0u && !full_dofs;
    // z = J_r^T and brow = J_r u0 on the matrix cores
    s.zshort = HE_LEG_ZROWS && TGS && s.legs && nr <= 32;
    zrows_mfma(s.z, lb, anc0, anc1, r.rho, r.dd, L, lane, nr <= 32, s.zshort);
    // joint-limit rows: the stored row over the joint's three dofs (its support is the joint's
    // ancestor chain, anc0: under zshort a leg joint, its dofs below KZ)
    const bool limrow = r.act && r.rb1 == -2;
    if (__ballot(limrow)) {  // wave-uniform
        const int bl = limrow ? r.rb0 : 0;
        const float g3[3] = {L.cx[r.rs_][0], L.cx[r.rs_][1], L.cx[r.rs_][2]};
        auto limit_dofs = [&](auto lo, auto hi) {
#pragma unroll
            for (int i = decltype(lo)::value; i < decltype(hi)::value; ++i) {
                const float v = i < 6 ? 0.f : (bl == (i < 6 ? 0 : (i - 6) / 3 + 1) ? g3[i < 6 ? 0 : (i - 6) % 3] : 0.f);
                ZV(s.z, i) = limrow ? v : ZV(s.z, i);
            }
        };
        limit_dofs(std::integral_constant<int, 0>{}, std::integral_constant<int, KZ>{});
        if (!s.zshort) limit_dofs(std::integral_constant<int, KZ>{}, std::integral_constant<int, NG>{});
    }
    // J_r u0 on the register pairs (dof i into sum i mod 4); over the legs' dofs only when every
    // row's support is there (the dropped terms are fma(0, u, s) = s: the same bits)
    s.brow = s.legs ? zdot_lds<KZ>(s.z, L.u0) : zdot_lds<NG>(s.z, L.u0);
    if (r.act && r.kind == 0) {
        const float g = L.cgap[row_slot_again(r.act)];
        // speculative: close within the solve's step; penetrating: recover at baumgarte per physics
        // step (TGS too: oracle contact_bias)
        s.brow += g >= 0.f ? g / hs : fmaxf(p.baumgarte * g / dt, -p.max_depenetration_velocity);
    }
    STAMP(PH_ROWS_JT);
    __builtin_amdgcn_s_setprio(kPrioSerial);
    zbs<NG - 1>(L.Lp, s.z, lb);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    STAMP(PH_ROWS_LT);
    // z <- D^-1/2 z: the scale of dof i is broadcast from lane i's register (no LDS)
    const float sdl = L.sDinv[lane], sdl2 = lane < NH ? L.sDinv[64 + lane] : 0.f;
    // then |zh_r|^2 and J_r (uf - u0) = zh_r . yh, yh_i broadcast from lane i (v_readlane: no LDS
    // loads to hoist into registers at the phase's register peak), four lanes per block into
    // four SGPRs (one hazard nop per block; through one SGPR the 75 products serialised: this
    // phase -10 %, the launch -0.5 % by A/B, bit-identical, round 4). Leg support: dofs 0..KZ-1
    // (zh is exactly zero past them: the same bits)
    const float yhl = L.yh[lane];
    if (s.legs) {
        scale_rows<0, KZ>(s.z, sdl, sdl2);
        s.diag = znorm2<KZ>(s.z);
        s.brow += zdot_lanes<KZ>(s.z, yhl, 0.f);
    } else {
        scale_rows<0>(s.z, sdl, sdl2);
        s.diag = znorm2<NG>(s.z);
        s.brow += zdot_lanes(s.z, yhl, lane < NH ? L.yh[64 + lane] : 0.f);
    }
    // dof groups of four touching a support body (wave-uniform, from lb)
    uint32_t live = 0u;
#pragma unroll
    for (int g = 0; g < NGRP; ++g)
        if (lb & kGroupBodies[g]) live |= 1u << g;
    STAMP(PH_ZROWS);
    // Delassus columns on the matrix cores: A[r][c] = sum_i zh_r[i] zh_c[i]
    if (nr <= 32) delassus_mfma<false>(s.z, s.acol, live);  // wave-uniform
    else if (nr <= 48) delassus_mfma48(s.z, s.acol, live);
    else delassus_mfma<true>(s.z, s.acol, live);
}

}  // namespace
