// he_phys_contacts.h -- the contact phase up to the slots: terrain distance (Terrain, terrain_of,
// terrain_dist), closest points of two segments (seg_seg), the slot store and the row keys
// (store_contact, row_key), the model reads issued ahead (GeomPrefetch, prefetch_geometry), then
// limit_slots, terrain_candidates, store_terrain_slots, self_pairs, reduce_overflow and gen_contacts.
// LDS: reads qw, pw, root_pos, q, u0, limmask, T.cbody; writes the slots (cx, cn, cgap, cbb, ckey),
// tbase, tcnt, nc, nterr, nlim, ncand, cf (zeroed). Scratch: IS (cand_gaps, cand_bodies, cand_order),
// lam (the pair list), Ib or Ic (the bodies' segments), Acc (bsph). On entry: the final poses qw / pw
// of this substep, the factorisation done (IS dead), lam's impulses already read by the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/humanoid_engine.h"
#include "he_math.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_phys_tree.h"
#include "he_topo.h"

namespace {

// terrain constants of the env, read once per contact phase (slope normal, step field)
struct Terrain {
    int kind;
    float sn, cs, step_h, step_l;
};
HE_DEV Terrain terrain_of(const he_sim_params& p, int kind) {
    Terrain t{kind, 0.f, 1.f, p.step_height, p.step_length};
    if (kind == 1) { t.sn = sinf(p.terrain_slope); t.cs = cosf(p.terrain_slope); }
    return t;
}
HE_DEV float terrain_dist(const Terrain& t, f3 x, f3& n) {
    if (t.kind == 1) {
        n = f3{-t.sn, 0.f, t.cs};
        return dot3(n, x);
    }
    n = f3{0.f, 0.f, 1.f};
    if (t.kind == 2) {
        float h = x.x > 0.f ? t.step_h * floorf(x.x / t.step_l) : 0.f;
        return x.z - h;
    }
    return x.z;
}

// closest points between segments p1q1 and p2q2 (Ericson, RTCD 5.1.9), branch-free: every case
// (both degenerate, one degenerate, general with its two t-clamps) is formed and selected, so a
// wave of mixed sphere / capsule pairs runs one path
HE_DEV void seg_seg(f3 p1, f3 q1, f3 p2, f3 q2, f3& c1, f3& c2) {
    const f3 d1 = q1 - p1, d2 = q2 - p2, r = p1 - p2;
    const float a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r);
    const float eps = 1e-12f;
    // divisions as v_rcp_f32 products (1 ulp; the fp64 oracle's tolerance covers it)
    const float ia = __builtin_amdgcn_rcpf(a), ie = __builtin_amdgcn_rcpf(e);
    const float c = dot3(d1, r), b = dot3(d1, d2), den = a * e - b * b;
    const float sg = den > eps ? __builtin_amdgcn_fmed3f((b * f - c * e) * __builtin_amdgcn_rcpf(den), 0.f, 1.f) : 0.f;
    const float tg = (b * sg + f) * ie;
    const float s_lo = __builtin_amdgcn_fmed3f(-c * ia, 0.f, 1.f);       // t clamped to 0 (and e degenerate)
    const float s_hi = __builtin_amdgcn_fmed3f((b - c) * ia, 0.f, 1.f);  // t clamped to 1
    float s = tg < 0.f ? s_lo : (tg > 1.f ? s_hi : sg);
    float t = tg < 0.f ? 0.f : (tg > 1.f ? 1.f : tg);
    const bool adeg = a <= eps, edeg = e <= eps;
    s = edeg ? s_lo : s;
    t = edeg ? 0.f : t;
    s = adeg ? 0.f : s;
    t = adeg ? (edeg ? 0.f : __builtin_amdgcn_fmed3f(f * ie, 0.f, 1.f)) : t;
    c1 = p1 + d1 * s;
    c2 = p2 + d2 * t;
}

HE_DEV void store_contact(Lds& L, int slot, int b0, int b1, f3 x, f3 n, float gap, int key) {
    L.cbb[slot] = b0 | ((b1 + 2) << 8);
    L.cx[slot][0] = x.x; L.cx[slot][1] = x.y; L.cx[slot][2] = x.z;
    L.cn[slot][0] = n.x; L.cn[slot][1] = n.y; L.cn[slot][2] = n.z;
    L.cgap[slot] = gap;
    L.ckey[slot] = key;
}
// 16-bit row keys (include/humanoid_engine.h cache layout)
HE_DEV int row_key(int b0, int b1, int sub, int kind) { return b0 | ((b1 + 2) << 5) | (sub << 10) | (kind << 14); }

// The contact phase's model reads (geometry of the lane's body: body lanes their own geom, corner
// lanes their box's; the self-collision pair indices of the lane's pairs). They depend on nothing a
// substep computes: issued after the factorisation, they land behind the free-velocity sweep.
constexpr int kPairRounds = (HE_MAX_PAIRS + W - 1) / W;
struct GeomPrefetch {
    float gv[10];  // geom_params of the lane's geometry body
    int gt;        // geom_type
    float grad;    // geom_radius
    int2 prs[kPairRounds];  // pair rd * W + lane (x = -1: none)
};
HE_DEV void prefetch_geometry(const Lds& L, const he_model& m, int lane, GeomPrefetch& g) {
    const int npairs = m.num_pairs;
    const int cb = L.T.cbody[lane];
    const int b = lane < NB ? lane : (cb >= 0 ? cb : 0);
    const float* gp = m.geom_params[b];
#pragma unroll
    for (int i = 0; i < 10; ++i) g.gv[i] = gp[i];
    g.gt = m.geom_type[b];
    g.grad = m.geom_radius[b];
#pragma unroll
    for (int rd = 0; rd < kPairRounds; ++rd) {
        const int pi = rd * W + lane;
        g.prs[rd] = *reinterpret_cast<const int2*>(m.pairs[pi < npairs ? pi : 0]);
        if (pi >= npairs) g.prs[rd].x = -1;
    }
    sync();
}

// ---------------------------------------------------------------------------------- contact slots
// joint-angle limit slots (oracle gen_limits), lane = joint b - 1: the rows limit_detect flagged,
// re-evaluated from the same state words, into slots [0, nlim). Returns nlim; nlim_all counts the
// flagged joints (past the capacity too).
HE_DEV int limit_slots(Lds& L, const he_sim_params& p, int lane, int maxc, int& nlim_all) {
    nlim_all = 0;
    if (!p.joint_limits) return 0;
    const uint32_t lm = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.limmask);
    const bool act = lane < NB - 1 && ((lm >> (lane + 1)) & 1u);
    const int pre = wave_prefix(act, lane, nlim_all);
    if (act && pre < maxc) {
        const int j = lane < NB - 1 ? lane : 0;
        float lg;
        f3 ld;
        angle_row(f3{L.q[3 * j], L.q[3 * j + 1], L.q[3 * j + 2]}, f3{L.u0[6 + 3 * j], L.u0[7 + 3 * j], L.u0[8 + 3 * j]},
                  p, lg, ld);
        // the row over the joint's dofs (-q^) travels in the contact position (unused by a limit)
        store_contact(L, pre, lane + 1, -2, ld * -1.f, f3{0.f, 0.f, 1.f}, lg, row_key(lane + 1, -2, 7, 0));
    }
    return nlim_all < maxc ? nlim_all : maxc;
}

// The lane's terrain candidates: a body lane (lane < 24) takes its sphere's centre or its capsule's
// end points, a corner lane (lane 24 + 8k + c, he_topo.h corner_body) corner c of the k-th box.
// Written by terrain_candidates, read by the slot stores of gen_contacts and reduce_overflow.
static_assert(NB % 8 == 0 && NB + 8 * HE_MAX_BOXES <= W, "corner lanes: 8-lane groups above the body lanes");
constexpr int kPts = 2;  // terrain points per lane
struct TerrainLanes {
    int body;      // the lane's geometry body
    bool corner;   // a box corner lane
    int cc;        // its corner index
    float cd[kPts];         // gap of point ci
    f3 cxs[kPts], cns[kPts];  // contact point about o, normal
    bool cand[kPts];        // gap < contact offset
    int rank[kPts];         // slot offset within the body (8: not kept)
    int myn, base;          // body lanes: points kept, and the exclusive prefix of them over the bodies
};
// Geometry (every lane, of its geometry body):
//  self segment P0-P1, radius rs: sphere P0 = P1 = centre; capsule from / to; box the capsule
//    proxy along its longest axis (radius geom_radius)
//  terrain points, radius rt: sphere the centre; capsule from, to; box corner c around its
//    centre Pc (world centre +- the world half-axes)
// Also writes each body's world segment (Ib; TGS: Ic) and bounding sphere (Acc) for self_pairs.
// Returns the number of terrain candidates kept.
template <bool TGS>
HE_DEV int terrain_candidates(Lds& L, const GeomPrefetch& g, const Terrain& ter, float off, bool self_col, int lane,
                              TerrainLanes& tc, Stamps& st) {
    const int cbody = L.T.cbody[lane];
    const bool corner = tc.corner = lane >= NB && cbody >= 0;
    const int tb_ = tc.body = lane < NB ? lane : (corner ? cbody : 0);
    const int cc = tc.cc = lane & 7;
    const f3 ow = f3{L.root_pos[0], L.root_pos[1], L.root_pos[2]};  // points are about o; the terrain is world
    const bool isS = g.gt == HE_GEOM_SPHERE, isC = g.gt == HE_GEOM_CAPSULE, isB = !isS && !isC;
    const f4 bq = isB ? f4{g.gv[6], g.gv[7], g.gv[8], g.gv[9]} : f4{0.f, 0.f, 0.f, 1.f};
    int ax = 0;
    float emax = g.gv[3];
    if (g.gv[4] > emax) { ax = 1; emax = g.gv[4]; }
    if (g.gv[5] > emax) { ax = 2; emax = g.gv[5]; }
    const float half = fmaxf(emax - g.grad, 0.f);
    // rotations as matrices (the box's local frame and the body's world rotation): mat-vecs
    // instead of quaternion applications
    f3 bc0, bc1, bc2, wc0, wc1, wc2;
    qcols(bq, bc0, bc1, bc2);
    qcols(f4{L.qw[tb_][0], L.qw[tb_][1], L.qw[tb_][2], L.qw[tb_][3]}, wc0, wc1, wc2);
    const f3 pwb = f3{L.pw[tb_][0], L.pw[tb_][1], L.pw[tb_][2]};
    const f3 dir = (ax == 0 ? bc0 : (ax == 1 ? bc1 : bc2)) * half;
    const f3 ctr = f3{g.gv[0], g.gv[1], g.gv[2]};
    const f3 l0 = isB ? ctr - dir : ctr;
    const f3 l1 = isB ? ctr + dir : (isC ? f3{g.gv[3], g.gv[4], g.gv[5]} : ctr);
    const float rs = isS ? g.gv[3] : (isC ? g.gv[6] : g.grad);
    const float rt = isS ? g.gv[3] : (isC ? g.gv[6] : 0.f);
    auto rot = [&](f3 v) { return (wc0 * v.x + wc1 * v.y) + wc2 * v.z; };
    const f3 P0 = pwb + rot(l0), P1 = pwb + rot(l1);
    STAMP(PH_TERRAIN_GEOM);
    if (self_col && lane < NB) {
        // world segments (the Ib scratch is dead after the subtree sums), and the bounding
        // sphere about the segment midpoint for the pair cull as one 16-byte record
        float* sg = TGS ? L.Ic[lane] : L.Ib[lane];  // TGS: Ib (own inertias) serves the iterations' bias
        sg[0] = P0.x; sg[1] = P0.y; sg[2] = P0.z; sg[3] = P1.x; sg[4] = P1.y; sg[5] = P1.z; sg[6] = rs;
        const f3 mid = (P0 + P1) * 0.5f;
        bsph(L)[lane] = make_float4(mid.x, mid.y, mid.z, 0.5f * norm3(P1 - P0) + rs);
    }
    // a corner lane's point: ((Pc +- ex) +- ey) +- ez, signs by the bits of c
    f3 X0 = P0;
    if (corner) {
        const f3 Pc = pwb + rot(ctr);
        const f3 ex = rot(bc0 * g.gv[3]), ey = rot(bc1 * g.gv[4]), ez = rot(bc2 * g.gv[5]);
        X0 = ((Pc + ((cc & 1) ? ex : ex * -1.f)) + ((cc & 2) ? ey : ey * -1.f)) + ((cc & 4) ? ez : ez * -1.f);
    }
    const int npts = lane < NB ? (isS ? 1 : (isC ? 2 : 0)) : (corner ? 1 : 0);
#pragma unroll
    for (int ci = 0; ci < kPts; ++ci) {
        const f3 x = ci == 0 ? X0 : P1;
        tc.cd[ci] = terrain_dist(ter, ow + x, tc.cns[ci]) - rt;
        tc.cxs[ci] = x - tc.cns[ci] * rt;
        tc.cand[ci] = ci < npts && tc.cd[ci] < off;
    }
    // a box keeps its 4 deepest corners (ties by index): a corner lane's rank among the 8 lanes
    // of its group, keys through xor swizzles (non-candidates keyed +inf never go first)
    // Only candidates beat a candidate, so a group of at most four candidates keeps them all whatever
    // their order (a foot flat on the ground: its four bottom corners). The ranking runs only when some
    // group holds five or more: the groups are the bytes of the candidates' ballot, counted in scalar
    // code (a byte's count + 3 reaches bit 3 from five on).
    bool kept0 = tc.cand[0];
    const uint64_t cb = __ballot(corner && tc.cand[0]);
    uint64_t cnt = cb - ((cb >> 1) & 0x5555555555555555ull);
    cnt = (cnt & 0x3333333333333333ull) + ((cnt >> 2) & 0x3333333333333333ull);
    cnt = (cnt + (cnt >> 4)) & 0x0F0F0F0F0F0F0F0Full;
    const bool crowded = ((cnt + 0x0303030303030303ull) & 0x0808080808080808ull) != 0ull;
    if (!HE_RANK_ON_DEMAND || __builtin_expect(crowded, 0)) {
        const float key = corner && tc.cand[0] ? tc.cd[0] : __builtin_inff();
        int r = 0;
        auto beat = [&](float kj, int sx) { r += (kj < key || (kj == key && (cc ^ sx) < cc)) ? 1 : 0; };
        beat(swizzle_xor<1>(key), 1);
        beat(swizzle_xor<2>(key), 2);
        beat(swizzle_xor<3>(key), 3);
        beat(swizzle_xor<4>(key), 4);
        beat(swizzle_xor<5>(key), 5);
        beat(swizzle_xor<6>(key), 6);
        beat(swizzle_xor<7>(key), 7);
        kept0 = tc.cand[0] && (!corner || r < 4);
    }
    const bool kept1 = tc.cand[1];
    // the kept points take the body's slots in point index order (box corners by corner index),
    // so that resting contacts keep their slots from one substep to the next (the warm start then
    // maps impulses one to one); rank[] becomes that slot offset within the body
    const uint64_t kb = __ballot(corner && kept0);
    const uint64_t bxm = __ballot(lane < NB && isB);
    const int kbox = ballot_below(bxm);
    const uint32_t grp = (uint32_t)(kb >> (corner ? (lane & ~7) : (NB + 8 * (kbox < HE_MAX_BOXES ? kbox : 0)))) & 0xFFu;
    tc.myn = lane < NB ? (isB ? __popc(grp) : (kept0 ? 1 : 0) + (kept1 ? 1 : 0)) : 0;
    int total;
    tc.base = wave_prefix3(tc.myn, total);  // over the body lanes (myn = 0 elsewhere)
    // a corner lane starts from its box body's base
    const int bbase = __builtin_amdgcn_ds_bpermute(4 * tb_, tc.base);
    if (corner) tc.base = bbase;
    tc.rank[0] = kept0 ? (corner ? __popc(grp & ((1u << cc) - 1u)) : 0) : 8;
    tc.rank[1] = kept1 ? (kept0 ? 1 : 0) : 8;
    return total;
}

// The terrain slot store: each kept point (candidate k = base + rank, in slot order) into slot(k)
// when keep(k). RECORD: also its gap and body for the reduction. The contact key's sub-index is the
// point's index on its body (a box's corner index).
template <bool RECORD, class Keep, class Slot>
HE_DEV void store_terrain_slots(Lds& L, const TerrainLanes& tc, Keep keep, Slot slot) {
#pragma unroll
    for (int ci = 0; ci < kPts; ++ci) {
        if (tc.cand[ci] && tc.rank[ci] < 4) {
            const int k = tc.base + tc.rank[ci];
            if constexpr (RECORD) {
                if (k < kCand) { cand_gaps(L)[k] = tc.cd[ci]; cand_bodies(L)[k] = tc.body; }
            }
            if (keep(k))
                store_contact(L, slot(k), tc.body, -1, tc.cxs[ci], tc.cns[ci], tc.cd[ci],
                              row_key(tc.body, -1, tc.corner ? tc.cc : ci, 0));
        }
    }
}

// Self pairs (oracle gen_contacts, the pair loop): broad phase (bounding spheres, survivors compacted
// in pair order into the lam scratch: lam's impulses must have been read), narrow phase W survivors
// per pass; `visit(hit, i, j, x, n, gap, k)` gets every hit with its candidate index k (in pair order
// after the terr_all terrain candidates). Reads the segments and spheres terrain_candidates wrote.
// Returns the hits.
template <bool TGS, class Visit>
HE_DEV int self_pairs(Lds& L, const GeomPrefetch& g, float off, int terr_all, int lane, Stamps& st, Visit visit) {
    sync();
    int* list = reinterpret_cast<int*>(L.lam);
    auto compact = [&](int skip) {  // survivors skip .. skip + W - 1 into the list
        int k = 0;
#pragma unroll
        for (int rd = 0; rd < kPairRounds; ++rd) {
            const int i = g.prs[rd].x, j = g.prs[rd].y;
            bool need = false;
            if (i >= 0) {
                const float4 bi = bsph(L)[i], bj = bsph(L)[j];
                const f3 d = f3{bi.x - bj.x, bi.y - bj.y, bi.z - bj.z};
                const float lim = bi.w + bj.w + off + 1e-3f;
                need = dot3(d, d) < lim * lim;
            }
            const uint64_t bm = __ballot(need);
            const int slot = k + ballot_below(bm) - skip;
            if (need && slot >= 0 && slot < W) list[slot] = (rd * W + lane) | (i << 16) | (j << 24);
            k += __popcll(bm);
        }
        sync();
        return k;
    };
    // broad phase: a pair whose bounding spheres (segment midpoint, half length + radius) are
    // apart by more than the contact offset plus a 1 mm guard cannot reach gap < offset
    const int nsurv = compact(0);
    STAMP(PH_SELF_SEGMENTS);
    int nhit = 0;
    for (int s0 = 0; s0 < nsurv; s0 += W) {
        bool hit = false;
        f3 px = f3{0.f, 0.f, 0.f}, pn = f3{0.f, 0.f, 0.f};
        float pgap = 0.f;
        int i = 0, j = 0;
        if (s0 + lane < nsurv) {
            const int e = list[lane];
            i = (e >> 16) & 0xFF;
            j = (e >> 24) & 0xFF;
            const float* si = TGS ? L.Ic[i] : L.Ib[i];
            const float* sj = TGS ? L.Ic[j] : L.Ib[j];
            const float ri = si[6], rj = sj[6];
            f3 ci, cj;
            seg_seg(f3{si[0], si[1], si[2]}, f3{si[3], si[4], si[5]}, f3{sj[0], sj[1], sj[2]}, f3{sj[3], sj[4], sj[5]}, ci, cj);
            const f3 dv = ci - cj;
            const float len = norm3(dv);
            pgap = len - ri - rj;
            if (pgap < off) {
                hit = true;
                pn = len > 1e-9f ? dv * __builtin_amdgcn_rcpf(len) : f3{0.f, 0.f, 1.f};
                px = cj + pn * (rj + 0.5f * pgap);
            }
        }
        int total;
        const int pre = wave_prefix(hit, lane, total);
        visit(hit, i, j, px, pn, pgap, terr_all + nhit + pre);
        nhit += total;
        if (__builtin_expect(s0 + W < nsurv, 0)) compact(s0 + W);  // more than W survivors: the next pass (rare)
    }
    return nhit;
}

// Overflow (rare, wave-uniform): the candidates are past the slots or the solver rows. The contacts
// are taken deepest first (smallest gap, ties in slot order), each kept while its rows still fit (a
// self pair or a body's first terrain point 3, its second 2, 1 after: oracle gen_contacts), and the
// kept ones are regenerated in slot order. Reads the gaps and bodies gen_contacts recorded (IS), uses
// the rank order's words. Returns the contact slots in use.
template <bool TGS>
HE_DEV int reduce_overflow(Lds& L, const GeomPrefetch& g, const Terrain& ter, float off, bool self_col, int lane, int maxc,
                           int nlim, int terr_all, int self_all, TerrainLanes& tc, Stamps& st) {
    const float* gl = cand_gaps(L);
    int *gb = cand_bodies(L), *gord = cand_order(L);
    sync();
    const int keep = maxc - nlim;
    const int T = terr_all + self_all < kCand ? terr_all + self_all : kCand;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // each candidate's depth rank -> the rank order
        const int k = h * W + lane;
        if (k < T) {
            const float gk = gl[k];
            int r = 0;
            for (int jj = 0; jj < T; ++jj) {  // uniform LDS reads (broadcast)
                const float g2 = gl[jj];
                r += (g2 < gk || (g2 == gk && jj < k)) ? 1 : 0;
            }
            gord[r] = k;
        }
    }
    sync();
    // the greedy pass in rank order (wave-uniform): candidate and body from registers by
    // v_readlane, the kept points per body in lane = body
    const int ko0 = lane < T ? gord[lane] : 0, ko1 = W + lane < T ? gord[W + lane < kCand ? W + lane : 0] : 0;
    const int kb0 = gb[ko0], kb1 = gb[ko1];
    uint64_t km[2] = {0ull, 0ull};
    int rows = nlim, kept_n = 0, pcnt = 0;
    for (int q = 0; q < T; ++q) {
        const int k = q < W ? __builtin_amdgcn_readlane(ko0, q & (W - 1)) : __builtin_amdgcn_readlane(ko1, q & (W - 1));
        const int b = q < W ? __builtin_amdgcn_readlane(kb0, q & (W - 1)) : __builtin_amdgcn_readlane(kb1, q & (W - 1));
        const int pc = b >= 0 ? __builtin_amdgcn_readlane(pcnt, b) : 0;
        const int cost = b < 0 ? 3 : (pc == 0 ? 3 : (pc == 1 ? 2 : 1));
        if (kept_n < keep && rows + cost <= MAXR) {
            rows += cost;
            ++kept_n;
            pcnt += lane == b ? 1 : 0;
            if (k < W) km[0] |= 1ull << (k & (W - 1));
            else km[1] |= 1ull << (k & (W - 1));
        }
    }
    auto before = [&](int k) {  // kept candidates below index k
        const uint64_t lo = k >= W ? km[0] : (k <= 0 ? 0ull : km[0] & ((~0ull) >> (W - k)));
        const uint64_t hi = k <= W ? 0ull : (k >= 2 * W ? km[1] : km[1] & ((~0ull) >> (2 * W - k)));
        return __popcll(lo) + __popcll(hi);
    };
    auto is_kept = [&](int k) { return k < 2 * W && ((km[k >= W ? 1 : 0] >> (k & (W - 1))) & 1ull); };
    terrain_candidates<TGS>(L, g, ter, off, self_col, lane, tc, st);
    store_terrain_slots<false>(L, tc, is_kept, [&](int k) { return nlim + before(k); });
    if (lane < NB) {
        const int s0 = nlim + before(tc.base);
        L.tbase[lane] = (int8_t)s0;
        L.tcnt[lane] = (int8_t)(nlim + before(tc.base + tc.myn) - s0);
    }
    if (lane == 0) L.nterr = nlim + before(terr_all);
    if (self_col) {
        self_pairs<TGS>(L, g, off, terr_all, lane, st, [&](bool hit, int i, int j, f3 px, f3 pn, float pgap, int k) {
            if (hit && is_kept(k)) store_contact(L, nlim + before(k), i, j, px, pn, pgap, row_key(i, j, 0, 0));
        });
    }
    return nlim + before(T);
}

// Contact slots (oracle gen_contacts): joint limits, terrain (bodies in order, box corners
// deepest-first), self pairs. Every contact generated is counted; when they exceed the capacity, the
// limits stay and the contacts are reduced to the deepest ones, kept in slot order (reduce_overflow).
// Writes the slots (cx, cn, cgap, cbb, ckey), tbase / tcnt, nc, nterr, nlim, ncand, and zeroes cf (the
// launch's last physics step, `last`).
// Scratch: IS (candidate records), lam (pair list), Ib / Ic (segments), Acc (bounding spheres).
// Returns the contact slots in use.
template <bool TGS>
HE_DEV int gen_contacts(Lds& L, const GeomPrefetch& g, const he_sim_params& p, int tkind, int lane, bool last, Stamps& st) {
    const int maxc = p.max_contacts < MAXC ? p.max_contacts : MAXC;
    const float off = p.contact_offset;
    const Terrain ter = terrain_of(p, tkind);
    const bool self_col = p.self_collision;
    int nlim_all = 0;
    const int nlim = limit_slots(L, p, lane, maxc, nlim_all);
    STAMP(PH_LIMIT_SLOTS);
    TerrainLanes tc;
    const int terr_all = terrain_candidates<TGS>(L, g, ter, off, self_col, lane, tc, st);
    STAMP(PH_TERRAIN_RANK);
    store_terrain_slots<true>(L, tc, [&](int k) { return nlim + k < maxc; }, [&](int k) { return nlim + k; });
    // rows of the body's patch: k points, k normal rows + 2 tangential (+ 1 torsional from k = 2)
    int rows_terr;  // solver rows of every terrain candidate kept (patch friction)
    wave_prefix3(tc.myn == 0 ? 0 : tc.myn + (tc.myn >= 2 ? 3 : 2), rows_terr);
    int nc = nlim + terr_all < maxc ? nlim + terr_all : maxc, self_all = 0;
    if (lane < NB) {  // the body's slot range, for the per-body force sums
        const int s0 = nlim + tc.base;
        L.tbase[lane] = (int8_t)(s0 < maxc ? s0 : maxc);
        L.tcnt[lane] = (int8_t)(s0 + tc.myn < maxc ? tc.myn : (s0 < maxc ? maxc - s0 : 0));
    }
    if (lane == 0) L.nterr = nc;
    STAMP(PH_TERRAIN_SLOTS);
    if (self_col) {
        self_all = self_pairs<TGS>(L, g, off, terr_all, lane, st, [&](bool hit, int i, int j, f3 px, f3 pn, float pgap, int k) {
            if (hit && k < kCand) { cand_gaps(L)[k] = pgap; cand_bodies(L)[k] = -1; }
            if (hit && nlim + k < maxc) store_contact(L, nlim + k, i, j, px, pn, pgap, row_key(i, j, 0, 0));
        });
        nc = nlim + terr_all + self_all < maxc ? nlim + terr_all + self_all : maxc;
    }
    const int ncand_all = nlim_all + terr_all + self_all;
    if (__builtin_expect((nlim + terr_all + self_all > maxc || nlim + rows_terr + 3 * self_all > MAXR) && nlim < maxc, 0))
        nc = reduce_overflow<TGS>(L, g, ter, off, self_col, lane, maxc, nlim, terr_all, self_all, tc, st);
    STAMP(PH_SELF_SLOTS);
    if (lane == 0) { L.nc = nc; L.nlim = nlim; L.ncand = ncand_all; }
    // cf is stored once per launch, after its last step: that step alone zeroes it, before
    // contact_forces_out adds the rows' impulses
    if (lane < NB && reports(last)) { L.cf[lane][0] = 0.f; L.cf[lane][1] = 0.f; L.cf[lane][2] = 0.f; }
    sync();
    return nc;
}

}  // namespace
