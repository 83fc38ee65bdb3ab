// he_phys_lds.h -- the physics step's LDS window (he_physics.hip is the map of the he_phys_*.h files):
// the sizes, the tree tables (BodyTopo) and the env's words (Lds) with the list of the words that serve
// twice within a substep, every accessor that views an Lds array as something else (bsph, cand_gaps /
// cand_bodies / cand_order, row_dirs, patch_radius), the wave's ordering point (sync), a phase's own
// view of LDS and of the lane (phase_lds, phase_lane), the SGPR helpers, the wave priorities and the
// phase stamps.
// LDS: defines the layout and touches none of it. On entry: nothing live; phase_lds() assumes the
// kernel's dynamic shared memory starts with the Lds (one 64-lane wave per workgroup).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/humanoid_engine.h"
#include "he_math.h"
#include "he_smpl_topo.h"

namespace {

constexpr int NB = HE_NUM_BODIES;
constexpr int ND = HE_NUM_DOF;
constexpr int NG = HE_NUM_GEN;
constexpr int MAXC = HE_MAX_CONTACTS;  // contact slots (points, joint limits)
constexpr int MAXR = HE_MAX_ROWS;      // solver rows, one per lane (patch friction, oracle build_rows)
constexpr int W = 64;
static_assert(MAXR <= W - 1, "solver rows must fit one per lane");
constexpr int kTgsMaxIt = 16;  // TGS position iterations per physics step (he_simulate checks; oracle TGS_MAXIT)
constexpr int kTgsBiasEvery = 2;  // TGS: the bias re-evaluated every second iteration (oracle g_bias_every)
static_assert(MAXC < W, "one slot per lane in the row-layout pass");
static_assert(smpl::kNG == NG && smpl::kNB == NB, "generated topology mismatch");

struct BodyTopo {
    int8_t depth[NB];
    int8_t chain[NB][9];
    int8_t dof0[NB];
    uint32_t anc_mask[NB];
    uint32_t sub_mask[NB];
    float local_pos[NB][3];  // joint offsets (model), read along every FK chain walk
    uint32_t jump4[NB];      // byte k: 2^k-th ancestor of body b (0xFF: none), for pointer jumping
    int16_t pack_start[NG];  // packed-row offset of dof i (smpl::kPackStart)
    int8_t dof_depth[NG];    // depth of dof i in the dof tree (smpl::kDofNanc - 1)
    int8_t cbody[W];         // corner lanes: the box body of lane 24 + 8k + c (PhysTopo::corner_body)
};

struct Lds {
    float q[ND], tgt[ND];
    float u0[NG], uf[NG], rhs[NG], coef[NG], sDinv[NG];
    float yh[NG];  // D^-1/2 L^-T (dt rhs): the free motion's share of the one L^-1 sweep
    float ql[NB][4], qw[NB][4];
    float pw[NB][3];  // body origins RELATIVE to the root origin o (world axes): every spatial quantity
                      // is taken about o, and fp32 keeps ~1e-7 m of them however far o is from the
                      // world origin (world = o + pw only where a world position is needed)
    float S[NG][6], IS[NG][6];
    float V[NB][6], F[NB][6];
    alignas(16) float Acc[NB][6];  // contact phase: the bodies' bounding spheres (bsph) instead
    float Ib[NB][10], Ic[NB][10];  // m, h(3), I(xx yy zz xy xz yz)
    alignas(16) float Lp[smpl::kNpack + 4];  // packed unit-lower factor L (row K: ancestors in chain
                                             // order); Lp[kNpack] is the elimination's store sink
    float cx[MAXC][3], cn[MAXC][3], cgap[MAXC];  // slot: point about o (a joint limit: its row), normal, gap
    int cbb[MAXC];                                // slot: body0 | (body1 + 2) << 8
    float lam[W];  // impulses of the last solve (lane = row): the warm-start cache and the forces
    float cf[NB][3];
    float dforce[ND];
    float root_pos[3], root_q[4];
    float qloc[NB][4];  // each joint's local rotation exp(q_b), from the kinematics (reused by integrate)
    int nc, nterr;                 // contact slots, of which limits + terrain (slots [0, nterr))
    int nlim;                      // joint-limit slots [0, nlim) (one row each: rows [0, nlim))
    uint32_t limmask;              // bodies whose joint-angle limit row is emitted this substep
    int ncand;                     // contacts generated (dropped = ncand - nc), last substep
    alignas(8) int imbook[14];     // fused imitation: the env's bookkeeping + motion metadata (ImitBook)
    unsigned long long sch_t0;     // dispatch order: the workgroup's start cycle (PhysArgs.cost)
    int sch_e;                     // this workgroup's env (PhysArgs.order; no register held through the substeps)
    int ckey[MAXC];                // 16-bit key of each slot's normal row (include/humanoid_engine.h)
    int wckey[W];                  // the previous solve's row keys (its impulses: lam)
    int nwc;                       // rows cached in wckey / lam
    int8_t tbase[NB], tcnt[NB];    // body b's terrain contacts: slots tbase[b] .. + tcnt[b]
    int8_t srow0[MAXC];            // first solver row of each slot
    int8_t rslot[W], rkind[W];     // solver row -> its slot, its kind (0 normal / limit, 1 2 tangential, 3 torsional)
    BodyTopo T;
    float Q[NG];  // external wrenches' and dof actuations' generalized force of this physics step (ext_wrench_terms; the EXT kernels only)
};

// LDS words that serve twice within a substep (the contract a kernel split has to keep):
//   IS   CRBA operand until factor_free; then gen_contacts' candidate gaps / bodies / rank order
//        (cand_gaps, cand_bodies, cand_order); from row_setup to contact_forces_out the rows' linear
//        directions (row_dirs, over the rank order's words: the reduction is done by then)
//   lam  the previous solve's impulses until substep() has read them (lam_prev); self_pairs' survivor
//        list; from row_setup to the solve's set-up the rows' friction bound weights; then the new
//        impulses
//   Ic / Ib  composite / own inertias; from terrain_candidates to the end of gen_contacts the bodies'
//        world segments live in Ib (PGS) or Ic (TGS: Ib keeps the own inertias for tgs_bias_at)
//   Acc  RNEA accelerations until body_forces; the external wrenches' subtree sums (ext_wrench_terms,
//        the EXT kernels); the midpoint's body forces; from terrain_candidates the
//        bounding spheres (bsph) and, after them, build_rows' patch radii (patch_radius), both dead
//        after row_setup; then tgs_bias_at's body forces
//   F    subtree forces until bias_midpoint's correction; build_rows' patch normals and centroids
//        until row_setup; then tgs_bias_at's joint velocities
//   V    body velocities until bias_midpoint / the row set-up; tgs_bias_at's scratch after
//   uf   PGS: midpoint velocity, then the solved velocity; TGS: the bias at the working velocity

// Work that nothing reads, left out (DESIGN §4.1 "Unread work"), each piece behind a switch of its own
// (1: left out, the default; 0: the parent's code, for tools/build_variant.py's A/B builds):
//   HE_REPORT_LAST_ONLY  dof_force and contact_forces are stored once per launch, from what the last
//        physics step left in LDS: the steps before it skip the iterations' drive sums, the drive and
//        joint-limit force outputs, the rows' force directions and the zeroing of cf
//   HE_LEG_ZROWS         the leg class of the <= 32-row TGS solve never reads Zh past dof KZ - 1: J^T's
//        zero fill and sign pass stop there (he_phys_rows.h RowSystem::zshort)
//   HE_RANK_ON_DEMAND    a box's corners are ranked only when some box has more than four candidates
#ifndef HE_REPORT_LAST_ONLY
#define HE_REPORT_LAST_ONLY 1
#endif
#ifndef HE_LEG_ZROWS
#define HE_LEG_ZROWS 1
#endif
#ifndef HE_RANK_ON_DEMAND
#define HE_RANK_ON_DEMAND 1
#endif
// whether a physics step computes the reported forces: the launch's last step (wave-uniform)
HE_DEV bool reports(bool last) { return !HE_REPORT_LAST_ONLY || last; }

// wave priority: s_setprio 3 over the serial chains (PGS rows, the elimination, the L^-T sweeps;
// +2.8 % A/B, r01; the midpoint's L^-1 and L^-T sweeps, -1.2 % physics launch A/B, r04) against the
// partner wave's throughput phases, 0 elsewhere
constexpr int kPrioSerial = 3;
constexpr int kPrioDefault = 0;

// wave-level ordering point: one wave per workgroup, LDS executes its instructions in order, so
// only the compiler must not move memory operations across phase boundaries
HE_DEV void sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

HE_DEV int dof_body(int i) { return i < 6 ? 0 : (i - 6) / 3 + 1; }

// A phase's own view of LDS and of the lane id, built from nothing that is live: an opaque zero
// offset on the LDS window (substep's lds_off, taken again) and the lane from the wave's mbcnt (one
// wave per workgroup: threadIdx.x). A per-lane LDS address formed from these is rebuilt beside its use
// (one or two integer VALU) instead of being hoisted out of the position iterations as a loop
// invariant, parked in scratch there and fetched back in front of the LDS read that needs it: a
// memory round trip on the step's dependent path (spills). (The mbcnt pair as volatile
// assembly: the builtins are merged with threadIdx.x's and hoisted like it.)
HE_DEV Lds& phase_lds() {
    extern __shared__ float smem[];
    int off = 0;
    asm volatile("" : "+v"(off));
    return *reinterpret_cast<Lds*>(reinterpret_cast<char*>(smem) + off);
}
HE_DEV int phase_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// a wave-uniform value into an SGPR (SGPRs that run out are parked in VGPR lanes, a v_readlane away;
// a uniform value left in a VGPR across the iterations is parked in scratch)
HE_DEV float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
HE_DEV int opaque_s(int x) {
    asm volatile("" : "+s"(x));
    return x;
}

// optional per-phase cycle stamps (diagnostic: PhysArgs.stamps != null), lane 0 accumulates
// s_memtime deltas per phase into stamps[block * HE_STAMP_SLOTS + phase] with a no-return vector
// atomic add (a load-add-store would put one global round trip into every phase it opens)
// phase ids of STAMP: the slot of each phase in PhysArgs.stamps. The other end is the PHASES list of
// tools/phase_profile.py (the same order, the same values); slots 14-19 are carved out of the contact
// generation, 20-21 out of the rows, 22 out of the PGS, 25-28 are the midpoint bias, 29-31 the TGS
// iterations
enum Phase : int {
    PH_KINEMATICS = 0, PH_INERTIA_RNEA, PH_SUBTREE_SUMS, PH_DRIVES, PH_CRBA, PH_FACTOR, PH_FREE_SOLVE,
    PH_CONTACT_GEN, PH_ZROWS, PH_DELASSUS, PH_PGS, PH_DU_SOLVE, PH_INTEGRATE, PH_FINAL_FK,
    PH_LIMIT_SLOTS, PH_SELF_SLOTS, PH_TERRAIN_RANK, PH_TERRAIN_SLOTS, PH_TERRAIN_GEOM, PH_SELF_SEGMENTS,
    PH_ROWS_JT, PH_ROWS_LT, PH_PGS_SETUP, PH_UNUSED, PH_FUSED,
    PH_MID_UM, PH_MID_RNEA, PH_MID_SUBTREE, PH_MID_LT, PH_TGS_BIAS, PH_TGS_RHS, PH_TGS_NEXT
};
static_assert(PH_FUSED == 24 && PH_TGS_NEXT == 31 && PH_TGS_NEXT < HE_STAMP_SLOTS, "phase ids: tools/phase_profile.py PHASES");
#ifndef HE_PHASE_STAMPS
#define HE_PHASE_STAMPS 0  // diagnostic twin library only (build.py PHASES_LIB)
#endif
struct Stamps { unsigned long long *slots, t_prev; };  // the env's slots (null: off), the last stamp's cycle count
#if !HE_PHASE_STAMPS
#define STAMP(id) \
    do {          \
    } while (0)
#else
#define STAMP(id) /* needs `Stamps& st` and `lane` in scope */                        \
    do {                                                                              \
        if (st.slots && lane == 0) {                                                  \
            unsigned long long _t = __builtin_readcyclecounter();                     \
            __hip_atomic_fetch_add(st.slots + (id), _t - st.t_prev, __ATOMIC_RELAXED, \
                                   __HIP_MEMORY_SCOPE_AGENT);                         \
            st.t_prev = _t;                                                           \
        }                                                                             \
    } while (0)
#endif

// the bodies' bounding spheres of the self-collision cull, in the RNEA acceleration scratch (dead
// from the midpoint bias until the next substep's kinematics)
HE_DEV float4* bsph(Lds& L) { return reinterpret_cast<float4*>(&L.Acc[0][0]); }
static_assert(sizeof(float4) * NB <= sizeof(float) * 6 * NB, "bounding spheres fit the Acc scratch");

// gen_contacts' reduction scratch in IS (dead after the CRBA): the contact candidates' gaps in
// candidate order [0, kCand), their bodies (-1: a self pair) [kCand, 2 kCand), the rank order
// [2 kCand, 3 kCand). After the reduction the last range holds the rows' linear directions (row_dirs,
// written by row_setup, read by contact_forces_out).
constexpr int kCand = 128;  // contact candidates considered by the reduction (a lying body: ~30)
static_assert(3 * kCand <= NG * 6, "reduction scratch fits IS");
static_assert(2 * kCand + 3 * W <= NG * 6, "per-row force directions fit IS");
HE_DEV float* cand_gaps(Lds& L) { return &L.IS[0][0]; }
HE_DEV int* cand_bodies(Lds& L) { return reinterpret_cast<int*>(&L.IS[0][0] + kCand); }
HE_DEV int* cand_order(Lds& L) { return reinterpret_cast<int*>(&L.IS[0][0] + 2 * kCand); }
HE_DEV float* row_dirs(Lds& L) { return &L.IS[0][0] + 2 * kCand; }

// build_rows' patch radii: the Acc words after the bounding spheres (read by row_setup)
HE_DEV float* patch_radius(Lds& L) { return &L.Acc[0][0] + 4 * NB; }
static_assert(5 * NB <= 6 * NB, "patch radii fit Acc after the bounding spheres");

}  // namespace
