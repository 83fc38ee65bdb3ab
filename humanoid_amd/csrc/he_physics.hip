// he_physics.hip -- articulated SMPL-humanoid step for gfx950 (replaces
// gym.simulate x control_freq_inv, puffer_phc/envs/humanoid_phc.py:131-134).
//
// Mapping: one environment per 64-lane workgroup (= one wave), all substeps of a policy step in
// one launch; HBM sees one coalesced read of the env's root/dof/target rows and one write of the
// root/dof/rigid-body/contact/dof-force rows. A workgroup is a single wave, so LDS hand-offs between
// phases need program order only (LDS executes a wave's instructions in order); no s_barrier is issued.
//
// One translation unit (the library's device_code_id and the parity records tied to it
// hash this TU's code object), its source by phase:
//   he_phys_lds.h       sizes, BodyTopo, Lds and the words that serve twice, the LDS accessors, sync,
//                       phase_lds / phase_lane, priorities, phase stamps
//   he_phys_spatial.h   spatial algebra, rotation exp / log
//   he_phys_lanes.h     cross-lane primitives, the reduce-scatter butterfly, lane predicates
//   he_phys_tree.h      subtree sums, pointer jumping, kinematics, joint limits, integration
//   he_phys_dynamics.h  body forces, external terms, drives, CRBA + factorisation, midpoint bias, the
//                       TGS iterations' bias / free motion / velocity update
//   he_phys_contacts.h  terrain and segment geometry, contact slots (gen_contacts)
//   he_phys_rows.h      solver rows, J^T and Delassus on the matrix cores (build_rows .. row_system)
//   he_phys_solve.h     the sweeps, the PGS and TGS solves, drive and contact force outputs
//   this file           the fused imitation epilogue's include, substep, the tables / state / cache
//                       loads and stores, physics_body, the kernels, the order kernel, the launchers
//
// The phases of one substep, in the order substep() runs them, each forced inline. Values that cross a
// phase boundary in registers travel in small structs (SROA dissolves them), all else in LDS. Every
// phase ends on a sync() unless its comment says otherwise (fp64 reference
// oracle/he_oracle_physics.c):
//   both   kinematics -> body_forces -> subtree_levels -> (EXT: ext_wrench_terms) -> drive_terms ->
//          factor_free (CRBA, sparse LTDL, yh = D^-1/2 L^-T dt rhs) -> prefetch_geometry ->
//          gen_contacts -> build_rows -> row_setup -> row_system (Zh = D^-1/2 L^-T J^T, A = Zh Zh^T)
//   PGS    (solver_type 0) bias_midpoint after the factorisation; solve_pgs -> pgs_velocity (no rows:
//          free_velocity) -> contact_forces_out, pgs_drive_out (last substep) -> integrate_bodies
//   TGS    (solver_type 1) K position iterations of hs = dt / K on the step's factor and contact set:
//          solve_tgs_rows (no rows: tgs_free_iterations), each iteration one sweep -> reduce_scatter_z
//          -> tgs_velocity -> tgs_advance (last substep: tgs_drive_acc; integrate_bodies, every second iteration
//          tgs_bias_at, tgs_rhs); then tgs_drive_out, contact_forces_out (last substep)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/humanoid_engine.h"
#include "he_kernels.h"
#include "he_math.h"
#include "he_phys_contacts.h"
#include "he_phys_dynamics.h"
#include "he_phys_lanes.h"
#include "he_phys_lds.h"
#include "he_phys_rows.h"
#include "he_phys_solve.h"
#include "he_phys_spatial.h"
#include "he_phys_tree.h"
#include "he_regla.h"
#include "he_smpl_topo.h"
#include "he_topo.h"

namespace {

// ---------------------------------------------------------------------------------- fused imitation
// he_env_step's imitation step (reward / reset / observations + the device reset of flagged envs)
// as the physics kernel's epilogue, from the post-step state in LDS: the same code as the stand-alone
// imitation kernel (he_imitation_env.h), with its float32 rounding (no contraction)
constexpr int GROUP = 32;
constexpr int HOT = HE_MOTION_HOT;
constexpr int COLD = HE_MOTION_COLD;
#pragma clang fp contract(off)
#include "he_imitation_env.h"
#pragma clang fp contract(fast)

// body b's rigid-body row (he_get_buffer RB_STATE layout) from the final kinematics: origin, world
// rotation, linear velocity of the origin, angular velocity
HE_DEV SimBody body_row(const Lds& L, int b) {
    SimBody s;
    const f3 r = f3{L.pw[b][0], L.pw[b][1], L.pw[b][2]};  // about o
    s.pos = f3{L.root_pos[0], L.root_pos[1], L.root_pos[2]} + r;
    s.rot = f4{L.qw[b][0], L.qw[b][1], L.qw[b][2], L.qw[b][3]};
    const f3 w = f3{L.V[b][0], L.V[b][1], L.V[b][2]};
    s.vel = f3{L.V[b][3], L.V[b][4], L.V[b][5]} + cross3(w, r);
    s.ang = w;
    return s;
}

// ---------------------------------------------------------------------------------- one substep
template <bool TGS, bool EXT>
HE_DEV void substep(Lds& L0, const PhysArgs& a0, const he_model* mp, int lane,
                    const float* mass_scale, float mu, int tkind, Stamps& st, bool first, bool last, bool ext_on) {
    // the launch arguments through an opaque offset too: their fields are re-read (scalar loads
    // from the kernarg segment) where used instead of being held in SGPRs across the substep loop
    int ao = 0;
    asm volatile("" : "+s"(ao));
    const PhysArgs& a = *reinterpret_cast<const PhysArgs*>(reinterpret_cast<const char*>(&a0) + ao);
    // opaque per substep: keeps the compiler from hoisting ~1k uniform model loads out of the
    // substep loop into SGPRs (which then spill into VGPR lanes)
    // (an opaque byte offset rather than an opaque pointer: the pointer keeps its global address
    // space, so the loads stay global_load / s_load instead of flat_load)
    int mo = 0;
    asm volatile("" : "+s"(mo));
    const he_model& m = *reinterpret_cast<const he_model*>(reinterpret_cast<const char*>(mp) + mo);
    // likewise an opaque VGPR base for LDS: addresses become base + immediate offset instead of
    // hundreds of hoisted uniform address constants
    int lds_off = 0;
    asm volatile("" : "+v"(lds_off));
    Lds& L = *reinterpret_cast<Lds*>(reinterpret_cast<char*>(&L0) + lds_off);
    // and the lane id: the many per-lane predicates of the unrolled algebra are then rebuilt
    // next to their use instead of being hoisted as loop invariants (TGS: taken afresh, so that the
    // kernel's own copy does not wait in scratch for the next substep's entry)
    if constexpr (TGS) lane = phase_lane();
    else asm volatile("" : "+v"(lane));
    const BodyTopo& T = L.T;
    const he_sim_params& p = a.p;
    const float dt = p.dt;
    // TGS (solver_type 1, oracle substep_tgs): K position iterations of hs = dt / K on this step's
    // factor and contact set; PGS: one step of hs = dt
    const int K = TGS ? (p.solver_iterations < 1 ? 1 : (p.solver_iterations > kTgsMaxIt ? kTgsMaxIt : p.solver_iterations)) : 1;
    // TGS: hs (and damp below) in SGPRs, so that neither is a VGPR value parked across the iterations
    const float hs = TGS ? uniform(dt / (float)K) : dt;
    __builtin_amdgcn_s_setprio(kPrioDefault);
    kinematics<true>(L, m, lane, a.p, !first);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    STAMP(PH_KINEMATICS);
    body_forces(L, m, p, lane, mass_scale);
    STAMP(PH_INERTIA_RNEA);
    // ---- subtree sums: F_b (forces) and composite inertias, in place by body levels
    __builtin_amdgcn_s_setprio(kPrioDefault);
    subtree_levels<16, smpl::kNumBodyLevels - 2>(&L.F[0][0], &L.Ic[0][0], lane);
    __builtin_amdgcn_s_setprio(kPrioDefault);
    STAMP(PH_SUBTREE_SUMS);
    if constexpr (EXT) ext_wrench_terms(L, m, a, lane, ext_on);
    drive_terms<TGS, EXT>(L, m, p, lane, hs);
    STAMP(PH_DRIVES);
    factor_free(L, m, lane, hs, st);
    STAMP(PH_FACTOR);
    if (!TGS && p.bias_midpoint) bias_midpoint(L, T, lane, p, st);
    GeomPrefetch g;
    prefetch_geometry(L, m, lane, g);
    STAMP(PH_FREE_SOLVE);
    // the previous solve's impulses (lane = row) before the self-pair list reuses L.lam as scratch
    const float lam_prev = L.lam[lane];
    const int nc = gen_contacts<TGS>(L, g, p, tkind, lane, last, st);
    const int nr = build_rows(L, lane, nc);
    STAMP(PH_CONTACT_GEN);
    RowDesc rd;
    row_setup(L, lane, nr, mu, lam_prev, last, rd);
    const float damp = TGS ? uniform(1.0f / (1.0f + dt * p.angular_damping)) : 1.0f / (1.0f + dt * p.angular_damping);
    TgsStep ts{K, hs, damp, last, 0.f, 0.f};
    if (nr > 0) {
        RowSystem rsys;
        row_system<TGS>(L, T, p, a.full_dofs, lane, nr, hs, rd, rsys, st);
        STAMP(PH_DELASSUS);
        float lamv;
        if constexpr (TGS) {
            lamv = solve_tgs_rows<EXT>(L, T, p, lane, nr, rd, rsys, ts, st);
        } else {
            lamv = solve_pgs(L, p, lane, nr, rd, rsys, st);
            pgs_velocity(L, T, lane, rsys.z, lamv);
        }
        if (last) contact_forces_out(L, lane, nc, rd.act, lamv, dt);
    }
    if (nr == 0) {  // nothing to warm-start the next solve from
        L.lam[lane] = 0.f;
        if (lane == 0) L.nwc = 0;
    }
    if (TGS && nr == 0) tgs_free_iterations<EXT>(L, T, p, lane, ts, st);
    if (!TGS && nr == 0) free_velocity(L, T, lane);
    STAMP(PH_DU_SOLVE);
    if constexpr (TGS) {  // TGS: the iterations integrated the positions and set the drive force
        if constexpr (EXT) {
            if (last) ext_actuation_out(L, a, lane);
        }
        STAMP(PH_INTEGRATE);
        return;
    }
    // ---- PGS: drive force actually applied, damping, clamps, write velocities
    if (last) pgs_drive_out(L, lane, nr, dt);
    if constexpr (EXT) {
        if (last) ext_actuation_out(L, a, lane);
    }
    integrate_bodies(L, T, lane, p, dt, damp, L.uf, true, !last);
    STAMP(PH_INTEGRATE);
}

// ---------------------------------------------------------------------------------- kernel body
// body-level and per-dof tree tables into LDS (constant memory -> LDS once per launch)
HE_DEV void load_tables(Lds& L, const PhysArgs& a, int lane) {
    const he_model& m = *a.model;
    if (lane < NB) {
        const PhysTopo& T = *a.topo;
        L.T.depth[lane] = T.body_depth[lane];
        for (int k = 0; k < 9; ++k) L.T.chain[lane][k] = T.body_chain[lane][k];
        L.T.dof0[lane] = T.body_dof0[lane];
        L.T.anc_mask[lane] = T.anc_mask[lane];
        L.T.sub_mask[lane] = T.sub_mask[lane];
        L.T.jump4[lane] = kJump4.v[lane < NB ? lane : 0];
        for (int c = 0; c < 3; ++c) L.T.local_pos[lane][c] = m.local_pos[lane][c];
    }
    L.T.cbody[lane] = a.topo->corner_body[lane];
    for (int i = lane; i < NG; i += W) {
        L.T.pack_start[i] = (int16_t)smpl::kPackStart[i];
        L.T.dof_depth[i] = (int8_t)(smpl::kDofNanc[i] - 1);
    }
}

// env e's root and dof rows into LDS, with the PD targets of this step (from the actions when given,
// written back to dof_targets)
HE_DEV void load_state(Lds& L, const PhysArgs& a, int e, int lane) {
    const float* rs = a.root_states + (size_t)e * 13;
    if (lane < 3) { L.root_pos[lane] = rs[lane]; L.u0[3 + lane] = rs[7 + lane]; L.u0[lane] = rs[10 + lane]; }
    if (lane < 4) L.root_q[lane] = rs[3 + lane];
    for (int d = lane; d < ND; d += W) {
        L.q[d] = a.dof_state[((size_t)e * ND + d) * 2];
        L.u0[6 + d] = a.dof_state[((size_t)e * ND + d) * 2 + 1];
        float t;
        if (a.actions) {  // humanoid_phc.py:1218-1228 + freeze :116-125
            float act = a.actions[(size_t)e * ND + d];
            if (a.clip_actions) act = fminf(fmaxf(act, -1.f), 1.f);
            t = a.frozen[d] ? 0.f : a.pd_offset[d] + a.pd_scale[d] * act;
            a.dof_targets[(size_t)e * ND + d] = t;
        } else {
            t = a.dof_targets[(size_t)e * ND + d];
        }
        L.tgt[d] = t;
    }
}

// The warm-start cache (include/humanoid_engine.h HE_CACHE_WORDS): words 0..6 the root pose as a
// signature, word 7 the row count, HE_CACHE_KEYS.. the 16-bit row keys (rows 2j / 2j + 1 in word j),
// HE_CACHE_LAMBDA.. the impulses. Lane = word, then word W + lane.
static_assert(HE_CACHE_KEYS + (MAXR + 1) / 2 <= HE_CACHE_LAMBDA && HE_CACHE_LAMBDA + MAXR <= HE_CACHE_WORDS &&
              HE_CACHE_WORDS <= 2 * W && HE_CACHE_LAMBDA < W, "cache layout");
// unpack into wckey / lam / nwc: valid while the root pose still equals the signature the previous
// step wrote (an external write -- a reset -- breaks it)
HE_DEV void cache_load(Lds& L, const PhysArgs& a, int e, int lane) {
    const float* rs = a.root_states + (size_t)e * 13;
    const float* cw = a.cache ? a.cache + (size_t)e * HE_CACHE_WORDS : nullptr;
    const float w1 = cw ? cw[lane] : 0.f;
    const float w2 = cw && lane < HE_CACHE_WORDS - W ? cw[W + (lane < HE_CACHE_WORDS - W ? lane : 0)] : 0.f;
    const float sig = lane < 3 ? rs[lane] : (lane < 7 ? rs[lane < 7 ? lane : 0] : 0.f);
    const bool diff = lane < 7 && __float_as_uint(w1) != __float_as_uint(sig);
    const bool valid = cw && a.p.warm_start && __ballot(diff) == 0ull;
    const int nw = valid ? __builtin_amdgcn_readlane(__float_as_int(w1), 7) : 0;
    const int nwc = nw < 0 ? 0 : (nw > MAXR ? MAXR : nw);
    constexpr int KW = (MAXR + 1) / 2;
    if (lane >= HE_CACHE_KEYS && lane < HE_CACHE_KEYS + KW) {
        const int j = lane - HE_CACHE_KEYS;
        const uint32_t kw = __float_as_uint(w1);
        L.wckey[2 * j] = (int)(kw & 0xFFFFu);
        L.wckey[2 * j + 1] = (int)(kw >> 16);
    }
    // impulses: rows 0 .. W - HE_CACHE_LAMBDA - 1 from the first read, the rest from the second
    if (lane >= HE_CACHE_LAMBDA) L.lam[lane - HE_CACHE_LAMBDA] = valid ? w1 : 0.f;
    if (lane < HE_CACHE_LAMBDA) L.lam[W - HE_CACHE_LAMBDA + lane] = valid && W + lane < HE_CACHE_WORDS ? w2 : 0.f;
    if (lane == 0) L.nwc = nwc;
}
// pack the last solve's rows: signature (the root pose just written), row count, row keys, impulses
HE_DEV void cache_store(const Lds& L, const PhysArgs& a, int e, int lane) {
    if (!a.cache) return;
    float* cw = a.cache + (size_t)e * HE_CACHE_WORDS;
    const int nwc = a.p.warm_start ? L.nwc : 0;
    constexpr int KW = (MAXR + 1) / 2;
    float v = 0.f;
    if (lane < 3) v = L.root_pos[lane];
    else if (lane < 7) v = L.root_q[lane < 7 ? lane - 3 : 0];
    else if (lane == 7) v = __int_as_float(nwc);
    else if (lane < HE_CACHE_KEYS + KW) {
        const int j = lane - HE_CACHE_KEYS;
        const uint32_t k0 = 2 * j < nwc ? (uint32_t)L.wckey[2 * j] & 0xFFFFu : 0u;
        const uint32_t k1 = 2 * j + 1 < nwc ? (uint32_t)L.wckey[2 * j + 1] & 0xFFFFu : 0u;
        v = __uint_as_float(k0 | (k1 << 16));
    } else if (lane >= HE_CACHE_LAMBDA) v = lane - HE_CACHE_LAMBDA < nwc ? L.lam[lane - HE_CACHE_LAMBDA] : 0.f;
    if (!a.p.warm_start) v = 0.f;
    cw[lane] = v;
    if (lane < HE_CACHE_WORDS - W) {
        const int r = W - HE_CACHE_LAMBDA + lane;
        cw[W + lane] = a.p.warm_start && r < nwc ? L.lam[r] : 0.f;
    }
}

// env e's outputs from LDS after the final kinematics: generalized state, rigid-body rows (lane =
// body), forces, contact counts. Returns the lane's body row (the fused epilogue reads its body from
// the same registers).
HE_DEV SimBody store_state(const Lds& L, const PhysArgs& a, int e, int lane) {
    float* rso = a.root_states + (size_t)e * 13;
    if (lane < 3) { rso[lane] = L.root_pos[lane]; rso[7 + lane] = L.u0[3 + lane]; rso[10 + lane] = L.u0[lane]; }
    if (lane < 4) rso[3 + lane] = L.root_q[lane];
    for (int d = lane; d < ND; d += W) {
        a.dof_state[((size_t)e * ND + d) * 2] = L.q[d];
        a.dof_state[((size_t)e * ND + d) * 2 + 1] = L.u0[6 + d];
        a.dof_force[(size_t)e * ND + d] = L.dforce[d];
    }
    const SimBody sb = body_row(L, lane < NB ? lane : 0);
    if (lane < NB) {
        float* rb = a.rb_state + ((size_t)e * NB + lane) * 13;
        rb[0] = sb.pos.x; rb[1] = sb.pos.y; rb[2] = sb.pos.z;
        rb[3] = sb.rot.x; rb[4] = sb.rot.y; rb[5] = sb.rot.z; rb[6] = sb.rot.w;
        rb[7] = sb.vel.x; rb[8] = sb.vel.y; rb[9] = sb.vel.z;
        rb[10] = sb.ang.x; rb[11] = sb.ang.y; rb[12] = sb.ang.z;
    }
    for (int t = lane; t < NB * 3; t += W) a.contact_forces[(size_t)e * NB * 3 + t] = L.cf[t / 3][t % 3];
    if (lane == 0 && a.num_contacts) a.num_contacts[e] = L.nc;
    if (lane == 0 && a.dropped) a.dropped[e] = L.ncand - L.nc;
    return sb;
}

// two waves per SIMD need at most 256 VGPRs + AGPRs. Unbounded, the allocator lands at 257 (one
// kernel-lifetime value parked in an AGPR) and the kernel falls to one wave per SIMD; the bound
// makes it fit without scratch. humanoid_amd/build.py checks the compiler's occupancy report and
// fails the build below 2 waves per SIMD either way. (Round 3 A/B, profiles/r03/ab_lt_pipe.txt:
// the pipelined midpoint L^-T with the bound +3.0 % against the grouped one without it, which
// fits in 251 unbounded.)
#ifndef HE_MIN_WAVES
#define HE_MIN_WAVES 2
#endif
template <bool TGS, bool EXT>
HE_DEV void physics_body(const PhysArgs& a) {
    extern __shared__ float smem[];
    Lds& L = *reinterpret_cast<Lds*>(smem);
    if ((int)blockIdx.x >= a.num_envs) return;  // the first-dispatch warm-up (warm_physics_kernels): no env
    int lane = threadIdx.x;
    // the env of this workgroup (launch_physics_order: heavy envs first); it and the start cycle wait
    // in LDS for the epilogue (no registers held through the substeps)
    // The order is rebuilt on the launch stream (he_engine.cpp); an index outside [0, num_envs) (a
    // stray write into the buffer) falls back to workgroup id = env instead of faulting.
    int e = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)e >= (unsigned)a.num_envs) e = (int)blockIdx.x;
    if (lane == 0) {
        L.sch_t0 = __builtin_readcyclecounter();
        L.sch_e = e;
    }
    // ---- tables, state, warm-start cache (TGS: each with a lane of its own, a short live range)
    load_tables(L, a, TGS ? phase_lane() : lane);
    load_state(L, a, e, TGS ? phase_lane() : lane);
    cache_load(L, a, e, TGS ? phase_lane() : lane);
    if constexpr (TGS) lane = phase_lane();
    if (a.fused && lane == 0) {  // fused imitation: bookkeeping + motion metadata (trips 1, 2) now
        const ImitArgs& im = a.im;
        const int64_t mid = clamp_mid(im.m, im.motion_ids[e]);
        const ImitBook bk = imitation_book(im, mid, f3{im.global_offset[3 * e], im.global_offset[3 * e + 1],
                                                       im.global_offset[3 * e + 2]},
                                           im.start_times[e], im.start_offsets[e], im.progress[e]);
        __builtin_memcpy(L.imbook, &bk, sizeof(ImitBook));
    }
    sync();
    if (a.p.joint_limits) {  // the first substep's limit rows, from the loaded state
        const bool joint = lane >= 1 && lane < NB;
        const int d = 3 * (joint ? lane - 1 : 0);
        limit_detect(L, lane, joint, f3{L.q[d], L.q[d + 1], L.q[d + 2]}, f3{L.u0[6 + d], L.u0[7 + d], L.u0[8 + d]}, a.p);
        sync();
    }
    const float* ms = a.mass_scale ? a.mass_scale + (size_t)e * NB : nullptr;
    // wave-uniform, into an SGPR: in a VGPR it is parked in scratch from one row set-up to the next
    const float mu = uniform(a.friction ? a.friction[e] : a.p.friction);
    int tk = (a.p.terrain && a.terrain_kind) ? a.terrain_kind[e] : 0;
    Stamps st{a.stamps ? a.stamps + (size_t)e * HE_STAMP_SLOTS : nullptr, __builtin_readcyclecounter()};
    // ---- substeps
    for (int s = 0; s < a.substeps; ++s) {
        // EXT: the wrench acts in the launch's leading ext_steps physics steps. The step at which its
        // hold ends starts as a launch's first step does (the joints' rotations from their angles, not
        // the integrator's cached ones), so one launch over the end of a hold gives the bits of two
        // launches split there.
        const bool first = EXT ? s == 0 || s == a.ext_steps : s == 0;
        substep<TGS, EXT>(L, a, a.model, lane, ms, mu, tk, st, first, s == a.substeps - 1, EXT && s < a.ext_steps);
    }
    // TGS: the epilogue's lane taken afresh, so that no address the prologue formed from the lane waits
    // in scratch through the substeps for the epilogue
    if constexpr (TGS) lane = phase_lane();
    // ---- fused imitation (he_env_step): the reference samples depend only on the env's motion
    // bookkeeping (read into LDS at the kernel's start), so their loads are issued here and land
    // behind the final kinematics and stores
    ImitRaw iraw;
    if (a.fused && lane < GROUP) {
        ImitBook bk;
        static_assert(sizeof(ImitBook) <= sizeof(L.imbook), "ImitBook fits its LDS words");
        __builtin_memcpy(&bk, L.imbook, sizeof(ImitBook));
        iraw = imitation_frames_load(a.im, lane, bk);  // loads only: the blends wait for the epilogue
    }
    // ---- outputs: generalized state, FK rigid-body state, forces
    e = L.sch_e;  // from LDS: not held through the substeps
    kinematics<false>(L, *a.model, lane, a.p, a.substeps > 0);
    STAMP(PH_FINAL_FK);
    const SimBody sb = store_state(L, a, e, lane);
    if (a.fused && lane < GROUP) {
        // he_env_step: the imitation step of this env on lanes 0..31 (lane = body), after every
        // physics store above has landed (a fused reset overwrites those rows)
        __threadfence_block();
        float pw = 0.0f;
        if (a.im.p.use_power_reward && lane < NB - 1)  // the joint's |tau . qdot| (humanoid_phc.py:1297-1305)
            pw = power_term(&L.dforce[3 * lane], &L.u0[6 + 3 * lane], 1);
        imitation_finish<false>(a.im, e, e, lane, lane == 0, imitation_frames_blend(iraw), sb, pw);
    }
    STAMP(PH_FUSED);
    cache_store(L, a, e, lane);
    if (a.cost && lane == 0) {  // this env's cycles, for the next launch's order
        const unsigned long long cyc = __builtin_readcyclecounter() - L.sch_t0;
        a.cost[e] = cyc > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cyc;
    }
}

// he_sim_params.solver_type 0 (PGS) and 1 (TGS): one instantiation each, so that the TGS iterations'
// register plan does not touch the PGS kernel's
__global__ void __launch_bounds__(64, HE_MIN_WAVES) physics_kernel(PhysArgs a) { physics_body<false, false>(a); }
__global__ void __launch_bounds__(64, HE_MIN_WAVES) physics_kernel_tgs(PhysArgs a) { physics_body<true, false>(a); }
// the same steps with external wrenches (PhysArgs.ext_wrench, he_apply_body_forces) and dof actuation
// forces (PhysArgs.dof_act, he_set_dof_actuation_forces): launched only while a wrench is pending or an
// actuation is set, so every other launch runs the two kernels above unchanged
__global__ void __launch_bounds__(64, HE_MIN_WAVES) physics_kernel_ext(PhysArgs a) { physics_body<false, true>(a); }
__global__ void __launch_bounds__(64, HE_MIN_WAVES) physics_kernel_tgs_ext(PhysArgs a) { physics_body<true, true>(a); }

}  // namespace

static_assert(sizeof(Lds) <= 20480, "two workgroups per SIMD (8 per CU) need <= 20 KB of LDS each");
size_t physics_lds_bytes() { return (sizeof(Lds) + 15) / 16 * 16; }

bool physics_phase_stamps() { return HE_PHASE_STAMPS != 0; }

namespace {
// launch_physics_order (he_kernels.h): one workgroup of 1024 threads (16 waves). The mean cost, then
// each env's class by its cost relative to the mean, kOrderClasses classes of mean / 32 from
// 0.5 x mean to 1.5 x mean (outside: the end classes; order_class), and order[] partitioned by
// class, the costliest class first: a longest-first order in steps of ~3 % of the mean. One pass
// sizes the classes, the second places every env after the costlier classes (order_wave).
constexpr int kOrderThreads = 1024;
constexpr int kOrderWaves = kOrderThreads / 64;
constexpr int kOrderClasses = 32;
// floor(32 c / mean) - 16 clamped to the classes, in integers (the host restates it exactly:
// tests/test_full_size.py): class >= m exactly when c >= T[m] = ceil((m + 16) tot / (32 n)), so the
// class is found by a binary search over the 31 thresholds (one 64-bit division per threshold, not
// per env)
__device__ __forceinline__ int order_class(uint32_t c, const uint32_t* thr) {
    int lo = 0;  // the largest m with c >= thr[m] (thr[0] = 0)
#pragma unroll
    for (int step = 16; step > 0; step >>= 1)
        if (lo + step < kOrderClasses && c >= thr[lo + step]) lo += step;
    return lo;
}
// Each wave takes the classes of its lanes' kOrderPer envs (env r0 + 1024 j + 64 w + lane, j <
// kOrderPer) one distinct class at a time (the first remaining element's class): the class's
// elements rank themselves by its ballots, and one lane adds their count to the class's LDS cursor
// (an atomic per distinct class and wave, not per env). The cursor's order between waves is the
// atomics', so envs of one class are not in env order; results do not depend on the order (envs
// never interact).
constexpr int kOrderPer = 4;
__device__ __forceinline__ void order_wave(const int (&k)[kOrderPer], int lane, int* cursor, int (&slot)[kOrderPer]) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long left[kOrderPer];
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) left[j] = __ballot(k[j] >= 0);
    for (;;) {
        int j0 = -1;
#pragma unroll
        for (int j = kOrderPer - 1; j >= 0; --j) j0 = left[j] ? j : j0;
        if (j0 < 0) break;
        int kc = 0;
#pragma unroll
        for (int j = 0; j < kOrderPer; ++j)
            if (j == j0) kc = __shfl(k[j], __builtin_ctzll(left[j]), 64);
        unsigned long long m[kOrderPer];
        int cnt = 0, before[kOrderPer];
#pragma unroll
        for (int j = 0; j < kOrderPer; ++j) {
            m[j] = __ballot(k[j] == kc);
            before[j] = cnt;
            cnt += __popcll(m[j]);
            left[j] &= ~m[j];
        }
        int b = 0;
        if (lane == 0) b = atomicAdd(&cursor[kc], cnt);
        b = __shfl(b, 0, 64);
#pragma unroll
        for (int j = 0; j < kOrderPer; ++j)
            if (k[j] == kc) slot[j] = b + before[j] + __popcll(m[j] & lt);
    }
}
__global__ void __launch_bounds__(kOrderThreads) physics_order_kernel(const uint32_t* cost, int32_t* order, int n) {
    __shared__ unsigned long long red[kOrderWaves];
    __shared__ int hist[kOrderClasses], cursor[kOrderClasses];
    __shared__ uint32_t thr[kOrderClasses];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    unsigned long long s = 0;
    for (int i = t; i < n; i += kOrderThreads) s += cost[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) red[w] = s;
    if (t < kOrderClasses) hist[t] = 0;
    __syncthreads();
    if (t < kOrderClasses) {
        unsigned long long tot = 0;
        for (int v = 0; v < kOrderWaves; ++v) tot += red[v];
        const unsigned long long d = 32ull * (unsigned long long)(n > 0 ? n : 1);
        const unsigned long long x = (unsigned long long)(t + 16) * tot;
        const unsigned long long T = t == 0 ? 0ull : (x + d - 1) / d;
        thr[t] = T > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)T;
    }
    __syncthreads();
    int k[kOrderPer], slot[kOrderPer];
    auto classes = [&](int r0) {
#pragma unroll
        for (int j = 0; j < kOrderPer; ++j) {
            const int e = r0 + kOrderThreads * j + t;
            k[j] = e < n ? order_class(cost[e], thr) : -1;
        }
    };
    for (int r0 = 0; r0 < n; r0 += kOrderPer * kOrderThreads) {  // the classes' sizes
        classes(r0);
        order_wave(k, lane, hist, slot);
    }
    __syncthreads();
    if (t == 0) {  // the costliest class first
        int acc = 0;
        for (int c = kOrderClasses - 1; c >= 0; --c) { cursor[c] = acc; acc += hist[c]; }
    }
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += kOrderPer * kOrderThreads) {
        classes(r0);
        order_wave(k, lane, cursor, slot);
#pragma unroll
        for (int j = 0; j < kOrderPer; ++j)
            if (k[j] >= 0) order[slot[j]] = r0 + kOrderThreads * j + t;
    }
}
}  // namespace

namespace {
__global__ void warm_tu_kernel() {}
}  // namespace

#define HE_RETURN_IF(x)                      \
    do {                                     \
        const hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_;     \
    } while (0)
hipError_t warm_physics_kernels(hipStream_t stream, int mode) {
    if (mode == 1) {
        warm_tu_kernel<<<1, 64, 0, stream>>>();
        return hipGetLastError();
    }
    PhysArgs pa{};
    physics_kernel<<<1, W, physics_lds_bytes(), stream>>>(pa);
    HE_RETURN_IF(hipGetLastError());
    physics_kernel_tgs<<<1, W, physics_lds_bytes(), stream>>>(pa);
    HE_RETURN_IF(hipGetLastError());
    physics_kernel_ext<<<1, W, physics_lds_bytes(), stream>>>(pa);
    HE_RETURN_IF(hipGetLastError());
    physics_kernel_tgs_ext<<<1, W, physics_lds_bytes(), stream>>>(pa);
    HE_RETURN_IF(hipGetLastError());
    physics_order_kernel<<<1, kOrderThreads, 0, stream>>>(nullptr, nullptr, 0);
    return hipGetLastError();
}

hipError_t launch_physics_order(const uint32_t* cost, int32_t* order, int num_envs, hipStream_t stream) {
    if (num_envs <= 0) return hipSuccess;
    physics_order_kernel<<<1, kOrderThreads, 0, stream>>>(cost, order, num_envs);
    return hipGetLastError();
}

hipError_t launch_physics(const PhysArgs& a, hipStream_t stream) {
    if (a.num_envs <= 0) return hipSuccess;
    const size_t lds = physics_lds_bytes();
    const bool ext = (a.ext_wrench && a.ext_steps > 0) || a.dof_act;  // a wrench pending or an actuation set
    if (ext && a.p.solver_type == 1) physics_kernel_tgs_ext<<<a.num_envs, W, lds, stream>>>(a);
    else if (ext) physics_kernel_ext<<<a.num_envs, W, lds, stream>>>(a);
    else if (a.p.solver_type == 1) physics_kernel_tgs<<<a.num_envs, W, lds, stream>>>(a);
    else physics_kernel<<<a.num_envs, W, lds, stream>>>(a);
    return hipGetLastError();
}
