// libhumanoid_solve.so: the solves with the joint-space inertia M a controller calls each step
// (include/humanoid_solve.h defines them). One launch, one 64-lane wave (= one block) per env, M never
// leaves the wave:
//   state      root row and the 69 (pos, vel) pairs into LDS; forward kinematics by tree level
//              (he_tree_state.h, the routine hd_dynamics.hip runs too, with the joints' accelerations
//              carried when the entry has any), the bodies' inertias and Newton-Euler wrenches about their
//              centres of mass,
//              their subtree sums about each joint's own origin, and per column the axis, the pivot and
//              F = I^c S (he_joint_space.h, which ht_task.hip shares);
//   solve_kernel (hs_forward_dynamics, hs_solve)
//              CRBA straight into regla::RegMat (lane j owns column j, H[i][j] = S_j . F_i on the
//              dof tree's pattern), the sparse L^T D L in registers (he_regla.h, deepest dof first, no
//              fill-in), the packed factor in LDS; then every right-hand side through
//              L^-T (solve_LT_vec_pipelined), D^-1 and L^-1 (solve_L_streamed), lane = dof. The k
//              vectors of hs_solve share the factor and take the same instructions one after another;
//   torque_kernel (hs_computed_torque)
//              no factorisation: w = RNEA at qdd = (0; qdd_des), the base block of M is the composite
//              inertia of the whole body (the root columns' F), a_b = M_bb^-1 (f_b - w_b) by a 6 x 6
//              L D L^T in every lane, tau = w - f + M_jb a_b with M_jb a_b = F_j . (a_b as a motion vector).
//              As hw_compute launches it (include/humanoid_wrench.h, hs_wrench.h) it also takes external
//              wrenches on the bodies and a prescribed base acceleration, and writes every joint's wrench
//              and every body's acceleration from what it has in LDS by then. As hg_compute launches it
//              (include/humanoid_derivatives.h, hs_derivs.h) it takes the whole generalised acceleration and
//              writes d tau / d q and d tau / d qd, a lane per direction, from its own pass through the tree.
// Spatial quantities of a subtree are referred to its own joint origin, never to a common far point: an
// entry of M is then exact to float32 of the descendant's own inertia (see columns()).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../include/humanoid_solve.h"
#include "he_host.h"
#include "he_joint_space.h"
#include "he_regla.h"
#include "he_topo.h"
#include "he_tree_state.h"
#include "hs_derivs.h"
#include "hs_wrench.h"

namespace {

static_assert(HS_FLAG_NO_GRAVITY == kFlagNoGravity, "columns() reads the flag");

struct Params {
    const TreeModel* model;
    const float* root;       // [N,13]
    const float* dof;        // [N*69,2]
    const float* gen_force;  // [N,75] or null
    const float* qdd_des;    // [N,69] (torque_kernel)
    const float* rhs;        // [N,k,75] (solve_kernel, k > 0)
    float* out;              // [N,75] qdd, or [N,k,75]; torque_kernel: tau [N,69] or null
    float* base_acc;         // [N,6] or null
    int k;                   // 0: forward dynamics
    uint32_t flags;
    // torque_kernel as hw_compute launches it (hs_wrench.h); all null from hs_computed_torque
    const float* base_acc_in;  // [N,6]: the prescribed base acceleration, or null (free base)
    const float* body_force;   // [N*24,3] or null
    const float* body_torque;  // [N*24,3] or null
    float* wrench;             // [N,24,6] or null
    float* body_acc;           // [N,24,6] or null
    int frame;                 // HW_FRAME_*
    // torque_kernel as hg_compute launches it (hs_derivs.h); all null from every other entry
    const float* acc;  // [N,75]: the generalised acceleration, or null (zero)
    float* dtau_dq;    // [N,75,75] or null
    float* dtau_dv;    // [N,75,75] or null
    float* tau_full;   // [N,75] or null
};

__global__ __launch_bounds__(kWave, 2) void solve_kernel(const Params P) {
    __shared__ Lds L;
    __shared__ Factor Fc;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    const bool hi = lane < NH;

    for (int i = lane; i < smpl::kNpack + 4; i += kWave) Fc.Lp[i] = 0.f;
    for (int i = lane; i < NG; i += kWave) {
        Fc.pack_start[i] = (int16_t)smpl::kPackStart[i];
        Fc.dof_depth[i] = (int8_t)(smpl::kDofNanc[i] - 1);
    }
    columns<false>(L, M, P, env, lane);  // ends on a barrier

    const int dj = Fc.dof_depth[lane], dj2 = hi ? Fc.dof_depth[kWave + lane] : 0;
    float D1 = 1.f, D2 = 1.f;
    {
        regla::RegMat H;
        H.cp[(NG + 1) / 2 - 1] = regla::f2v{0.f, 0.f};  // the pairs' unused halves
        H.cp2[(NH + 1) / 2 - 1] = regla::f2v{0.f, 0.f};
        const bool arm = (P.flags & HS_FLAG_ARMATURE) != 0;
        const float arm1 = arm && lane >= 6 ? M.armature[lane >= 6 ? lane - 6 : 0] : 0.f;
        const float arm2 = arm && hi ? M.armature[hi ? kWave - 6 + lane : 0] : 0.f;
        const ColS s1 = load_S(L.SF[lane], lane);
        const ColS s2 = load_S(L.SF[hi ? kWave + lane : NG - 1], NG - 1);
        regla::static_for<0, NG, 1>([&](auto i) { crba_row<decltype(i)::value>(H, L, s1, s2, arm1, arm2, lane); });
        // the factorisation carries one right-hand side along; the solves below replay it from the
        // stored factor instead, so that every vector of a call takes the same instructions
        float z1 = 0.f, z2 = 0.f;
        regla::factor_pipelined(H, D1, D2, Fc.Lp, dj, dj2, z1, z2);
    }
    __syncthreads();
    const float dinv1 = 1.f / D1, dinv2 = 1.f / D2;
    const float* row1 = Fc.Lp + Fc.pack_start[lane];
    const float* row2 = Fc.Lp + Fc.pack_start[hi ? kWave + lane : 0];

    const int k = P.k > 0 ? P.k : 1;
    for (int j = 0; j < k; ++j) {  // wave-uniform trip count
        float y1, y2 = 0.f;
        if (P.k > 0) {
            const float* b = P.rhs + (env * k + j) * NG;
            y1 = b[lane];
            if (hi) y2 = b[kWave + lane];
        } else {
            const float* f = P.gen_force ? P.gen_force + env * NG : nullptr;
            y1 = (f ? f[lane] : 0.f) - L.bias[lane];
            if (hi) y2 = (f ? f[kWave + lane] : 0.f) - L.bias[kWave + lane];
        }
        regla::solve_LT_vec_pipelined(Fc.Lp, dj, dj2, y1, y2);
        y1 *= dinv1;
        y2 *= dinv2;
        regla::solve_L_streamed(row1, row2, y1, y2);
        float* o = P.out + (env * k + j) * NG;
        o[lane] = y1;
        if (hi) o[kWave + lane] = y2;
    }
}

__global__ __launch_bounds__(kWave) void torque_kernel(const Params P) {
    __shared__ Lds L;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    if (P.dtau_dq || P.dtau_dv || P.tau_full) {  // hg_compute: its own path through the tree, in its own LDS
        extern __shared__ float deriv_lds[];
        derivatives(L, M, P, deriv_lds, env, lane);
        return;
    }
    if (P.qdd_des) {
        columns<true>(L, M, P, env, lane);  // L.bias = w, the RNEA force at qdd = (0; qdd_des); ends on a barrier
    } else {  // hw_compute without desired accelerations: everything at qdd = 0, which columns<false> is
        for (int d = lane; d < ND; d += kWave) L.qdd[d] = 0.f;
        columns<false>(L, M, P, env, lane);
    }
    if (P.body_force || P.body_torque) reaction_external(L, M, P, env, lane);

    // the base block of M: row i = (F_i's linear part, F_i's angular part) of root column i, the
    // composite inertia of the whole body about o. The same small solve in every lane.
    const float* f = P.gen_force ? P.gen_force + env * NG : nullptr;
    float y[6];
    if (P.base_acc_in) {  // prescribed base: no solve
#pragma unroll
        for (int i = 0; i < 6; ++i) y[i] = P.base_acc_in[env * 6 + i];
    } else {
        float A[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const v3 n = ld3(L.SF[i] + 6), p = ld3(L.SF[i] + 9);
            A[i][0] = p.x, A[i][1] = p.y, A[i][2] = p.z, A[i][3] = n.x, A[i][4] = n.y, A[i][5] = n.z;
            y[i] = (f ? f[i] : 0.f) - L.bias[i];
        }
        // A = Lb D Lb^T in place (lower triangle), then the two substitutions
        float dinv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            float d = A[j][j];
#pragma unroll
            for (int s = 0; s < j; ++s) d -= A[j][s] * A[j][s] * A[s][s];
            A[j][j] = d;
            dinv[j] = 1.f / d;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                float v = A[i][j];
#pragma unroll
                for (int s = 0; s < j; ++s) v -= A[i][s] * A[j][s] * A[s][s];
                A[i][j] = v * dinv[j];
            }
        }
#pragma unroll
        for (int i = 1; i < 6; ++i)
#pragma unroll
            for (int s = 0; s < i; ++s) y[i] -= A[i][s] * y[s];
#pragma unroll
        for (int i = 0; i < 6; ++i) y[i] *= dinv[i];
#pragma unroll
        for (int i = 4; i >= 0; --i)
#pragma unroll
            for (int s = i + 1; s < 6; ++s) y[i] -= A[s][i] * y[s];
    }

    if (P.base_acc && lane < 6) {
        float v = y[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) v = lane == i ? y[i] : v;
        P.base_acc[env * 6 + lane] = v;
    }
    if (P.out) {
        const bool arm = (P.flags & HS_FLAG_ARMATURE) != 0;
        const v3 al{y[0], y[1], y[2]}, aw{y[3], y[4], y[5]};
        for (int d = lane; d < ND; d += kWave) {
            const int c = 6 + d;
            float t = L.bias[c] - (f ? f[c] : 0.f);
            if (arm) t += M.armature[d] * L.qdd[d];
            // M_jb a_b = F_c . (a_b as a motion vector about the column's pivot: (aw, al + aw x pivot))
            t += dot(ld3(L.SF[c] + 9), al + cross(aw, ld3(L.SF[c] + 3))) + dot(ld3(L.SF[c] + 6), aw);
            P.out[env * ND + d] = t;
        }
    }
    if (P.wrench || P.body_acc) reaction_outputs(L, P, env, lane, v3{y[0], y[1], y[2]}, v3{y[3], y[4], y[5]});
}

}  // namespace

struct hs_solver : QueryHandle<TreeModel> {};
struct hw_reaction : QueryHandle<TreeModel> {};  // the second family's handle (include/humanoid_wrench.h)
struct hg_derivatives : QueryHandle<TreeModel> {};  // the third family's (include/humanoid_derivatives.h)

namespace {

// The refusals the entry points share, in the order the headers list them, around `own`, the
// entry point's own; then the launch. Every buffer of the call is in P; the handle is read last.
// flags_all: the entry's flag bits; lds: the dynamic LDS its path of the kernel indexes (hs_derivs.h).
template <class Handle, class Own>
int launch(Handle* h, const char* who, void (*kernel)(Params), Params& P, void* stream, Own own,
           uint32_t flags_all = HS_FLAGS_ALL, size_t lds = 0) {
    if (check_call(who, h, P.root, P.dof)) return 1;
    if (own()) return 1;
    if (check_flags(who, P.flags, flags_all)) return 1;
    if (check_aligned(who, {P.root, P.dof, P.gen_force, P.qdd_des, P.rhs, P.out, P.base_acc, P.base_acc_in, P.body_force,
                            P.body_torque, P.wrench, P.body_acc, P.acc, P.dtau_dq, P.dtau_dv, P.tau_full}))
        return 1;
    P.model = h->d_model;
    hipLaunchKernelGGL(kernel, dim3(h->num_envs), dim3(kWave), lds, static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char* hs_last_error(void) { return last_error(); }
int hs_version(void) { return 1; }

int hs_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    if (check_tree_depth(model)) return 1;
    return check_factored_tree(model);
}

int hs_create(int device, const he_model* model, const float gravity[3], int num_envs, hs_solver** out) {
    return query_create("hs_create", device, model, gravity, num_envs, out, hs_validate_model, fill_tree_model);
}

int hs_destroy(hs_solver* h) { return query_destroy(h); }

int hs_forward_dynamics(hs_solver* h, const float* root_state, const float* dof_state, const float* gen_force,
                        float* qdd_out, uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.gen_force = gen_force;
    P.out = qdd_out;
    P.k = 0;
    P.flags = flags;
    return launch(h, "hs_forward_dynamics", solve_kernel, P, stream,
                  [&] { return qdd_out ? 0 : fail("hs_forward_dynamics: null output buffer"); });
}

int hs_computed_torque(hs_solver* h, const float* root_state, const float* dof_state, const float* qdd_des,
                       const float* gen_force, float* tau_out, float* base_acc_out, uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.qdd_des = qdd_des;
    P.gen_force = gen_force;
    P.out = tau_out;
    P.base_acc = base_acc_out;
    P.flags = flags;
    return launch(h, "hs_computed_torque", torque_kernel, P, stream, [&] {
        if (!qdd_des) return fail("hs_computed_torque: null desired acceleration");
        if (!tau_out && !base_acc_out) return fail("hs_computed_torque: no output buffer");
        return 0;
    });
}

int hs_solve(hs_solver* h, const float* root_state, const float* dof_state, const float* rhs, float* out, int k,
             uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.rhs = rhs;
    P.out = out;
    P.k = k;
    P.flags = flags;
    return launch(h, "hs_solve", solve_kernel, P, stream, [&] {
        if (!rhs) return fail("hs_solve: null right-hand side");
        if (!out) return fail("hs_solve: null output buffer");
        if (rhs == out) return fail("hs_solve: rhs and out are the same buffer (the solve is not in place)");
        if (k < 1 || k > HS_MAX_RHS) return fail("hs_solve: k = %d outside 1..%d", k, HS_MAX_RHS);
        return 0;
    });
}

}  // extern "C"

// ---- the joint-reaction queries (include/humanoid_wrench.h, the hw_ entry points): a second entry-point
// family of this library on torque_kernel, whose device code is hs_wrench.h
static_assert(HW_FLAG_ARMATURE == HS_FLAG_ARMATURE && HW_FLAG_NO_GRAVITY == HS_FLAG_NO_GRAVITY &&
                  HW_FLAGS_ALL == HS_FLAGS_ALL,
              "torque_kernel reads one set of flag bits");

extern "C" {

const char* hw_last_error(void) { return last_error(); }
int hw_version(void) { return 1; }
int hw_validate_model(const he_model* model) { return hs_validate_model(model); }

int hw_create(int device, const he_model* model, const float gravity[3], int num_envs, hw_reaction** out) {
    return query_create("hw_create", device, model, gravity, num_envs, out, hw_validate_model, fill_tree_model);
}

int hw_destroy(hw_reaction* h) { return query_destroy(h); }

int hw_compute(hw_reaction* h, const float* root_state, const float* dof_state, const float* qdd_des,
               const float* base_acc, const float* body_force, const float* body_torque, const hw_outputs* out,
               int frame, uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.qdd_des = qdd_des;
    P.base_acc_in = base_acc;
    P.body_force = body_force;
    P.body_torque = body_torque;
    P.frame = frame;
    P.flags = flags;
    if (out) P.wrench = out->wrench, P.out = out->tau, P.base_acc = out->base_acc, P.body_acc = out->body_acc;
    return launch(h, "hw_compute", torque_kernel, P, stream, [&] {
        if (!out) return fail("hw_compute: null output struct");
        if (!out->wrench && !out->tau && !out->base_acc && !out->body_acc) return fail("hw_compute: no output buffer");
        if (frame != HW_FRAME_WORLD && frame != HW_FRAME_BODY)
            return fail("hw_compute: frame %d outside 0..1 (HW_FRAME_WORLD, HW_FRAME_BODY)", frame);
        return 0;
    });
}

}  // extern "C"

// ---- the dynamics derivatives (include/humanoid_derivatives.h, the hg_ entry points): a third family of
// this library on torque_kernel, whose device code is hs_derivs.h
static_assert(HG_FLAG_ARMATURE == HS_FLAG_ARMATURE && HG_FLAG_NO_GRAVITY == HS_FLAG_NO_GRAVITY &&
                  !(HG_FLAG_BY_DIRECTION & HS_FLAGS_ALL),
              "torque_kernel reads one set of flag bits");

extern "C" {

const char* hg_last_error(void) { return last_error(); }
int hg_version(void) { return 1; }
int hg_validate_model(const he_model* model) { return hs_validate_model(model); }

int hg_create(int device, const he_model* model, const float gravity[3], int num_envs, hg_derivatives** out) {
    return query_create("hg_create", device, model, gravity, num_envs, out, hg_validate_model, fill_tree_model);
}

int hg_destroy(hg_derivatives* h) { return query_destroy(h); }

int hg_compute(hg_derivatives* h, const float* root_state, const float* dof_state, const float* acc,
               const hg_outputs* out, uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.acc = acc;
    P.flags = flags;
    if (out) P.dtau_dq = out->dtau_dq, P.dtau_dv = out->dtau_dv, P.tau_full = out->tau;
    return launch(
        h, "hg_compute", torque_kernel, P, stream,
        [&] {
            if (!out) return fail("hg_compute: null output struct");
            const float* outs[HG_NUM_OUTPUTS] = {out->dtau_dq, out->dtau_dv, out->tau};
            if (!outs[0] && !outs[1] && !outs[2]) return fail("hg_compute: no output buffer");
            for (int i = 0; i < HG_NUM_OUTPUTS; ++i) {
                if (!outs[i]) continue;
                if (outs[i] == root_state || outs[i] == dof_state || outs[i] == acc)
                    return fail("hg_compute: an output is also an input buffer");
                for (int j = 0; j < i; ++j)
                    if (outs[i] == outs[j]) return fail("hg_compute: two outputs are the same buffer");
            }
            return 0;
        },
        HG_FLAGS_ALL, kDerivLds);
}

}  // extern "C"
