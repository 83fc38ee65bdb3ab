// libhumanoid_task.so: task-space control in one launch (include/humanoid_task.h defines it). One
// 64-lane wave (= one block) per env; M and its factor never leave the wave, no Jacobian tensor is read:
//   factor     state, forward kinematics, composite inertias and the columns' S and F (he_joint_space.h,
//              what hs_solve.hip runs), CRBA into regla::RegMat, the sparse L^T D L in registers, the
//              packed factor in LDS: solve_kernel's first half, instruction for instruction;
//   rows       per task row: the point x = p_body + R_body point and the row's Jdot qd from the body's
//              A, Wd and w (wave-uniform, LDS broadcasts); the Jacobian row in registers, lane = column,
//              from the lane's own S (axis, pivot) about x, masked by the body's ancestor set; then
//              through L^-T, D^-1, L^-1 as a right-hand side of hs_solve. xdd_free is one wave sum.
//              Kept in LDS, [k][76]: force mode and lambda_inv keep Z = D^-1/2 L^-T J_r^T, the vector
//              half way through the solve, because J M^-1 J^T = Z Z^T: one array instead of Y and J, and
//              a Gram matrix, symmetric and positive by construction; joint mode keeps Y;
//   gram       A = X X^T (joint mode: the base columns are stored as zeros), a lane per entry of the lower
//              triangle, each one chain of fused multiply-adds in column order over 16-byte LDS reads;
//              lambda_inv mirrors it;
//   small      the k x k Cholesky A = G G^T in LDS, lane i = row i (row-Crout: the dot products of
//              tests' reference in the same order), the pivot by a lane broadcast; the two substitutions,
//              the running vector in registers, one broadcast per step;
//   control    u = J^T F with the Jacobian entries formed again in registers (force mode) or Yj^T F
//              from LDS (joint mode), then M^-1 (f + u - c) once more through the stored factor.
// The per-row storage is dynamic LDS sized by the launch's k.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/humanoid_task.h"
#include "he_host.h"
#include "he_joint_space.h"
#include "he_regla.h"
#include "he_topo.h"
#include "he_tree_state.h"

namespace {

static_assert(HT_FLAG_NO_GRAVITY == kFlagNoGravity, "columns() reads the flag");

struct Params {
    const TreeModel* model;
    const float* root;       // [N,13]
    const float* dof;        // [N*69,2]
    const float* qdd_des;    // null: columns<false> does not read it
    const float* gen_force;  // [N,75] or null
    const float* xdd_des;    // [N,k] (control)
    float *jac, *jminv, *lambda_inv, *bias_acc, *free_acc;  // ht_task_terms: each null or written
    float *u_out, *f_out, *qdd_out;                          // ht_task_control: likewise
    float damping;
    int k;
    int control;  // 0: ht_task_terms
    int mode;
    uint32_t flags;
    ht_row rows[HT_MAX_ROWS];  // in the kernel arguments: wave-uniform reads, nothing to keep in step on the device
};

// a row of X: the 75 columns and a zero, so that a row is 19 aligned 16-byte blocks
constexpr int XS = NG + 1;
// dynamic LDS of a launch with k rows, in floats: X [k][76], A [k][k + 1], the task vector [k]
constexpr int dyn_floats(int k) { return k * XS + k * (k + 1) + k; }
// the dynamic region follows the static one: its base is 16-byte aligned when their sizes add up to a multiple
static_assert((sizeof(Lds) + sizeof(Factor)) % 16 == 0 && XS % 4 == 0, "X's rows are read as float4");

// the sum over the wave, in every lane and with the same bits in every lane (a + b = b + a at each level)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float pick(v3 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : v.z; }

// what the row loop knows of a row: the point relative to its body's origin and to o, in the world
struct RowPoint {
    int body, axis;
    v3 r, x;
};
__device__ __forceinline__ RowPoint row_point(const Lds& L, const ht_row& row) {
    const v3 r = mul(ldm(L.R[row.body]), v3{row.point[0], row.point[1], row.point[2]});
    return RowPoint{row.body, row.axis, r, ld3(L.P[row.body]) + r};
}

// J_r[c] of the lane's column: the column's motion vector about x (linear rows) or its axis (angular)
__device__ __forceinline__ float jac_entry(const ColS& s, const RowPoint& p, bool on) {
    const v3 v = p.axis < 3 ? s.v0 + cross(s.w, p.x - s.pv) : s.w;
    return on ? pick(v, p.axis < 3 ? p.axis : p.axis - 3) : 0.f;
}

extern __shared__ float dyn_lds[];

__global__ __launch_bounds__(kWave, 2) void task_kernel(const Params P) {
    __shared__ Lds L;
    __shared__ Factor Fc;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;
    const bool hi = lane < NH;
    const int k = P.k;

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
        const bool arm = (P.flags & HT_FLAG_ARMATURE) != 0;
        const float arm1 = arm && lane >= 6 ? M.armature[lane >= 6 ? lane - 6 : 0] : 0.f;
        const float arm2 = arm && hi ? M.armature[hi ? kWave - 6 + lane : 0] : 0.f;
        const ColS s1 = load_S(L.SF[lane], lane);
        const ColS s2 = load_S(L.SF[hi ? kWave + lane : NG - 1], NG - 1);
        regla::static_for<0, NG, 1>([&](auto i) { crba_row<decltype(i)::value>(H, L, s1, s2, arm1, arm2, lane); });
        float z1 = 0.f, z2 = 0.f;
        regla::factor_pipelined(H, D1, D2, Fc.Lp, dj, dj2, z1, z2);
    }
    __syncthreads();
    const float dinv1 = 1.f / D1, dinv2 = 1.f / D2;
    const float* row1 = Fc.Lp + Fc.pack_start[lane];
    const float* row2 = Fc.Lp + Fc.pack_start[hi ? kWave + lane : 0];

    float* X = dyn_lds;            // [k][XS]
    float* A = X + k * XS;         // [k][k + 1]: the lower triangle, then its Cholesky factor
    float* tv = A + k * (k + 1);   // [k] r = xdd_des - xdd_free, then F
    const bool joint = P.control && P.mode == HT_MODE_JOINT;
    const bool keep_z = P.control ? !joint : P.lambda_inv != nullptr;  // X = Z: J M^-1 J^T = Z Z^T
    const bool want_free = P.control || P.free_acc;
    const bool want_solve = want_free || P.jminv || keep_z;

    // the lane's columns once more (not kept across the factorisation, whose registers they would cost)
    const ColS s1 = load_S(L.SF[lane], lane);
    const ColS s2 = load_S(L.SF[hi ? kWave + lane : NG - 1], NG - 1);
    const int j1 = col_joint(lane), j2 = col_joint(hi ? kWave + lane : NG - 1);
    const float* f = P.gen_force ? P.gen_force + env * NG : nullptr;
    const float f1 = f ? f[lane] : 0.f, f2 = f && hi ? f[kWave + lane] : 0.f;
    const float fc1 = f1 - L.bias[lane], fc2 = hi ? f2 - L.bias[kWave + lane] : 0.f;
    const float sq1 = sqrtf(dinv1), sq2 = sqrtf(dinv2);

    for (int j = 0; j < k; ++j) {  // wave-uniform trip count, and every branch below is the whole wave's
        const RowPoint p = row_point(L, P.rows[j]);
        const uint32_t anc = M.anc[p.body];
        float y1 = jac_entry(s1, p, anc >> j1 & 1u);
        float y2 = hi ? jac_entry(s2, p, anc >> j2 & 1u) : 0.f;
        const size_t o = (env * k + j) * NG;
        if (P.jac) {
            P.jac[o + lane] = y1;
            if (hi) P.jac[o + kWave + lane] = y2;
        }
        // Jdot qd: the point's acceleration at qdd = 0
        const v3 w = ld3(L.W[p.body]), wd = ld3(L.Wd[p.body]);
        const v3 acc = p.axis < 3 ? ld3(L.A[p.body]) + cross(wd, p.r) + cross(w, cross(w, p.r)) : wd;
        const float bj = pick(acc, p.axis < 3 ? p.axis : p.axis - 3);
        if (P.bias_acc && lane == 0) P.bias_acc[env * k + j] = bj;
        if (!want_solve) continue;

        regla::solve_LT_vec_pipelined(Fc.Lp, dj, dj2, y1, y2);
        if (keep_z) {
            X[j * XS + lane] = y1 * sq1;
            if (lane <= NH) X[j * XS + kWave + lane] = hi ? y2 * sq2 : 0.f;  // lane 11: the row's pad
        }
        y1 *= dinv1;
        y2 *= dinv2;
        regla::solve_L_streamed(row1, row2, y1, y2);
        if (joint) {  // Yj: the base columns are not part of it
            X[j * XS + lane] = lane < 6 ? 0.f : y1;
            if (lane <= NH) X[j * XS + kWave + lane] = hi ? y2 : 0.f;
        }
        if (P.jminv) {
            P.jminv[o + lane] = y1;
            if (hi) P.jminv[o + kWave + lane] = y2;
        }
        if (want_free) {
            const float fa = wave_sum(fmaf(y2, fc2, y1 * fc1)) + bj;
            if (lane == 0) {
                if (P.free_acc) P.free_acc[env * k + j] = fa;
                if (P.control) tv[j] = P.xdd_des[env * k + j] - fa;
            }
        }
    }
    if (!keep_z && !joint) return;
    __syncthreads();

    // A = X X^T: a lane per entry of the lower triangle, one chain of fused multiply-adds in column order
    const int ld = k + 1;
    for (int e = lane; e < k * (k + 1) / 2; e += kWave) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const int jj = e - i * (i + 1) / 2;
        const float4* xi = reinterpret_cast<const float4*>(X + i * XS);
        const float4* xj = reinterpret_cast<const float4*>(X + jj * XS);
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < XS / 4; ++q) {
            const float4 v = xi[q], w = xj[q];
            a = fmaf(v.w, w.w, fmaf(v.z, w.z, fmaf(v.y, w.y, fmaf(v.x, w.x, a))));
        }
        if (P.control) {
            A[i * ld + jj] = i == jj ? a + P.damping : a;
        } else {  // one triangle, mirrored: exactly symmetric
            P.lambda_inv[(env * k + i) * k + jj] = a;
            P.lambda_inv[(env * k + jj) * k + i] = a;
        }
    }
    if (!P.control) return;
    __syncthreads();

    // A = G G^T in place, lane i = row i: G[i][j] = (A[i][j] - sum_m<j G[i][m] G[j][m]) / G[j][j]
    const bool act = lane < k;
    float* Ai = A + (act ? lane : 0) * ld;
    for (int j = 0; j < k; ++j) {
        float s = 0.f;
        if (act && lane >= j) {
            const float* Aj = A + j * ld;
            s = Ai[j];
#pragma unroll 4
            for (int m = 0; m < j; ++m) s = fmaf(-Ai[m], Aj[m], s);
        }
        const float g = sqrtf(__shfl(s, j));
        if (act && lane >= j) Ai[j] = lane == j ? g : s / g;
        __syncthreads();
    }
    // G y = r, then G^T F = y: lane i carries entry i, the step's entry is broadcast
    float t = act ? tv[lane] : 0.f;
    for (int j = 0; j < k; ++j) {
        const float yj = __shfl(t, j) / A[j * ld + j];
        if (lane == j) t = yj;
        if (act && lane > j) t = fmaf(-Ai[j], yj, t);
    }
    for (int j = k - 1; j >= 0; --j) {
        const float xj = __shfl(t, j) / A[j * ld + j];
        if (lane == j) t = xj;
        if (lane < j) t = fmaf(-A[j * ld + lane], xj, t);
    }
    if (act) {
        tv[lane] = t;
        if (P.f_out) P.f_out[env * k + lane] = t;
    }
    if (!P.u_out && !P.qdd_out) return;
    __syncthreads();

    // u = J^T F (the entries formed again: a cross product a row) or (0_6; Yj^T F)
    float u1 = 0.f, u2 = 0.f;
    for (int j = 0; j < k; ++j) {
        const float fj = tv[j];
        if (joint) {
            u1 = fmaf(fj, X[j * XS + lane], u1);
            if (hi) u2 = fmaf(fj, X[j * XS + kWave + lane], u2);
        } else {
            const RowPoint p = row_point(L, P.rows[j]);
            const uint32_t anc = M.anc[p.body];
            u1 = fmaf(fj, jac_entry(s1, p, anc >> j1 & 1u), u1);
            if (hi) u2 = fmaf(fj, jac_entry(s2, p, anc >> j2 & 1u), u2);
        }
    }
    if (joint && lane < 6) u1 = 0.f;  // the base is not actuated: exact zeros
    if (P.u_out) {
        P.u_out[env * NG + lane] = u1;
        if (hi) P.u_out[env * NG + kWave + lane] = u2;
    }
    if (!P.qdd_out) return;
    float y1 = (f1 + u1) - L.bias[lane], y2 = hi ? (f2 + u2) - L.bias[kWave + lane] : 0.f;
    regla::solve_LT_vec_pipelined(Fc.Lp, dj, dj2, y1, y2);
    y1 *= dinv1;
    y2 *= dinv2;
    regla::solve_L_streamed(row1, row2, y1, y2);
    P.qdd_out[env * NG + lane] = y1;
    if (hi) P.qdd_out[env * NG + kWave + lane] = y2;
}

}  // namespace

struct ht_task : QueryHandle<TreeModel> {
    int k = 0;  // 0: no rows yet
    ht_row rows[HT_MAX_ROWS] = {};
};

namespace {

// the checks the two entry points share, in the order the header lists them: the query libraries'
// (he_host.h) with the task's own in between; the handle is read last
int launch(ht_task* h, const char* who, Params& P, std::initializer_list<const void*> buffers, bool any_output,
           void* stream) {
    if (check_call(who, h, P.root, P.dof)) return 1;
    if (P.control && !P.xdd_des) return fail("%s: null desired acceleration", who);
    if (!any_output) return fail("%s: no output buffer", who);
    if (check_flags(who, P.flags, HT_FLAGS_ALL)) return 1;
    if (P.mode != HT_MODE_FORCE && P.mode != HT_MODE_JOINT) return fail("%s: unknown mode %d", who, P.mode);
    if (!(P.damping >= 0.f) || !std::isfinite(P.damping))
        return fail("%s: damping %g is negative or not finite", who, (double)P.damping);
    if (check_aligned(who, buffers)) return 1;
    if (h->k < 1) return fail("%s: no rows set (ht_set_rows)", who);
    P.model = h->d_model;
    P.k = h->k;
    std::memcpy(P.rows, h->rows, sizeof(P.rows));
    hipLaunchKernelGGL(task_kernel, dim3(h->num_envs), dim3(kWave), dyn_floats(h->k) * sizeof(float),
                       static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char* ht_last_error(void) { return last_error(); }
int ht_version(void) { return 1; }

int ht_validate_model(const he_model* model) {
    if (check_model(model, "model", HE_MAX_BOXES)) return 1;
    if (check_tree_depth(model)) return 1;
    return check_factored_tree(model);
}

int ht_create(int device, const he_model* model, const float gravity[3], int num_envs, ht_task** out) {
    return query_create("ht_create", device, model, gravity, num_envs, out, ht_validate_model, fill_tree_model);
}

int ht_destroy(ht_task* h) { return query_destroy(h); }

int ht_set_rows(ht_task* h, const ht_row* rows, int k) {
    if (!h) return fail("ht_set_rows: null handle");
    if (!rows) return fail("ht_set_rows: null row array");
    if (k < 1 || k > HT_MAX_ROWS) return fail("ht_set_rows: k = %d outside 1..%d", k, HT_MAX_ROWS);
    for (int r = 0; r < k; ++r) {
        if (rows[r].body < 0 || rows[r].body >= NB)
            return fail("ht_set_rows: row %d names body %d, outside 0..%d", r, rows[r].body, NB - 1);
        if (rows[r].axis < 0 || rows[r].axis > 5)
            return fail("ht_set_rows: row %d has axis %d, outside 0..5", r, rows[r].axis);
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(rows[r].point[c])) return fail("ht_set_rows: row %d has a point that is not finite", r);
    }
    std::memset(h->rows, 0, sizeof(h->rows));  // nothing of the old rows survives
    std::memcpy(h->rows, rows, k * sizeof(ht_row));
    h->k = k;
    return 0;
}

int ht_task_terms(ht_task* h, const float* root_state, const float* dof_state, const float* gen_force, float* jac_out,
                  float* jminv_out, float* lambda_inv_out, float* bias_acc_out, float* free_acc_out, uint32_t flags,
                  void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.gen_force = gen_force;
    P.jac = jac_out;
    P.jminv = jminv_out;
    P.lambda_inv = lambda_inv_out;
    P.bias_acc = bias_acc_out;
    P.free_acc = free_acc_out;
    P.flags = flags;
    return launch(h, "ht_task_terms", P,
                  {root_state, dof_state, gen_force, jac_out, jminv_out, lambda_inv_out, bias_acc_out, free_acc_out},
                  jac_out || jminv_out || lambda_inv_out || bias_acc_out || free_acc_out, stream);
}

int ht_task_control(ht_task* h, const float* root_state, const float* dof_state, const float* xdd_des,
                    const float* gen_force, int mode, float damping, float* gen_force_out, float* task_force_out,
                    float* qdd_out, uint32_t flags, void* stream) {
    Params P{};
    P.root = root_state;
    P.dof = dof_state;
    P.xdd_des = xdd_des;
    P.gen_force = gen_force;
    P.control = 1;
    P.mode = mode;
    P.damping = damping;
    P.u_out = gen_force_out;
    P.f_out = task_force_out;
    P.qdd_out = qdd_out;
    P.flags = flags;
    return launch(h, "ht_task_control", P, {root_state, dof_state, xdd_des, gen_force, gen_force_out, task_force_out, qdd_out},
                  gen_force_out || task_force_out || qdd_out, stream);
}

}  // extern "C"
