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
// The kernel's second family (include/humanoid_ik.h, the hk_ entry points in ht_ik.h, included last) loops
// these stages: an inverse-kinematics iteration is the force-mode control pass at a resting, gravity-free
// pose with the rows' clamped position errors in place of r, its qdd integrated on the joint manifold
// into the iterate, which lives in the output buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/humanoid_ik.h"
#include "../../include/humanoid_task.h"
#include "he_host.h"
#include "he_joint_space.h"
#include "he_regla.h"
#include "he_topo.h"
#include "he_tree_state.h"

namespace {

static_assert(HT_FLAG_NO_GRAVITY == kFlagNoGravity, "columns() reads the flag");
static_assert(HK_FLAG_ARMATURE == HT_FLAG_ARMATURE && !(HK_FLAGS_ALL & HT_FLAG_NO_GRAVITY), "hk_solve's flags reach the kernel");
constexpr int kControlTask = 1, kControlIk = 2;

struct Params {
    const TreeModel* model;
    const float* root;       // [N,13]
    const float* dof;        // [N*69,2]
    const float* qdd_des;    // null: columns<false> does not read it
    const float* gen_force;  // [N,75] or null
    const float* xdd_des;    // [N,k] (control)
    float *jac, *jminv, *lambda_inv, *bias_acc, *free_acc;  // ht_task_terms: each null or written
    float *u_out, *f_out, *qdd_out;                          // ht_task_control: likewise
    // hk_solve: root and dof above are the iterate (root_out, dof_out) and xdd_des the targets [N,k]
    const float *root_in, *dof_in;  // the starting pose
    const float* target_rot;        // [N,24,4] or null
    const float* limits;            // [2,69] lower, upper (the handle's)
    float *root_out, *dof_out;      // = root, dof
    float* residual;                // [N,k] or null
    float step_clip;
    int iterations;
    float damping;
    int k;
    int control;  // 0: ht_task_terms, kControlTask: ht_task_control, kControlIk: hk_solve
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

// ---- the inverse kinematics' rotations (include/humanoid_ik.h): unit quaternions xyzw, because the rotation
// vector of a product is read off a quaternion to float32 of itself at every angle, and off a matrix only
// to float32 of 1
struct q4 {
    float x, y, z, w;
};
// quat(exp([v]x)) = (v sin(th / 2) / th, cos(th / 2)); below 1e-3 rad the series, where rodrigues() takes its own
__device__ __forceinline__ q4 exp_quat(v3 v) {
    const float t2 = dot(v, v);
    float s, c;
    if (t2 < 1e-6f) {
        s = 0.5f - t2 * (1.f / 48.f);
        c = 1.f - t2 * 0.125f;
    } else {
        const float th = sqrtf(t2);
        s = sinf(0.5f * th) / th;
        c = cosf(0.5f * th);
    }
    return q4{v.x * s, v.y * s, v.z * s, c};
}
__device__ __forceinline__ q4 mul(q4 a, q4 b) {
    return q4{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
              a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
// xyzw as stored, normalised; norm zero: the identity, as quat_matrix() reads it
__device__ __forceinline__ q4 load_quat(const float* p) {
    const q4 q{p[0], p[1], p[2], p[3]};
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 < 1e-24f) return q4{0.f, 0.f, 0.f, 1.f};
    const float s = 1.f / sqrtf(n2);
    return q4{q.x * s, q.y * s, q.z * s, q.w * s};
}
// the rotation vector of a quaternion (any norm but the series' own), angle in [0, pi]: the inverse of exp_quat
__device__ __forceinline__ v3 rotvec(q4 q) {
    const float sg = q.w < 0.f ? -1.f : 1.f;
    const float w = sg * q.w;
    const v3 v{sg * q.x, sg * q.y, sg * q.z};
    const float s2 = dot(v, v);
    float f;  // angle / |v|
    if (s2 < 2.5e-7f) {
        f = (2.f - s2 * (2.f / 3.f) / (w * w)) / w;  // 2 atan(s / w) / s
    } else {
        const float sn = sqrtf(s2);
        f = 2.f * atan2f(sn, w) / sn;
    }
    return v * f;
}
// a rotation matrix as a quaternion, by its largest of trace and diagonal (Shepperd): no cancellation at any angle
__device__ __forceinline__ q4 matrix_quat(const m3& m) {
    const float tr = m.a00 + m.a11 + m.a22;
    if (tr > 0.f) {
        const float s = 2.f * sqrtf(tr + 1.f), r = 1.f / s;
        return q4{(m.a21 - m.a12) * r, (m.a02 - m.a20) * r, (m.a10 - m.a01) * r, 0.25f * s};
    }
    if (m.a00 > m.a11 && m.a00 > m.a22) {
        const float s = 2.f * sqrtf(1.f + m.a00 - m.a11 - m.a22), r = 1.f / s;
        return q4{0.25f * s, (m.a01 + m.a10) * r, (m.a02 + m.a20) * r, (m.a21 - m.a12) * r};
    }
    if (m.a11 > m.a22) {
        const float s = 2.f * sqrtf(1.f + m.a11 - m.a00 - m.a22), r = 1.f / s;
        return q4{(m.a01 + m.a10) * r, 0.25f * s, (m.a12 + m.a21) * r, (m.a02 - m.a20) * r};
    }
    const float s = 2.f * sqrtf(1.f + m.a22 - m.a00 - m.a11), r = 1.f / s;
    return q4{(m.a02 + m.a20) * r, (m.a12 + m.a21) * r, 0.25f * s, (m.a10 - m.a01) * r};
}

// a row's error at the pose in L (wave-uniform): target - x[axis] with the root's world position p0, or
// rotvec(R_des R_body^T)[axis - 3]
__device__ __forceinline__ float row_error(const Lds& L, const ht_row& row, v3 p0, float target, const float* target_rot,
                                           size_t env) {
    if (row.axis < 3) {
        const RowPoint p = row_point(L, row);
        return target - pick(p0 + p.x, row.axis);
    }
    const q4 qb = matrix_quat(ldm(L.R[row.body]));
    // formed here: the host has refused an angular row without target_rot, and a null one is not offset
    const q4 qe = mul(load_quat(target_rot + (env * NB + row.body) * 4), q4{-qb.x, -qb.y, -qb.z, qb.w});
    return pick(rotvec(qe), row.axis - 3);
}

// hk_solve's integration of the step dq (in L.bias, the columns' order) into the iterate: lane = body. The
// root by its world rates, joint b by theta <- rotvec(exp(theta) exp(dq_b)), clamped to the limits when asked.
__device__ __forceinline__ void integrate(const Lds& L, const Params& P, size_t env, int lane) {
    if (lane == 0) {
        float* root = P.root_out + env * 13;
        st3(root, ld3(root) + ld3(L.bias));
        q4 q = mul(exp_quat(ld3(L.bias + 3)), load_quat(root + 3));
        const float s = 1.f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        root[3] = q.x * s, root[4] = q.y * s, root[5] = q.z * s, root[6] = q.w * s;
    } else if (lane < NB) {
        const int d = 3 * (lane - 1);
        v3 th = rotvec(mul(exp_quat(ld3(L.q + d)), exp_quat(ld3(L.bias + 6 + d))));
        if (P.flags & HK_FLAG_LIMITS) {
            const v3 lo = ld3(P.limits + d), up = ld3(P.limits + ND + d);
            th = v3{fminf(fmaxf(th.x, lo.x), up.x), fminf(fmaxf(th.y, lo.y), up.y), fminf(fmaxf(th.z, lo.z), up.z)};
        }
        float* dof = P.dof_out + (env * ND + d) * 2;
        dof[0] = th.x, dof[2] = th.y, dof[4] = th.z;
    }
}

extern __shared__ float dyn_lds[];

// One pass over the stages of the file's head, from the state in P.root / P.dof: ht_task_terms' and
// ht_task_control's whole launch, and one iteration of hk_solve, whose step it leaves in L.bias (true:
// there is a step to integrate). Fc's tables are filled; every store sits behind its own pointer.
template <bool IK>
__device__ __forceinline__ bool task_pass(Lds& L, Factor& Fc, const Params& P, const TreeModel& M, size_t env, int lane,
                                          bool last) {
    const bool hi = lane < NH;
    const int k = P.k;
    constexpr bool ik = IK;  // = (P.control == kControlIk): a copy of the pass each, so that the calls of
                             // include/humanoid_task.h run no code of the loop's and keep their registers
    float* X = dyn_lds;            // [k][XS]
    float* A = X + k * XS;         // [k][k + 1]: the lower triangle, then its Cholesky factor
    float* tv = A + k * (k + 1);   // [k] r = xdd_des - xdd_free, then F

    columns<false>(L, M, P, env, lane);  // ends on a barrier

    if (ik) {  // the rows' errors at the iterate: clamped into r, or after the last iteration the residual
        const v3 p0 = ld3(L.qdd);  // the root's world position (columns<false> leaves L.qdd alone)
        for (int j = 0; j < k; ++j) {
            const float e = row_error(L, P.rows[j], p0, P.xdd_des[env * k + j], P.target_rot, env);
            if (lane == 0) {
                if (last)
                    P.residual[env * k + j] = e;
                else
                    tv[j] = fminf(fmaxf(e, -P.step_clip), P.step_clip);
            }
        }
        if (last) return false;
    }

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

    const bool joint = P.control && P.mode == HT_MODE_JOINT;
    const bool keep_z = P.control ? !joint : P.lambda_inv != nullptr;  // X = Z: J M^-1 J^T = Z Z^T
    const bool want_free = P.control == kControlTask || P.free_acc;    // hk_solve: c = 0 and Jdot qd = 0, r is in tv
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
    if (!keep_z && !joint) return false;
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
    if (!P.control) return false;
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
    if (!P.u_out && !P.qdd_out && !ik) return false;
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
    if (!P.qdd_out && !ik) return false;
    float y1 = (f1 + u1) - L.bias[lane], y2 = hi ? (f2 + u2) - L.bias[kWave + lane] : 0.f;
    regla::solve_LT_vec_pipelined(Fc.Lp, dj, dj2, y1, y2);
    y1 *= dinv1;
    y2 *= dinv2;
    regla::solve_L_streamed(row1, row2, y1, y2);
    if (ik) {  // the step, where integrate()'s body lanes gather it (c has been read: it was zero)
        L.bias[lane] = y1;
        if (hi) L.bias[kWave + lane] = y2;
        return true;
    }
    P.qdd_out[env * NG + lane] = y1;
    if (hi) P.qdd_out[env * NG + kWave + lane] = y2;
    return false;
}

__global__ __launch_bounds__(kWave, 2) void task_kernel(const Params P) {
    __shared__ Lds L;
    __shared__ Factor Fc;
    const int lane = threadIdx.x;
    const size_t env = blockIdx.x;
    const TreeModel& M = *P.model;

    for (int i = lane; i < smpl::kNpack + 4; i += kWave) Fc.Lp[i] = 0.f;
    for (int i = lane; i < NG; i += kWave) {
        Fc.pack_start[i] = (int16_t)smpl::kPackStart[i];
        Fc.dof_depth[i] = (int8_t)(smpl::kDofNanc[i] - 1);
    }
    // ht_task_terms and ht_task_control: one pass, in a copy of its own, the code these calls ran before the
    // loop existed.
    if (P.control != kControlIk) {
        task_pass<false>(L, Fc, P, M, env, lane, false);
        return;
    }
    // hk_solve: the starting pose into the iterate with every velocity zero (an element is read and written
    // by the same lane: the buffers may be the same), then `iterations` passes, each integrated into the
    // iterate, and one more as far as the errors when the residual is asked for. A barrier stands between
    // every write of the iterate and its next read.
    for (int d = lane; d < ND; d += kWave) {
        const size_t o = (env * ND + d) * 2;
        const float th = P.dof_in[o];
        P.dof_out[o] = th;
        P.dof_out[o + 1] = 0.f;
    }
    if (lane < 13) {
        const float v = P.root_in[env * 13 + lane];
        P.root_out[env * 13 + lane] = lane < 7 ? v : 0.f;
    }
    __syncthreads();
    const int passes = P.iterations + (P.residual ? 1 : 0);
    for (int it = 0; it < passes; ++it) {
        // the lane anew in every pass: whatever a pass derives from it (addresses, the lane's model entries)
        // is formed inside the pass, as in a launch of one pass, and not kept in registers across the loop,
        // where the factorisation has none to spare
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if (ln < 3) L.qdd[ln] = P.root_out[env * 13 + ln];  // row_error()'s p0
        if (task_pass<true>(L, Fc, P, M, env, ln, it == P.iterations)) {
            __syncthreads();
            integrate(L, P, env, ln);
            __syncthreads();
        }
    }
}

}  // namespace

struct ht_task : QueryHandle<TreeModel> {
    int k = 0;  // 0: no rows yet
    ht_row rows[HT_MAX_ROWS] = {};
};

namespace {

// h?_set_rows of the file's two families: the refusals, each leaving the handle's rows as they were
template <class Handle>
int set_rows(const char* who, Handle* h, const ht_row* rows, int k) {
    if (!h) return fail("%s: null handle", who);
    if (!rows) return fail("%s: null row array", who);
    if (k < 1 || k > HT_MAX_ROWS) return fail("%s: k = %d outside 1..%d", who, k, HT_MAX_ROWS);
    for (int r = 0; r < k; ++r) {
        if (rows[r].body < 0 || rows[r].body >= NB)
            return fail("%s: row %d names body %d, outside 0..%d", who, r, rows[r].body, NB - 1);
        if (rows[r].axis < 0 || rows[r].axis > 5) return fail("%s: row %d has axis %d, outside 0..5", who, r, rows[r].axis);
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(rows[r].point[c])) return fail("%s: row %d has a point that is not finite", who, r);
    }
    std::memset(h->rows, 0, sizeof(h->rows));  // nothing of the old rows survives
    std::memcpy(h->rows, rows, k * sizeof(ht_row));
    h->k = k;
    return 0;
}

// the launch of a checked call: the handle's model and rows into the arguments, one wave per env
template <class Handle>
int launch_rows(const Handle& h, Params& P, void* stream) {
    P.model = h.d_model;
    P.k = h.k;
    std::memcpy(P.rows, h.rows, sizeof(P.rows));
    hipLaunchKernelGGL(task_kernel, dim3(h.num_envs), dim3(kWave), dyn_floats(h.k) * sizeof(float),
                       static_cast<hipStream_t>(stream), P);
    HE_CHECK(hipGetLastError());
    return 0;
}

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
    return launch_rows(*h, P, stream);
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

int ht_set_rows(ht_task* h, const ht_row* rows, int k) { return set_rows("ht_set_rows", h, rows, k); }

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
    P.control = kControlTask;
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

#include "ht_ik.h"
