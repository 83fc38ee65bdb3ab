/*
 * humanoid_task.h -- C ABI of libhumanoid_task.so, task-space control of the MI355X (gfx950) humanoid
 * engine: for a set of task rows (velocity components of points on bodies) the task Jacobian J, J M^-1,
 * the inverse operational-space inertia J M^-1 J^T, the velocity-product acceleration Jdot qd, and the
 * generalised force that gives the task a desired acceleration, formed from the root and dof state in
 * one launch. M is built, factored and applied in registers, one env per 64-lane wave; nothing of size
 * 75 x 75 is written to memory and no Jacobian tensor is refreshed.
 *
 * The library is separate from the engine, dynamics and solve libraries and only READS the engine's
 * state buffers through device pointers: nothing here is linked into any of them.
 *
 * Conventions (those of humanoid_solve.h)
 *   - every entry point returns 0 on success, non-zero on failure; ht_last_error() gives the text;
 *   - float pointers are DEVICE pointers on the handle's device, owned by the caller, contiguous and
 *     4-byte aligned; `stream` is a hipStream_t (NULL = default stream); no call synchronises the host;
 *   - all device arithmetic is float32; nothing is read but root_state [N,13] and dof_state [N*69,2]
 *     (the engine's HE_BUF_ROOT_STATE / HE_BUF_DOF_STATE, or arrays laid out like them) and the
 *     vectors named below. The kernel runs its own forward kinematics, so it is right immediately
 *     after an indexed state write.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates)
 *
 * M [75,75], c [75], the body Jacobians jac [24,6,75], the kinematics (R_b, p_b, w_b) and the column
 * order (root linear 3, root angular 3, the 69 child-frame dof rates) are exactly those of
 * humanoid_dynamics.h; generalised accelerations qdd are the time derivatives of those velocities,
 * generalised forces their duals. HT_FLAG_ARMATURE (on by default) puts model.armature on M's dof
 * diagonal; HT_FLAG_NO_GRAVITY leaves gravity out of c. Gravity is the vector given to ht_create.
 *
 * Task rows. k rows, 1 <= k <= HT_MAX_ROWS, the same for every env, set by ht_set_rows. Row r names a
 * body, an axis and a point given in the body's frame (zero: the body origin):
 *   axis 0..2: the world linear velocity component x / y / z of the point x = p_body + R_body point,
 *              J_r = jac[body, axis] + (jac[body, 3:6] x (R_body point))[axis]   (column by column);
 *   axis 3..5: the world angular velocity component axis - 3 of the body, J_r = jac[body, axis]; the
 *              point is ignored.
 * J_r is exactly zero in every column whose joint is not an ancestor-or-self of the body.
 *
 * With f = gen_force (NULL: 0) and, at qdd = 0, the bodies' origin accelerations A_b and angular
 * accelerations Wd_b (the velocity products alone: Wd_b = Wd_a + w_a x (R_b u_b),
 * A_b = A_a + Wd_a x d + w_a x (w_a x d), d = p_b - p_a, both zero for the root):
 *   Y          = J M^-1                 [k,75]   jminv
 *   Lambda^-1  = J M^-1 J^T             [k,k]    lambda_inv (written exactly symmetric)
 *   b          = Jdot qd                [k]      bias_acc: the rows' accelerations at qdd = 0,
 *                linear row:  (A_body + Wd_body x r + w_body x (w_body x r))[axis],  r = R_body point,
 *                angular row: Wd_body[axis - 3];
 *   xdd_free   = Y (f - c) + b          [k]      free_acc: the task acceleration when only f acts.
 * The task acceleration of any qdd is J qdd + b.
 *
 * ht_task_control. With r = xdd_des - xdd_free and damping lambda >= 0, which is added to A's diagonal as
 * given and so carries A's units (force mode: those of Lambda^-1, acceleration per force; joint mode:
 * those of Yj Yj^T, their square):
 *   HT_MODE_FORCE:  A = Lambda^-1 + lambda I,  F = A^-1 r,  u = J^T F  [75]: the operational-space
 *                   force, the minimum of u^T M^-1 u (the kinetic-energy metric) that reaches xdd_des;
 *   HT_MODE_JOINT:  Yj = Y[:, 6:],  A = Yj Yj^T + lambda I,  F = A^-1 r,  u = (0_6; Yj^T F): the joint
 *                   torque of minimum Euclidean norm that reaches xdd_des with the floating base
 *                   unactuated; its six base entries are exactly zero;
 *   qdd = M^-1 (f + u - c)   [75].
 * With lambda = 0, J qdd + b = xdd_des. A is factored by a k x k Cholesky; a row set whose A is singular
 * (dependent rows, lambda = 0) gives non-finite outputs, not an error.
 *
 * The solves with M are the sparse L^T D L factorisation of humanoid_solve.h. Every row of a call goes
 * through the same instructions, so a row's jac, jminv, bias_acc and free_acc have the same bits in any
 * row set that holds it, and an output's bits do not depend on which other outputs were asked for.
 */
#ifndef HUMANOID_TASK_H
#define HUMANOID_TASK_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HT_MAX_ROWS 32           /* task rows of one handle */

/* flags of ht_task_terms and ht_task_control */
#define HT_FLAG_ARMATURE 1u      /* bit 0: model.armature on the dof diagonal of M */
#define HT_FLAG_NO_GRAVITY 2u    /* bit 1: c without gravity */
#define HT_FLAGS_DEFAULT HT_FLAG_ARMATURE
#define HT_FLAGS_ALL (HT_FLAG_ARMATURE | HT_FLAG_NO_GRAVITY)

/* mode of ht_task_control */
#define HT_MODE_FORCE 0          /* u = J^T (Lambda^-1 + lambda I)^-1 r */
#define HT_MODE_JOINT 1          /* u = (0_6; Yj^T (Yj Yj^T + lambda I)^-1 r) */

typedef struct ht_row {
    int32_t body;                /* 0..23 */
    int32_t axis;                /* 0..2 linear x y z of the point, 3..5 angular x y z of the body */
    float point[3];              /* in the body's frame; ignored by an angular row */
} ht_row;

typedef struct ht_task ht_task;

const char* ht_last_error(void);
int ht_version(void);

/* The host-side check ht_create applies to a model (no device needed): exactly that of
 * hs_validate_model, the tree the factorisation is unrolled for included. */
int ht_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model and the gravity vector to
 * it. Non-zero for a null output pointer, num_envs < 1, a null gravity vector or a refused model. A new
 * handle has no rows. */
int ht_create(int device, const he_model* model, const float gravity[3], int num_envs, ht_task** out);
int ht_destroy(ht_task* h);

/* rows: a HOST array of k rows, copied; a second call replaces the first set whole. The call is refused,
 * and the handle keeps the rows it had, for a null handle or array, k outside 1..HT_MAX_ROWS, a body
 * outside 0..23, an axis outside 0..5 or a point that is not finite. No device call is made. */
int ht_set_rows(ht_task* h, const ht_row* rows, int k);

/* Each call below is one launch for all envs. It is refused, before any launch and with nothing
 * written, for a null handle, a null state pointer, a null required input, no output at all, flag bits
 * outside HT_FLAGS_ALL, an unknown mode, a damping that is negative or not finite, a buffer that is not
 * 4-byte aligned, or a handle without rows (checked last). k below is the handle's row count. */

/* gen_force f32 [N,75] or NULL (zero). Outputs, each f32 and each NULL or written: jac_out [N,k,75],
 * jminv_out [N,k,75], lambda_inv_out [N,k,k], bias_acc_out [N,k], free_acc_out [N,k]. A NULL output is
 * neither computed nor written; at least one is required. */
int ht_task_terms(ht_task* h, const float* root_state, const float* dof_state, const float* gen_force,
                  float* jac_out, float* jminv_out, float* lambda_inv_out, float* bias_acc_out, float* free_acc_out,
                  uint32_t flags, void* stream);

/* xdd_des f32 [N,k]; gen_force f32 [N,75] or NULL (zero); mode HT_MODE_FORCE or HT_MODE_JOINT; damping
 * the lambda above. Outputs, each f32 and each NULL or written: gen_force_out [N,75] (u), task_force_out
 * [N,k] (F), qdd_out [N,75]; at least one is required. */
int ht_task_control(ht_task* h, const float* root_state, const float* dof_state, const float* xdd_des,
                    const float* gen_force, int mode, float damping, float* gen_force_out, float* task_force_out,
                    float* qdd_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_TASK_H */
