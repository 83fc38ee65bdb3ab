/*
 * humanoid_ik.h -- C ABI of the inverse-kinematics queries of the MI355X (gfx950) humanoid engine: the
 * pose (root position and orientation, 69 exp-map dof angles) that puts points of bodies at target
 * places and bodies at target orientations, found by damped least-squares steps in the kinetic-energy
 * metric, every iteration of every env inside one launch. This is the position-level question of a
 * keypoint tracker: head and hand targets, foot placements, keypoints without joint rotations.
 *
 * The entry points are a second family inside libhumanoid_task.so, under this header and the prefix
 * hk_: an iteration is the task kernel's force-mode solve at a resting, gravity-free copy of the state
 * with the position error in place of the desired acceleration, so the kernel is the task kernel with a
 * loop around it. Like the ht_ family it only READS the state buffers it is given; the pose it finds is
 * written to buffers of the caller's.
 *
 * Conventions (those of humanoid_task.h)
 *   - every entry point returns 0 on success, non-zero on failure; hk_last_error() gives the text;
 *   - float pointers are DEVICE pointers on the handle's device, owned by the caller, contiguous and
 *     4-byte aligned; `stream` is a hipStream_t (NULL = default stream); no call synchronises the host;
 *   - all device arithmetic is float32; quaternions are xyzw.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates)
 *
 * The task rows are humanoid_task.h's (ht_row: a body, an axis 0..5, a point in the body's frame;
 * 1 <= k <= HT_MAX_ROWS of them, the same for every env), set by hk_set_rows. M [75,75], the row
 * Jacobian J [k,75] and the column order (root linear 3, root angular 3, the 69 child-frame dof rates)
 * are humanoid_task.h's and humanoid_dynamics.h's.
 *
 * Pose. q = (root position [3], root quaternion [4], dof angles [69]), the position halves of
 * root_state [N,13] and dof_state [N*69,2]. The kinematics are humanoid_dynamics.h's:
 * R_0 = R(root quaternion), R_b = R_parent exp([theta_b]x), p_b = p_parent + R_parent local_pos[b].
 * A root quaternion or a target quaternion of norm zero stands for the identity.
 *
 * Row errors at a pose, e [k]:
 *   linear row  (axis 0..2): e_r = target[r] - (p_body + R_body point)[axis], in the world frame;
 *   angular row (axis 3..5): e_r = rotvec(R_des R_body^T)[axis - 3], with R_des the rotation of the
 *                            quaternion target_rot[env, body], normalised, and rotvec the rotation
 *                            vector with its angle in [0, pi]; target[r] is ignored.
 *
 * One iteration at pose q, with every velocity zero and gravity left out, so that c = 0 and Jdot qd = 0:
 *   eb = clamp(e, -step_clip, +step_clip)        componentwise
 *   A  = J M^-1 J^T + damping I                  [k,k]
 *   F  = A^-1 eb
 *   dq = M^-1 J^T F                              [75]
 * which is exactly ht_task_control in HT_MODE_FORCE with xdd_des = eb and gen_force = NULL at that state,
 * taking its qdd. With damping = 0 the step satisfies J dq = eb and has the least dq^T M dq among the
 * steps that do. HK_FLAG_ARMATURE (on by default) has the meaning of HT_FLAG_ARMATURE.
 *
 * Integration, by the columns' own meaning:
 *   root position     p_0 <- p_0 + dq[0:3]
 *   root orientation  quat <- normalise(quat(exp([dq[3:6]]x)) (x) quat): a world-frame angular rate
 *                     multiplies on the left;
 *   joint b           theta_b <- rotvec(exp([theta_b]x) exp([dq_b]x)), dq_b = dq[6 + 3 (b - 1) : 9 + 3 (b - 1)]:
 *                     a child-frame relative rate multiplies on the right;
 *   HK_FLAG_LIMITS (on by default): theta <- clamp(theta, model.dof_lower, model.dof_upper), componentwise.
 * The iterate is rounded to float32 after every iteration: it lives in root_out and dof_out.
 *
 * After `iterations` iterations root_out and dof_out hold the final pose, every velocity entry exactly
 * zero, and residual_out the unclamped e at that pose.
 *
 * root_out may be root_state and dof_out may be dof_state (an env's rows are read before they are
 * written); no other two buffers may overlap. Nothing else is read or written.
 *
 * A posture term is not part of the iteration: the joints that no row moves stay where they were.
 */
#ifndef HUMANOID_IK_H
#define HUMANOID_IK_H

#include <stdint.h>

#include "humanoid_task.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HK_MAX_ITERATIONS 64

/* flags of hk_solve; bit 1, the query libraries' no-gravity bit, is not one: gravity never enters */
#define HK_FLAG_ARMATURE 1u      /* bit 0: model.armature on the dof diagonal of M */
#define HK_FLAG_LIMITS 4u        /* bit 2: the dof angles are clamped to the model's limits after every iteration */
#define HK_FLAGS_DEFAULT (HK_FLAG_ARMATURE | HK_FLAG_LIMITS)
#define HK_FLAGS_ALL (HK_FLAG_ARMATURE | HK_FLAG_LIMITS)

typedef struct hk_solver hk_solver;

const char* hk_last_error(void);
int hk_version(void);

/* The host-side check hk_create applies to a model (no device needed): that of ht_validate_model. */
int hk_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model, its dof limits included, to
 * it. Non-zero for a null output pointer, num_envs < 1, a null gravity vector (the argument is the query
 * libraries'; its value is not used) or a refused model. A new handle has no rows. */
int hk_create(int device, const he_model* model, const float gravity[3], int num_envs, hk_solver** out);
int hk_destroy(hk_solver* h);

/* rows: a HOST array of k rows, copied; a second call replaces the first set whole. The refusals are
 * those of ht_set_rows, and a refused call leaves the handle's rows as they were. */
int hk_set_rows(hk_solver* h, const ht_row* rows, int k);

/* One launch for all envs. root_state f32 [N,13] and dof_state f32 [N*69,2] hold the starting pose (their
 * velocity entries are not read); target f32 [N,k]; target_rot f32 [N,24,4] or NULL; root_out f32 [N,13];
 * dof_out f32 [N*69,2]; residual_out f32 [N,k] or NULL (then the residual is not computed). Refused,
 * before any launch and with nothing written, in this order: a null handle; a null state pointer; a null
 * target; a null root_out or dof_out; flag bits outside HK_FLAGS_ALL; iterations outside
 * 1..HK_MAX_ITERATIONS; a damping that is negative or not finite; a step_clip that is not finite or not
 * positive; a buffer that is not 4-byte aligned; a handle without rows; an angular row without target_rot. */
int hk_solve(hk_solver* h, const float* root_state, const float* dof_state, const float* target,
             const float* target_rot, int iterations, float damping, float step_clip, float* root_out,
             float* dof_out, float* residual_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_IK_H */
