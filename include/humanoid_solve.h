/*
 * humanoid_solve.h -- C ABI of libhumanoid_solve.so, the joint-space solves of the MI355X (gfx950)
 * humanoid engine: the solves with the mass matrix M that a controller calls each step (forward
 * dynamics, computed torque, M^-1 applied to a block of vectors), formed from the root and dof state
 * in one launch. M is built, factored and applied in registers, one env per 64-lane wave; nothing of
 * size 75 x 75 is written to memory.
 *
 * The library is separate from libhumanoid_engine.so and libhumanoid_dynamics.so and only READS the
 * engine's state buffers through device pointers: nothing here is linked into either.
 *
 * Conventions (those of humanoid_dynamics.h)
 *   - every entry point returns 0 on success, non-zero on failure; hs_last_error() gives the text;
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
 * M [75,75] and c [75] are exactly the mass matrix and the bias force that humanoid_dynamics.h defines,
 * in the same column order: root linear 3, root angular 3, the 69 child-frame dof rates; generalised
 * accelerations qdd are the time derivatives of those velocities, generalised forces their duals.
 * HS_FLAG_ARMATURE (on by default) puts model.armature on M's dof diagonal; HS_FLAG_NO_GRAVITY leaves
 * gravity out of c. Gravity is the vector given to hs_create.
 *
 * hs_forward_dynamics:   qdd = M^-1 (gen_force - c).
 * hs_computed_torque:    the unique base acceleration a_b [6] and joint torque tau [69] with
 *                            M (a_b; qdd_des) + c - gen_force = (0_6; tau),
 *                        the floating-base inverse dynamics: the base is not actuated, so its
 *                        acceleration follows from the joints'. tau is not clamped to any effort limit.
 * hs_solve:              out[e,j] = M[e]^-1 rhs[e,j] for the k rows j of each env. A Jacobian block
 *                        jac[e,b] ([6,75]) as rhs gives J_b M^-1, and J_b M^-1 J_b^T is the inverse
 *                        operational-space inertia of body b.
 *
 * The solve is the sparse L^T D L factorisation on the dof tree (no fill-in), deepest dof first;
 * every right-hand side of a call goes through the same instructions, so a row of a k-row call has the
 * bits of the one-row call on it.
 */
#ifndef HUMANOID_SOLVE_H
#define HUMANOID_SOLVE_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HS_MAX_RHS 32            /* rows per env of one hs_solve call */

/* flags of the three solves */
#define HS_FLAG_ARMATURE 1u      /* bit 0: model.armature on the dof diagonal of M */
#define HS_FLAG_NO_GRAVITY 2u    /* bit 1: c without gravity (no effect on hs_solve) */
#define HS_FLAGS_DEFAULT HS_FLAG_ARMATURE
#define HS_FLAGS_ALL (HS_FLAG_ARMATURE | HS_FLAG_NO_GRAVITY)

typedef struct hs_solver hs_solver;

const char* hs_last_error(void);
int hs_version(void);

/* The host-side check hs_create applies to a model (no device needed): non-zero, with the reason in
 * hs_last_error(), for a null model, one hd_validate_model would refuse (body / dof counts other than
 * 24 / 69, a bad pair count, body 0 not the root, bodies out of DFS order, an unknown geom type, a
 * chain deeper than 8 joints, too many box geoms), or a tree other than the one the factorisation is
 * unrolled for. */
int hs_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernels need of the model and the gravity vector to
 * it. Non-zero for a null output pointer, num_envs < 1, a null gravity vector or a refused model. */
int hs_create(int device, const he_model* model, const float gravity[3], int num_envs, hs_solver** out);
int hs_destroy(hs_solver* h);

/* Each call below is one launch for all envs. It is refused, before any launch and with nothing
 * written, for a null handle, a null state pointer, a null required input or output, k out of range
 * or flag bits outside HS_FLAGS_ALL. */

/* gen_force f32 [N,75] or NULL (zero); qdd_out f32 [N,75]. */
int hs_forward_dynamics(hs_solver* h, const float* root_state, const float* dof_state, const float* gen_force,
                        float* qdd_out, uint32_t flags, void* stream);

/* qdd_des f32 [N,69]; gen_force f32 [N,75] or NULL (zero); tau_out f32 [N,69] and base_acc_out f32
 * [N,6]: either may be NULL (not written), not both. */
int hs_computed_torque(hs_solver* h, const float* root_state, const float* dof_state, const float* qdd_des,
                       const float* gen_force, float* tau_out, float* base_acc_out, uint32_t flags, void* stream);

/* rhs and out f32 [N,k,75], 1 <= k <= HS_MAX_RHS; the k rows of an env share one factorisation.
 * rhs == out is refused; any other overlap is the caller's error. */
int hs_solve(hs_solver* h, const float* root_state, const float* dof_state, const float* rhs, float* out, int k,
             uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_SOLVE_H */
