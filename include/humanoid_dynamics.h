/*
 * humanoid_dynamics.h -- C ABI of libhumanoid_dynamics.so, the dynamics-query tensors of the MI355X
 * (gfx950) humanoid engine: one HIP kernel that forms, for the state the engine is in, the body
 * Jacobians, the joint-space inertia and the gravity / Coriolis force of every env. It is the product
 * side of Isaac Gym's acquire_jacobian_tensor / acquire_mass_matrix_tensor (+ refresh_*), plus the
 * bias force those two leave out.
 *
 * The library is separate from libhumanoid_engine.so and only READS the engine's state buffers through
 * device pointers: nothing here is linked into the engine, whose device code stays as it is.
 *
 * Conventions (those of humanoid_engine.h)
 *   - every entry point returns 0 on success, non-zero on failure; hd_last_error() gives the text;
 *   - float pointers passed to hd_compute are DEVICE pointers on the handle's device, owned by the
 *     caller; `stream` is a hipStream_t (NULL = default stream); hd_compute does not synchronise the host;
 *   - quaternions are xyzw, Z-up; all device arithmetic is float32.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates; everything else follows from them)
 *
 * Kinematics. Body 0 is the floating root: origin p_0 = root_state[0:3], rotation R_0 = the matrix of
 * the (normalised) quaternion root_state[3:7]. Body b >= 1 hangs on its parent a = parents[b] by an
 * exp-map ball joint: with the joint's three dof positions th = dof_state[3(b-1) .. 3(b-1)+2, 0],
 *   R_b = R_a exp([th]x)   (Rodrigues),     p_b = p_a + R_a local_pos[b].
 * The kernel runs this forward kinematics itself from root_state and dof_state; it does not read the
 * rigid-body state buffer, so it is right immediately after an indexed state write.
 *
 * Generalised velocity qd [75], Isaac Gym's floating-base column order, root first, linear before
 * angular:
 *   qd[0:3]  = root_state[7:10]   the linear velocity of the root ORIGIN, world frame;
 *   qd[3:6]  = root_state[10:13]  the root's angular velocity, world frame;
 *   qd[6+d]  = dof_state[d, 1]    the 69 dof velocities.
 * The dof velocities of joint b are the engine's CHILD-FRAME RELATIVE RATES u_b of the ball joint: the
 * angular velocity of body b relative to its parent, in body b's own frame (the pose flows as
 * R_a exp([th]x) exp([e u_b]x)). They are NOT the time derivatives of the exp-map coordinates th (the two
 * agree only at th = 0). The world angular velocity of body b is w_b = w_a + R_b u_b.
 *
 * Jacobian jac [N,24,6,75] f32. Rows of body b: (linear velocity of the body ORIGIN p_b [3], world
 * angular velocity [3]). Defining property: jac[e,b] @ qd[e] == rb_state[e,b,7:13]. Columns:
 *   root linear i:   (e_i, 0);            root angular i:  (e_i x (p_b - p_0), e_i);
 *   dof i of joint j, for b in j's subtree (j itself included), a = R_j e_i:   (a x (p_b - p_j), a);
 *   exactly zero for every body outside j's subtree.
 *
 * Mass matrix mass [N,75,75] f32: the symmetric M with  1/2 qd^T M qd = kinetic energy,
 *   M = sum_b  m_b Jc_b^T Jc_b + Jw_b^T (R_b I_b R_b^T) Jw_b,
 * Jc_b the Jacobian of body b's centre of mass p_b + R_b com[b], Jw_b its angular rows, I_b the body's
 * inertia about its centre of mass (model.inertia). M[i,k] is exactly zero when neither column's joint
 * is an ancestor-or-self of the other's. HD_FLAG_ARMATURE (on by default: it is the inertia the
 * engine's own solve uses) adds model.armature[d] to M[6+d, 6+d]; without it M is the CRBA inertia.
 *
 * Bias force bias [N,75] f32: c with  M qdd + c = tau,  the generalised force that holds qdd = 0 (RNEA):
 * gravity plus the velocity products (Coriolis, centrifugal, gyroscopic), qdd being the time
 * derivative of qd as defined above (root origin acceleration, root angular acceleration in the world,
 * child-frame rate derivatives). Gravity is the vector given to hd_create; HD_FLAG_NO_GRAVITY leaves
 * it out. Armature does not enter c.
 */
#ifndef HUMANOID_DYNAMICS_H
#define HUMANOID_DYNAMICS_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HD_JAC_ROWS 6            /* per body: origin linear velocity 3, world angular velocity 3 */

/* hd_compute flags */
#define HD_FLAG_ARMATURE 1u      /* bit 0: model.armature on the dof diagonal of the mass matrix */
#define HD_FLAG_NO_GRAVITY 2u    /* bit 1: the bias force without gravity (velocity products only) */
#define HD_FLAGS_DEFAULT HD_FLAG_ARMATURE
#define HD_FLAGS_ALL (HD_FLAG_ARMATURE | HD_FLAG_NO_GRAVITY)

typedef struct hd_dynamics hd_dynamics;

const char* hd_last_error(void);
int hd_version(void);

/* The host-side check hd_create applies to a model (no device needed): non-zero, with the reason in
 * hd_last_error(), for a null model or one he_set_model would refuse (body / dof counts other than
 * 24 / 69, a bad pair count, body 0 not the root, bodies out of DFS order, an unknown geom type, a
 * chain deeper than 8 joints, too many box geoms). */
int hd_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model (tree, joint offsets,
 * masses, centres of mass, inertias, armature) and the gravity vector to it. Non-zero for a null
 * output pointer, num_envs < 1, a null gravity vector or a refused model. */
int hd_create(int device, const he_model* model, const float gravity[3], int num_envs, hd_dynamics** out);
int hd_destroy(hd_dynamics* h);

/* One launch for all envs. root_state f32 [N,13] and dof_state f32 [N*69,2] are the engine's
 * HE_BUF_ROOT_STATE / HE_BUF_DOF_STATE (or arrays laid out like them). Outputs: jac_out f32
 * [N,24,6,75], mass_out f32 [N,75,75], bias_out f32 [N,75], contiguous and 4-byte aligned; a NULL
 * output is not computed or written, at least one must be given. Non-zero (reason in hd_last_error)
 * for a null handle, a null state pointer, all outputs null, or flag bits outside HD_FLAGS_ALL. */
int hd_compute(hd_dynamics* h, const float* root_state, const float* dof_state, float* jac_out,
               float* mass_out, float* bias_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_DYNAMICS_H */
