/*
 * humanoid_wrench.h -- C ABI of the joint-reaction queries of the MI355X (gfx950) humanoid engine: the
 * wrench every joint transmits and the acceleration of every body, for a given motion (desired joint
 * accelerations, a prescribed or a free base) and given external wrenches, in one launch. These are the
 * outputs of inverse dynamics that joint-load rewards and limits, force-sensor and IMU emulation, the
 * analysis of a reference motion (what the ground must supply) and a momentum observer read.
 *
 * The entry points are a second family inside libhumanoid_solve.so, under this header and the prefix
 * hw_: the computed-torque kernel already forms every subtree's Newton-Euler wrench and composite
 * inertia about its own joint origin; here it writes them instead of reducing them to the joint torques
 * alone. Like the hs_ family it only READS the engine's state buffers through device pointers.
 *
 * Conventions (those of humanoid_solve.h)
 *   - every entry point returns 0 on success, non-zero on failure; hw_last_error() gives the text;
 *   - float pointers are DEVICE pointers on the handle's device, owned by the caller, contiguous and
 *     4-byte aligned; `stream` is a hipStream_t (NULL = default stream); no call synchronises the host;
 *   - quaternions are xyzw, Z-up; all device arithmetic is float32; inputs are never written.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates; everything else follows from them)
 *
 * Kinematics, the generalised velocity qd [75] and its column order (root linear 3, root angular 3, the
 * 69 child-frame dof rates) are humanoid_dynamics.h's; M [75,75] and c [75] are its mass matrix and bias
 * force (humanoid_solve.h). They are not repeated here.
 *
 * Per body b: p_b the origin (= the origin of joint b, which ties b to its parent), R_b the rotation,
 * c_b = p_b + R_b com[b] the centre of mass, w_b the angular velocity, I_wb = R_b I_b R_b^T the inertia
 * about c_b in world axes, m_b the mass, g the gravity vector given to hw_create (HW_FLAG_NO_GRAVITY: 0).
 * sub(j) is the set of bodies of the subtree rooted at j, j included. Jc_b [3,75] is the Jacobian of c_b,
 * Jw_b [3,75] the angular rows of the body Jacobian.
 *
 * External wrench. body_force f_b and body_torque t_b [N*24,3] are a force acting AT THE CENTRE OF MASS
 * of body b and a torque, both in world axes: he_apply_body_forces' convention with HE_SPACE_GLOBAL. A
 * NULL array is zero. There is no other convention; a force at another point x is the force at c_b with
 * the torque (x - c_b) x f added by the caller. Their generalised force is
 *     G = sum_b Jc_b^T f_b + Jw_b^T t_b.
 *
 * Accelerations. The generalised acceleration is qdd = (a_b; qdd_des), qdd_des [N,69] (NULL: zero).
 *   base_acc given (prescribed base): a_b = base_acc [N,6]; its linear part is the time derivative of
 *       the root origin's world velocity, its angular part that of the root's angular velocity.
 *   base_acc NULL (free base): a_b is the base acceleration for which nothing acts on the root, that is
 *       hs_computed_torque's a_b with gen_force = G.
 * a_cb and wd_b are the acceleration of c_b and the angular acceleration of body b at that qdd, velocity
 * products included.
 *
 *   wrench   [N,24,6]  force 3, then torque 3 (linear before angular, as everywhere here): the wrench the
 *                      parent exerts on body j through joint j, about the joint origin p_j,
 *                        F_j = sum_{b in sub(j)} [ m_b (a_cb - g) - f_b ]
 *                        N_j = sum_{b in sub(j)} [ I_wb wd_b + w_b x I_wb w_b - t_b
 *                                                  + (c_b - p_j) x (m_b (a_cb - g) - f_b) ]
 *                      frame HW_FRAME_WORLD: in world axes; HW_FRAME_BODY: both parts in body j's axes
 *                      (R_j^T F_j, R_j^T N_j), the form a sensor on the body reads.
 *                      j = 0: the wrench something outside must exert on the root. With a free base it is
 *                      the 6 x 6 solve's rounding residual, written as computed and not forced to zero;
 *                      with a prescribed base it is the external wrench the motion leaves unexplained.
 *   tau      [N,69]    tau_d = (R_j e_i) . N_j + armature_d qdd_d for dof d = 3 (j - 1) + i, the armature
 *                      term under HW_FLAG_ARMATURE (on by default)
 *   base_acc [N,6]     the a_b used; with a prescribed base a copy of the input
 *   body_acc [N,24,6]  the acceleration of body b's origin (3), then its angular acceleration (3), in
 *                      world axes: d/dt of the linear and angular velocity columns of HE_BUF_RB_STATE
 *
 * Identities, with M and c WITHOUT armature:
 *   (F_0, N_0)           = (M qdd + c - G)[0:6]
 *   tau without armature = (M qdd + c - G)[6:]
 *   free base, no external wrench: tau and base_acc are hs_computed_torque's (the same bits)
 *   at rest (qd = 0), qdd = 0 with a prescribed base, no external wrench: F_j = -m_sub(j) g
 *
 * A far-away env loses no accuracy: every lever is formed relative to the root origin, and every
 * subtree's wrench and inertia are referred to the subtree's own joint origin, so a hand's wrench is
 * exact to float32 of the hand's own and not of the whole body's.
 */
#ifndef HUMANOID_WRENCH_H
#define HUMANOID_WRENCH_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HW_WRENCH_ROWS 6         /* force 3, torque 3; body_acc: linear 3, angular 3 */
#define HW_NUM_OUTPUTS 4

/* the frame of `wrench` */
#define HW_FRAME_WORLD 0
#define HW_FRAME_BODY 1

/* flags: humanoid_solve.h's bits */
#define HW_FLAG_ARMATURE 1u      /* bit 0: armature_d qdd_d in tau */
#define HW_FLAG_NO_GRAVITY 2u    /* bit 1: g = 0 */
#define HW_FLAGS_DEFAULT HW_FLAG_ARMATURE
#define HW_FLAGS_ALL (HW_FLAG_ARMATURE | HW_FLAG_NO_GRAVITY)

typedef struct hw_reaction hw_reaction;

/* The four outputs of hw_compute, in the table's order. A NULL member is neither computed nor written.
 * An output's bits do not depend on which others are asked for. */
typedef struct hw_outputs {
    float* wrench;    /* [N,24,6] */
    float* tau;       /* [N,69] */
    float* base_acc;  /* [N,6] */
    float* body_acc;  /* [N,24,6] */
} hw_outputs;

const char* hw_last_error(void);
int hw_version(void);

/* The host-side check hw_create applies to a model (no device needed): that of hs_validate_model. */
int hw_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model and the gravity vector to it.
 * Non-zero for a null output pointer, num_envs < 1, a null gravity vector or a refused model. */
int hw_create(int device, const he_model* model, const float gravity[3], int num_envs, hw_reaction** out);
int hw_destroy(hw_reaction* h);

/* One launch for all envs. root_state f32 [N,13] and dof_state f32 [N*69,2] are the engine's
 * HE_BUF_ROOT_STATE / HE_BUF_DOF_STATE (or arrays laid out like them); qdd_des f32 [N,69] or NULL
 * (zero); base_acc f32 [N,6] or NULL (free base); body_force, body_torque f32 [N*24,3] or NULL (zero).
 * Refusals, in this order, each with "hw_compute" in the reason and before any launch: a null handle; a
 * null state pointer; a null `out`; all four outputs null; `frame` outside 0..1; flag bits outside
 * HW_FLAGS_ALL; a buffer that is not 4-byte aligned. */
int hw_compute(hw_reaction* h, const float* root_state, const float* dof_state, const float* qdd_des,
               const float* base_acc, const float* body_force, const float* body_torque, const hw_outputs* out,
               int frame, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_WRENCH_H */
