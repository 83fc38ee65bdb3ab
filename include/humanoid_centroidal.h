/*
 * humanoid_centroidal.h -- C ABI of the centroidal-dynamics queries of the MI355X (gfx950) humanoid
 * engine: one HIP kernel that forms, for the state the engine is in, the centre of mass, its velocity,
 * the linear momentum and the angular momentum about the centre of mass, the centroidal momentum matrix
 * A_G, its rate term Adot_G qd and the kinetic and potential energy of every env. These are the
 * quantities balance controllers regulate (CoM PD, angular-momentum damping, capture point) and RL
 * rewards read (CoM height and velocity, energy, momentum).
 *
 * The entry points are a second family inside libhumanoid_dynamics.so, under this header and the
 * prefix hc_: the kernel shares the dynamics kernel's path from the state to the composite inertias,
 * stops there and writes 1.9 KB per env where the mass matrix takes 22.5 KB. Like the hd_ family it only
 * READS the engine's state buffers through device pointers.
 *
 * Conventions (those of humanoid_engine.h)
 *   - every entry point returns 0 on success, non-zero on failure; hc_last_error() gives the text;
 *   - pointers passed to hc_compute are DEVICE pointers on the handle's device, owned by the caller;
 *     `stream` is a hipStream_t (NULL = default stream); hc_compute does not synchronise the host;
 *   - quaternions are xyzw, Z-up; all device arithmetic is float32.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates; everything else follows from them)
 *
 * Kinematics, the generalised velocity qd [75] and its column order (root linear 3, root angular 3,
 * the 69 child-frame dof rates) are humanoid_dynamics.h's; they are not repeated here.
 *
 * Per body b: c_b = p_b + R_b com[b] the world centre of mass, v_b the velocity of that point, w_b the
 * body's world angular velocity, I_wb = R_b I_b R_b^T the inertia about c_b in world axes, m_b the mass;
 * m = sum_b m_b. Jc_b [3,75] is the Jacobian of c_b (v_b = Jc_b qd), Jw_b [3,75] the angular rows of the
 * body Jacobian (w_b = Jw_b qd).
 *
 *   com      [N,3]     sum_b m_b c_b / m, world frame
 *   com_vel  [N,3]     sum_b m_b v_b / m
 *   momentum [N,6]     P = sum_b m_b v_b (3), then L_G = sum_b (c_b - com) x m_b v_b + I_wb w_b (3):
 *                      linear before angular, as the rows of the body Jacobians
 *   cmm      [N,6,75]  the centroidal momentum matrix A_G, momentum = A_G qd: column i is
 *                      sum_b m_b Jc_b[:,i]  and  sum_b (c_b - com) x m_b Jc_b[:,i] + I_wb Jw_b[:,i]
 *   cmm_bias [N,6]     Adot_G qd: the time derivative of `momentum` at qdd = 0, so that
 *                      d/dt momentum = A_G qdd + cmm_bias. With a_b, wd_b the acceleration of c_b and the
 *                      angular acceleration of body b at qdd = 0 (humanoid_dynamics.h's bias force is
 *                      built on the same two):
 *                      sum_b m_b a_b  and  sum_b (c_b - com) x m_b a_b + I_wb wd_b + w_b x I_wb w_b
 *                      (the term sum_b (v_b - com_vel) x m_b v_b of the product rule is -com_vel x P = 0).
 *                      With no external force but gravity, d/dt momentum = (m g, 0).
 *   energy   [N,2]     kinetic 1/2 sum_b (m_b |v_b|^2 + w_b^T I_wb w_b) (no armature), then potential
 *                      -m g . com with the gravity vector given to hc_create
 *
 * Identities, with M and c humanoid_dynamics.h's mass matrix WITHOUT armature and bias force WITHOUT
 * gravity, r = com - p_0:
 *   A_G[0:3]   = M[0:3]
 *   A_G[3:6]   = M[3:6] - r x M[0:3]             per column
 *   A_G[3:6, 3:6] is the centroidal (locked) inertia: the average angular velocity is A_G[3:6,3:6]^-1 L_G
 *   A_G[0:3, 0:3] = m 1,  A_G[3:6, 0:3] = 0
 *   cmm_bias[0:3] = c[0:3],  cmm_bias[3:6] = c[3:6] - r x c[0:3]
 *   kinetic    = 1/2 qd^T M qd
 * Armature never reaches the base rows of M and gravity enters only the potential energy, so there are
 * no flags.
 *
 * A far-away env loses no accuracy in anything but `com` itself: every lever is formed relative to the
 * root origin p_0, and the world centre of mass is p_0 + r, formed once at the end.
 */
#ifndef HUMANOID_CENTROIDAL_H
#define HUMANOID_CENTROIDAL_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_MOMENTUM_ROWS 6       /* linear momentum 3, angular momentum about the centre of mass 3 */
#define HC_NUM_OUTPUTS 6

typedef struct hc_centroidal hc_centroidal;

/* The six outputs of hc_compute, in the table's order: device pointers to float32 arrays, contiguous
 * and 4-byte aligned (no more: com's 12-byte rows fall on every alignment). A NULL member is neither
 * computed nor written. An output's bits do not depend on which others are asked for. */
typedef struct hc_outputs {
    float* com;       /* [N,3] */
    float* com_vel;   /* [N,3] */
    float* momentum;  /* [N,6] */
    float* cmm;       /* [N,6,75] */
    float* cmm_bias;  /* [N,6] */
    float* energy;    /* [N,2] kinetic, potential */
} hc_outputs;

const char* hc_last_error(void);
int hc_version(void);

/* The host-side check hc_create applies to a model (no device needed): that of hd_validate_model. */
int hc_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model and the gravity vector to it.
 * Non-zero for a null output pointer, num_envs < 1, a null gravity vector or a refused model. */
int hc_create(int device, const he_model* model, const float gravity[3], int num_envs, hc_centroidal** out);
int hc_destroy(hc_centroidal* h);

/* One launch for all envs. root_state f32 [N,13] and dof_state f32 [N*69,2] are the engine's
 * HE_BUF_ROOT_STATE / HE_BUF_DOF_STATE (or arrays laid out like them). Refusals, in this order, each
 * with "hc_compute" in the reason: a null handle; a null state pointer; a null `out`; all six outputs
 * null; a state or output pointer that is not 4-byte aligned. */
int hc_compute(hc_centroidal* h, const float* root_state, const float* dof_state, const hc_outputs* out,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_CENTROIDAL_H */
