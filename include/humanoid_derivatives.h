/*
 * humanoid_derivatives.h -- C ABI of the dynamics derivatives of the MI355X (gfx950) humanoid engine: how
 * the inverse dynamics tau = M(q) a + c(q, qd) changes with the pose and with the generalised velocity,
 * for every env in one launch. They are what every linearising method starts from: LQR about a pose,
 * iLQR / DDP, linear MPC, gain scheduling, the sensitivity of a computed-torque law. With the solves of
 * humanoid_solve.h they give the derivatives of the forward dynamics (see the end of the definitions).
 *
 * The entry points are a third family inside libhumanoid_solve.so, under this header and the prefix hg_:
 * the computed-torque kernel forms the bodies' velocities, accelerations and Newton-Euler wrenches, and
 * here it also propagates their exact tangents along the tree (no differencing on the device). Like the
 * hs_ family it only READS the engine's state buffers through device pointers.
 *
 * Conventions (those of humanoid_solve.h)
 *   - every entry point returns 0 on success, non-zero on failure; hg_last_error() gives the text;
 *   - float pointers are DEVICE pointers on the handle's device, owned by the caller, contiguous and
 *     4-byte aligned; `stream` is a hipStream_t (NULL = default stream); no call synchronises the host;
 *   - quaternions are xyzw, Z-up; all device arithmetic is float32; inputs are never written.
 *
 * ---------------------------------------------------------------------------------------------
 * DEFINITIONS (what a test restates; everything else follows from them)
 *
 * Take q, qd, the column order and the two flags from humanoid_dynamics.h.
 *   - qd[0:3] is the root origin's linear velocity in the world.
 *   - qd[3:6] is the root's angular velocity in the world.
 *   - qd[6+d] is the child-frame relative rate of the ball joints.
 *
 * For a direction delta in R^75 the moved pose q (+) delta is the pose after flowing for unit time at
 * generalised velocity delta:
 *   - the root position moves by delta[0:3];
 *   - the root rotation becomes exp([delta[3:6]]x) R_0;
 *   - joint b becomes R_a exp([theta_b]x) exp([delta_b]x).
 * This is the map of the inverse kinematics' own step (humanoid_ik.h). The velocity components qd and the
 * acceleration components a keep their values, in their own coordinates.
 *
 * With tau(q, qd, a) = M(q) a + c(q, qd), all 75 rows including the six base rows:
 *   - dtau_dq[e, i, j] = d/d eps tau_i(q (+) eps e_j, qd, a) at eps = 0;
 *   - dtau_dv[e, i, j] = d tau_i / d qd_j.
 * Both are [N,75,75] float32. tau [N,75] is M a + c itself, the base rows included.
 *
 * Consequences:
 *   - Both are exactly zero where column j's joint and row i's joint are not ancestor-or-self related
 *     (the pattern of M). The kernel writes these zeros; it does not compute them.
 *   - Columns 0-2 of dtau_dq are exactly zero, because gravity is uniform. So are columns 0-2 of
 *     dtau_dv: no force depends on the root's linear velocity.
 *   - dtau_dv does not depend on a, on gravity or on the armature: its bits are the same under every
 *     acc and every flag.
 *   - The armature does not enter either derivative. It enters only tau, through M a.
 *   - dtau_dq is affine in a: dtau_dq(a) - dtau_dq(0) is linear in a.
 *   - c without gravity is homogeneous of degree 2 in qd. Hence dtau_dv . qd = 2 c, with c taken under
 *     the no-gravity flag.
 *
 * The forward dynamics qdd = M^-1 (gen_force - c) then has, at fixed gen_force,
 *     d qdd / d q   = -M^-1 dtau_dq at a = qdd,
 *     d qdd / d qd  = -M^-1 dtau_dv,
 *     d qdd / d tau =  M^-1,
 * M with the armature when the flag is set (the armature does not enter dtau_dq, but it enters qdd and
 * M^-1). Under HG_FLAG_BY_DIRECTION the matrices are written transposed, [e, j, i]: row j is the
 * derivative along direction j, a right-hand side of the M^-1 solve of humanoid_solve.h as it stands, in
 * chunks of at most 32 rows.
 */
#ifndef HUMANOID_DERIVATIVES_H
#define HUMANOID_DERIVATIVES_H

#include <stdint.h>

#include "humanoid_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HG_NUM_OUTPUTS 3

/* flags: humanoid_solve.h's bits, and the layout */
#define HG_FLAG_ARMATURE 1u      /* bit 0: armature_d a_d in tau */
#define HG_FLAG_NO_GRAVITY 2u    /* bit 1: g = 0 */
#define HG_FLAG_BY_DIRECTION 4u  /* bit 2: dtau_dq, dtau_dv as [e, j, i] */
#define HG_FLAGS_DEFAULT HG_FLAG_ARMATURE
#define HG_FLAGS_ALL (HG_FLAG_ARMATURE | HG_FLAG_NO_GRAVITY | HG_FLAG_BY_DIRECTION)

typedef struct hg_derivatives hg_derivatives;

/* The three outputs of hg_compute. A NULL member is neither computed nor written. An output's bits do
 * not depend on which others are asked for. */
typedef struct hg_outputs {
    float* dtau_dq;  /* [N,75,75] */
    float* dtau_dv;  /* [N,75,75] */
    float* tau;      /* [N,75]: M a + c */
} hg_outputs;

const char* hg_last_error(void);
int hg_version(void);

/* The host-side check hg_create applies to a model (no device needed): that of hs_validate_model. */
int hg_validate_model(const he_model* model);

/* Binds HIP device `device` and copies what the kernel needs of the model and the gravity vector to it.
 * Non-zero for a null output pointer, num_envs < 1, a null gravity vector or a refused model. */
int hg_create(int device, const he_model* model, const float gravity[3], int num_envs, hg_derivatives** out);
int hg_destroy(hg_derivatives* h);

/* One launch for all envs. root_state f32 [N,13] and dof_state f32 [N*69,2] are the engine's
 * HE_BUF_ROOT_STATE / HE_BUF_DOF_STATE (or arrays laid out like them); acc f32 [N,75] is the generalised
 * acceleration a (base 6, then the 69 joints), or NULL (zero).
 * Refusals, in this order, each with "hg_compute" in the reason and before any launch: a null handle; a
 * null state pointer; a null `out`; all three outputs null; an output that is also an input (root_state,
 * dof_state or acc) or two outputs that are the same buffer; flag bits outside HG_FLAGS_ALL; a buffer
 * that is not 4-byte aligned. */
int hg_compute(hg_derivatives* h, const float* root_state, const float* dof_state, const float* acc,
               const hg_outputs* out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANOID_DERIVATIVES_H */
