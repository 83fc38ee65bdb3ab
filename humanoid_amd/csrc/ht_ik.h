// ht_ik.h -- the inverse-kinematics queries of libhumanoid_task.so (include/humanoid_ik.h, the hk_ entry
// points): the family's handle, its refusals and its one launch. ht_task.hip includes this file last: one
// translation unit, one library, two public headers. The kernel is task_kernel itself, with
// Params::control = kControlIk: its passes, the row errors and the integration are in ht_task.hip.
#pragma once
#include "../../include/humanoid_ik.h"
#include "he_host.h"
#include "he_tree_state.h"

struct hk_solver : QueryHandle<TreeModel> {
    DeviceArray<float> d_limits;  // [2,69] the model's dof_lower, dof_upper
    int k = 0;                    // 0: no rows yet
    ht_row rows[HT_MAX_ROWS] = {};
};

extern "C" {

// the translation unit has one error text: hk_last_error and ht_last_error read the same one
const char* hk_last_error(void) { return last_error(); }
int hk_version(void) { return 1; }

int hk_validate_model(const he_model* model) { return ht_validate_model(model); }

int hk_create(int device, const he_model* model, const float gravity[3], int num_envs, hk_solver** out) {
    if (query_create("hk_create", device, model, gravity, num_envs, out, hk_validate_model, fill_tree_model)) return 1;
    float limits[2 * ND];
    for (int d = 0; d < ND; ++d) limits[d] = model->dof_lower[d], limits[ND + d] = model->dof_upper[d];
    const hipError_t e = (*out)->d_limits.assign(limits, 2 * ND);
    if (e != hipSuccess) {  // *out is null on every failure
        query_destroy(*out);
        *out = nullptr;
        return fail("hk_create: the dof limits: %s", hipGetErrorString(e));
    }
    return 0;
}

int hk_destroy(hk_solver* h) { return query_destroy(h); }

int hk_set_rows(hk_solver* h, const ht_row* rows, int k) { return set_rows("hk_set_rows", h, rows, k); }

int hk_solve(hk_solver* h, const float* root_state, const float* dof_state, const float* target, const float* target_rot,
             int iterations, float damping, float step_clip, float* root_out, float* dof_out, float* residual_out,
             uint32_t flags, void* stream) {
    const char* who = "hk_solve";
    if (check_call(who, h, root_state, dof_state)) return 1;
    if (!target) return fail("%s: null target", who);
    if (!root_out || !dof_out) return fail("%s: null output state pointer", who);
    if (check_flags(who, flags, HK_FLAGS_ALL)) return 1;
    if (iterations < 1 || iterations > HK_MAX_ITERATIONS)
        return fail("%s: iterations = %d outside 1..%d", who, iterations, HK_MAX_ITERATIONS);
    if (!(damping >= 0.f) || !std::isfinite(damping))
        return fail("%s: damping %g is negative or not finite", who, (double)damping);
    if (!(step_clip > 0.f) || !std::isfinite(step_clip))
        return fail("%s: step_clip %g is not positive or not finite", who, (double)step_clip);
    if (check_aligned(who, {root_state, dof_state, target, target_rot, root_out, dof_out, residual_out})) return 1;
    if (h->k < 1) return fail("%s: no rows set (hk_set_rows)", who);
    if (!target_rot)
        for (int r = 0; r < h->k; ++r)
            if (h->rows[r].axis >= 3) return fail("%s: row %d is angular and target_rot is null", who, r);
    Params P{};
    P.root = P.root_out = root_out;  // the kernel's passes read the iterate
    P.dof = P.dof_out = dof_out;
    P.root_in = root_state;
    P.dof_in = dof_state;
    P.xdd_des = target;
    P.target_rot = target_rot;
    P.limits = h->d_limits;
    P.residual = residual_out;
    P.step_clip = step_clip;
    P.iterations = iterations;
    P.damping = damping;
    P.control = kControlIk;
    P.mode = HT_MODE_FORCE;
    P.flags = flags | HT_FLAG_NO_GRAVITY;  // gravity never enters: c = 0 at the resting iterate
    return launch_rows(*h, P, stream);
}

}  // extern "C"
