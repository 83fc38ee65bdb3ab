// he_forces.hip -- external wrench preparation for gfx950 (he_apply_body_forces and
// he_apply_body_forces_at_pos; gym.apply_rigid_body_force_tensors, puffer_phc/envs/render_env.py:105-126)
// and the dof actuation forces' (he_set_dof_actuation_forces; dof_actuation_kernel below).
//
// One thread per body row: the caller's (force, torque) or (force, application point) rows in
// `space` and the body's current rigid-body row become the engine's world-axis (torque, force at the
// CoM) row, overwritten or accumulated. The physics kernels (he_physics.hip, the EXT instantiations)
// only ever see that row. Plain vector loads and stores: each thread owns its row.
#include <hip/hip_runtime.h>

#include "../../include/humanoid_engine.h"
#include "he_kernels.h"
#include "he_math.h"

namespace {

constexpr int NB = HE_NUM_BODIES;
constexpr int ND = HE_NUM_DOF;

__global__ void __launch_bounds__(256) body_wrench_kernel(WrenchArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    const int b = r % NB;
    const float* rb = a.rb_state + (size_t)r * 13;
    const f4 q = f4{rb[3], rb[4], rb[5], rb[6]};
    const bool local = a.space == HE_SPACE_LOCAL;
    f3 f = f3{0.f, 0.f, 0.f}, t = f3{0.f, 0.f, 0.f};
    if (a.force) {
        const float* s = a.force + (size_t)r * 3;
        f = f3{s[0], s[1], s[2]};
        if (local) f = qapply(q, f);
    }
    if (a.second) {
        const float* s = a.second + (size_t)r * 3;
        f3 v = f3{s[0], s[1], s[2]};
        if (a.at_pos) {
            // the application point about the body's CoM: a local point is in the body frame (about the
            // body origin), a global / env one in the world frame the rigid-body rows are in
            const he_model& m = *a.model;
            const f3 c = qapply(q, f3{m.com[b][0], m.com[b][1], m.com[b][2]});  // CoM about the body origin
            const f3 x = local ? qapply(q, v) : v - f3{rb[0], rb[1], rb[2]};
            t = cross3(x - c, f);
        } else {
            t = local ? qapply(q, v) : v;
        }
    }
    float* w = a.wrench + (size_t)r * 6;
    if (a.accumulate) {
        t = t + f3{w[0], w[1], w[2]};
        f = f + f3{w[3], w[4], w[5]};
    }
    w[0] = t.x; w[1] = t.y; w[2] = t.z;
    w[3] = f.x; w[4] = f.y; w[5] = f.z;
}

// One thread per (row, dof): the actuation the physics kernels add to Q[6 + d]
__global__ void __launch_bounds__(256) dof_actuation_kernel(DofActArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.count * ND) return;
    const int i = t / ND, d = t - i * ND;
    const int e = a.ids ? a.ids[i] : i;
    if (e < 0 || e >= a.num_envs) return;
    const size_t o = (size_t)e * ND + d;
    const float lim = a.model->effort[d];
    const float v = a.src[o];
    a.act[o] = a.modes[d] == HE_DOF_MODE_EFFORT ? fminf(fmaxf(v, -lim), lim) : 0.f;
}

__global__ void warm_tu_kernel() {}
}  // namespace

hipError_t warm_forces_kernels(hipStream_t stream, int mode) {
    if (mode == 1) {
        warm_tu_kernel<<<1, 64, 0, stream>>>();
        return hipGetLastError();
    }
    WrenchArgs wa{};
    body_wrench_kernel<<<1, 256, 0, stream>>>(wa);  // rows 0: every thread leaves at the guard
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    DofActArgs da{};
    dof_actuation_kernel<<<1, 256, 0, stream>>>(da);  // count 0 likewise
    return hipGetLastError();
}

hipError_t launch_body_wrench(const WrenchArgs& a, hipStream_t stream) {
    if (a.rows <= 0) return hipSuccess;
    body_wrench_kernel<<<(a.rows + 255) / 256, 256, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_dof_actuation(const DofActArgs& a, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    dof_actuation_kernel<<<(a.count * ND + 255) / 256, 256, 0, stream>>>(a);
    return hipGetLastError();
}
