// he_probe.hip -- the joint-space vector solves of he_regla.h on their own, in both forms of their
// lane-masked updates (under EXEC, and as FMA + select), for tests/test_gpu_masked_solves.py.
#include "he_kernels.h"
#include "he_regla.h"

namespace {
using namespace regla;

// one wave per vector: the packed factor into LDS in the engine's layout (Lds::Lp: row K at
// kPackStart[K], the entry of the ancestor at depth d at offset d), then y <- L^-T y and y <- L^-1 y
// of the same vector in each form. out[form][v][dof], form = 0 L^-T under EXEC, 1 L^-T select,
// 2 L^-1 under EXEC, 3 L^-1 select.
__global__ void __launch_bounds__(W) masked_solve_probe_kernel(const float* __restrict__ factor,
                                                              const float* __restrict__ y, int n,
                                                              float* __restrict__ out) {
    __shared__ alignas(16) float Lp[kNpack + 4];
    __shared__ int16_t pack_start[NG];
    __shared__ int8_t dof_depth[NG];
    const int lane = threadIdx.x;
    const int v = blockIdx.x;
    for (int i = lane; i < kNpack + 4; i += W) Lp[i] = i < kNpack ? factor[i] : 0.f;
    for (int i = lane; i < NG; i += W) {
        pack_start[i] = (int16_t)kPackStart[i];
        dof_depth[i] = (int8_t)(kDofNanc[i] - 1);
    }
    __syncthreads();
    const bool hi = lane < NH;
    const float y1 = y[(size_t)v * NG + lane];
    const float y2 = hi ? y[(size_t)v * NG + 64 + lane] : 0.f;
    const int dj = dof_depth[lane], dj2 = hi ? dof_depth[64 + lane] : 0;
    const float* row1 = Lp + pack_start[lane];
    const float* row2 = Lp + pack_start[hi ? 64 + lane : 0];
    auto store = [&](int form, float a, float b) {
        float* o = out + ((size_t)form * n + v) * NG;
        o[lane] = a;
        if (hi) o[64 + lane] = b;
    };
    float a = y1, b = y2;
    solve_LT_vec_pipelined<true>(Lp, dj, dj2, a, b);
    store(0, a, b);
    a = y1, b = y2;
    solve_LT_vec_pipelined<false>(Lp, dj, dj2, a, b);
    store(1, a, b);
    a = y1, b = y2;
    solve_L_streamed<true>(row1, row2, a, b);
    store(2, a, b);
    a = y1, b = y2;
    solve_L_streamed<false>(row1, row2, a, b);
    store(3, a, b);
}
}  // namespace

hipError_t launch_masked_solve_probe(const float* factor, const float* y, int n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    masked_solve_probe_kernel<<<n, W, 0, stream>>>(factor, y, n, out);
    return hipGetLastError();
}
