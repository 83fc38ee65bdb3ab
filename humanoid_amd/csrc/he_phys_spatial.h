// he_phys_spatial.h -- spatial (6-D) algebra on plain float arrays (si_apply, dot6, crm, crf,
// body_force) and the physics kernel's short rotation-vector exponential and logarithm (here,
// half_sincos, atan01, pqexp, pqlog).
// LDS: none by name; the callers pass rows of Lds arrays (Ib / Ic, V, F, Acc, S) as pointers. On
// entry: nothing live.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "he_math.h"

namespace {

// spatial inertia (m, h, I6) applied to V=(w, v): n = I w + h x v ; f = m v - h x w
HE_DEV void si_apply(const float* I, const float* V, float* F) {
    f3 h = f3{I[1], I[2], I[3]};
    f3 w = f3{V[0], V[1], V[2]}, v = f3{V[3], V[4], V[5]};
    f3 hv = cross3(h, v), hw = cross3(h, w);
    F[0] = I[4] * w.x + I[7] * w.y + I[8] * w.z + hv.x;
    F[1] = I[7] * w.x + I[5] * w.y + I[9] * w.z + hv.y;
    F[2] = I[8] * w.x + I[9] * w.y + I[6] * w.z + hv.z;
    F[3] = I[0] * v.x - hw.x;
    F[4] = I[0] * v.y - hw.y;
    F[5] = I[0] * v.z - hw.z;
}
HE_DEV float dot6(const float* a, const float* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
// motion cross V x Sm
HE_DEV void crm(const float* V, const float* S, float* O) {
    f3 w = f3{V[0], V[1], V[2]}, v = f3{V[3], V[4], V[5]};
    f3 sw = f3{S[0], S[1], S[2]}, sv = f3{S[3], S[4], S[5]};
    f3 a = cross3(w, sw), b = cross3(w, sv) + cross3(v, sw);
    O[0] = a.x; O[1] = a.y; O[2] = a.z; O[3] = b.x; O[4] = b.y; O[5] = b.z;
}
// force cross V x* F
HE_DEV void crf(const float* V, const float* Fm, float* O) {
    f3 w = f3{V[0], V[1], V[2]}, v = f3{V[3], V[4], V[5]};
    f3 n = f3{Fm[0], Fm[1], Fm[2]}, f = f3{Fm[3], Fm[4], Fm[5]};
    f3 a = cross3(w, n) + cross3(v, f), b = cross3(w, f);
    O[0] = a.x; O[1] = a.y; O[2] = a.z; O[3] = b.x; O[4] = b.y; O[5] = b.z;
}

// RNEA body force f = I a + v x* (I v)
HE_DEV void body_force(const float* I, const float* A, const float* V, float* F) {
    float IA[6], IV[6], X[6];
    si_apply(I, A, IA);
    si_apply(I, V, IV);
    crf(V, IV, X);
    for (int x = 0; x < 6; ++x) F[x] = IA[x] + X[x];
}

// rotation-vector exponential / logarithm for the physics kernel, short instruction sequences (the
// integration runs them in every TGS position iteration): v_sqrt_f32 and v_rcp_f32 (1 ulp), sin / cos
// of the half angle by their Taylor series up to x^9 / x^10 (|x| <= 1: error < 3e-8, below fp32
// rounding; a step turning a joint by more than 2 rad takes ocml's sincosf), atan on [0, 1] by
// Abramowitz-Stegun 4.4.49 (|error| <= 1e-8). The fp64 oracle's tolerance covers them. The imitation
// kernel keeps he_math.h's forms, which follow torch's rounding.
// a polynomial's second coefficient materialised where it is used (the FMAs take the others as
// literals): left to the compiler, it is hoisted out of the TGS iterations into a register held
// through them, and that register pushes the loop's long-lived state into scratch
template <uint32_t BITS>
HE_DEV float here(void) {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "n"(BITS));
    return r;
}
HE_DEV void half_sincos(float x, float& sn, float& cs) {
    const float x2 = x * x;
    float ps = fmaf(x2, 2.75573192e-6f, here<0xb9500d01u>());  // -1.98412698e-4
    ps = fmaf(x2, ps, 8.33333333e-3f);
    ps = fmaf(x2, ps, -1.66666667e-1f);
    sn = fmaf(x * x2, ps, x);
    float pc = fmaf(x2, -2.75573192e-7f, here<0x37d00d01u>());  // 2.48015873e-5
    pc = fmaf(x2, pc, -1.38888889e-3f);
    pc = fmaf(x2, pc, 4.16666667e-2f);
    pc = fmaf(x2, pc, -0.5f);
    cs = fmaf(x2, pc, 1.0f);
    // the large-angle lanes, rare: tested once for the wave, so that the common case is one scalar branch
    // not taken and ocml's argument reduction sits behind the hot stream (the series' value on such a
    // lane is finite or inf and is replaced)
    if (__builtin_expect(__ballot(x > 1.0f) != 0ull, 0)) {
        if (x > 1.0f) sincosf(x, &sn, &cs);
    }
}
HE_DEV float atan01(float t) {  // t in [0, 1]
    const float t2 = t * t;
    float p = fmaf(t2, 0.0028662257f, here<0xbc846e02u>());  // -0.0161657367
    p = fmaf(t2, p, 0.0429096138f);
    p = fmaf(t2, p, -0.0752896400f);
    p = fmaf(t2, p, 0.1065626393f);
    p = fmaf(t2, p, -0.1420889944f);
    p = fmaf(t2, p, 0.1999355085f);
    p = fmaf(t2, p, -0.3333314528f);
    return fmaf(t * t2, p, t);
}
HE_DEV f4 pqexp(f3 v) {
    const float th = __builtin_amdgcn_sqrtf(dot3(v, v));
    float sh, ch;
    half_sincos(0.5f * th, sh, ch);
    const float s = sh * __builtin_amdgcn_rcpf(th);
    f4 r = f4{v.x * s, v.y * s, v.z * s, ch};
    if (__ballot(th < 1e-8f) != 0ull) {
        const f4 r0 = qnormalize(f4{0.5f * v.x, 0.5f * v.y, 0.5f * v.z, 1.f});
        if (th < 1e-8f) r = r0;
    }
    return r;
}
HE_DEV f3 pqlog(f4 q) {
    if (q.w < 0.f) q = qneg(q);
    const float s = __builtin_amdgcn_sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
    // atan2(s, w) on the first quadrant (s > 0, w >= 0): the smaller over the larger, then pi / 2 - a
    const float lo = fminf(s, q.w), hi = fmaxf(s, q.w);
    const float a = atan01(lo * __builtin_amdgcn_rcpf(hi));
    const float ang = s > q.w ? 1.57079632679f - a : a;
    const float k = s < 1e-8f ? 2.f : 2.f * ang * __builtin_amdgcn_rcpf(s);  // the small-angle lanes: 2 q
    return f3{q.x * k, q.y * k, q.z * k};
}

}  // namespace
