// he_phys_lanes.h -- cross-lane primitives of the one-wave workgroup: wave-wide OR and prefix counts
// (wave_or, wave_prefix, ballot_below, wave_prefix3), the lane exchanges (swizzle_xor, swap32, swap16,
// dpp, xpose4) with the MFMA tile vector types, the reduce-scatter butterfly (rs_dpp, reduce_scatter)
// and the lane predicates as constant exec masks (lanes_body, lanes_hi, lanes_joint_dof).
// LDS: none (ds_swizzle / ds_bpermute use the crossbar only). On entry: all 64 lanes active.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "he_math.h"
#include "he_phys_lds.h"
#include "he_regla.h"

namespace {

// OR over the wave as a wave-uniform value: quad and row DPP mirrors, then the 16- and 32-lane
// permlane swaps (no LDS crossbar round trips)
HE_DEV uint32_t wave_or(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xF, 0xF, false);  // row_half_mirror
    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xF, 0xF, false);  // row_mirror
    const auto r16 = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = r16[0] | r16[1];
    const auto r32 = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    x = r32[0] | r32[1];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// wave-wide exclusive prefix count of `flag` (uint64 ballot)
HE_DEV int wave_prefix(bool flag, int lane, int& total) {
    uint64_t m = __ballot(flag);
    total = __popcll(m);
    uint64_t below = lane == 0 ? 0ull : (m & ((~0ull) >> (64 - lane)));
    return __popcll(below);
}

// lanes below this one set in a ballot (v_mbcnt)
HE_DEV int ballot_below(uint64_t bm) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
}
// wave-wide exclusive prefix of a small count v (0..7): three bit ballots, v_mbcnt per bit
HE_DEV int wave_prefix3(int v, int& total) {
    int pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t bm = __ballot((v >> k) & 1);
        pre += ballot_below(bm) << k;
        total += __popcll(bm) << k;
    }
    return pre;
}

// the value of lane ^ S (S < 32): ds_swizzle in bitmask mode (and 0x1F, xor S)
template <int S>
HE_DEV float swizzle_xor(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (S << 10)));
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
HE_DEV void swap32(float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}
HE_DEV void swap16(float& a, float& b) {  // odd 16-lane rows of a <-> even rows of b
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}
template <int CTRL>
HE_DEV float dpp(float x) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, false)); }

// One butterfly stage of a wave reduce-scatter below 16 lanes: the partner (DPP pattern CTRL, an
// involution flipping lane bit B) gets the half this lane drops; lanes with bit B keep the upper
// half. H = values kept.
template <int H, int CTRL, uint64_t BITMASK>
HE_DEV void rs_dpp(float* v) {
    const bool up = regla::lanes<BITMASK>();
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float send = up ? v[j] : v[j + H];
        const float keep = up ? v[j + H] : v[j];
        v[j] = keep + dpp<CTRL>(send);
    }
}

// Reduce-scatter of N = 64 or 16 per-lane values: returns sum over all lanes of v[idx(lane)], with
// idx = lane (N = 64) or lane >> 2 (N = 16). Pairings by lane-bit flips 32, 16 (permlane swaps),
// 15 (row mirror), 7 (half-row mirror), 2, 1 (quad perms): independent, so every lane's result
// covers all 64 lanes once; 63 exchanges + 63 adds for 64 values (vs 6 x 64 for all-reduce).
template <int N>
HE_DEV float reduce_scatter(float (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N / 2; ++j) { swap32(v[j], v[j + N / 2]); v[j] += v[j + N / 2]; }
#pragma unroll
    for (int j = 0; j < N / 4; ++j) { swap16(v[j], v[j + N / 4]); v[j] += v[j + N / 4]; }
    rs_dpp<N / 8, 0x140, 0xFF00FF00FF00FF00ull>(v);  // row_mirror: lane ^ 15
    rs_dpp<N / 16, 0x141, 0xF0F0F0F0F0F0F0F0ull>(v);  // row_half_mirror: lane ^ 7
    if constexpr (N == 64) {
        rs_dpp<2, 0x4E, 0xCCCCCCCCCCCCCCCCull>(v);  // quad_perm [2,3,0,1]: lane ^ 2
        rs_dpp<1, 0xB1, 0xAAAAAAAAAAAAAAAAull>(v);  // quad_perm [1,0,3,2]: lane ^ 1
    } else {
        v[0] += dpp<0x4E>(v[0]);  // the 4 lanes of a quad hold the same index: all-reduce them
        v[0] += dpp<0xB1>(v[0]);
    }
    return v[0];
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
HE_DEV void xpose4(float (&r)[4]) {  // r[i] <- (group g: r[g] of group i)
    swap32(r[0], r[2]);
    swap32(r[1], r[3]);
    swap16(r[0], r[1]);
    swap16(r[2], r[3]);
}

// lane predicates of the TGS iterations' helpers as constant exec masks, rematerialised at each use
// (regla::lanes: two s_mov): a v_cmp result would be hoisted out of the iterations into an SGPR pair
// held through them, and the kernel runs out of SGPRs
HE_DEV bool lanes_body() { return regla::lanes<(1ull << NB) - 1ull>(); }        // lane < NB
HE_DEV bool lanes_hi() { return regla::lanes<(1ull << regla::NH) - 1ull>(); }   // lane < NH (dofs 64..74)
HE_DEV bool lanes_joint_dof() { return regla::lanes<~0x3Full>(); }             // lane >= 6

}  // namespace
