// he_tree_state.h -- from an env's root and dof state to its bodies' kinematics: the routine the two
// query libraries (hd_dynamics.hip, hs_solve.hip) share, with its helpers, the model it reads and that
// model's host-side fill and check. Nothing of the engine includes it.
// One 64-lane wave per env, lanes 0..23 one body each; origins are relative to the root origin
// o = p_0, so levers stay below a body length wherever the env stands in the world. What a kernel
// refers the inertias and wrenches to (o, or each joint's own origin) is its own and stays in its file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/humanoid_engine.h"
#include "he_host.h"

// internal linkage, as he_host.h: each library carries its own copy
namespace {

constexpr int NB = HE_NUM_BODIES;
constexpr int ND = HE_NUM_DOF;
constexpr int NG = HE_NUM_GEN;
constexpr int kWave = 64;
constexpr int kMaxDepth = 8;  // joints on the longest chain (he_topo.h body_chain)

struct v3 {
    float x, y, z;
};
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ v3 cross(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// S . F = w . n + v . p in one fixed order of fused multiply-adds
__device__ __forceinline__ float dot6(v3 w, v3 v, v3 n, v3 p) {
    return fmaf(v.z, p.z, fmaf(v.y, p.y, fmaf(v.x, p.x, fmaf(w.z, n.z, fmaf(w.y, n.y, w.x * n.x)))));
}
__device__ __forceinline__ v3 ld3(const float* p) { return v3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, v3 a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

// a 3x3 matrix in named registers (row-major): no indexed register arrays, so nothing goes to scratch
struct m3 {
    float a00, a01, a02, a10, a11, a12, a20, a21, a22;
};
__device__ __forceinline__ v3 mul(const m3& m, v3 v) {
    return v3{m.a00 * v.x + m.a01 * v.y + m.a02 * v.z, m.a10 * v.x + m.a11 * v.y + m.a12 * v.z,
              m.a20 * v.x + m.a21 * v.y + m.a22 * v.z};
}
__device__ __forceinline__ m3 mul(const m3& a, const m3& b) {
    return m3{a.a00 * b.a00 + a.a01 * b.a10 + a.a02 * b.a20, a.a00 * b.a01 + a.a01 * b.a11 + a.a02 * b.a21,
              a.a00 * b.a02 + a.a01 * b.a12 + a.a02 * b.a22, a.a10 * b.a00 + a.a11 * b.a10 + a.a12 * b.a20,
              a.a10 * b.a01 + a.a11 * b.a11 + a.a12 * b.a21, a.a10 * b.a02 + a.a11 * b.a12 + a.a12 * b.a22,
              a.a20 * b.a00 + a.a21 * b.a10 + a.a22 * b.a20, a.a20 * b.a01 + a.a21 * b.a11 + a.a22 * b.a21,
              a.a20 * b.a02 + a.a21 * b.a12 + a.a22 * b.a22};
}
__device__ __forceinline__ m3 ldm(const float* p) { return m3{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }
__device__ __forceinline__ void stm(float* p, const m3& m) {
    p[0] = m.a00, p[1] = m.a01, p[2] = m.a02, p[3] = m.a10, p[4] = m.a11, p[5] = m.a12, p[6] = m.a20, p[7] = m.a21,
    p[8] = m.a22;
}

// exp([v]x) = 1 + A K + B K^2, A = sin(th) / th, B = (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2 (no
// cancellation); below 1e-3 rad the series (the next terms are under 1e-14)
__device__ __forceinline__ m3 rodrigues(v3 v) {
    const float t2 = dot(v, v);
    float A, B;
    if (t2 < 1e-6f) {
        A = 1.f - t2 * (1.f / 6.f);
        B = 0.5f - t2 * (1.f / 24.f);
    } else {
        const float th = sqrtf(t2);
        const float sh = sinf(0.5f * th);
        A = sinf(th) / th;
        B = 2.f * sh * sh / t2;
    }
    const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z;
    const float xy = B * v.x * v.y, xz = B * v.x * v.z, yz = B * v.y * v.z;
    return m3{1.f - B * (yy + zz), xy - A * v.z, xz + A * v.y, xy + A * v.z, 1.f - B * (xx + zz), yz - A * v.x,
              xz - A * v.y, yz + A * v.x, 1.f - B * (xx + yy)};
}

__device__ __forceinline__ m3 quat_matrix(float x, float y, float z, float w) {
    const float n2 = x * x + y * y + z * z + w * w;
    if (n2 < 1e-24f) return m3{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    const float s = 2.f / n2;
    return m3{1.f - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w), s * (x * y + z * w),
              1.f - s * (x * x + z * z), s * (y * z - x * w), s * (x * z - y * w), s * (y * z + x * w),
              1.f - s * (x * x + y * y)};
}

__device__ __forceinline__ int col_joint(int c) { return c < 6 ? 0 : 1 + (c - 6) / 3; }

// what the kernels read of the model (fill_tree_model)
struct TreeModel {
    int32_t parent[NB];
    int32_t depth[NB];
    uint32_t anc[NB];  // bit a: a is ancestor-or-self of b
    uint32_t sub[NB];  // bit d: d in subtree(b)
    float local_pos[NB][3];
    float mass[NB];
    float com[NB][3];
    float inertia[NB][6];  // xx yy zz xy xz yz
    float armature[ND];
    float gravity[3];
    int32_t max_depth;
};

// a model that passed check_tree_depth, as the kernels read it
void fill_tree_model(const he_model* model, const float gravity[3], TreeModel& tm) {
    tm = TreeModel{};
    for (int b = 0; b < NB; ++b) {
        const int a = model->parents[b];
        tm.parent[b] = a;
        tm.depth[b] = b == 0 ? 0 : tm.depth[a] + 1;
        tm.anc[b] = (b == 0 ? 0u : tm.anc[a]) | 1u << b;
        if (tm.depth[b] > tm.max_depth) tm.max_depth = tm.depth[b];
        tm.mass[b] = model->mass[b];
        for (int c = 0; c < 3; ++c) tm.local_pos[b][c] = model->local_pos[b][c], tm.com[b][c] = model->com[b][c];
        for (int c = 0; c < 6; ++c) tm.inertia[b][c] = model->inertia[b][c];
    }
    for (int b = 0; b < NB; ++b)
        for (int d = 0; d < NB; ++d)
            if (tm.anc[d] >> b & 1u) tm.sub[b] |= 1u << d;
    for (int d = 0; d < ND; ++d) tm.armature[d] = model->armature[d];
    for (int c = 0; c < 3; ++c) tm.gravity[c] = gravity[c];
}

// tree_kinematics' own bound on a model that passed check_model: one pass per tree level
int check_tree_depth(const he_model* model) {
    int depth[NB] = {0};
    for (int b = 1; b < NB; ++b) {
        depth[b] = depth[model->parents[b]] + 1;
        if (depth[b] > kMaxDepth) return fail("model: body %d is %d joints from the root, at most %d", b, depth[b], kMaxDepth);
    }
    return 0;
}

// One env's kinematic state: a view of the kernel's own LDS arrays. A view and not the storage, and the
// model by pointer below and not by reference, because hd_dynamics.hip is built with SLP vectorisation,
// whose pairing decides which products of a contracted sum round. The pairing follows the shape of the
// LDS objects (one struct pairs differently from seven arrays), and a reference parameter, dereferenceable
// as a whole, lets a branch on a model field become selects, which re-pairs its block. In this form
// dynamics_kernel's bits are those it had with the routine inline (tools/lib_identity.py --queries).
struct TreeState {
    float *q, *u, *qdd;  // [69] dof positions, velocities; the joints' accelerations (tree_kinematics<true>) or null
    float (*R)[9];       // [24] world rotation, row-major
    float (*P)[3];       // origin relative to the root origin o
    float (*W)[3];       // world angular velocity
    float (*Wd)[3];      // world angular acceleration (root's: 0)
    float (*A)[3];       // origin acceleration (root's: 0)
};

// State load, the joints' Rodrigues matrices, then one pass per tree level into S; ends on a barrier.
// QDD: the joints' accelerations qdd_des [N,69] enter the bodies' angular accelerations (the root's
// accelerations stay 0: its columns are the caller's); otherwise everything is at qdd = 0.
template <bool QDD>
__device__ __forceinline__ void tree_kinematics(const TreeState& S, const TreeModel* M, const float* root_state,
                                                const float* dof_state, const float* qdd_des, size_t env, int lane) {
    for (int d = lane; d < ND; d += kWave) {
        const float* row = dof_state + (env * ND + d) * 2;
        S.q[d] = row[0];
        S.u[d] = row[1];
        if (QDD) S.qdd[d] = qdd_des[env * ND + d];
    }
    const float* root = root_state + env * 13;
    m3 Rl{};  // body b >= 1: the joint's rotation; filled after the barrier below
    int depth = -1, parent = 0;
    if (lane < NB) {
        depth = M->depth[lane];
        parent = M->parent[lane];
        if (lane == 0) {
            stm(S.R[0], quat_matrix(root[3], root[4], root[5], root[6]));
            st3(S.P[0], v3{0.f, 0.f, 0.f});
            st3(S.W[0], ld3(root + 10));
            st3(S.Wd[0], v3{0.f, 0.f, 0.f});
            st3(S.A[0], v3{0.f, 0.f, 0.f});
        }
    }
    __syncthreads();
    if (lane >= 1 && lane < NB) Rl = rodrigues(ld3(&S.q[3 * (lane - 1)]));

    // one pass per tree level (max_depth is the model's: the same in every lane)
    const int levels = M->max_depth;
    for (int lvl = 1; lvl <= levels; ++lvl) {
        if (depth == lvl) {
            const int b = lane, a = parent;
            const m3 Ra = ldm(S.R[a]);
            const v3 wa = ld3(S.W[a]), wda = ld3(S.Wd[a]);
            const m3 Rb = mul(Ra, Rl);
            const v3 d = mul(Ra, ld3(M->local_pos[b]));
            const v3 wrel = mul(Rb, ld3(&S.u[3 * (b - 1)]));
            v3 wd = wda + cross(wa, wrel);
            if (QDD) wd = wd + mul(Rb, ld3(&S.qdd[3 * (b - 1)]));
            stm(S.R[b], Rb);
            st3(S.P[b], ld3(S.P[a]) + d);
            st3(S.W[b], wa + wrel);
            st3(S.Wd[b], wd);
            st3(S.A[b], ld3(S.A[a]) + cross(wda, d) + cross(wa, cross(wa, d)));
        }
        __syncthreads();
    }
}

// body b in the world: mass, the centre of mass relative to the body origin (rc) and to o (c), and
// I_w = R I R^T about the centre of mass (dynamics_kernel's; hs_solve.hip's columns() keeps these lines
// and the Newton-Euler ones inline, where a call measured 1 % slower)
struct BodyWorld {
    float m;
    v3 rc, c;
    float wxx, wyy, wzz, wxy, wxz, wyz;
};
__device__ __forceinline__ BodyWorld body_world(const TreeState& S, const TreeModel* M, int b) {
    const m3 R = ldm(S.R[b]);
    const float m = M->mass[b];
    const v3 rc = mul(R, ld3(M->com[b]));
    const v3 c = ld3(S.P[b]) + rc;
    const float* ib = M->inertia[b];
    const m3 I{ib[0], ib[3], ib[4], ib[3], ib[1], ib[5], ib[4], ib[5], ib[2]};
    const m3 RI = mul(R, I);
    const float wxx = RI.a00 * R.a00 + RI.a01 * R.a01 + RI.a02 * R.a02;
    const float wyy = RI.a10 * R.a10 + RI.a11 * R.a11 + RI.a12 * R.a12;
    const float wzz = RI.a20 * R.a20 + RI.a21 * R.a21 + RI.a22 * R.a22;
    const float wxy = RI.a00 * R.a10 + RI.a01 * R.a11 + RI.a02 * R.a12;
    const float wxz = RI.a00 * R.a20 + RI.a01 * R.a21 + RI.a02 * R.a22;
    const float wyz = RI.a10 * R.a20 + RI.a11 * R.a21 + RI.a12 * R.a22;
    return BodyWorld{m, rc, c, wxx, wyy, wzz, wxy, wxz, wyz};
}

}  // namespace
