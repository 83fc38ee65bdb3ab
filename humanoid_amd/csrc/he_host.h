// he_host.h -- the host layer shared by the C-ABI libraries (engine, renderer and the query libraries:
// dynamics, solves, task): the error text, the HIP call check, device selection, the buffer alignment
// check, the structural he_model check and the owning device array; then what the query libraries share
// beyond that, their handle, its creation and destruction and the refusals every call of theirs makes.
// Host code only, and nothing but the HIP runtime API and the standard library, so a plain C++ compiler
// builds it (tests/host/ does, against a counting allocator, under a sanitizer).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <memory>
#include <string>

// Everything here has internal linkage: each library keeps an error text of its own, also when all
// of them are loaded into one process. A library made of several translation units includes this
// header in one of them and hands the others a function (the engine: he_fail_text).
namespace {

thread_local std::string g_err;

__attribute__((format(printf, 1, 2))) int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

const char* last_error() { return g_err.c_str(); }

#define HE_CHECK(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// make `device` the calling thread's device, or say why not
int select_device(int device, const char* who) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return fail("%s: no HIP device visible (there is no CPU path)", who);
    if (device < 0 || device >= count) return fail("%s: device %d of %d", who, device, count);
    HE_CHECK(hipSetDevice(device));
    return 0;
}

// the alignment every kernel assumes of a caller's buffers (plain dword accesses); null passes
bool misaligned(std::initializer_list<const void*> ps) {
    uintptr_t al = 0;
    for (const void* p : ps) al |= reinterpret_cast<uintptr_t>(p);
    return (al & 3u) != 0;
}

// The structure every kernel of the libraries is built for: the body and dof counts, the pair
// table's bound, body 0 as the root, parents before children, the three geom types and at most
// max_boxes boxes (the physics kernel's corner lanes). A template over include/humanoid_engine.h's
// he_model, whose array lengths are the counts, so that this header needs no other.
template <class Model>
int check_model(const Model* m, const char* who, int max_boxes) {
    constexpr int nb = sizeof(Model::parents) / sizeof(Model::parents[0]);
    constexpr int nd = sizeof(Model::armature) / sizeof(Model::armature[0]);
    constexpr int max_pairs = sizeof(Model::pairs) / sizeof(Model::pairs[0]);
    if (!m) return fail("%s: null model", who);
    if (m->num_bodies != nb || m->num_dof != nd)
        return fail("%s: the kernels are built for %d bodies / %d dofs (got %d / %d)", who, nb, nd, m->num_bodies,
                    m->num_dof);
    if (m->num_pairs < 0 || m->num_pairs > max_pairs) return fail("%s: bad pair count %d", who, m->num_pairs);
    if (m->parents[0] != -1) return fail("%s: body 0 must be the root", who);
    for (int b = 1; b < nb; ++b)
        if (m->parents[b] < 0 || m->parents[b] >= b) return fail("%s: bodies must be in DFS order", who);
    int boxes = 0;
    for (int b = 0; b < nb; ++b) {
        const int t = m->geom_type[b];
        if (t < 0 || t > 2) return fail("%s: body %d has geom type %d (sphere 0, capsule 1, box 2)", who, b, t);
        boxes += t == 2;
    }
    if (boxes > max_boxes)
        return fail("%s: %d box geoms (the physics kernel's corner lanes hold at most %d)", who, boxes, max_boxes);
    return 0;
}

// Device memory with one owner: freed when the owner goes, moved but never copied. A handle's arrays
// are members, so deleting the handle frees them; a function builds new arrays in locals and moves
// them into the handle after its last step, so a failed step leaves nothing behind and the handle as
// it was. DeviceBytes is the untyped form (sizes in bytes).
class DeviceBytes {
public:
    DeviceBytes() = default;
    DeviceBytes(const DeviceBytes&) = delete;
    DeviceBytes& operator=(const DeviceBytes&) = delete;
    DeviceBytes(DeviceBytes&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBytes& operator=(DeviceBytes&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DeviceBytes() { release(); }

    // a fresh allocation (what was held is freed first); zero bytes still allocate 16
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc(&p_, bytes > 0 ? bytes : 16);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    hipError_t fill(int byte, size_t bytes) { return hipMemset(p_, byte, bytes); }
    hipError_t upload(const void* host, size_t bytes) { return hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice); }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    void* get() const { return p_; }

private:
    void* p_ = nullptr;
};

// the typed form: sizes in elements, and it converts to the T* the launch arguments take
template <typename T>
class DeviceArray : public DeviceBytes {
public:
    hipError_t alloc(size_t n) { return DeviceBytes::alloc(n * sizeof(T)); }
    hipError_t fill(int byte, size_t n) { return DeviceBytes::fill(byte, n * sizeof(T)); }
    hipError_t upload(const T* host, size_t n) { return DeviceBytes::upload(host, n * sizeof(T)); }
    hipError_t assign(const T* host, size_t n) {  // a fresh allocation holding host[0..n)
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : upload(host, n);
    }
    T* get() const { return static_cast<T*>(DeviceBytes::get()); }
    operator T*() const { return get(); }
};

// ---- the query libraries (hd_dynamics.hip, hs_solve.hip, ht_task.hip): each answers questions about
// the engine's current state with one kernel that reads a device copy of the model. What follows knows
// neither the model nor the kernels: the library hands in its model check and the fill of its device model.

// what a query handle holds; a library's handle derives from it and adds what is its own
template <class DeviceModel>
struct QueryHandle {
    using Model = DeviceModel;
    int device = 0;
    int num_envs = 0;
    DeviceArray<DeviceModel> d_model;
};

// h?_create. validate(model): the library's h?_validate_model; fill(model, gravity, dm): a validated
// model as the kernel reads it. *out is null on every failure.
template <class Handle, class HostModel, class Validate, class Fill>
int query_create(const char* who, int device, const HostModel* model, const float gravity[3], int num_envs, Handle** out,
                 Validate validate, Fill fill) {
    if (!out) return fail("%s: null output pointer", who);
    *out = nullptr;
    if (num_envs < 1) return fail("%s: num_envs %d < 1", who, num_envs);
    if (!gravity) return fail("%s: null gravity vector", who);
    if (validate(model)) return 1;
    typename Handle::Model dm;
    fill(model, gravity, dm);
    if (select_device(device, who)) return 1;
    std::unique_ptr<Handle> h(new Handle);  // a failed step below frees it and its array
    h->device = device;
    h->num_envs = num_envs;
    HE_CHECK(h->d_model.assign(&dm, 1));
    *out = h.release();
    return 0;
}

// h?_destroy
template <class Handle>
int query_destroy(Handle* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;
    return 0;
}

// The refusals every query call makes, in the order the public headers list them: handle and state
// pointers first, flags and alignment last. Three pieces, because an entry point's own refusals (a null
// right-hand side, no output buffer, the mode) sit between them and keep their place.
int check_call(const char* who, const void* handle, const void* root_state, const void* dof_state) {
    if (!handle) return fail("%s: null handle", who);
    if (!root_state || !dof_state) return fail("%s: null state pointer", who);
    return 0;
}
int check_flags(const char* who, uint32_t flags, uint32_t all) {
    if (flags & ~all) return fail("%s: unknown flag bits 0x%x", who, flags & ~all);
    return 0;
}
int check_aligned(const char* who, std::initializer_list<const void*> buffers) {
    if (misaligned(buffers)) return fail("%s: every buffer must be 4-byte aligned", who);
    return 0;
}

}  // namespace
