// he_host.h -- the host layer shared by the four C-ABI libraries (engine, renderer, dynamics, solves):
// the error text, the HIP call check, device selection, the buffer alignment check, the structural
// he_model check and the owning device array. Host code only, and nothing but the HIP runtime API and the standard library, so a
// plain C++ compiler builds it (tests/host/ does, against a counting allocator, under a sanitizer).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

// Everything here has internal linkage: each library keeps an error text of its own, also when all
// four are loaded into one process. A library made of several translation units includes this
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

}  // namespace
