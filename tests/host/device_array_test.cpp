// Ownership of humanoid_amd/csrc/he_host.h's device arrays and of the query libraries' handles, on the
// CPU: this file is the HIP runtime (a counting allocator over malloc that can be told to fail the k-th
// allocation or the k-th copy), so the program links no HIP and runs under the host compiler's sanitizers
// (tests/test_host_layer.py).
#include "he_host.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

namespace {
std::set<void*> live;          // allocations not yet freed
int allocs = 0, copies = 0;    // calls so far
int frees = 0, bad_frees = 0;  // hipFree calls; those of a pointer that is not live (a double free)
int fail_alloc = -1, fail_copy = -1;
size_t last_bytes = 0;
int devices = 0;

void reset(int fail_alloc_at = -1, int fail_copy_at = -1) {
    allocs = copies = frees = bad_frees = 0;
    fail_alloc = fail_alloc_at;
    fail_copy = fail_copy_at;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    last_bytes = bytes;
    if (allocs++ == fail_alloc) {
        *p = reinterpret_cast<void*>(0x10);  // garbage: an owner that kept it would free it
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    ++frees;
    if (!live.erase(p)) {
        ++bad_frees;
        return hipErrorInvalidValue;
    }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemset(void* p, int byte, size_t bytes) {
    std::memset(p, byte, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (copies++ == fail_copy) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "refused by the test"; }
hipError_t hipGetDeviceCount(int* n) {
    *n = devices;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
}

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {

// a sequence of six arrays, as he_create_envs' table pass makes them
int six_arrays(size_t n) {
    DeviceArray<float> a[6];
    for (auto& x : a) {
        HE_CHECK(x.alloc(n));
        HE_CHECK(x.fill(0xFF, n));
    }
    return 0;
}

int test_failed_allocation_leaves_nothing() {
    for (int k = -1; k < 6; ++k) {
        reset(k);
        const int rc = six_arrays(100);
        EXPECT(rc == (k < 0 ? 0 : 1));
        EXPECT(allocs == (k < 0 ? 6 : k + 1));
        EXPECT(live.empty() && bad_frees == 0);
        EXPECT(frees == (k < 0 ? 6 : k));
        if (k >= 0) EXPECT(std::strstr(last_error(), "alloc") && std::strstr(last_error(), "device_array_test.cpp"));
    }
    return 0;
}

int test_move_assignment_frees_the_replaced_array_once() {
    reset();
    {
        DeviceArray<int32_t> a, b;
        EXPECT(a.alloc(8) == hipSuccess && b.alloc(8) == hipSuccess);
        int32_t *pa = a, *pb = b;
        a = std::move(b);
        EXPECT(frees == 1 && !live.count(pa) && live.count(pb));
        EXPECT(a.get() == pb && b.get() == nullptr);
        DeviceArray<int32_t>& self = a;
        a = std::move(self);
        EXPECT(frees == 1 && a.get() == pb);
        DeviceArray<int32_t> c(std::move(a));
        EXPECT(frees == 1 && a.get() == nullptr && c.get() == pb);
        EXPECT(c.alloc(4) == hipSuccess);  // a fresh allocation frees what was held
        EXPECT(frees == 2 && !live.count(pb) && live.size() == 1);
    }
    EXPECT(live.empty() && bad_frees == 0 && frees == 3);
    return 0;
}

// the staged replace of he_load_motions / he_ingest_clips: new tables in a local, moved into the handle
// after the last step
struct Tables {
    DeviceArray<float> hot, cold, lengths, dt;
    DeviceArray<int64_t> starts, nframes;
    int count = 0;
    bool holds(const std::set<void*>& s) const {
        return s == std::set<void*>{hot.get(), cold.get(), lengths.get(), dt.get(), starts.get(), nframes.get()};
    }
};
struct Handle {
    Tables motions;
};

int reload(Handle& h, int m) {
    const float f[4] = {1.f, 2.f, 3.f, 4.f};
    const int64_t i[4] = {1, 2, 3, 4};
    Tables t;
    HE_CHECK(t.hot.alloc(4));
    HE_CHECK(t.cold.alloc(4));
    HE_CHECK(t.lengths.assign(f, 4));
    HE_CHECK(t.dt.assign(f, 4));
    HE_CHECK(t.starts.assign(i, 4));
    HE_CHECK(t.nframes.assign(i, 4));
    HE_CHECK(t.hot.upload(f, 4));
    HE_CHECK(t.cold.upload(f, 4));
    t.count = m;
    h.motions = std::move(t);
    return 0;
}

int test_staged_replace() {
    reset();
    {
        Handle h;
        EXPECT(reload(h, 3) == 0 && h.motions.count == 3 && live.size() == 6);
        const std::set<void*> old = live;
        for (int step = 0; step < 12; ++step) {  // each of the six allocations, then each of the six copies
            const int copy = step - 6;
            reset(step < 6 ? step : -1, step < 6 ? -1 : copy);
            EXPECT(reload(h, 5) == 1);
            EXPECT(live == old && h.motions.holds(old) && h.motions.count == 3);  // the old set alive, the new freed
            // freed: the new arrays made before the failing step (the i-th assign's copy follows allocation 2 + i)
            EXPECT(bad_frees == 0 && frees == (step < 6 ? step : copy < 4 ? 3 + copy : 6));
        }
        reset();
        EXPECT(reload(h, 5) == 0 && h.motions.count == 5);
        EXPECT(frees == 6 && bad_frees == 0 && live.size() == 6);  // the old set freed, each array once
        for (void* p : old) EXPECT(!live.count(p));
        EXPECT(h.motions.holds(live));
    }
    EXPECT(live.empty() && bad_frees == 0);
    return 0;
}

int test_zero_length_array() {
    reset();
    DeviceArray<float> a;
    EXPECT(a.alloc(0) == hipSuccess && last_bytes == 16 && live.size() == 1 && a.get() != nullptr);
    a.release();
    EXPECT(live.empty() && frees == 1 && a.get() == nullptr);
    a.release();  // nothing held: no call
    EXPECT(frees == 1 && bad_frees == 0);
    return 0;
}

int test_select_device() {
    devices = 0;
    EXPECT(select_device(0, "x_create") == 1 && std::strstr(last_error(), "x_create: no HIP device"));
    devices = 2;
    EXPECT(select_device(2, "x_create") == 1 && std::strstr(last_error(), "device 2 of 2"));
    EXPECT(select_device(1, "x_create") == 0);
    return 0;
}

// check_model reads the counts off the struct it is given
struct SmallModel {
    int32_t num_bodies, num_dof, num_pairs;
    int32_t parents[3], geom_type[3];
    float armature[6];
    int32_t pairs[4][2];
};

int test_check_model() {
    const SmallModel ok{3, 6, 4, {-1, 0, 1}, {0, 1, 2}, {}, {}};
    EXPECT(check_model(&ok, "m", 1) == 0);
    EXPECT(check_model(static_cast<const SmallModel*>(nullptr), "m", 1) == 1 && std::strstr(last_error(), "m: null model"));
    SmallModel m = ok;
    m.num_bodies = 2;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "3 bodies / 6 dofs"));
    m = ok, m.num_pairs = 5;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "pair"));
    m = ok, m.parents[0] = 0;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "root"));
    m = ok, m.parents[1] = 2;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "DFS"));
    m = ok, m.geom_type[1] = 7;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "geom type 7"));
    m = ok, m.geom_type[0] = 2;
    EXPECT(check_model(&m, "m", 1) == 1 && std::strstr(last_error(), "2 box geoms"));
    return 0;
}

// the query libraries' create and destroy, with a toy handle, model and checks in the libraries' places
struct ToyHost {
    int32_t n;
};
struct ToyModel {
    int32_t n;
    float gravity[3];
};
struct ToyHandle : QueryHandle<ToyModel> {
    int rows = 7;  // a library's own member
};
int toy_validate(const ToyHost* m) { return m && m->n > 0 ? 0 : fail("model: refused by the test"); }
void toy_fill(const ToyHost* m, const float gravity[3], ToyModel& dm) {
    dm = ToyModel{m->n, {gravity[0], gravity[1], gravity[2]}};
}
int toy_create(int device, const ToyHost* m, const float* gravity, int num_envs, ToyHandle** out) {
    return query_create("x_create", device, m, gravity, num_envs, out, toy_validate, toy_fill);
}

int test_query_create_and_destroy() {
    const ToyHost ok{5}, bad{0};
    const float g[3] = {0.f, 0.f, -9.81f};
    ToyHandle* const stale = reinterpret_cast<ToyHandle*>(0x10);  // a failure must not leave it in *out
    ToyHandle* h = stale;
    devices = 2;
    // each argument refusal, in create's order: *out null, nothing allocated
    reset();
    EXPECT(toy_create(0, &ok, g, 4, nullptr) == 1 && !std::strcmp(last_error(), "x_create: null output pointer"));
    EXPECT(toy_create(0, nullptr, nullptr, 0, &h) == 1 && !std::strcmp(last_error(), "x_create: num_envs 0 < 1") && !h);
    h = stale;
    EXPECT(toy_create(0, nullptr, nullptr, 4, &h) == 1 && !std::strcmp(last_error(), "x_create: null gravity vector") && !h);
    h = stale;
    EXPECT(toy_create(0, &bad, g, 4, &h) == 1 && !std::strcmp(last_error(), "model: refused by the test") && !h);
    h = stale;
    EXPECT(toy_create(2, &ok, g, 4, &h) == 1 && !std::strcmp(last_error(), "x_create: device 2 of 2") && !h);
    devices = 0;
    h = stale;
    EXPECT(toy_create(0, &ok, g, 4, &h) == 1 && std::strstr(last_error(), "x_create: no HIP device") && !h);
    EXPECT(allocs == 0 && frees == 0 && live.empty());
    devices = 2;
    // a failed allocation, then a failed copy: the handle and its array are gone
    reset(0);
    h = stale;
    EXPECT(toy_create(1, &ok, g, 4, &h) == 1 && std::strstr(last_error(), "d_model.assign") && !h);
    EXPECT(allocs == 1 && live.empty() && frees == 0 && bad_frees == 0);
    reset(-1, 0);
    h = stale;
    EXPECT(toy_create(1, &ok, g, 4, &h) == 1 && std::strstr(last_error(), "d_model.assign") && !h);
    EXPECT(allocs == 1 && copies == 1 && live.empty() && frees == 1 && bad_frees == 0);
    // success: the handle as asked, the filled model in its array; destroy frees that array, once
    reset();
    EXPECT(toy_create(1, &ok, g, 4, &h) == 0 && h && h != stale);
    EXPECT(h->device == 1 && h->num_envs == 4 && h->rows == 7 && live.size() == 1 && live.count(h->d_model.get()));
    const ToyModel* dm = h->d_model;
    EXPECT(last_bytes == sizeof(ToyModel) && dm->n == 5 && dm->gravity[2] == g[2]);
    EXPECT(query_destroy(h) == 0 && live.empty() && frees == 1 && bad_frees == 0);
    EXPECT(query_destroy(static_cast<ToyHandle*>(nullptr)) == 0 && frees == 1);
    return 0;
}

// the refusals every query call makes, piece by piece
int test_query_call_checks() {
    int x[2] = {0, 0};
    const void* odd = reinterpret_cast<const char*>(x) + 2;
    EXPECT(check_call("x_call", nullptr, x, x) == 1 && !std::strcmp(last_error(), "x_call: null handle"));
    EXPECT(check_call("x_call", x, nullptr, x) == 1 && !std::strcmp(last_error(), "x_call: null state pointer"));
    EXPECT(check_call("x_call", x, x, nullptr) == 1 && !std::strcmp(last_error(), "x_call: null state pointer"));
    EXPECT(check_call("x_call", x, x, x) == 0);
    EXPECT(check_flags("x_call", 3u, 3u) == 0);
    EXPECT(check_flags("x_call", 13u, 3u) == 1 && !std::strcmp(last_error(), "x_call: unknown flag bits 0xc"));
    EXPECT(check_aligned("x_call", {x, nullptr, x + 1}) == 0);
    EXPECT(check_aligned("x_call", {x, odd}) == 1 && !std::strcmp(last_error(), "x_call: every buffer must be 4-byte aligned"));
    return 0;
}

}  // namespace

int main() {
    if (test_failed_allocation_leaves_nothing() || test_move_assignment_frees_the_replaced_array_once() ||
        test_staged_replace() || test_zero_length_array() || test_select_device() || test_check_model() ||
        test_query_create_and_destroy() || test_query_call_checks())
        return 1;
    std::puts("he_host ownership: ok");
    return 0;
}
