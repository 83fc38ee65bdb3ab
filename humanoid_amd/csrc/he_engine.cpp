// he_engine.cpp -- C-ABI implementation of libhumanoid_engine.so (include/humanoid_engine.h).
// Owns the device state (he_host.h DeviceArray members), the device model/topology blobs and the
// device motion library, and launches the gfx950 kernels on the caller's stream. No host
// synchronisation on any compute entry point; allocation happens only in the he_set_* / he_create_envs
// / he_load_motions / he_ingest_clips calls, which change the engine only after their last step.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cmath>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/humanoid_engine.h"
#include "he_host.h"
#include "he_kernels.h"
#include "he_topo.h"

// error text for the other C-ABI translation units (he_rollout.hip)
int he_fail_text(const char* text) {
    g_err = text;
    return 1;
}

// the device motion library (he_load_motions / he_ingest_clips build one and move it into the engine)
struct MotionTables {
    DeviceArray<float> hot, cold, lengths, dt;
    DeviceArray<int64_t> starts, nframes;
    int count = 0;  // motions; 0: nothing loaded
};

// the tables of M motions over F frames: the frame records allocated, the per-motion arrays filled
static int stage_motion_tables(MotionTables& t, int64_t F, int M, const float* lengths, const float* dt,
                               const int64_t* starts, const int64_t* nframes) {
    HE_CHECK(t.hot.alloc((size_t)F * HE_NUM_BODIES * HE_MOTION_HOT));
    HE_CHECK(t.cold.alloc((size_t)F * HE_NUM_BODIES * HE_MOTION_COLD));
    HE_CHECK(t.lengths.assign(lengths, M));
    HE_CHECK(t.dt.assign(dt, M));
    HE_CHECK(t.starts.assign(starts, M));
    HE_CHECK(t.nframes.assign(nframes, M));
    t.count = M;
    return 0;
}

// One included buffer as the env-state kernel reads it (env_state_kernel below): where env 0's row
// starts, the words of a row, and where the row lies in an env's packed state.
struct StateField {
    uint32_t* base;
    int32_t words, offset;
};

struct he_engine {
    int device = 0;
    he_sim_params params{};
    he_model model{};
    bool has_model = false;
    DeviceArray<he_model> d_model;
    DeviceArray<PhysTopo> d_topo;
    DeviceArray<float> d_rest;      // [24,3] zero-pose body origins in the root frame
    int num_envs = 0;
    // the per-env buffers; env_buffers() below states their shapes, types and initial contents
    DeviceArray<float> root, dof_state, rb, cf, dof_force, targets, cache;
    DeviceArray<int32_t> num_contacts, dropped;
    DeviceArray<float> init_root;
    DeviceArray<int32_t> meta_cache;  // the imitation kernel's per-env motion-metadata cache
    bool component_limits = false;  // a dof bound inside (-pi + guard, pi - guard): not implemented
    int fused_step = -1;            // he_env_step as one launch: 1 / 0 (he_set_fused_step), -1 auto
    // borrowed from the caller (he_set_env_properties), who keeps them alive
    const float *mass_scale = nullptr, *friction = nullptr;
    const int32_t* terrain_kind = nullptr;
    DeviceArray<float> pd_offset, pd_scale;
    DeviceArray<int32_t> frozen;
    int clip_actions = 1;
    bool has_pd = false;
    he_eval_buffers eval{};  // borrowed device pointers (he_set_eval)
    int has_eval = 0;
    he_amp_buffers amp{};    // borrowed device pointers (he_set_amp)
    int has_amp = 0;
    MotionTables motions;
    unsigned long long* stamps = nullptr;  // borrowed (he_set_debug_stamps)
    // the physics launch's dispatch order (he_kernels.h launch_physics_order), rebuilt from the envs'
    // cycle counts every order_every launches; HE_PHYS_ORDER=0 keeps workgroup id = env
    DeviceArray<int32_t> order;
    DeviceArray<uint32_t> cost;
    int order_every = 8;
    long long launches = 0;
    // HE_TGS_LEGS=0 in the environment: no leg class (physics_kernel_tgs's Zh products over every dof
    // for every env; the results are the same bits, tests/test_full_size.py checks it)
    int full_dofs = 0;
    // the order rebuild runs on the launch's stream, and order_ready is recorded behind it: a physics
    // launch on another stream waits for it, so no workgroup reads a half-written order (a rebuild
    // on a side stream, beside the imitation step, made both slower: r06 A/B)
    hipEvent_t order_ready = nullptr;
    long long order_seq = 0;          // rebuilds issued
    long long order_seen_seq = -1;    // the rebuild the last physics launch waited for, on ...
    hipStream_t order_seen_stream = nullptr;  // ... this stream
    // external wrenches (he_apply_body_forces): the world-axis (torque, force at the CoM) rows
    // and the gym.simulate() calls they still act in (0: nothing pending; the rows are then overwritten
    // by the next call, not accumulated into)
    DeviceArray<float> wrench;
    int wrench_hold = 0;
    // torque control (he_set_dof_drive_modes, he_set_dof_actuation_forces): the dofs' drive modes (`model`
    // keeps the caller's gains; d_model has zero gains on the dofs that are not POS), and the engine's
    // own [N,69] clamped actuation, handed to the physics launches while act_set
    int32_t modes[HE_NUM_DOF] = {};
    DeviceArray<int32_t> d_modes;
    DeviceArray<float> dof_act;
    bool act_set = false;
    // the packed env state (he_save_envs / he_load_envs / he_clone_envs): one StateField per buffer whose
    // env_buffers() row says `state`, built by he_create_envs from that table
    DeviceArray<StateField> state_desc;
    int state_fields = 0, state_words = 0;

    ~he_engine() {
        if (order_ready) (void)hipEventDestroy(order_ready);
    }
};

namespace {
// A per-env buffer of the engine: what he_get_buffer calls it (-1: internal), its array, rows per env,
// columns (0: one-dimensional), element type, the byte every element starts as, and whether its row is
// part of an env's state (include/humanoid_engine.h "env state": the packed state is the rows that say
// so, in this order). The table drives he_create_envs, he_get_buffer and the state layout; a new buffer
// is a member of he_engine and a row here.
struct EnvBuffer {
    int kind;
    DeviceBytes* mem;
    int rows, cols, dtype, fill;
    bool state;
    int words() const { return rows * (cols ? cols : 1); }            // per env; both dtypes: 4 bytes
    size_t bytes(int N) const { return (size_t)N * words() * 4; }
};

constexpr int HE_META_WORDS = 8;  // the imitation kernel's per-env motion-metadata cache row

std::vector<EnvBuffer> env_buffers(he_engine* h) {
    const int F32 = HE_DTYPE_F32, I32 = HE_DTYPE_I32, NB = HE_NUM_BODIES, ND = HE_NUM_DOF;
    return {
        {HE_BUF_ROOT_STATE, &h->root, 1, 13, F32, 0, true},
        {HE_BUF_DOF_STATE, &h->dof_state, ND, 2, F32, 0, true},
        {HE_BUF_RB_STATE, &h->rb, NB, 13, F32, 0, true},
        {HE_BUF_CONTACT_FORCE, &h->cf, NB, 3, F32, 0, true},
        {HE_BUF_DOF_FORCE, &h->dof_force, ND, 0, F32, 0, true},
        {HE_BUF_DOF_TARGET, &h->targets, 1, ND, F32, 0, true},
        {HE_BUF_NUM_CONTACTS, &h->num_contacts, 1, 0, I32, 0, true},
        {HE_BUF_DROPPED_CONTACTS, &h->dropped, 1, 0, I32, 0, true},
        {HE_BUF_CONTACT_CACHE, &h->cache, 1, HE_CACHE_WORDS, F32, 0, true},
        {HE_BUF_INIT_ROOT_STATE, &h->init_root, 1, 13, F32, 0, true},
        // scheduling hints whose values reach no result; the order is a permutation of the envs, which
        // copying rows between envs would break
        {HE_BUF_PHYS_ORDER, &h->order, 1, 0, I32, 0, false},
        {HE_BUF_PHYS_COST, &h->cost, 1, 0, I32, 0, false},
        // derived from the motion tables: invalidated for every env a state is written to, not copied
        {-1, &h->meta_cache, 1, HE_META_WORDS, I32, 0xFF, false},  // motion -1: empty
        {-1, &h->wrench, NB, 6, F32, 0, true},
        {-1, &h->dof_act, 1, ND, F32, 0, true},
    };
}
}  // namespace

extern "C" {

const char* he_last_error(void) { return last_error(); }
int he_version(void) { return 1; }

int he_device_count(int* count) {
    HE_CHECK(hipGetDeviceCount(count));
    return 0;
}

int he_create(const he_sim_params* params, int device, he_engine** out) {
    if (!params || !out) return fail("he_create: null argument");
    if (select_device(device, "he_create")) return 1;
    hipDeviceProp_t prop;
    HE_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("he_create: device %d is %s; this build targets gfx950 (MI355X)", device, prop.gcnArchName);
    if (params->max_contacts < 1 || params->max_contacts > HE_MAX_CONTACTS)
        return fail("he_create: max_contacts must be in [1, %d]", HE_MAX_CONTACTS);
    if (params->dt <= 0.f) return fail("he_create: dt must be positive");
    if (params->substeps < 1 || params->substeps > 16) return fail("he_create: substeps must be in [1, 16]");
    if (!(params->max_joint_velocity > 0.f) || !(params->max_angular_velocity > 0.f))
        return fail("he_create: max_joint_velocity and max_angular_velocity must be positive");
    // sim_params.physx.solver_type (isaacgym_env.py:16): 0 PGS, 1 TGS with solver_iterations position
    // iterations (num_position_iterations, :17) per physics step
    if (params->solver_type != 0 && params->solver_type != 1)
        return fail("he_create: solver_type must be 0 (PGS) or 1 (TGS), got %d", params->solver_type);
    if (params->solver_type == 1 && (params->solver_iterations < 1 || params->solver_iterations > 16))
        return fail("he_create: TGS needs solver_iterations (position iterations) in [1, 16]");
    he_engine* h = new he_engine();
    h->device = device;
    h->params = *params;
    *out = h;
    return 0;
}

int he_set_model(he_engine* h, const he_model* model) {
    if (!h || !model) return fail("he_set_model: null argument");
    if (check_model(model, "he_set_model", HE_MAX_BOXES)) return 1;
    PhysTopo topo{};
    he_build_topo(*model, topo);
    if (topo.nnz > HE_NNZ_MAX) return fail("he_set_model: mass-matrix pattern too large (%d)", topo.nnz);
    // the zero pose's body origins in the root frame: every local rotation is the identity, so the
    // joint offsets add up along the chain (the Default state init's rigid-body rows)
    float rest[HE_NUM_BODIES][3] = {};
    for (int b = 1; b < HE_NUM_BODIES; ++b)
        for (int c = 0; c < 3; ++c) rest[b][c] = rest[model->parents[b]][c] + model->local_pos[b][c];
    // the device copies in locals first: a refused or failed call leaves the previous model in place
    HE_CHECK(hipSetDevice(h->device));
    DeviceArray<he_model> d_model;
    DeviceArray<PhysTopo> d_topo;
    DeviceArray<float> d_rest;
    HE_CHECK(d_model.assign(model, 1));
    HE_CHECK(d_topo.assign(&topo, 1));
    HE_CHECK(d_rest.assign(&rest[0][0], HE_NUM_BODIES * 3));
    int32_t modes[HE_NUM_DOF];
    for (int d = 0; d < HE_NUM_DOF; ++d) modes[d] = HE_DOF_MODE_POS;
    DeviceArray<int32_t> d_modes;
    HE_CHECK(d_modes.assign(modes, HE_NUM_DOF));
    h->d_modes = std::move(d_modes);
    std::memcpy(h->modes, modes, sizeof(modes));
    h->act_set = false;
    h->d_model = std::move(d_model);
    h->d_topo = std::move(d_topo);
    h->d_rest = std::move(d_rest);
    h->model = *model;
    // the kernel holds every joint's rotation angle below pi - 0.02 (the exp-map branch cut); dof
    // bounds inside that band would need per-component rows (the oracle has them, the kernel not)
    h->component_limits = false;
    for (int d = 0; d < HE_NUM_DOF; ++d)
        if (std::fabs(model->dof_lower[d]) < 3.1215f || std::fabs(model->dof_upper[d]) < 3.1215f) h->component_limits = true;
    h->has_model = true;
    return 0;
}

static int warm_kernels(int device);

// The packed env state's layout, from the table alone (host only; no buffer need exist): the included
// rows in table order, each at the offset the ones before it leave.
static int state_layout(he_engine* h, he_state_layout* out) {
    he_state_layout l{};
    l.version = HE_STATE_VERSION;
    for (const EnvBuffer& b : env_buffers(h)) {
        if (!b.state) continue;
        if (l.num_fields == HE_STATE_MAX_FIELDS)
            return fail("env state: more than HE_STATE_MAX_FIELDS (%d) buffers in the state", HE_STATE_MAX_FIELDS);
        l.fields[l.num_fields++] = he_state_field{b.kind, l.words, b.words(), b.dtype};
        l.words += b.words();
    }
    *out = l;
    return 0;
}

// allocates and initialises every per-env buffer; the caller releases them all when this fails
static int init_env_buffers(he_engine* h, int N, const float* host_start_xy) {
    for (const EnvBuffer& b : env_buffers(h)) {
        HE_CHECK(b.mem->alloc(b.bytes(N)));
        HE_CHECK(b.mem->fill(b.fill, b.bytes(N)));
    }
    // humanoid_phc.py:340-347: start pose (x, y) + z 0.89, identity rotation, zero velocity
    std::vector<float> root((size_t)N * 13, 0.f);
    for (int e = 0; e < N; ++e) {
        float* r = &root[(size_t)e * 13];
        r[0] = host_start_xy ? host_start_xy[2 * e] : 0.f;
        r[1] = host_start_xy ? host_start_xy[2 * e + 1] : 0.f;
        r[2] = 0.89f;
        r[6] = 1.f;
    }
    HE_CHECK(h->root.upload(root.data(), root.size()));
    // _initial_humanoid_root_states (humanoid_phc.py:522-523): the creation poses, zero velocities
    HE_CHECK(h->init_root.upload(root.data(), root.size()));
    // dispatch order: the identity until the first rebuild
    std::vector<int32_t> ord((size_t)N);
    for (int e = 0; e < N; ++e) ord[e] = e;
    HE_CHECK(h->order.upload(ord.data(), ord.size()));
    // the env-state kernel's view of the table: one StateField per included buffer
    he_state_layout layout;
    if (state_layout(h, &layout)) return 1;
    std::vector<StateField> desc;
    for (const EnvBuffer& b : env_buffers(h))
        if (b.state) {
            const he_state_field& f = layout.fields[desc.size()];
            desc.push_back(StateField{static_cast<uint32_t*>(b.mem->get()), f.words, f.offset_words});
        }
    HE_CHECK(h->state_desc.assign(desc.data(), desc.size()));
    h->state_fields = layout.num_fields;
    h->state_words = layout.words;
    return 0;
}

int he_create_envs(he_engine* h, int num_envs, const float* host_start_xy) {
    if (!h) return fail("he_create_envs: null handle");
    if (!h->has_model) return fail("he_create_envs: call he_set_model first");
    if (num_envs <= 0) return fail("he_create_envs: num_envs must be positive");
    if (h->num_envs) return fail("he_create_envs: envs already created");
    HE_CHECK(hipSetDevice(h->device));
    // before any allocation: a failed warm-up leaves nothing behind to leak or re-allocate
    if (warm_kernels(h->device)) return 1;
    if (init_env_buffers(h, num_envs, host_start_xy)) {
        for (const EnvBuffer& b : env_buffers(h)) b.mem->release();  // as before the call: a retry is valid
        h->state_desc.release();
        h->state_fields = h->state_words = 0;
        return 1;
    }
    if (const char* v = std::getenv("HE_PHYS_ORDER")) h->order_every = std::atoi(v);
    if (const char* v = std::getenv("HE_TGS_LEGS")) h->full_dofs = std::atoi(v) == 0;
    h->num_envs = num_envs;
    return 0;
}

int he_destroy(he_engine* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    delete h;
    return 0;
}

int he_get_buffer(he_engine* h, int kind, void** dptr, int64_t* shape, int* ndim, int* dtype) {
    if (!h || !dptr || !shape || !ndim || !dtype) return fail("he_get_buffer: null argument");
    if (!h->num_envs) return fail("he_get_buffer: no envs created");
    for (const EnvBuffer& b : env_buffers(h)) {
        if (b.kind != kind || kind < 0) continue;
        *dptr = b.mem->get();
        *dtype = b.dtype;
        *ndim = b.cols ? 2 : 1;
        shape[0] = (int64_t)h->num_envs * b.rows;
        if (b.cols) shape[1] = b.cols;
        return 0;
    }
    return fail("he_get_buffer: unknown buffer kind %d", kind);
}

int he_set_dof_targets(he_engine* h, const float* src, void* stream) {
    if (!h || !src) return fail("he_set_dof_targets: null argument");
    if (src == h->targets) return 0;
    HE_CHECK(hipMemcpyAsync(h->targets, src, (size_t)h->num_envs * HE_NUM_DOF * sizeof(float),
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

namespace {
static __global__ void copy_rows_kernel(float* dst, const float* src, const int32_t* ids, int k, int row, int num_rows) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * row) return;
    int i = t / row, c = t - i * row;
    int id = ids[i];
    if (id < 0 || id >= num_rows) return;
    dst[(size_t)id * row + c] = src[(size_t)id * row + c];
}

static int copy_rows(float* dst, const float* src, const int32_t* ids, int k, int row, int num_rows, void* stream,
              const char* what) {
    if (!src || !ids) return fail("%s: null argument", what);
    if (k < 0) return fail("%s: negative count", what);
    if (k == 0 || src == dst) return 0;
    int total = k * row;
    copy_rows_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(dst, src, ids, k, row, num_rows);
    HE_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

namespace {
// The one kernel behind he_save_envs (PACK: env rows -> packed rows), he_load_envs (UNPACK: packed rows
// -> env rows) and he_clone_envs (CLONE: env src[i] -> env dst[i]). Block x is the entry i, and thread
// blockIdx.y * blockDim.x + threadIdx.x the word w of the entry's packed row: a wave's 64 lanes move 64
// consecutive words of the packed row and, but where a field ends inside the wave, 64 consecutive words
// of the buffer (256 B either side, the coalesced form; the rows are 13, 138, 312, ... words and an
// env's packed row `W` words with W odd, so a row, a field and an env's share of a buffer start at any
// word: one dword per lane takes every alignment alike). Past the packed row the next HE_META_WORDS
// threads invalidate the written env's motion-metadata cache row (UNPACK and CLONE). An id outside
// 0..num_envs-1 skips its entry, as copy_rows_kernel does; so does a CLONE entry with src == dst.
enum { STATE_PACK = 0, STATE_UNPACK = 1, STATE_CLONE = 2 };
constexpr int STATE_BLOCK = 256;

static __global__ void env_state_kernel(const StateField* __restrict__ desc, int num_fields, int W,
                                        int32_t* __restrict__ meta_cache, const int32_t* __restrict__ ids,
                                        const int32_t* __restrict__ dst_ids, uint32_t* packed, int k, int num_envs,
                                        int mode) {
    const int i = blockIdx.x;
    const int w = blockIdx.y * blockDim.x + threadIdx.x;
    if (i >= k || w >= W + HE_META_WORDS) return;
    const int from = ids ? ids[i] : i;                   // the env read (PACK, CLONE) or written (UNPACK)
    const int to = mode == STATE_CLONE ? dst_ids[i] : from;
    if (from < 0 || from >= num_envs || to < 0 || to >= num_envs) return;
    if (mode == STATE_CLONE && from == to) return;
    if (w >= W) {
        if (mode != STATE_PACK) meta_cache[(size_t)to * HE_META_WORDS + (w - W)] = -1;
        return;
    }
    int f = 0;  // the field of word w: the offsets ascend and the first is 0
    while (f + 1 < num_fields && w >= desc[f + 1].offset) ++f;
    const StateField d = desc[f];
    const int c = w - d.offset;  // < d.words: the fields are contiguous and w < W
    if (mode == STATE_PACK)
        packed[(size_t)i * W + w] = d.base[(size_t)from * d.words + c];
    else if (mode == STATE_UNPACK)
        d.base[(size_t)from * d.words + c] = packed[(size_t)i * W + w];
    else
        d.base[(size_t)to * d.words + c] = d.base[(size_t)from * d.words + c];
}

// the refusals of the three calls in the header's order, then the launch
static int move_env_state(he_engine* h, const int32_t* ids, const int32_t* dst_ids, int k, void* packed, int mode,
                          void* stream, const char* what) {
    if (!h) return fail("%s: null handle", what);
    if (!h->num_envs) return fail("%s: no envs created", what);
    if (mode == STATE_CLONE) {
        if (!ids || !dst_ids) return fail("%s: null id array", what);
    } else {
        if (!packed) return fail("%s: null state buffer", what);
        if (!ids && k != h->num_envs) return fail("%s: null ids (only k == num_envs may leave them out)", what);
    }
    if (k < 0 || k > h->num_envs) return fail("%s: k = %d outside 0..%d", what, k, h->num_envs);
    if (misaligned({ids, dst_ids, packed})) return fail("%s: every buffer must be 4-byte aligned", what);
    if (k == 0) return 0;
    const dim3 grid(k, (h->state_words + HE_META_WORDS + STATE_BLOCK - 1) / STATE_BLOCK);
    env_state_kernel<<<grid, STATE_BLOCK, 0, (hipStream_t)stream>>>(h->state_desc, h->state_fields, h->state_words,
                                                                    h->meta_cache, ids, dst_ids,
                                                                    static_cast<uint32_t*>(packed), k, h->num_envs, mode);
    HE_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

int he_state_layout_get(he_engine* h, he_state_layout* out) {
    if (!h) return fail("he_state_layout_get: null handle");
    if (!out) return fail("he_state_layout_get: null layout");
    return state_layout(h, out);
}

int he_save_envs(he_engine* h, const int32_t* ids, int k, void* dst, void* stream) {
    return move_env_state(h, ids, nullptr, k, dst, STATE_PACK, stream, "he_save_envs");
}
int he_load_envs(he_engine* h, const int32_t* ids, int k, const void* src, void* stream) {
    return move_env_state(h, ids, nullptr, k, const_cast<void*>(src), STATE_UNPACK, stream, "he_load_envs");
}
int he_clone_envs(he_engine* h, const int32_t* src_ids, const int32_t* dst_ids, int k, void* stream) {
    return move_env_state(h, src_ids, dst_ids, k, nullptr, STATE_CLONE, stream, "he_clone_envs");
}

int he_get_sim_state(he_engine* h, he_sim_state* out) {
    if (!h) return fail("he_get_sim_state: null handle");
    if (!h->num_envs) return fail("he_get_sim_state: no envs created");
    if (!out) return fail("he_get_sim_state: null sim state");
    *out = he_sim_state{HE_STATE_VERSION, h->wrench_hold, h->act_set ? 1 : 0, (int64_t)h->launches};
    return 0;
}
int he_set_sim_state(he_engine* h, const he_sim_state* in) {
    if (!h) return fail("he_set_sim_state: null handle");
    if (!h->num_envs) return fail("he_set_sim_state: no envs created");
    if (!in) return fail("he_set_sim_state: null sim state");
    if (in->version != HE_STATE_VERSION)
        return fail("he_set_sim_state: version %u, this library reads %d", in->version, HE_STATE_VERSION);
    if (in->wrench_hold < 0 || in->launches < 0)
        return fail("he_set_sim_state: negative wrench_hold or launches (%d, %lld)", in->wrench_hold, (long long)in->launches);
    h->wrench_hold = in->wrench_hold;
    h->act_set = in->act_set != 0;
    h->launches = in->launches;
    return 0;
}

// The env step's kernels (physics, imitation, motion ingestion, indexed row copies) each pay a
// one-time first-dispatch cost (~0.4-0.8 ms per kernel on the MI355X; 16-30 ms under rocprofv3's
// kernel tracing), paid here once per process and device at env creation, instead of by the setup's
// first full reset or by a timed step (he_kernels.h: warm_*_kernels). The rollout handoff kernels
// (he_rollout.hip, include/humanoid_rollout.h) are not on the env step and are not warmed: they pay
// theirs at the first Experience store. Serialised by a mutex (engines may be created from several
// threads); a failed warm-up is not recorded, so the next he_create_envs retries it.
static int warm_kernels(int device) {
    static std::mutex mu;
    static bool warmed[64] = {};
    const int wm = std::getenv("HE_WARM_MODE") ? std::atoi(std::getenv("HE_WARM_MODE")) : 2;
    if (wm <= 0 || device < 0 || device >= 64) return 0;
    std::lock_guard<std::mutex> lock(mu);
    if (warmed[device]) return 0;
    if (wm == 2) {
        copy_rows_kernel<<<1, 256>>>(nullptr, nullptr, nullptr, 0, 1, 0);
        HE_CHECK(hipGetLastError());
    }
    HE_CHECK(warm_physics_kernels(nullptr, wm));
    HE_CHECK(warm_imitation_kernels(nullptr, wm));
    HE_CHECK(warm_ingest_kernels(nullptr, wm));
    HE_CHECK(warm_forces_kernels(nullptr, wm));
    HE_CHECK(hipDeviceSynchronize());
    warmed[device] = true;
    return 0;
}

int he_set_root_state_indexed(he_engine* h, const float* src, const int32_t* ids, int k, void* stream) {
    if (!h) return fail("he_set_root_state_indexed: null handle");
    return copy_rows(h->root, src, ids, k, 13, h->num_envs, stream, "he_set_root_state_indexed");
}
int he_set_dof_state_indexed(he_engine* h, const float* src, const int32_t* ids, int k, void* stream) {
    if (!h) return fail("he_set_dof_state_indexed: null handle");
    return copy_rows(h->dof_state, src, ids, k, HE_NUM_DOF * 2, h->num_envs, stream, "he_set_dof_state_indexed");
}
int he_set_dof_targets_indexed(he_engine* h, const float* src, const int32_t* ids, int k, void* stream) {
    if (!h) return fail("he_set_dof_targets_indexed: null handle");
    return copy_rows(h->targets, src, ids, k, HE_NUM_DOF, h->num_envs, stream, "he_set_dof_targets_indexed");
}

int he_set_env_properties(he_engine* h, const float* mass_scale, const float* friction, const int32_t* terrain_kind) {
    if (!h) return fail("he_set_env_properties: null handle");
    h->mass_scale = mass_scale;
    h->friction = friction;
    h->terrain_kind = terrain_kind;
    h->params.terrain = terrain_kind ? 1 : 0;
    return 0;
}

int he_set_pd_params(he_engine* h, const float* host_offset, const float* host_scale, const int32_t* host_frozen_mask,
                     int clip_actions) {
    if (!h || !host_offset || !host_scale) return fail("he_set_pd_params: null argument");
    HE_CHECK(hipSetDevice(h->device));
    std::vector<int32_t> fz(HE_NUM_DOF, 0);
    if (host_frozen_mask) std::memcpy(fz.data(), host_frozen_mask, sizeof(int32_t) * HE_NUM_DOF);
    DeviceArray<float> offset, scale;
    DeviceArray<int32_t> frozen;
    HE_CHECK(offset.assign(host_offset, HE_NUM_DOF));
    HE_CHECK(scale.assign(host_scale, HE_NUM_DOF));
    HE_CHECK(frozen.assign(fz.data(), HE_NUM_DOF));
    h->pd_offset = std::move(offset);
    h->pd_scale = std::move(scale);
    h->frozen = std::move(frozen);
    h->clip_actions = clip_actions;
    h->has_pd = true;
    return 0;
}

namespace {
// num_simulate gym.simulate() calls = num_simulate x SimParams.substeps physics steps of dt / substeps
static PhysArgs phys_args(he_engine* h, int num_simulate, const float* actions) {
    PhysArgs a{};
    a.p = h->params;
    a.p.dt = h->params.dt / (float)h->params.substeps;
    a.model = h->d_model;
    a.topo = h->d_topo;
    a.root_states = h->root;
    a.dof_state = h->dof_state;
    a.dof_targets = h->targets;
    a.actions = actions;
    a.pd_offset = h->pd_offset;
    a.pd_scale = h->pd_scale;
    a.frozen = h->frozen;
    a.clip_actions = h->clip_actions;
    a.rb_state = h->rb;
    a.contact_forces = h->cf;
    a.dof_force = h->dof_force;
    a.num_contacts = h->num_contacts;
    a.dropped = h->dropped;
    a.cache = h->cache;
    a.mass_scale = h->mass_scale;
    a.friction = h->friction;
    a.terrain_kind = h->terrain_kind;
    a.num_envs = h->num_envs;
    a.substeps = num_simulate * h->params.substeps;
    a.stamps = h->stamps;
    const bool ordered = h->order_every > 0;
    a.order = ordered ? h->order : nullptr;
    a.cost = ordered ? h->cost : nullptr;
    a.full_dofs = h->full_dofs;
    // a pending wrench covers the launch's leading gym.simulate() calls, as many as its hold has left
    if (h->wrench_hold > 0) {
        const int cover = h->wrench_hold < num_simulate ? h->wrench_hold : num_simulate;
        a.ext_wrench = h->wrench;
        a.ext_steps = cover * h->params.substeps;
        h->wrench_hold -= cover;
    }
    a.dof_act = h->act_set ? h->dof_act.get() : nullptr;
    return a;
}

static int apply_wrench(he_engine* h, const float* force, const float* second, int at_pos, int space, int hold,
                        void* stream, const char* what) {
    if (!h) return fail("%s: null handle", what);
    if (!h->num_envs) return fail("%s: no envs created", what);
    if (space != HE_SPACE_ENV && space != HE_SPACE_LOCAL && space != HE_SPACE_GLOBAL)
        return fail("%s: space must be HE_SPACE_ENV (0), HE_SPACE_LOCAL (1) or HE_SPACE_GLOBAL (2), got %d", what, space);
    if (hold < 1) return fail("%s: hold must be >= 1 (gym.simulate() calls), got %d", what, hold);
    if (at_pos && (!force || !second)) return fail("%s: force and pos must both be given", what);
    if (!force && !second) {  // clear
        h->wrench_hold = 0;
        return 0;
    }
    WrenchArgs a{};
    a.force = force;
    a.second = second;
    a.rb_state = h->rb;
    a.model = h->d_model;
    a.wrench = h->wrench;
    a.rows = h->num_envs * HE_NUM_BODIES;
    a.space = space;
    a.at_pos = at_pos;
    a.accumulate = h->wrench_hold > 0;
    HE_CHECK(launch_body_wrench(a, (hipStream_t)stream));
    h->wrench_hold = hold;
    return 0;
}
}  // namespace

int he_apply_body_forces(he_engine* h, const float* force, const float* torque, int space, int hold, void* stream) {
    return apply_wrench(h, force, torque, 0, space, hold, stream, "he_apply_body_forces");
}
int he_apply_body_forces_at_pos(he_engine* h, const float* force, const float* pos, int space, int hold, void* stream) {
    return apply_wrench(h, force, pos, 1, space, hold, stream, "he_apply_body_forces_at_pos");
}

// Drive modes: the device model again with zero gains on the dofs that are not POS (drive_terms then
// yields tau = 0, coef = 0 and an effort scale of 1 there: no kernel knows about modes), the modes for
// the actuation's preparation kernel. Built in locals and moved in after the last step.
int he_set_dof_drive_modes(he_engine* h, const int32_t* host_modes) {
    if (!h) return fail("he_set_dof_drive_modes: null handle");
    if (!host_modes) return fail("he_set_dof_drive_modes: null modes");
    if (!h->has_model) return fail("he_set_dof_drive_modes: call he_set_model first");
    for (int d = 0; d < HE_NUM_DOF; ++d) {
        const int m = host_modes[d];
        if (m == HE_DOF_MODE_VEL)
            return fail("he_set_dof_drive_modes: dof %d asks for DOF_MODE_VEL (2): the engine has no velocity "
                        "target tensor; use 0 (NONE), 1 (POS) or 3 (EFFORT)", d);
        if (m != HE_DOF_MODE_NONE && m != HE_DOF_MODE_POS && m != HE_DOF_MODE_EFFORT)
            return fail("he_set_dof_drive_modes: dof %d has mode %d, out of range: 0 (NONE), 1 (POS) or 3 (EFFORT)", d, m);
    }
    he_model dev = h->model;
    for (int d = 0; d < HE_NUM_DOF; ++d)
        if (host_modes[d] != HE_DOF_MODE_POS) dev.stiffness[d] = dev.damping[d] = 0.f;
    HE_CHECK(hipSetDevice(h->device));
    DeviceArray<he_model> d_model;
    DeviceArray<int32_t> d_modes;
    HE_CHECK(d_model.assign(&dev, 1));
    HE_CHECK(d_modes.assign(host_modes, HE_NUM_DOF));
    h->d_model = std::move(d_model);  // releasing the old copies waits for the launches that read them
    h->d_modes = std::move(d_modes);
    std::memcpy(h->modes, host_modes, sizeof(h->modes));
    h->act_set = false;
    return 0;
}

namespace {
static int set_actuation(he_engine* h, const float* src, const int32_t* ids, int k, bool indexed, void* stream,
                         const char* what) {
    if (!h) return fail("%s: null handle", what);
    if (!h->num_envs) return fail("%s: no envs created", what);
    if (indexed) {
        if (!src || !ids) return fail("%s: null argument", what);
        if (k < 0) return fail("%s: negative count", what);
        if (k == 0) return 0;
    } else if (!src) {  // clear
        h->act_set = false;
        return 0;
    }
    const size_t n = (size_t)h->num_envs * HE_NUM_DOF;
    // rows an indexed write does not list keep what was set, or zero when nothing was
    if (indexed && !h->act_set) HE_CHECK(hipMemsetAsync(h->dof_act, 0, n * sizeof(float), (hipStream_t)stream));
    DofActArgs a{};
    a.src = src;
    a.ids = indexed ? ids : nullptr;
    a.modes = h->d_modes;
    a.model = h->d_model;
    a.act = h->dof_act;
    a.count = indexed ? k : h->num_envs;
    a.num_envs = h->num_envs;
    HE_CHECK(launch_dof_actuation(a, (hipStream_t)stream));
    h->act_set = true;
    return 0;
}
}  // namespace

int he_set_dof_actuation_forces(he_engine* h, const float* src, void* stream) {
    return set_actuation(h, src, nullptr, 0, false, stream, "he_set_dof_actuation_forces");
}
int he_set_dof_actuation_forces_indexed(he_engine* h, const float* src, const int32_t* ids, int k, void* stream) {
    return set_actuation(h, src, ids, k, true, stream, "he_set_dof_actuation_forces_indexed");
}

// the physics launch, then every order_every launches the next launches' dispatch order from this
// one's per-env cycles (heavy envs first, he_kernels.h launch_physics_order)
static int physics_and_order(he_engine* h, const PhysArgs& a, hipStream_t stream) {
    if (a.order && h->order_seq > 0 && (h->order_seen_seq != h->order_seq || h->order_seen_stream != stream)) {
        HE_CHECK(hipStreamWaitEvent(stream, h->order_ready, 0));
        h->order_seen_seq = h->order_seq;
        h->order_seen_stream = stream;
    }
    HE_CHECK(launch_physics(a, stream));
    if (a.order && ++h->launches % h->order_every == 0) {
        if (!h->order_ready) HE_CHECK(hipEventCreateWithFlags(&h->order_ready, hipEventDisableTiming));
        HE_CHECK(launch_physics_order(h->cost, h->order, h->num_envs, stream));
        HE_CHECK(hipEventRecord(h->order_ready, stream));
        h->order_seen_seq = ++h->order_seq;
        h->order_seen_stream = stream;
    }
    return 0;
}

int he_simulate(he_engine* h, int num_simulate, void* stream) {
    if (!h || !h->num_envs) return fail("he_simulate: no envs");
    if (h->params.joint_limits && h->component_limits)
        return fail("he_simulate: dof ranges inside +-(pi - 0.02) need per-component limit rows (not implemented)");
    if (num_simulate < 1) return fail("he_simulate: num_simulate must be >= 1");
    if (physics_and_order(h, phys_args(h, num_simulate, nullptr), (hipStream_t)stream)) return 1;
    return 0;
}

int he_step_actions(he_engine* h, const float* actions, int num_simulate, void* stream) {
    if (!h || !h->num_envs || !actions) return fail("he_step_actions: bad arguments");
    if (!h->has_pd) return fail("he_step_actions: call he_set_pd_params first");
    if (h->params.joint_limits && h->component_limits)
        return fail("he_step_actions: dof ranges inside +-(pi - 0.02) need per-component limit rows (not implemented)");
    if (num_simulate < 1) return fail("he_step_actions: num_simulate must be >= 1");
    if (physics_and_order(h, phys_args(h, num_simulate, actions), (hipStream_t)stream)) return 1;
    return 0;
}

int he_refresh(he_engine* h, void* stream) {
    (void)stream;
    if (!h) return fail("he_refresh: null handle");
    return 0;
}

// new motion tables: the imitation kernel's per-env metadata cache (keyed by motion id) is stale
static hipError_t invalidate_meta_cache(he_engine* h) {
    if (!h->num_envs) return hipSuccess;
    return h->meta_cache.fill(0xFF, (size_t)h->num_envs * HE_META_WORDS);
}

int he_load_motions(he_engine* h, int64_t F, int M, const float* gts, const float* grs, const float* lrs,
                    const float* gvs, const float* gavs, const float* dvs, const int64_t* length_starts,
                    const int64_t* num_frames, const float* lengths, const float* dt) {
    if (!h) return fail("he_load_motions: null handle");
    if (F <= 0 || M <= 0 || !gts || !grs || !lrs || !gvs || !gavs || !dvs || !length_starts || !num_frames ||
        !lengths || !dt)
        return fail("he_load_motions: bad arguments");
    for (int i = 0; i < M; ++i) {
        if (num_frames[i] < 1 || length_starts[i] < 0 || length_starts[i] + num_frames[i] > F)
            return fail("he_load_motions: motion %d frames [%lld, +%lld) outside the %lld-frame table", i,
                        (long long)length_starts[i], (long long)num_frames[i], (long long)F);
        // a one-frame motion has length 0: its sampling phase is 0/0 (and the reference cannot load one)
        if (num_frames[i] < 2)
            return fail("he_load_motions: motion %d has %lld frame(s), a motion needs at least 2", i,
                        (long long)num_frames[i]);
    }
    HE_CHECK(hipSetDevice(h->device));
    const int B = HE_NUM_BODIES;
    std::vector<float> hot((size_t)F * B * HE_MOTION_HOT), cold((size_t)F * B * HE_MOTION_COLD, 0.f);
    for (int64_t f = 0; f < F; ++f)
        for (int b = 0; b < B; ++b) {
            float* r = &hot[((size_t)f * B + b) * HE_MOTION_HOT];
            const size_t i3 = ((size_t)f * B + b) * 3, i4 = ((size_t)f * B + b) * 4;
            r[0] = gts[i3]; r[1] = gts[i3 + 1]; r[2] = gts[i3 + 2];
            r[3] = grs[i4]; r[4] = grs[i4 + 1]; r[5] = grs[i4 + 2]; r[6] = grs[i4 + 3];
            r[7] = gvs[i3]; r[8] = gvs[i3 + 1]; r[9] = gvs[i3 + 2];
            r[10] = gavs[i3]; r[11] = gavs[i3 + 1]; r[12] = gavs[i3 + 2];
            float* c = &cold[((size_t)f * B + b) * HE_MOTION_COLD];
            c[0] = lrs[i4]; c[1] = lrs[i4 + 1]; c[2] = lrs[i4 + 2]; c[3] = lrs[i4 + 3];
            if (b > 0) {
                const size_t d3 = ((size_t)f * (B - 1) + b - 1) * 3;
                c[4] = dvs[d3]; c[5] = dvs[d3 + 1]; c[6] = dvs[d3 + 2];
            }
        }
    // the new tables in a local: a failure frees them and leaves the loaded library in place
    MotionTables t;
    if (stage_motion_tables(t, F, M, lengths, dt, length_starts, num_frames)) return 1;
    HE_CHECK(t.hot.upload(hot.data(), hot.size()));
    HE_CHECK(t.cold.upload(cold.data(), cold.size()));
    HE_CHECK(invalidate_meta_cache(h));
    h->motions = std::move(t);
    return 0;
}

int he_ingest_clips(he_engine* h, int num_clips, const int64_t* host_num_frames, const double* host_fps,
                    const float* pose_quat_global, const float* root_trans, int num_motions,
                    const int32_t* host_motion_clip, void* stream) {
    if (!h) return fail("he_ingest_clips: null handle");
    if (!h->has_model) return fail("he_ingest_clips: call he_set_model first");
    if (num_clips <= 0 || !host_num_frames || !host_fps || !pose_quat_global || !root_trans)
        return fail("he_ingest_clips: bad arguments");
    if (num_motions <= 0) num_motions = num_clips;
    if (!host_motion_clip && num_motions != num_clips)
        return fail("he_ingest_clips: motion->clip map required when num_motions != num_clips");
    std::vector<int64_t> cstart(num_clips), cnf(num_clips);
    std::vector<float> cdt(num_clips);
    int64_t F = 0;
    for (int c = 0; c < num_clips; ++c) {
        // a one-frame clip has length 0: its sampling phase is 0/0 (and the reference cannot load one)
        if (host_num_frames[c] < 2)
            return fail("he_ingest_clips: clip %d has %lld frame(s), a clip needs at least 2", c,
                        (long long)host_num_frames[c]);
        if (!(host_fps[c] > 0.0) || !std::isfinite(host_fps[c]))  // NaN fails the first test
            return fail("he_ingest_clips: clip %d has %lld frames at %g fps", c, (long long)host_num_frames[c],
                        host_fps[c]);
        cstart[c] = F;
        cnf[c] = host_num_frames[c];
        cdt[c] = (float)(1.0 / host_fps[c]);
        F += host_num_frames[c];
    }
    std::vector<int64_t> ms(num_motions), mn(num_motions);
    std::vector<float> ml(num_motions), mdt(num_motions);
    for (int i = 0; i < num_motions; ++i) {
        const int c = host_motion_clip ? host_motion_clip[i] : i;
        if (c < 0 || c >= num_clips) return fail("he_ingest_clips: motion %d maps to clip %d of %d", i, c, num_clips);
        ms[i] = cstart[c];
        mn[i] = cnf[c];
        // motion_lib.py:376-379: curr_len = 1/fps * (num_frames - 1) in python floats -> float32
        ml[i] = (float)(1.0 / host_fps[c] * (double)(cnf[c] - 1));
        mdt[i] = (float)(1.0 / host_fps[c]);
    }
    HE_CHECK(hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    HE_CHECK(hipStreamSynchronize(st));  // tables may be in use by queued kernels
    // the new tables and the kernel's temporaries in locals: every return frees what it leaves
    // behind, and a failure leaves the loaded library in place
    MotionTables t;
    if (stage_motion_tables(t, F, num_motions, ml.data(), mdt.data(), ms.data(), mn.data())) return 1;
    DeviceArray<int64_t> d_cs, d_cn;
    DeviceArray<float> d_cdt, scratch;
    HE_CHECK(d_cs.assign(cstart.data(), num_clips));
    HE_CHECK(d_cn.assign(cnf.data(), num_clips));
    HE_CHECK(d_cdt.assign(cdt.data(), num_clips));
    HE_CHECK(scratch.alloc((size_t)F * HE_NUM_BODIES * 3));
    const hipError_t e = launch_ingest(pose_quat_global, root_trans, h->d_model.get()->parents,
                                       &h->d_model.get()->local_pos[0][0], d_cs, d_cn, d_cdt, num_clips, F, t.hot,
                                       t.cold, scratch, st);
    HE_CHECK(hipStreamSynchronize(st));  // before the temporaries go, whatever the launch said
    HE_CHECK(e);
    HE_CHECK(invalidate_meta_cache(h));
    h->motions = std::move(t);
    return 0;
}

namespace {
static MotionDev motion_dev(he_engine* h) {
    const MotionTables& m = h->motions;
    return MotionDev{m.hot, m.cold, m.starts, m.nframes, m.lengths, m.dt, m.count};
}

static int imit_common(he_engine* h, const he_imitation_params* p, const he_env_motion* em, ImitArgs& a, const char* what) {
    if (!h || !p || !em) return fail("%s: null argument", what);
    if (!h->num_envs) return fail("%s: no envs", what);
    if (!h->motions.count) return fail("%s: call he_load_motions first", what);
    if (!em->motion_ids || !em->start_times || !em->start_offsets || !em->global_offset || !em->progress)
        return fail("%s: he_env_motion has null buffers", what);
    a = ImitArgs{};
    a.p = *p;
    a.m = motion_dev(h);
    a.root_states = h->root;
    a.dof_state = h->dof_state;
    a.rb_state = h->rb;
    a.contact_forces = h->cf;
    a.dof_force = h->dof_force;
    a.dof_targets = h->targets;
    a.motion_ids = em->motion_ids;
    a.start_times = em->start_times;
    a.start_offsets = em->start_offsets;
    a.global_offset = em->global_offset;
    a.progress = em->progress;
    a.ev = h->eval;
    a.has_eval = h->has_eval;
    a.init_root = h->init_root;
    a.rest_pos = h->d_rest;
    a.meta_cache = h->meta_cache;
    if (p->state_init < HE_STATE_INIT_DEFAULT || p->state_init > HE_STATE_INIT_HYBRID)
        return fail("%s: state_init %d is not a StateInit (0 Default, 1 Start, 2 Random, 3 Hybrid)", what, p->state_init);
    if (p->state_init == HE_STATE_INIT_HYBRID && !(p->hybrid_init_prob >= 0.f && p->hybrid_init_prob <= 1.f))
        return fail("%s: hybrid_init_prob must be in [0, 1]", what);
    return 0;
}
// the AMP update that follows an imitation launch (he_set_amp)
static hipError_t amp_after(he_engine* h, const ImitArgs& ia, int mode, hipStream_t stream) {
    if (!h->has_amp) return hipSuccess;
    AmpArgs a{};
    a.m = ia.m;
    a.rb_state = h->rb;
    a.dof_state = h->dof_state;
    a.motion_ids = ia.motion_ids;
    a.start_times = ia.start_times;
    a.reset = ia.reset;
    a.env_ids = ia.env_ids;
    a.count = ia.count;
    a.mode = mode;
    a.control_dt = ia.p.control_dt;
    a.amp = h->amp;
    a.ip = ia.p;
    a.phases = ia.phases;
    a.seed = ia.seed;
    a.step = ia.step;
    return launch_amp(a, stream);
}
}  // namespace

int he_imitation_step(he_engine* h, const he_imitation_params* p, const he_env_motion* em, float* obs, float* rew,
                      float* reward_raw, uint8_t* reset, uint8_t* terminate, void* stream) {
    ImitArgs a;
    if (imit_common(h, p, em, a, "he_imitation_step")) return 1;
    if (!obs || !rew || !reward_raw || !reset || !terminate) return fail("he_imitation_step: null output");
    a.obs = obs; a.rew = rew; a.reward_raw = reward_raw; a.reset = reset; a.terminate = terminate;
    a.count = h->num_envs;
    a.mode = 0;
    HE_CHECK(launch_imitation(a, (hipStream_t)stream));
    HE_CHECK(amp_after(h, a, 0, (hipStream_t)stream));
    return 0;
}

int he_set_eval(he_engine* h, const he_eval_buffers* b) {
    if (!h) return fail("he_set_eval: null engine");
    if (!b) {
        h->has_eval = 0;
        return 0;
    }
    if (!b->num_steps || !b->history || !b->sums) return fail("he_set_eval: num_steps, history and sums are required");
    if (b->frame < 0) return fail("he_set_eval: negative frame");
    h->eval = *b;
    h->has_eval = 1;
    return 0;
}

int he_reset_envs(he_engine* h, const he_imitation_params* p, const he_env_motion* em, const int32_t* env_ids, int k,
                  const float* phases, float* obs, uint8_t* reset, uint8_t* terminate, void* stream) {
    ImitArgs a;
    if (imit_common(h, p, em, a, "he_reset_envs")) return 1;
    if (k < 0) return fail("he_reset_envs: negative count");
    if (k == 0) return 0;
    if (!env_ids || !phases || !obs || !reset || !terminate) return fail("he_reset_envs: null argument");
    a.obs = obs; a.reset = reset; a.terminate = terminate;
    a.env_ids = env_ids;
    a.count = k;
    a.phases = phases;
    a.mode = 2;
    HE_CHECK(launch_imitation(a, (hipStream_t)stream));
    HE_CHECK(amp_after(h, a, 2, (hipStream_t)stream));
    return 0;
}

int he_env_step(he_engine* h, const he_imitation_params* p, const he_env_motion* em, const float* actions,
                int num_simulate, uint64_t seed, uint64_t step_index, float* obs, float* rew, float* reward_raw,
                uint8_t* reset, uint8_t* terminate, void* stream) {
    if (!h || !h->num_envs || !actions) return fail("he_env_step: bad arguments");
    // auto: one launch while the envs fit one round of waves on the chip (2 per SIMD: launch and
    // tail latency dominate there); past it two launches, because the imitation step at one env
    // per 250-VGPR wave adds more than the stand-alone kernel costs at full occupancy (r02 A/B at
    // 4096 envs: 0.218 against 0.209 ms per step)
    const bool fused = h->fused_step == 1 || (h->fused_step < 0 && h->num_envs <= 2048);
    if (h->has_eval || !fused) {  // eval recording lives in the stand-alone imitation kernel
        if (he_step_actions(h, actions, num_simulate, stream)) return 1;
        return he_imitation_reset_step(h, p, em, seed, step_index, obs, rew, reward_raw, reset, terminate, stream);
    }
    // one launch: actions -> PD targets -> physics -> the imitation step with the device reset of
    // flagged envs in the physics kernel's epilogue (the same results as the two launches)
    if (!h->has_pd) return fail("he_env_step: call he_set_pd_params first");
    if (num_simulate < 1) return fail("he_env_step: num_simulate must be >= 1");
    if (h->params.joint_limits && h->component_limits)
        return fail("he_env_step: dof ranges inside +-(pi - 0.02) need per-component limit rows (not implemented)");
    ImitArgs a;
    if (imit_common(h, p, em, a, "he_env_step")) return 1;
    if (!obs || !rew || !reward_raw || !reset || !terminate) return fail("he_env_step: null output");
    a.obs = obs; a.rew = rew; a.reward_raw = reward_raw; a.reset = reset; a.terminate = terminate;
    a.count = h->num_envs;
    a.mode = 1;
    a.seed = seed;
    a.step = step_index;
    PhysArgs pa = phys_args(h, num_simulate, actions);
    pa.fused = 1;
    pa.im = a;
    // with the heavy-first dispatch order as the two-launch form (the epilogue indexes the ordered
    // env): bit-identical to the unordered launch; at 4096 envs configs[4] 5 % faster, configs[1] / [2]
    // within 0.3 % (profiles/r05/ab_fused_order.txt)
    if (physics_and_order(h, pa, (hipStream_t)stream)) return 1;
    HE_CHECK(amp_after(h, a, 1, (hipStream_t)stream));
    return 0;
}

int he_set_fused_step(he_engine* h, int enable) {
    if (!h) return fail("he_set_fused_step: null engine");
    h->fused_step = enable < 0 ? -1 : (enable != 0);
    return 0;
}

int he_imitation_reset_step(he_engine* h, const he_imitation_params* p, const he_env_motion* em, uint64_t seed,
                            uint64_t step_index, float* obs, float* rew, float* reward_raw, uint8_t* reset,
                            uint8_t* terminate, void* stream) {
    ImitArgs a;
    if (imit_common(h, p, em, a, "he_imitation_reset_step")) return 1;
    if (!obs || !rew || !reward_raw || !reset || !terminate) return fail("he_imitation_reset_step: null output");
    a.obs = obs; a.rew = rew; a.reward_raw = reward_raw; a.reset = reset; a.terminate = terminate;
    a.count = h->num_envs;
    a.mode = 1;
    a.seed = seed;
    a.step = step_index;
    HE_CHECK(launch_imitation(a, (hipStream_t)stream));
    HE_CHECK(amp_after(h, a, 1, (hipStream_t)stream));
    return 0;
}

int he_set_amp(he_engine* h, const he_amp_buffers* b) {
    if (!h) return fail("he_set_amp: null engine");
    if (!b) {
        h->has_amp = 0;
        return 0;
    }
    if (!b->amp_obs) return fail("he_set_amp: amp_obs is required");
    if (b->num_steps < 1 || b->num_steps > HE_AMP_MAX_STEPS)
        return fail("he_set_amp: num_steps must be in [1, %d]", HE_AMP_MAX_STEPS);
    if ((reinterpret_cast<uintptr_t>(b->amp_obs) | reinterpret_cast<uintptr_t>(b->amp_obs_demo)) & 15)
        return fail("he_set_amp: buffers must be 16-byte aligned");
    h->amp = *b;
    h->has_amp = 1;
    return 0;
}

int he_amp_observations(int k, const float* root_pos, const float* root_rot, const float* root_vel,
                        const float* root_ang_vel, const float* dof_pos, const float* dof_vel,
                        const float* key_body_pos, float* out, void* stream) {
    if (k < 0) return fail("he_amp_observations: negative count");
    if (k == 0) return 0;
    if (!root_pos || !root_rot || !root_vel || !root_ang_vel || !dof_pos || !dof_vel || !key_body_pos || !out)
        return fail("he_amp_observations: null argument");
    AmpArgs a{};
    a.count = k;
    a.root_pos = root_pos; a.root_rot = root_rot; a.root_vel = root_vel; a.root_ang_vel = root_ang_vel;
    a.dof_pos = dof_pos; a.dof_vel = dof_vel; a.key_pos = key_body_pos; a.out = out;
    HE_CHECK(launch_amp_function(a, (hipStream_t)stream));
    return 0;
}

int he_motion_state(he_engine* h, int k, const int64_t* ids, const float* times, const float* offset, float* rg_pos,
                    float* rb_rot, float* body_vel, float* body_ang_vel, float* dof_pos, float* dof_vel, void* stream) {
    if (!h) return fail("he_motion_state: null handle");
    if (!h->motions.count) return fail("he_motion_state: call he_load_motions first");
    if (k < 0 || (k > 0 && (!ids || !times))) return fail("he_motion_state: bad arguments");
    MotionStateArgs a{};
    a.m = motion_dev(h);
    a.k = k;
    a.ids = ids;
    a.times = times;
    a.offset = offset;
    a.rg_pos = rg_pos; a.rb_rot = rb_rot; a.body_vel = body_vel; a.body_ang_vel = body_ang_vel;
    a.dof_pos = dof_pos; a.dof_vel = dof_vel;
    HE_CHECK(launch_motion_state(a, (hipStream_t)stream));
    return 0;
}

int he_set_debug_stamps(he_engine* h, uint64_t* device_buffer) {
    if (!h) return fail("he_set_debug_stamps: null handle");
    if (device_buffer && !physics_phase_stamps())
        return fail("he_set_debug_stamps: this library is built without phase stamps "
                    "(load libhumanoid_engine_phases.so, e.g. HE_ENGINE_LIB=humanoid_amd/libhumanoid_engine_phases.so)");
    h->stamps = reinterpret_cast<unsigned long long*>(device_buffer);
    return 0;
}

int he_probe_masked_solves(const float* factor, const float* y, int n, float* out, void* stream) {
    if (!factor || !y || !out) return fail("he_probe_masked_solves: null buffer");
    if (n < 0) return fail("he_probe_masked_solves: n = %d", n);
    HE_CHECK(launch_masked_solve_probe(factor, y, n, out, static_cast<hipStream_t>(stream)));
    return 0;
}

float he_hash_uniform(uint64_t seed, uint64_t step, uint32_t env) {
    uint64_t z = seed * 0x9E3779B97F4A7C15ull ^ (step + 0x632BE59BD9B4E019ull) * 0xBF58476D1CE4E5B9ull ^
                 ((uint64_t)env + 0x2545F4914F6CDD1Dull) * 0x94D049BB133111EBull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

}  // extern "C"
