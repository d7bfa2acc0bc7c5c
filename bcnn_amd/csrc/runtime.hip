// runtime.hip -- device, memory, stream and event entry points of the C-ABI (include/bcnn_hip.h).
// Replaces the bcnn_cuda_* helper family (reference src/bcnn_utils.c:101-201). No process-global
// library handles: the state is per host thread -- one current stream, and the tables of library-private device scratch and
// pinned host staging.
#include "common.h"

#include <cstring>
#include <vector>

namespace bcnn_hip {
static thread_local hipStream_t g_stream = nullptr;  // nullptr = null stream (PyTorch-ROCm default)
hipStream_t current_stream() { return g_stream; }
void set_current_stream(hipStream_t st) { g_stream = st; }  // internal: side-stream sections (conv.hip)

int current_device() {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) { fprintf(stderr, "[bcnn_hip] device ordinal %d out of range\n", dev); exit(1); }
    return dev;
}

// ---- library-private device scratch (common.h: ScratchSlot) ------------------------------------------------------------------
// Growth: a request below `min_floats` gets min_floats, a larger one `need * grow_num / grow_den` (1/1: exactly what was asked).
struct ScratchPolicy { size_t min_floats; unsigned grow_num, grow_den; };
static constexpr ScratchPolicy kScratchPolicy[] = {  // in ScratchSlot order
    /* REDUCE        */ {1u << 16, 2, 1},
    /* BN_CONSTS     */ {4096 * 4, 2, 1},  // 4,096 float4
    /* FOLD_ROWCONST */ {8192, 2, 1},
    /* COL           */ {0, 1, 1},
    /* DMA           */ {1u << 20, 3, 2},
    /* DMA_DW        */ {1u << 20, 3, 2},
    /* WINO          */ {0, 1, 1},
    /* WINO_DW       */ {0, 1, 1},
    /* WINO43_U      */ {1u << 20, 1, 1},
    /* WINO43_TAIL   */ {0, 1, 1},
    /* WFUSED_U      */ {1u << 20, 1, 1},
    /* WFUSED_TAIL   */ {0, 1, 1},
    /* W43FF_U       */ {1u << 20, 1, 1},
    /* W43FF_TAIL    */ {0, 1, 1},
    /* DETECT        */ {1u << 16, 1, 1},  // the caller's record capacity already carries the headroom
    /* IMAGES        */ {1u << 18, 5, 4},  // 1 MiB to start with; frame sizes vary from batch to batch
    /* AUGMENT       */ {1u << 18, 1, 1},  // 1 MiB to start with; a loader's batches all have one size
    /* INTERP        */ {1u << 14, 2, 1},  // 64 KiB: 4 floats per output row / column, 2 per input row / column
    /* SOFTMAX_LOSS  */ {2048 * 6, 1, 1},  // 48 KiB: a double and four ints per workgroup of the largest capped grid
    /* AUGMENT_LABEL */ {1u << 16, 1, 1},  // 256 KiB to start with; a loader's batches all have one size
    /* LABEL_MAP     */ {1u << 18, 5, 4},  // 1 MiB to start with; image sizes vary from batch to batch
};
static_assert(sizeof(kScratchPolicy) / sizeof(kScratchPolicy[0]) == SCRATCH_SLOTS, "one policy row per ScratchSlot");
struct ScratchBlock { float* p = nullptr; size_t cap = 0; };
static thread_local ScratchBlock g_scratch[kMaxDevices][SCRATCH_SLOTS];

float* scratch(ScratchSlot slot, size_t floats) {
    ScratchBlock& b = g_scratch[current_device()][slot];
    if (b.p == nullptr || b.cap < floats) {
        const ScratchPolicy& pol = kScratchPolicy[slot];
        if (b.p) {
            HIP_CHECK(hipDeviceSynchronize());  // launches still reading the old block, on the current or the side stream
            HIP_CHECK(hipFree(b.p));
        }
        b.cap = floats < pol.min_floats ? pol.min_floats : floats * pol.grow_num / pol.grow_den;
        HIP_CHECK(hipMalloc((void**)&b.p, b.cap * sizeof(float)));
    }
    return b.p;
}

// ---- library-private pinned host staging (common.h: StageSlot) ----------------------------------------------------------------
// `copied` is recorded behind the latest copy out of the block; `generation` counts the calls that handed the block out.
struct StageBlock { uint8_t* p = nullptr; size_t cap = 0; hipEvent_t copied = nullptr; bool in_flight = false; uint64_t generation = 0; };
static thread_local StageBlock g_stage[kMaxDevices][STAGE_SLOTS];

uint8_t* host_stage(StageSlot slot, size_t bytes) {
    StageBlock& s = g_stage[current_device()][slot];
    if (s.in_flight) {
        HIP_CHECK(hipEventSynchronize(s.copied));
        s.in_flight = false;
    }
    if (!s.copied) HIP_CHECK(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    if (s.p == nullptr || s.cap < bytes) {
        if (s.p) HIP_CHECK(hipHostFree(s.p));
        s.cap = bytes + bytes / 4;
        HIP_CHECK(hipHostMalloc((void**)&s.p, s.cap, hipHostMallocDefault));
    }
    ++s.generation;
    return s.p;
}

uint8_t* host_stage_extend(StageSlot slot, size_t keep, size_t bytes) {
    StageBlock& s = g_stage[current_device()][slot];
    if (s.p != nullptr && s.cap >= bytes) return s.p;
    uint8_t* grown = nullptr;
    const size_t cap = bytes + bytes / 4;
    HIP_CHECK(hipHostMalloc((void**)&grown, cap, hipHostMallocDefault));
    if (s.p) {
        memcpy(grown, s.p, keep);
        HIP_CHECK(hipHostFree(s.p));
    }
    s.p = grown;
    s.cap = cap;
    return s.p;
}

uint64_t stage_generation(StageSlot slot) { return g_stage[current_device()][slot].generation; }

uint8_t* stage_upload(StageSlot slot, ScratchSlot device_slot, size_t upload_bytes, size_t device_bytes, hipStream_t st) {
    StageBlock& s = g_stage[current_device()][slot];
    uint8_t* block_d = reinterpret_cast<uint8_t*>(scratch(device_slot, (device_bytes + 3) / 4));
    HIP_CHECK(hipMemcpyAsync(block_d, s.p, upload_bytes, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s.copied, st));
    s.in_flight = true;
    return block_d;
}

// ---- per-kernel-class event timing ---------------------------------------------------------------
struct KRecord { int cls; hipEvent_t a, b; double flops, bytes, useful; };
static thread_local bool g_prof_on = false;
static thread_local std::vector<KRecord>* g_records = nullptr;
static thread_local std::vector<hipEvent_t>* g_event_pool = nullptr;
static hipEvent_t pool_event() {
    if (!g_event_pool) g_event_pool = new std::vector<hipEvent_t>();
    if (!g_event_pool->empty()) { hipEvent_t e = g_event_pool->back(); g_event_pool->pop_back(); return e; }
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    return e;
}
KTimer::KTimer(int cls, double flops, double bytes, double useful_flops) : idx(-1) {
    if (!g_prof_on) return;
    if (!g_records) g_records = new std::vector<KRecord>();
    KRecord r{cls, pool_event(), pool_event(), flops, bytes, useful_flops < 0 ? flops : useful_flops};
    HIP_CHECK(hipEventRecord(r.a, g_stream));
    idx = (int)g_records->size();
    g_records->push_back(r);
}
KTimer::~KTimer() {
    if (idx >= 0) HIP_CHECK(hipEventRecord((*g_records)[idx].b, g_stream));
}

// ---- dispatch trace ------------------------------------------------------------------------------
thread_local bool g_trace_on = false;
static thread_local std::vector<char>* g_trace_log = nullptr;
void trace_kernel_slow(const char* name) {
    if (!g_trace_log) g_trace_log = new std::vector<char>();
    if (g_trace_log->size() > (8u << 20)) return;  // a forgotten trace must not grow without bound
    g_trace_log->insert(g_trace_log->end(), name, name + strlen(name));
    g_trace_log->push_back('\n');
}

// The first device-touching HIP call initialises the runtime, and that initialisation re-seeds / consumes libc's
// rand() (measured: srand(7); hipMalloc; rand() differs from run to run, tools/exp/dbg_rand.py). The reference's
// builders -- and this build's, for source compatibility -- draw their initial weights from rand()
// (bcnn_tensor.c:53-58), so a program that calls srand(seed) before building its net would get different parameters
// in every run and on every rank of a data-parallel job. Every entry point that can be the first to touch a device
// therefore forces the initialisation here, with the caller's generator state parked aside (rand() and random()
// share it in glibc; initstate / setstate swap it out and back).
__global__ void warm_kernel(float* p) { if (p && threadIdx.x == 0) p[0] = 1.0f; }

static void warm_device_keeping_rand_state() {
    static thread_local unsigned long long warmed = 0;  // bit per device ordinal
    static thread_local bool any = false;
    int dev = 0;
    if (any) {  // the runtime itself is up: hipGetDevice is a plain query now
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || ((warmed >> dev) & 1ull)) return;
    }
    char scratch_state[256];
    char* user_state = initstate(1u, scratch_state, sizeof(scratch_state));  // park the caller's generator
    void* p = nullptr;
    (void)hipFree(nullptr);
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipMalloc(&p, 256) == hipSuccess) {
        // memset, a kernel launch and a copy: queue creation and code-object loading happen on first use
        float h = 0.f;
        (void)hipMemsetAsync(p, 0, 256, nullptr);
        warm_kernel<<<1, 64, 0, nullptr>>>((float*)p);
        (void)hipMemcpy(&h, p, sizeof(float), hipMemcpyDeviceToHost);
        (void)hipDeviceSynchronize();
        (void)hipFree(p);
    }
    (void)hipDeviceSynchronize();
    if (user_state) setstate(user_state);
    any = true;
    if (dev >= 0 && dev < 64) warmed |= 1ull << dev;
}

__global__ void fill_f32_kernel(float* __restrict__ x, size_t n, float v) {
    // scalar head up to 16-byte alignment, 16-byte stores on the body, scalar tail
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;
    if (head > n) head = n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (i < head) x[i] = v;
    float* body = x + head;
    const size_t nb = n - head, n4 = nb / 4;
    float4* b4 = reinterpret_cast<float4*>(body);
    const float4 v4 = make_float4(v, v, v, v);
    for (size_t j = i; j < n4; j += stride) b4[j] = v4;
    for (size_t j = n4 * 4 + i; j < nb; j += stride) body[j] = v;
}
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void bcnn_hip_set_device(int id) {
    HIP_CHECK(hipSetDevice(id));
    warm_device_keeping_rand_state();
}

int bcnn_hip_get_device(void) {
    int id = 0;
    HIP_CHECK(hipGetDevice(&id));
    return id;
}

const char* bcnn_hip_device_name(void) {
    static thread_local char name[256];
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, bcnn_hip_get_device()));
    snprintf(name, sizeof(name), "%s", prop.gcnArchName);
    return name;
}

float* bcnn_hip_malloc_f32(size_t n) {
    float* p = nullptr;
    if (n == 0) return nullptr;
    warm_device_keeping_rand_state();
    HIP_CHECK(hipMalloc((void**)&p, n * sizeof(float)));
    HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(float), current_stream()));
    return p;
}

int* bcnn_hip_malloc_i32(size_t n) {
    int* p = nullptr;
    if (n == 0) return nullptr;
    warm_device_keeping_rand_state();
    HIP_CHECK(hipMalloc((void**)&p, n * sizeof(int)));
    HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(int), current_stream()));
    return p;
}

void bcnn_hip_free(void* p) {
    if (p) HIP_CHECK(hipFree(p));
}

void bcnn_hip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, current_stream()));
    HIP_CHECK(hipStreamSynchronize(current_stream()));
}

void bcnn_hip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, current_stream()));
    HIP_CHECK(hipStreamSynchronize(current_stream()));
}

void bcnn_hip_memcpy_d2d(void* dst, const void* src, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, current_stream()));
}

void bcnn_hip_fill_f32(float* x, size_t n, float value) {
    if (n == 0) return;
    if (value == 0.0f) {
        HIP_CHECK(hipMemsetAsync(x, 0, n * sizeof(float), current_stream()));
        return;
    }
    fill_f32_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, current_stream()>>>(x, n, value);
    KERNEL_CHECK();
}

void bcnn_hip_sync(void) { HIP_CHECK(hipStreamSynchronize(current_stream())); }

void* bcnn_hip_stream_create(void) {
    hipStream_t s;
    warm_device_keeping_rand_state();
    // the highest priority the device offers: work that shares the device with this library's own side stream (the weight
    // gradients of a backward pass, conv.hip) is the pass's critical chain
    int prio_lo = 0, prio_hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_hi));
    return (void*)s;
}

void bcnn_hip_stream_destroy(void* stream) {
    if (stream) HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
}

void bcnn_hip_set_stream(void* stream) { g_stream = (hipStream_t)stream; }
void* bcnn_hip_get_stream(void) { return (void*)g_stream; }

void* bcnn_hip_event_create(void) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    return (void*)e;
}

void bcnn_hip_event_destroy(void* ev) {
    if (ev) HIP_CHECK(hipEventDestroy((hipEvent_t)ev));
}

void bcnn_hip_event_record(void* ev) { HIP_CHECK(hipEventRecord((hipEvent_t)ev, current_stream())); }
void bcnn_hip_event_sync(void* ev) { HIP_CHECK(hipEventSynchronize((hipEvent_t)ev)); }

float bcnn_hip_event_elapsed_ms(void* start, void* stop) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop));
    return ms;
}

void bcnn_hip_profile_enable(int on) { g_prof_on = (on != 0); }

void bcnn_hip_profile_reset(void) {
    if (!g_records) return;
    HIP_CHECK(hipStreamSynchronize(current_stream()));
    for (auto& r : *g_records) { g_event_pool->push_back(r.a); g_event_pool->push_back(r.b); }
    g_records->clear();
}

int bcnn_hip_profile_num_classes(void) { return K_NUM; }

const char* bcnn_hip_profile_class_name(int cls) {
    static const char* names[K_NUM] = {"conv_fwd", "conv_dw", "conv_dx", "bn_fwd", "bn_bwd", "pool",
                                       "eltwise_act", "gemm", "sgd", "depthwise_fwd", "depthwise_bwd",
                                       "conv_fwd_winograd", "conv_dx_winograd", "conv_dw_winograd",
                                       "conv_fwd_winograd43", "conv_dx_winograd43", "conv_dw_winograd43"};
    return (cls >= 0 && cls < K_NUM) ? names[cls] : "?";
}

void bcnn_hip_profile_read(int cls, double* ms, long long* launches, double* flops, double* bytes) {
    double t = 0, f = 0, b = 0;
    long long n = 0;
    if (g_records) {
        HIP_CHECK(hipStreamSynchronize(current_stream()));
        for (auto& r : *g_records) {
            if (r.cls != cls) continue;
            float e = 0.f;
            HIP_CHECK(hipEventElapsedTime(&e, r.a, r.b));
            t += e; f += r.flops; b += r.bytes; ++n;
        }
    }
    if (ms) *ms = t;
    if (launches) *launches = n;
    if (flops) *flops = f;
    if (bytes) *bytes = b;
}

void bcnn_hip_trace_enable(int on) {
    g_trace_on = (on != 0);
    if (on && g_trace_log) g_trace_log->clear();
}

size_t bcnn_hip_trace_read(char* buf, size_t cap) {
    const size_t len = g_trace_log ? g_trace_log->size() : 0;
    if (buf && cap > 0) {
        const size_t n = len < cap - 1 ? len : cap - 1;
        if (n) memcpy(buf, g_trace_log->data(), n);
        buf[n] = 0;
    }
    return len;
}

double bcnn_hip_profile_read_useful_flops(int cls) {
    double u = 0;
    if (g_records)
        for (auto& r : *g_records)
            if (r.cls == cls) u += r.useful;
    return u;
}

}  // extern "C"
