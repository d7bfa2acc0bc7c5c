// common.h -- shared device/host helpers for the gfx950 kernels (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "../../include/bcnn_hip.h"

// Reference convention (src/bcnn_utils.h:174-195): print and exit on any device error.
#define HIP_CHECK(expr)                                                                        \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            fprintf(stderr, "[bcnn_hip] %s:%d: %s failed: %s\n", __FILE__, __LINE__, #expr,    \
                    hipGetErrorString(_e));                                                    \
            exit((int)_e);                                                                     \
        }                                                                                      \
    } while (0)

#define KERNEL_CHECK() HIP_CHECK(hipGetLastError())

// A/B switches for kernel experiments (alternative tiles, forcing the fallback kernels, ...) exist only in the
// EXPERIMENT build of the library (make exp -> ../lib/libbcnn_hip_exp.so, -DBCNN_HIP_EXPERIMENT; used by tools/exp
// and by tests/test_fallback_paths.py through BCNN_HIP_LIB). The product build reads no environment variable.
#ifdef BCNN_HIP_EXPERIMENT
#define BCNN_EXP_ENV(name) getenv(name)
#else
#define BCNN_EXP_ENV(name) ((const char*)nullptr)
#endif

namespace bcnn_hip {

hipStream_t current_stream();
void set_current_stream(hipStream_t st);  // runtime.hip

// The calling thread's device ordinal, checked against the bound of the per-device tables (exits outside it). runtime.hip
constexpr int kMaxDevices = 64;
int current_device();

// ---- library-private device scratch (runtime.hip) -----------------------------------------------------------------------------
// Grow-only blocks, one per host thread, device and slot; not zero-filled. A thread drives at most two streams at a time: the
// current stream and, inside a backward pass, the weight-gradient side stream (conv.hip). No slot is used on both. A block that
// must grow is freed after hipDeviceSynchronize (queued readers may be on either stream); each slot's growth rule (minimum,
// headroom) is its row of the policy table in runtime.hip.
enum ScratchSlot {
    SCRATCH_REDUCE,        // current stream: split partials of the channel / GEMM reductions (blas1.hip and its callers)
    SCRATCH_BN_CONSTS,     // current stream: batch-norm per-channel constants, finalize -> apply (float4: scratch_f4)
    SCRATCH_FOLD_ROWCONST, // current stream: row constants of a batch-norm folded into a 1x1 convolution (conv.hip, forward)
    SCRATCH_COL,           // current stream: col buffer of the few-channel data gradient (conv_igemm.hip)
    SCRATCH_DMA,           // current stream: LDS-DMA weight packs, padded input of the few-channel forward (conv_igemm_dma.hip)
    SCRATCH_DMA_DW,        // side stream: padded input of the few-channel weight gradient (conv_igemm_dma.hip)
    SCRATCH_WINO,          // current stream: V, M, U of the three-kernel F(2x2,3x3) forward / data gradient (conv_winograd.hip)
    SCRATCH_WINO_DW,       // side stream: V, M, U of the three-kernel F(2x2,3x3) weight gradient (conv_winograd.hip)
    SCRATCH_WINO43_U,      // current stream: packed U of the F(4x4,3x3) forward / data gradient (conv_winograd43b.hip)
    SCRATCH_WINO43_TAIL,   // current stream: piece outputs of its K-split tail (U is still being read)
    SCRATCH_WFUSED_U,      // current stream: packed U of the fused F(2x2,3x3) forward / data gradient (conv_winograd_fused.hip)
    SCRATCH_WFUSED_TAIL,   // current stream: piece outputs of its K-split tail
    SCRATCH_W43FF_U,       // current stream: packed U of the first-form F(4x4,3x3) (experiment build, wino43_first_form_exp.h)
    SCRATCH_W43FF_TAIL,    // current stream: piece outputs of its K-split tail (experiment build)
    SCRATCH_DETECT,        // current stream: image sizes, counts, sort order and box records of the batched YOLO decode (detect.hip)
    SCRATCH_IMAGES,        // current stream: descriptors, tap tables and uint8 pixels of the batched input fill (image_fill.hip)
    SCRATCH_AUGMENT,       // current stream: records, channel sums, tap tables, raw and augmented uint8 samples of a training batch (augment.hip)
    SCRATCH_INTERP,        // current stream: tap and contributor-range tables of one bilinear interpolation call (interp.hip)
    SCRATCH_SOFTMAX_LOSS,  // current stream: per-workgroup loss and count partials of one softmax-loss forward (softmax_loss.hip)
    SCRATCH_AUGMENT_LABEL, // current stream: records, tap tables and raw uint8 masks of a batch of label maps (augment_label.hip)
    SCRATCH_LABEL_MAP,     // current stream: descriptors, truth bytes, counts and label bytes of one label-map call (label_map.hip)
    SCRATCH_SLOTS
};
// A block of at least `floats` floats for `slot` on the calling thread's device; valid until that slot's next call.
float* scratch(ScratchSlot slot, size_t floats);
inline float4* scratch_f4(ScratchSlot slot, size_t n) { return reinterpret_cast<float4*>(scratch(slot, n * 4)); }

// ---- library-private pinned host staging (runtime.hip) ------------------------------------------------------------------------
// The host side of "stage a batch in pinned memory, send it up in one copy": grow-only blocks, one per host thread, device and
// slot. The one rule: the copy in flight out of a block is waited for before the block is overwritten or freed. Two slots never
// wait for each other, so an image batch and its label batch overlap.
enum StageSlot {
    STAGE_IMAGES,        // descriptors, tap tables and pixels / JPEG coefficients of the batched input fill (image_fill.hip, jpeg_pixels.hip)
    STAGE_AUGMENT,       // records, channel sums, tap tables, samples, JPEG tables and staged effects of a training batch (augment.hip)
    STAGE_AUGMENT_LABEL, // records, tap tables and raw uint8 masks of a batch of label maps (augment_label.hip)
    STAGE_LABEL_MAP,     // descriptors, truth bytes, counts and label bytes of one label-map call, both ways (label_map.hip)
    STAGE_SLOTS
};
// The slot's block on the calling thread's device, at least `bytes` long (a new one has bytes / 4 of headroom; contents are not
// kept). Waits first for the copy that stage_upload queued out of it. Valid until the slot's next host_stage call.
uint8_t* host_stage(StageSlot slot, size_t bytes);
// The same block, at least `bytes` long, with its first `keep` bytes as they are: for a caller that has laid a batch out
// before it learns how much rides along. No copy is in flight there; the block host_stage returned may have moved.
uint8_t* host_stage_extend(StageSlot slot, size_t keep, size_t bytes);
// Queues ONE copy of the block's first `upload_bytes` on `st` into the block of `device_bytes` of `device_slot` and marks the
// copy as in flight. Returns the device block.
uint8_t* stage_upload(StageSlot slot, ScratchSlot device_slot, size_t upload_bytes, size_t device_bytes, hipStream_t st);
// Counts the slot's host_stage calls on the calling thread's device. A _begin / _run pair keeps it, with current_device(), to
// tell that no other call has taken the block in between.
uint64_t stage_generation(StageSlot slot);

// dy *= act'(y) in place and dbias += the per-channel sums of the result (depthwise.hip's backward). blas1.hip
void activation_backward_grad_bias(const float* y, float* dy, float* dbias, int n, int c, int hw, int act);

// Optional per-kernel-class timing with HIP events on the launch stream (off by default; bench.py turns it
// on to report the roofline of the dominant kernel from inside the timed region). runtime.hip.
enum KClass { K_CONV_FWD = 0, K_CONV_DW, K_CONV_DX, K_BN_FWD, K_BN_BWD, K_POOL, K_ELTWISE_ACT, K_GEMM, K_SGD,
              K_DEPTHWISE_FWD, K_DEPTHWISE_BWD,
              K_CONV_FWD_WINO, K_CONV_DX_WINO, K_CONV_DW_WINO,  // Winograd F(2x2,3x3) layers: FLOPs = what the MFMAs execute
              K_CONV_FWD_WINO43, K_CONV_DX_WINO43,              // Winograd F(4x4,3x3) layers, likewise (36 positions per 4 x 4 outputs)
              K_CONV_DW_WINO43,
              K_NUM };
struct KTimer {
    int idx;
    // useful_flops: the part of `flops` that is not padding (Winograd tiles hanging over an odd-sized plane); < 0: all of it
    KTimer(int cls, double flops, double bytes, double useful_flops = -1.0);
    ~KTimer();
};

// Dispatch trace (bcnn_hip_trace_*, off by default): dispatchers name the kernel family they launch. runtime.hip
extern thread_local bool g_trace_on;
void trace_kernel_slow(const char* name);
inline void trace_kernel(const char* name) { if (g_trace_on) trace_kernel_slow(name); }
// a name that ends in a count the host chose, e.g. conv_dx_classes:4
inline void trace_kernel_count(const char* prefix, int count) {
    if (!g_trace_on) return;
    char name[64];
    snprintf(name, sizeof(name), "%s%d", prefix, count);
    trace_kernel_slow(name);
}

constexpr int kWave = 64;      // CDNA wavefront
constexpr int kCUs = 256;      // MI355X
constexpr int kXCDs = 8;

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// what a float4 access needs of a pointer; an absent (null) optional tensor passes
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#ifndef STREAM_GRID_PER_CU
#define STREAM_GRID_PER_CU 8
#endif
// grid for a grid-stride streaming kernel: enough blocks to fill the chip, capped (guide G11).
inline int stream_grid(size_t work_items, int block) {
    size_t need = (work_items + block - 1) / block;
    size_t cap = (size_t)kCUs * STREAM_GRID_PER_CU;
    if (need < 1) need = 1;
    return (int)(need < cap ? need : cap);
}

// a / d by multiply-high with magic = ceil(2^32 / d): exact while a * d < 2^32; the host passes magic 0 where that does not
// hold for the largest dividend of the launch (or d == 1), and the kernel divides (pool2d.hip, interp.hip)
struct FastDiv {
    unsigned d, magic;
};
inline FastDiv make_fdiv(unsigned d, unsigned long long max_dividend) {
    FastDiv f;
    f.d = d;
    f.magic = d > 1 && max_dividend * d < (1ULL << 32) ? (unsigned)((0x100000000ULL + d - 1) / d) : 0u;
    return f;
}

#ifdef __HIPCC__
__device__ __forceinline__ unsigned fdiv(unsigned a, const FastDiv& f) { return f.magic ? __umulhi(a, f.magic) : a / f.d; }

// XCD-aware block remap: the dispatcher places block b on XCD b % 8; give each XCD a contiguous run
// of logical tiles so neighbours (which share operand panels / halos) hit the same L2.
// Bijective for any nblk (guide section 5 "XCD swizzle must be bijective").
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk / kXCDs, r = nblk % kXCDs;
    const int xcd = bid % kXCDs, idx = bid / kXCDs;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Wave-wide sum on the DPP path (no LDS crossbar round trips, ~8 vector-ALU instructions); result valid in LANE 63 only.
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));  // row_mirror: 16-lane sums
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1, 3
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2, 3
    return v;
}

// block-wide sum of one value; result valid in thread 0. `red` holds >= blockDim/64 floats.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) t += red[i];
    }
    return t;
}

// The activation map, bcnn_activation_layer.c:90-146. exp/log are evaluated in double exactly
// where the reference does, so results agree to rounding of the final float conversion.
__device__ __forceinline__ float act_fwd(float x, int act, float slope) {
    switch (act) {
        case BCNN_HIP_ACT_TANH: {
            const float t = 2 * x;
            const double e = exp((double)t);
            return (float)(e - 1) / ((float)e + 1);
        }
        case BCNN_HIP_ACT_RELU: return x * (float)(x > 0);  // a multiply: -0.0f for negatives, NaN propagates
        case BCNN_HIP_ACT_LRELU: return x > 0 ? x : 0.1f * x;
        case BCNN_HIP_ACT_RAMP: return x * (float)(x > 0) + 0.1f * x;
        case BCNN_HIP_ACT_SOFTPLUS: return (float)log((double)(1.0f + (float)exp((double)x)));
        case BCNN_HIP_ACT_ABS: return fabsf(x);
        case BCNN_HIP_ACT_CLAMP: return (x < 0) ? 0.f : ((x > 1) ? 1.f : x);
        case BCNN_HIP_ACT_LOGISTIC: return 1.0f / (1.0f + (float)exp((double)(-x)));
        case BCNN_HIP_ACT_PRELU: return x > 0 ? x : slope * x;
        // appended, no reference counterpart (torch's relu6 / hardsigmoid). `+ 0.f`: +0 for every x <= 0, whichever zero
        // fmaxf(-0, +0) picks; a NaN goes through (fmaxf alone would turn it into 0)
        case BCNN_HIP_ACT_RELU6: return x != x ? x : fminf(fmaxf(x, 0.f), 6.f) + 0.f;
        case BCNN_HIP_ACT_HARD_SIGMOID: return x != x ? x : fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.0f;
        default: return x;
    }
}
// The self-gated activations (hard-swish, swish, mish): their derivative is no function of the output, so no fused
// epilogue and no `act` argument but the stand-alone activation entry points' (activation.hip) takes them.
__host__ __device__ __forceinline__ bool act_needs_input(int act) {
    return act == BCNN_HIP_ACT_HARD_SWISH || act == BCNN_HIP_ACT_SWISH || act == BCNN_HIP_ACT_MISH;
}

// Activations cheap enough to fuse into a producer's epilogue (no double-precision exp/log). The
// other three (tanh, softplus, logistic) run as a separate in-place pass (activation.hip) so that
// the MFMA kernels keep their register budget. So do the appended ones (relu6, hard-sigmoid: not measured inside an
// epilogue yet; the self-gated three never fuse), in both directions: the switches of act_fwd_cheap / act_bwd_cheap
// hold the reference's ids only.
__host__ __device__ __forceinline__ bool act_is_cheap(int act) {
    return act != BCNN_HIP_ACT_TANH && act != BCNN_HIP_ACT_SOFTPLUS && act != BCNN_HIP_ACT_LOGISTIC &&
           act < BCNN_HIP_ACT_RELU6;
}
__device__ __forceinline__ float act_fwd_cheap(float x, int act, float slope) {
    switch (act) {
        case BCNN_HIP_ACT_RELU: return x * (float)(x > 0);
        case BCNN_HIP_ACT_LRELU: return x > 0 ? x : 0.1f * x;
        case BCNN_HIP_ACT_RAMP: return x * (float)(x > 0) + 0.1f * x;
        case BCNN_HIP_ACT_ABS: return fabsf(x);
        case BCNN_HIP_ACT_CLAMP: return (x < 0) ? 0.f : ((x > 1) ? 1.f : x);
        case BCNN_HIP_ACT_PRELU: return x > 0 ? x : slope * x;
        default: return x;
    }
}
__device__ __forceinline__ float act_bwd_cheap(float y, int act, float slope) {
    switch (act) {
        case BCNN_HIP_ACT_TANH: return 1 - y * y;
        case BCNN_HIP_ACT_RELU: return (float)(y > 0);
        case BCNN_HIP_ACT_LRELU: return y > 0 ? 1.0f : 0.1f;
        case BCNN_HIP_ACT_RAMP: return (float)(y > 0) + 0.1f;
        case BCNN_HIP_ACT_ABS: return y >= 0 ? 1.0f : -1.0f;
        case BCNN_HIP_ACT_CLAMP: return (float)(y > 0.0f && y < 1.0f);
        case BCNN_HIP_ACT_LOGISTIC: return (1 - y) * y;
        case BCNN_HIP_ACT_PRELU: return y > 0 ? 1.0f : slope;
        default: return 1.0f;
    }
}
__host__ __device__ __forceinline__ bool act_bwd_is_cheap(int act) {
    return act != BCNN_HIP_ACT_SOFTPLUS && act < BCNN_HIP_ACT_RELU6;
}

// derivative factor from the POST-activation value, bcnn_activation_layer.c:165-226
__device__ __forceinline__ float act_bwd_factor(float y, int act, float slope) {
    switch (act) {
        case BCNN_HIP_ACT_TANH: return 1 - y * y;
        case BCNN_HIP_ACT_RELU: return (float)(y > 0);
        case BCNN_HIP_ACT_LRELU: return y > 0 ? 1.0f : 0.1f;
        case BCNN_HIP_ACT_RAMP: return (float)(y > 0) + 0.1f;
        case BCNN_HIP_ACT_SOFTPLUS: return 1.0f / (1.0f + (float)exp((double)(-y)));
        case BCNN_HIP_ACT_ABS: return y >= 0 ? 1.0f : -1.0f;
        case BCNN_HIP_ACT_CLAMP: return (float)(y > 0.0f && y < 1.0f);
        case BCNN_HIP_ACT_LOGISTIC: return (1 - y) * y;
        case BCNN_HIP_ACT_PRELU: return y > 0 ? 1.0f : slope;
        case BCNN_HIP_ACT_RELU6: return (float)(y > 0.0f && y < 6.0f);
        case BCNN_HIP_ACT_HARD_SIGMOID: return (y > 0.0f && y < 1.0f) ? 1 / 6.0f : 0.f;
        default: return 1.0f;
    }
}
#endif  // __HIPCC__

}  // namespace bcnn_hip
