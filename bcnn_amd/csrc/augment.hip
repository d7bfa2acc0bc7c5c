// augment.hip -- the input tensor of a training batch from the data loader's raw uint8 samples, on the device: horizontal
// flip, shift onto a grey canvas, scale (bip_resize_bilinear's rule, pasted back at the shift's origin), rotation (16.16
// inverse map, fp32 blend), contrast about the per-channel integer mean, brightness, centre crop to the net input and the
// uint8 -> float conversion into NCHW planes. One host-to-device copy of one staging block and two kernel launches per
// batch, whatever its size. The host draws every parameter (rand() in the reference's order) and does every float ->
// integer step (cos / sin, the contrast gain, the resize taps); the kernels below do integer work and fp32 products and
// sums in the host's order, uncontracted (-ffp-contract=off), so the result is the host loader's bit for bit
// (bcnn_amd/host/bcnn_data.c, bip_augment.c, bip_min.c).
//
// Why two kernels through a uint8 scratch and not one workgroup per sample with the stages in LDS: the contrast stage
// needs the mean of the whole rotated sample, so a sample cannot be one pointwise pass. Every stage before it IS a
// pointwise function of the raw sample (a rotated pixel reads 4 scaled pixels, each of which reads 4 shifted pixels, each
// of which is one raw byte or the canvas), so the first kernel computes the rotated image straight from the raw bytes, a
// lane per pixel, with no barrier and no intermediate image, and adds its channel sums with one integer atomicAdd per
// wave. That works the same for a 28 x 28 digit and for a 160 x 160 x 3 list sample (two stage images of it are 150 KiB
// of a CU's 160 KiB of LDS: the LDS design would need a scratch route and a size switch as well), spreads a batch of 128
// CIFAR samples over 2,000 waves instead of 128 workgroups, and leaves no size at which the route changes (DESIGN.md
// section 16).
#include "common.h"

#include <cstdint>
#include <cstring>

#include "../host/bip_resize_tap.h"
#include "store_run.h"

namespace bcnn_hip {
namespace {

constexpr int kAugBlock = 256;
constexpr int kCanvas = 128;     // what a shifted sample is pasted onto (bcnn_data.c)

struct AugParams {
    uint32_t rec_off, sum_off, tap_off, pix_off;  // in the staging block, bytes from its first byte
    uint32_t s4_off;                              // the rotated samples, same layout as the raw ones
    int sw, sh;                                   // stored sample
    int H, W, cx, cy;                             // destination plane and where it sits in the sample
    int swap;
    int blocks_per_sample;                        // of the kernel that reads this
    int runs_per_row;
};

// One sample as the stages see it
struct Sample {
    const uint8_t* __restrict__ px;
    const int2* __restrict__ tapx;
    const int2* __restrict__ tapy;
    int w, h, flags, x_ul, y_ul;
};

template <int C>
__device__ __forceinline__ int32_t flipped(const Sample& s, int x, int y, int k) {
    if (s.flags & BCNN_HIP_AUG_FLIP) x = s.w - 1 - x;
    return s.px[((size_t)y * s.w + x) * C + k];
}
template <int C>
__device__ __forceinline__ int32_t shifted(const Sample& s, int x, int y, int k) {
    if (!(s.flags & BCNN_HIP_AUG_SHIFT)) return flipped<C>(s, x, y, k);
    const long long X = (long long)x + s.x_ul, Y = (long long)y + s.y_ul;
    return (X >= 0 && X < s.w && Y >= 0 && Y < s.h) ? flipped<C>(s, (int)X, (int)Y, k) : kCanvas;
}
template <int C>
__device__ __forceinline__ int32_t scaled(const Sample& s, int x, int y, int k) {
    if (s.flags & BCNN_HIP_AUG_SCALE) {
        const int2 tx = s.tapx[x], ty = s.tapy[y];
        if (tx.x >= 0 && ty.x >= 0) {  // covered by the resized image
            const int x1 = tx.x + (s.w > 1 ? 1 : 0), y1 = ty.x + (s.h > 1 ? 1 : 0);
            return bip_resize_blend(shifted<C>(s, tx.x, ty.x, k), shifted<C>(s, x1, ty.x, k), shifted<C>(s, tx.x, y1, k),
                                    shifted<C>(s, x1, y1, k), tx.y, ty.y);
        }
    }
    return shifted<C>(s, x, y, k);
}

// Stages 1 to 4 of every pixel of the batch -> s4, and the channel sums the contrast stage needs. A lane per pixel.
template <int C>
__global__ __launch_bounds__(kAugBlock) void augment_geometry_kernel(uint8_t* __restrict__ block, AugParams p) {
    const int b = blockIdx.x / p.blocks_per_sample;
    const int pix = (blockIdx.x - b * p.blocks_per_sample) * kAugBlock + threadIdx.x;
    const bcnn_hip_augment_record r = reinterpret_cast<const bcnn_hip_augment_record*>(block + p.rec_off)[b];
    const size_t sample_bytes = (size_t)p.sw * p.sh * C;
    Sample s;
    s.px = block + p.pix_off + b * sample_bytes;
    s.tapx = reinterpret_cast<const int2*>(block + p.tap_off) + (size_t)b * (p.sw + p.sh);
    s.tapy = s.tapx + p.sw;
    s.w = p.sw;
    s.h = p.sh;
    s.flags = r.flags;
    s.x_ul = r.x_ul;
    s.y_ul = r.y_ul;
    uint32_t sum[C];
#pragma unroll
    for (int k = 0; k < C; ++k) sum[k] = 0;
    if (pix < p.sw * p.sh) {
        const int y = pix / p.sw, x = pix - y * p.sw;
        uint8_t* __restrict__ out = block + p.s4_off + b * sample_bytes + (size_t)pix * C;
        if (r.flags & BCNN_HIP_AUG_ROTATE) {
            const int32_t cxr = p.sw / 2, cyr = p.sh / 2;
            const uint32_t u = (uint32_t)(x - cxr), v = (uint32_t)(y - cyr);
            const int32_t px = (int32_t)((uint32_t)r.ca * u - (uint32_t)r.sa * v + ((uint32_t)cxr << 16));
            const int32_t py = (int32_t)((uint32_t)r.sa * u + (uint32_t)r.ca * v + ((uint32_t)cyr << 16));
            const int32_t mx = px >> 16, my = py >> 16;
            if (mx >= 0 && mx < p.sw - 1 && my >= 0 && my < p.sh - 1) {
                const float fx = (float)(px - (int32_t)((uint32_t)mx << 16)) / 65536;
                const float fy = (float)(py - (int32_t)((uint32_t)my << 16)) / 65536;
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const float p00 = (float)scaled<C>(s, mx, my, k), p01 = (float)scaled<C>(s, mx + 1, my, k);
                    const float p10 = (float)scaled<C>(s, mx, my + 1, k), p11 = (float)scaled<C>(s, mx + 1, my + 1, k);
                    const float level = p00 * (1 - fx) * (1 - fy) + p01 * (fx) * (1 - fy) + p10 * (1 - fx) * (fy) +
                                        p11 * (fx) * (fy);
                    sum[k] = (uint8_t)level;
                }
            }  // else 0
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) sum[k] = (uint32_t)scaled<C>(s, x, y, k);
        }
#pragma unroll
        for (int k = 0; k < C; ++k) out[k] = (uint8_t)sum[k];
    }
    if (r.flags & BCNN_HIP_AUG_CONTRAST) {  // uniform over the block: every lane reaches the shuffles
        uint32_t* __restrict__ sums = reinterpret_cast<uint32_t*>(block + p.sum_off) + b * 4;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            uint32_t t = sum[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
            if ((threadIdx.x & 63) == 0) atomicAdd(&sums[k], t);
        }
    }
}

__device__ __forceinline__ int32_t clamp_u8(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Stages 5 to 8: contrast, brightness, centre crop, conversion. A lane owns kRun consecutive destination pixels of one row
// of one sample and writes them into all C planes.
template <int C>
__global__ __launch_bounds__(kAugBlock) void augment_convert_kernel(const uint8_t* __restrict__ block,
                                                                    float* __restrict__ dst, AugParams p) {
    const int b = blockIdx.x / p.blocks_per_sample;
    const int run = (blockIdx.x - b * p.blocks_per_sample) * kAugBlock + threadIdx.x;
    const int y = run / p.runs_per_row;
    if (y >= p.H) return;
    const int x0 = (run - y * p.runs_per_row) * kRun;
    const int len = min(kRun, p.W - x0);
    const bcnn_hip_augment_record r = reinterpret_cast<const bcnn_hip_augment_record*>(block + p.rec_off)[b];
    const uint32_t* __restrict__ sums = reinterpret_cast<const uint32_t*>(block + p.sum_off) + b * 4;
    const bool contrast = (r.flags & BCNN_HIP_AUG_CONTRAST) != 0;
    const uint8_t* __restrict__ row =
        block + p.s4_off + (((size_t)b * p.sh + (y + p.cy)) * p.sw + (x0 + p.cx)) * C;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int ks = (C == 3 && p.swap) ? 2 - k : k;
        const int32_t mean = contrast ? (int32_t)(sums[ks] / (uint32_t)(p.sw * p.sh)) : 0;
        float v[kRun];
#pragma unroll
        for (int j = 0; j < kRun; ++j) {
            int32_t px = 0;
            if (j < len) {
                px = row[j * C + ks];
                if (contrast) px = clamp_u8((((px - mean) * r.gain + (1 << 11)) >> 12) + mean);
                px = clamp_u8(px + r.brightness);
            }
            v[j] = ((float)px - 127.5f) * (1 / 127.5f);
        }
        store_run(dst + (((size_t)b * C + k) * p.H + y) * p.W + x0, v, len);
    }
}

// Pinned host side of the staging block (image_fill.hip's pattern): grow-only, one per host thread and device. `copied`
// is recorded behind the latest copy out of it; the next call waits for it before it overwrites (or frees) the block.
struct HostStage { uint8_t* p = nullptr; size_t cap = 0; hipEvent_t copied = nullptr; bool in_flight = false; };
thread_local HostStage g_stage[kMaxDevices];

uint8_t* host_stage(size_t bytes) {
    HostStage& s = g_stage[current_device()];
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
    return s.p;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int C>
void launch(uint8_t* block_d, float* dst_d, AugParams p, int num, hipStream_t st) {
    p.blocks_per_sample = ceil_div((long long)p.sw * p.sh, kAugBlock);
    augment_geometry_kernel<C><<<dim3((unsigned)(p.blocks_per_sample * num)), kAugBlock, 0, st>>>(block_d, p);
    KERNEL_CHECK();
    p.runs_per_row = ceil_div(p.W, kRun);
    p.blocks_per_sample = ceil_div((long long)p.runs_per_row * p.H, kAugBlock);
    augment_convert_kernel<C><<<dim3((unsigned)(p.blocks_per_sample * num)), kAugBlock, 0, st>>>(block_d, dst_d, p);
    KERNEL_CHECK();
}

}  // namespace
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_augment_batch(float* dst_d, int n, int c, int h, int w, int num_samples, int src_w, int src_h,
                           const uint8_t* pixels, const bcnn_hip_augment_record* records, const int32_t* taps,
                           int swap_to_bgr) {
    if (!dst_d || !pixels || !records || n < 1 || h < 1 || w < 1 || c < 1 || c > 4 || num_samples < 1 || num_samples > n ||
        src_w < w || src_h < h || (long long)src_w * src_h > 0x7fffffff / (c * (long long)num_samples))
        return 1;
    // ---- every refusal comes before anything is staged or queued
    const size_t num = (size_t)num_samples, sample_bytes = (size_t)src_w * src_h * c, sample_taps = (size_t)src_w + src_h;
    bool any_scale = false;
    for (size_t b = 0; b < num; ++b) any_scale = any_scale || (records[b].flags & BCNN_HIP_AUG_SCALE);
    if (any_scale && !taps) return 1;
    const size_t rec_bytes = align_up(num * sizeof(bcnn_hip_augment_record), 16), sum_bytes = num * 4 * sizeof(uint32_t);
    const size_t tap_bytes = any_scale ? num * sample_taps * 2 * sizeof(int32_t) : 0;
    const size_t pix_bytes = align_up(num * sample_bytes, 16);
    const size_t total = rec_bytes + sum_bytes + tap_bytes + pix_bytes;
    if (total + pix_bytes > (size_t)0x7fffffff) return 1;
    for (size_t b = 0; any_scale && b < num; ++b) {
        if (!(records[b].flags & BCNN_HIP_AUG_SCALE)) continue;
        const int32_t* t = taps + b * sample_taps * 2;
        for (size_t i = 0; i < sample_taps; ++i) {
            const int extent = i < (size_t)src_w ? src_w : src_h;
            if (t[2 * i] < -1 || t[2 * i] > (extent >= 2 ? extent - 2 : 0)) return 1;
        }
    }

    // the staging block: [records][channel sums, zero][taps][pixels]; behind it on the device, the rotated samples
    uint8_t* stage = host_stage(total);
    AugParams p;
    p.rec_off = 0;
    p.sum_off = (uint32_t)rec_bytes;
    p.tap_off = (uint32_t)(rec_bytes + sum_bytes);
    p.pix_off = (uint32_t)(rec_bytes + sum_bytes + tap_bytes);
    p.s4_off = (uint32_t)total;
    memcpy(stage, records, num * sizeof(bcnn_hip_augment_record));
    memset(stage + p.sum_off, 0, sum_bytes);
    if (any_scale) memcpy(stage + p.tap_off, taps, tap_bytes);
    memcpy(stage + p.pix_off, pixels, num * sample_bytes);
    if (!any_scale)  // no tap table was staged: no record may ask for one
        for (size_t b = 0; b < num; ++b) reinterpret_cast<bcnn_hip_augment_record*>(stage)[b].flags &= ~BCNN_HIP_AUG_SCALE;

    // ---- one copy, two launches
    uint8_t* block_d = reinterpret_cast<uint8_t*>(scratch(SCRATCH_AUGMENT, (total + pix_bytes + 3) / 4));
    hipStream_t st = current_stream();
    HIP_CHECK(hipMemcpyAsync(block_d, stage, total, hipMemcpyHostToDevice, st));
    HostStage& hs = g_stage[current_device()];
    HIP_CHECK(hipEventRecord(hs.copied, st));
    hs.in_flight = true;

    p.sw = src_w;
    p.sh = src_h;
    p.H = h;
    p.W = w;
    p.cx = (src_w - w) / 2;
    p.cy = (src_h - h) / 2;
    p.swap = (swap_to_bgr && c == 3) ? 1 : 0;
    p.blocks_per_sample = p.runs_per_row = 0;
    switch (c) {
        case 1: launch<1>(block_d, dst_d, p, num_samples, st); break;
        case 2: launch<2>(block_d, dst_d, p, num_samples, st); break;
        case 3: launch<3>(block_d, dst_d, p, num_samples, st); break;
        default: launch<4>(block_d, dst_d, p, num_samples, st); break;
    }
    return 0;
}

}  // extern "C"
