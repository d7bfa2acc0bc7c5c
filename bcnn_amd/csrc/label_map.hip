// label_map.hip -- one class index per pixel of every image of a batch, at each image's own size, from an [n][C][h][w]
// tensor on the device: bilinear resampling of a per-image rectangle of the plane fused with the argmax over the classes,
// and, on request, the confusion counts against truth maps of the images' sizes. The upsampled C x H x W floats never
// exist; a pixel costs one byte of result. One host-to-device copy, one kernel whatever the image sizes, one
// device-to-host copy, one stream synchronise (include/bcnn_hip.h: bcnn_hip_label_maps_batch).
//
// The arithmetic is label_map_rule.h and nothing else (rectangle, taps through interp_rule.h, the seven-rounding blend,
// first maximum on strict >, the class of a truth byte through softmax_loss_rule.h, the block layout); this file is
// compiled with -ffp-contract=off like the rest of the library.
//
// One block per call, on the device (SCRATCH_LABEL_MAP) and pinned on the host (STAGE_LABEL_MAP), the same layout on both sides:
//   [descriptors, one per image][truth bytes][counts: C * C + 2 words][label bytes]
// The host fills the first three parts (the counts with zeros) and copies that prefix in; the kernel writes the last two,
// and that suffix is copied back (without truths there are no counts, without `labels` no label bytes). Label and truth
// bytes have the plan's layout: rows of round_up(out_w, 4) bytes, every image on a 16-byte boundary.
//
// Kernel. An item is four consecutive output pixels of one row of one image; a lane owns one item and stores its four
// labels as one 32-bit word (rows are padded to four bytes: never a partial store, never a byte store). A workgroup of 256
// lanes belongs to one image: the descriptors carry the prefix of workgroup counts, the image index is found from
// blockIdx.x alone by a binary search over it, so it is wave-uniform and the descriptor arrives by scalar loads. The lane
// forms its row tap and its four column taps once from the rule, then walks the C classes with the taps in registers:
// per class sixteen 4-byte loads on two source rows (a wave-uniform plane base in scalar registers plus a 32-bit lane
// offset), the blend and four compare-selects, unrolled by two classes so that 32 loads per lane are in flight at four
// waves per SIMD (unrolled by four the kernel spills at that occupancy; the SLP vectorizer is off for this file, Makefile). Running best value and index are 8 registers; there is no C-sized array, so one
// kernel serves every C. Evaluation: the lane reads its four truth bytes as one word and counts with integer atomics --
// into a C x C LDS tile flushed once per workgroup (C <= 64), or straight to memory (the scheme of
// softmax_loss_confusion); ignored and out-of-range pixels always go through two LDS words. Integer atomics only: the
// counts do not depend on the order. They are 32-bit on the device and widened on the host: a call stages fewer than
// 2^31 pixels, so no count of one call can pass 32 bits, LDS atomics are 32-bit natively and the copy back is half.
#include "common.h"

#include <cstdint>
#include <cstring>

#include "label_map_rule.h"

namespace bcnn_hip {
namespace {

constexpr int kLmBlock = 256;
constexpr int kLmLdsClasses = 64;  // the largest C whose C x C tile lives in LDS (16 KiB)

// Per-image record at the head of the block. Read through scalar loads: every field is wave-uniform.
struct alignas(16) LabelMapDesc {
    int out_w, out_h;
    int roi_x, roi_y, roi_w, roi_h;
    unsigned first_wg;          // workgroups of the images in front
    unsigned items;             // out_h * items_per_row
    unsigned items_per_row;     // round_up(out_w, 4) / 4
    unsigned ipr_magic;         // FastDiv of items_per_row over [0, items)
    unsigned offset;            // of the image's bytes inside the label block, and inside the truth block
    float step_w, step_h;       // bcnn_interp_step of the two axes of the rectangle
    int pad[3];
};
static_assert(sizeof(LabelMapDesc) == 64, "sixteen words per image");
static_assert(sizeof(bcnn_label_map_geom) == sizeof(bcnn_hip_label_map_image), "one layout for the rule and the C ABI");

struct LabelMapParams {
    int C, H, W;
    int num_images;
    int align_corners;
    int ignore_label;
};

enum { LM_PLAIN = 0, LM_EVAL = 1, LM_EVAL_LDS = 2 };

template <int MODE>
__global__ __launch_bounds__(kLmBlock, 4) void label_map_kernel(const float* __restrict__ x,
                                                             const LabelMapDesc* __restrict__ descs,
                                                             const uint8_t* __restrict__ truths,
                                                             unsigned* __restrict__ counts, uint8_t* __restrict__ labels,
                                                             const LabelMapParams p) {
    constexpr bool kEval = MODE != LM_PLAIN, kLds = MODE == LM_EVAL_LDS;
    __shared__ unsigned tile[kLds ? kLmLdsClasses * kLmLdsClasses : 1];
    __shared__ unsigned other[2];  // ignored, out of range
    if (kEval) {
        if (kLds)
            for (int k = threadIdx.x; k < p.C * p.C; k += kLmBlock) tile[k] = 0u;
        if (threadIdx.x < 2) other[threadIdx.x] = 0u;
        __syncthreads();
    }
    // the image of this workgroup: the last one whose first_wg is <= blockIdx.x (wave-uniform)
    int b = 0;
    for (int hi = p.num_images; hi - b > 1;) {
        const int mid = b + (hi - b) / 2;
        if (descs[mid].first_wg <= blockIdx.x) b = mid; else hi = mid;
    }
    const LabelMapDesc d = descs[b];
    const unsigned item = (blockIdx.x - d.first_wg) * kLmBlock + threadIdx.x;
    if (item < d.items) {
        const FastDiv dq = {d.items_per_row, d.ipr_magic};
        const unsigned oy = fdiv(item, dq), q = item - oy * d.items_per_row;
        int y0, y1;
        float h0, h1;
        bcnn_interp_tap(d.roi_h, d.step_h, p.align_corners, (int)oy, &y0, &y1, &h1);
        h0 = 1.0f - h1;
        int x0[4], x1[4];
        float w0[4], w1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // the columns past out_w repeat the last one: no garbage is read
            bcnn_interp_tap(d.roi_w, d.step_w, p.align_corners, min((int)q * 4 + e, d.out_w - 1), &x0[e], &x1[e], &w1[e]);
            w0[e] = 1.0f - w1[e];
        }
        // One wave-uniform base per class (scalar registers, advanced by a plane per class) plus sixteen per-lane byte
        // offsets inside the plane: a plane is at most 2^30 elements (the entry point refuses more), so 32 bits hold them.
        const size_t plane_bytes = (size_t)p.H * p.W * sizeof(float);
        const char* __restrict__ xc = reinterpret_cast<const char*>(x) + (size_t)b * p.C * plane_bytes;
        const unsigned row0 = (unsigned)(d.roi_y + y0) * p.W + d.roi_x, row1 = (unsigned)(d.roi_y + y1) * p.W + d.roi_x;
        unsigned oa[4], ob[4], oc[4], od[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            oa[e] = (row0 + x0[e]) * 4u; ob[e] = (row0 + x1[e]) * 4u;
            oc[e] = (row1 + x0[e]) * 4u; od[e] = (row1 + x1[e]) * 4u;
        }
#define LM_AT(o) (*reinterpret_cast<const float*>(xc + (o)))
        float best[4];
        int arg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            best[e] = bcnn_label_map_value(LM_AT(oa[e]), LM_AT(ob[e]), LM_AT(oc[e]), LM_AT(od[e]), w0[e], w1[e], h0, h1);
            arg[e] = 0;
        }
#pragma unroll 2
        for (int c = 1; c < p.C; ++c) {
            xc += plane_bytes;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = bcnn_label_map_value(LM_AT(oa[e]), LM_AT(ob[e]), LM_AT(oc[e]), LM_AT(od[e]), w0[e], w1[e], h0, h1);
                bcnn_label_map_argmax_step(v, c, &best[e], &arg[e]);
            }
        }
#undef LM_AT
        const size_t at = (size_t)d.offset + (size_t)oy * d.items_per_row * 4 + (size_t)q * 4;
        if (labels)
            *reinterpret_cast<uint32_t*>(labels + at) =
                (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[2] << 16 | (uint32_t)arg[3] << 24;
        if (kEval) {
            const uint32_t tw = *reinterpret_cast<const uint32_t*>(truths + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((int)q * 4 + e >= d.out_w) continue;  // row padding: no pixel
                int cls;
                const int kind = bcnn_label_map_truth((unsigned char)(tw >> (8 * e) & 255u), p.ignore_label, p.C, &cls);
                if (kind != BCNN_SL_VALID) atomicAdd(&other[kind == BCNN_SL_IGNORED ? 0 : 1], 1u);
                else if (kLds) atomicAdd(&tile[cls * p.C + arg[e]], 1u);
                else atomicAdd(&counts[(size_t)cls * p.C + arg[e]], 1u);
            }
        }
    }
    if (kEval) {
        __syncthreads();
        if (kLds)
            for (int k = threadIdx.x; k < p.C * p.C; k += kLmBlock)
                if (tile[k]) atomicAdd(&counts[k], tile[k]);
        if (threadIdx.x < 2 && other[threadIdx.x]) atomicAdd(&counts[p.C * p.C + threadIdx.x], other[threadIdx.x]);
    }
}

// Optional timing of the kernel alone (bcnn_hip_label_maps_kernel_ms): the call is synchronous, so device events recorded
// around it from outside span the two copies as well.
struct LabelMapTimer { bool on = false; hipEvent_t a = nullptr, b = nullptr; float ms = -1.0f; };
thread_local LabelMapTimer g_lm_timer;

inline const bcnn_label_map_geom* geoms(const bcnn_hip_label_map_image* imgs) {
    return reinterpret_cast<const bcnn_label_map_geom*>(imgs);
}

}  // namespace
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_label_map_fit(int fit, int W, int H, int iw, int ih, bcnn_hip_label_map_image* out) {
    if (!out) return 1;
    return bcnn_label_map_fit(fit, W, H, iw, ih, reinterpret_cast<bcnn_label_map_geom*>(out));
}

int bcnn_hip_label_maps_plan(const bcnn_hip_label_map_image* imgs, int num_images, int c, int h, int w, int with_truths,
                             unsigned* row_strides, unsigned long long* offsets, unsigned long long* total_bytes) {
    if (!imgs || num_images < 1 || c < 1 || c > BCNN_LABEL_MAP_MAX_CLASSES || h < 1 || w < 1) return 1;
    for (int b = 0; b < num_images; ++b)
        if (!bcnn_label_map_geom_ok(geoms(imgs) + b, h, w)) return 1;
    return bcnn_label_map_plan(geoms(imgs), num_images, with_truths ? 1 : 0, row_strides, offsets, total_bytes);
}

float bcnn_hip_label_maps_kernel_ms(int enable) {
    LabelMapTimer& t = g_lm_timer;
    if (enable && !t.a) {
        HIP_CHECK(hipEventCreate(&t.a));
        HIP_CHECK(hipEventCreate(&t.b));
    }
    t.on = enable != 0;
    return t.ms;
}

int bcnn_hip_label_maps_batch(const float* x_d, int n, int c, int h, int w, int align_corners,
                              const bcnn_hip_label_map_image* imgs, int num_images, uint8_t* const* labels,
                              const int* label_strides, const uint8_t* const* truths, const int* truth_strides,
                              int ignore_label, long long* counts, long long* ignored, long long* out_of_range) {
    // ---- every refusal comes before anything is staged or queued
    if (!x_d || !imgs || n < 1 || num_images < 1 || num_images > n || (!labels && !truths) || (truths && !counts) ||
        ignore_label >= 256 || (long long)h * w > (1ll << 30))
        return 1;
    unsigned long long label_bytes;
    if (bcnn_hip_label_maps_plan(imgs, num_images, c, h, w, truths ? 1 : 0, nullptr, nullptr, &label_bytes) != 0) return 1;
    for (int b = 0; b < num_images; ++b) {
        if ((labels && (!labels[b] || (label_strides && label_strides[b] < imgs[b].out_w))) ||
            (truths && (!truths[b] || (truth_strides && truth_strides[b] < imgs[b].out_w))))
            return 1;
    }
    // ---- the block: [descriptors][truths][counts][labels]
    const size_t desc_bytes = (size_t)num_images * sizeof(LabelMapDesc);
    const size_t truth_at = desc_bytes, truth_bytes = truths ? (size_t)label_bytes : 0;
    const size_t count_at = truth_at + truth_bytes, count_words = truths ? (size_t)c * c + 2 : 0;
    const size_t label_at = count_at + align_up(count_words * sizeof(unsigned), 16);
    const size_t total = label_at + (labels ? (size_t)label_bytes : 0);
    // the pinned side: every call ends in a stream synchronise, so this slot never has a copy in flight to wait for
    uint8_t* stage = host_stage(STAGE_LABEL_MAP, total);
    LabelMapDesc* desc = reinterpret_cast<LabelMapDesc*>(stage);
    const bcnn_label_map_geom* g = geoms(imgs);
    unsigned long long wgs = 0, at = 0;
    for (int b = 0; b < num_images; ++b) {
        LabelMapDesc& d = desc[b];
        memset(&d, 0, sizeof(d));
        d.out_w = g[b].out_w; d.out_h = g[b].out_h;
        d.roi_x = g[b].roi_x; d.roi_y = g[b].roi_y; d.roi_w = g[b].roi_w; d.roi_h = g[b].roi_h;
        d.items_per_row = bcnn_label_map_row_stride(g[b].out_w) / 4;
        d.items = d.items_per_row * (unsigned)g[b].out_h;  // below 2^29: the label block is within 2^31 bytes
        d.ipr_magic = make_fdiv(d.items_per_row, d.items).magic;
        d.first_wg = (unsigned)wgs;
        d.offset = (unsigned)at;
        d.step_w = bcnn_interp_step(g[b].roi_w, g[b].out_w, align_corners ? 1 : 0);
        d.step_h = bcnn_interp_step(g[b].roi_h, g[b].out_h, align_corners ? 1 : 0);
        if (truths) {
            const size_t row = (size_t)d.items_per_row * 4, stride = truth_strides ? (size_t)truth_strides[b] : (size_t)g[b].out_w;
            uint8_t* dst = stage + truth_at + at;
            for (int y = 0; y < g[b].out_h; ++y) memcpy(dst + y * row, truths[b] + y * stride, (size_t)g[b].out_w);
        }
        wgs += (d.items + kLmBlock - 1) / kLmBlock;
        at += align_up((size_t)d.items * 4, 16);
    }
    if (truths) memset(stage + count_at, 0, count_words * sizeof(unsigned));

    // ---- one copy in, one kernel, one copy back, one synchronise
    uint8_t* block_d = reinterpret_cast<uint8_t*>(scratch(SCRATCH_LABEL_MAP, (total + 3) / 4));
    hipStream_t st = current_stream();
    HIP_CHECK(hipMemcpyAsync(block_d, stage, label_at, hipMemcpyHostToDevice, st));
    LabelMapParams p;
    p.C = c; p.H = h; p.W = w;
    p.num_images = num_images;
    p.align_corners = align_corners ? 1 : 0;
    p.ignore_label = ignore_label;
    const LabelMapDesc* desc_d = reinterpret_cast<const LabelMapDesc*>(block_d);
    const uint8_t* truths_d = truths ? block_d + truth_at : nullptr;
    unsigned* counts_d = truths ? reinterpret_cast<unsigned*>(block_d + count_at) : nullptr;
    uint8_t* labels_d = labels ? block_d + label_at : nullptr;
    const dim3 grid((unsigned)wgs);
    LabelMapTimer& timer = g_lm_timer;
    if (timer.on) HIP_CHECK(hipEventRecord(timer.a, st));
    if (!truths) {
        trace_kernel("label_map");
        label_map_kernel<LM_PLAIN><<<grid, kLmBlock, 0, st>>>(x_d, desc_d, truths_d, counts_d, labels_d, p);
    } else if (c <= kLmLdsClasses) {
        trace_kernel("label_map:eval:lds");
        label_map_kernel<LM_EVAL_LDS><<<grid, kLmBlock, 0, st>>>(x_d, desc_d, truths_d, counts_d, labels_d, p);
    } else {
        trace_kernel("label_map:eval");
        label_map_kernel<LM_EVAL><<<grid, kLmBlock, 0, st>>>(x_d, desc_d, truths_d, counts_d, labels_d, p);
    }
    KERNEL_CHECK();
    if (timer.on) HIP_CHECK(hipEventRecord(timer.b, st));
    HIP_CHECK(hipMemcpyAsync(stage + count_at, block_d + count_at, total - count_at, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (timer.on) HIP_CHECK(hipEventElapsedTime(&timer.ms, timer.a, timer.b));

    // ---- rows to the caller's buffers at the caller's strides; counts widened and added
    if (labels) {
        at = 0;
        for (int b = 0; b < num_images; ++b) {
            const size_t row = (size_t)desc[b].items_per_row * 4, stride = label_strides ? (size_t)label_strides[b] : (size_t)g[b].out_w;
            const uint8_t* src = stage + label_at + at;
            for (int y = 0; y < g[b].out_h; ++y) memcpy(labels[b] + y * stride, src + y * row, (size_t)g[b].out_w);
            at += align_up(row * g[b].out_h, 16);
        }
    }
    if (truths) {
        const unsigned* cw = reinterpret_cast<const unsigned*>(stage + count_at);
        for (size_t k = 0; k < (size_t)c * c; ++k) counts[k] += (long long)cw[k];
        if (ignored) *ignored += (long long)cw[(size_t)c * c];
        if (out_of_range) *out_of_range += (long long)cw[(size_t)c * c + 1];
    }
    return 0;
}

}  // extern "C"
