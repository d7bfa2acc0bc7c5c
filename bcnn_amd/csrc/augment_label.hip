// augment_label.hip -- the class-index label maps of a training batch on the device: what bcnn_hip_augment_batch
// (augment.hip) does to the images, done to their masks. The label of a pixel is ONE byte of the sample's raw mask, or the
// fill byte: the pull-back through flip, shift, scale and rotation of ../host/bip_label_warp.h, the header libbip's
// bip_warp_label_map and the loader's host route (../host/bcnn_data_segmentation.c) are written on as well, so the three
// agree byte for byte. The host made every draw and every float -> integer step (the records and tap tables are the image
// batch's own); the kernel does integer work only.
//
// One pinned staging block [records][taps][maps] goes up in ONE copy on the current stream and ONE kernel follows: a
// pointwise function of one mask byte per pixel -- wave64, no LDS, no atomics, no barrier. The block is the slot STAGE_AUGMENT_LABEL of the
// library's pinned table (common.h), not the image batch's STAGE_AUGMENT, so a call does not wait for the copy of the image
// batch that is still in flight; the device side is the slot SCRATCH_AUGMENT_LABEL of the scratch table.
// The minimum traffic is 1 byte read and 4 bytes written per pixel, so the stores are what matters: when w % 4 == 0 and
// the tensor is 16-byte aligned a lane owns four consecutive pixels of a row and issues one 16-byte store (a wave writes
// 1 KiB of consecutive floats); otherwise a lane owns one pixel. The mask bytes are a gather through the cache (a rotated
// row walks a slanted line of the 1-byte map; neighbouring lanes stay within a few cache lines). The record is read once
// per workgroup: the sample index comes from blockIdx alone, so the load is scalar. The rotation's two fixed-point
// products are per pixel.
#include "common.h"

#include <cstdint>
#include <cstring>

#include "../host/bip_label_warp.h"

namespace bcnn_hip {
namespace {

constexpr int kLabelBlock = 256;

struct LabelParams {
    uint32_t rec_off, tap_off, map_off;  // in the staging block, bytes from its first byte
    int w, h, fill;
    int items_per_row;      // lanes per row: w (one pixel each) or w / 4
    int blocks_per_sample;
};

// kV4: a lane owns pixels x0 .. x0 + 3 of one row (w % 4 == 0: a lane's four never straddle a row) and stores one float4.
template <bool kV4>
__global__ __launch_bounds__(kLabelBlock) void augment_label_kernel(const uint8_t* __restrict__ block,
                                                                    float* __restrict__ dst, LabelParams p) {
    const int b = blockIdx.x / p.blocks_per_sample;  // workgroup-uniform
    const int item = (blockIdx.x - b * p.blocks_per_sample) * kLabelBlock + threadIdx.x;
    const int y = item / p.items_per_row;
    if (y >= p.h) return;
    const int x0 = (item - y * p.items_per_row) * (kV4 ? 4 : 1);
    const bcnn_hip_augment_record r = reinterpret_cast<const bcnn_hip_augment_record*>(block + p.rec_off)[b];
    bip_label_sample s;
    s.map = block + p.map_off + (size_t)b * p.w * p.h;
    s.tapx = reinterpret_cast<const int32_t*>(block + p.tap_off) + (size_t)b * (p.w + p.h) * 2;
    s.tapy = s.tapx + 2 * (size_t)p.w;
    s.w = p.w;
    s.h = p.h;
    s.flags = r.flags;
    s.x_ul = r.x_ul;
    s.y_ul = r.y_ul;
    s.ca = r.ca;
    s.sa = r.sa;
    s.fill = p.fill;
    float* __restrict__ out = dst + ((size_t)b * p.h + y) * p.w + x0;
    if constexpr (kV4) {
        // the four source offsets first, then the four byte loads: independent gathers in flight together
        int64_t at[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) at[j] = bip_label_source(&s, x0 + j, y);
        int32_t lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) lab[j] = s.map[at[j] < 0 ? 0 : at[j]];   // byte 0 of the sample's own map: in bounds
        float4 v;
        v.x = (float)(at[0] < 0 ? p.fill : lab[0]);
        v.y = (float)(at[1] < 0 ? p.fill : lab[1]);
        v.z = (float)(at[2] < 0 ? p.fill : lab[2]);
        v.w = (float)(at[3] < 0 ? p.fill : lab[3]);
        *reinterpret_cast<float4*>(out) = v;
    } else {
        *out = (float)bip_label_warp(&s, x0, y);
    }
}

}  // namespace
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" int bcnn_hip_augment_label_batch(float* label_d, int n, int h, int w, int num_samples, const uint8_t* maps,
                                            const bcnn_hip_augment_record* records, const int32_t* taps, int fill) {
    // ---- every refusal comes before anything is staged or queued
    if (!label_d || !maps || !records || n < 1 || h < 1 || w < 1 || num_samples < 1 || num_samples > n || fill < 0 || fill > 255)
        return 1;
    const size_t num = (size_t)num_samples, map_bytes = (size_t)w * h, sample_taps = ((size_t)w + h) * 2;
    if (map_bytes > (size_t)0x7fffffff / num) return 1;
    bool any_scale = false;
    for (size_t b = 0; b < num; ++b) any_scale = any_scale || (records[b].flags & BCNN_HIP_AUG_SCALE);
    if (any_scale && !taps) return 1;
    const size_t rec_bytes = align_up(num * sizeof(bcnn_hip_augment_record), 16);
    const size_t tap_bytes = any_scale ? align_up(num * sample_taps * sizeof(int32_t), 16) : 0;
    const size_t total = rec_bytes + tap_bytes + num * map_bytes;
    if (total > (size_t)0x7fff0000) return 1;  // the block, and every lane index of the launch, below 2 GiB
    if (any_scale)  // the range taps_in_range (augment.hip) allows: index + 1 stays inside the sample
        for (size_t b = 0; b < num; ++b)
            if (!bip_label_taps_ok(records[b].flags, taps + b * sample_taps, taps + b * sample_taps + 2 * (size_t)w, w, h))
                return 1;

    uint8_t* stage = host_stage(STAGE_AUGMENT_LABEL, total);
    memcpy(stage, records, num * sizeof(bcnn_hip_augment_record));
    if (any_scale) memcpy(stage + rec_bytes, taps, num * sample_taps * sizeof(int32_t));
    memcpy(stage + rec_bytes + tap_bytes, maps, num * map_bytes);

    // ---- one copy, one launch
    hipStream_t st = current_stream();
    uint8_t* block_d = stage_upload(STAGE_AUGMENT_LABEL, SCRATCH_AUGMENT_LABEL, total, total, st);

    LabelParams p;
    p.rec_off = 0;
    p.tap_off = (uint32_t)rec_bytes;
    p.map_off = (uint32_t)(rec_bytes + tap_bytes);
    p.w = w;
    p.h = h;
    p.fill = fill;
    const bool v4 = w % 4 == 0 && al16(label_d);
    p.items_per_row = v4 ? w / 4 : w;
    p.blocks_per_sample = ceil_div((long long)p.items_per_row * h, kLabelBlock);
    const dim3 grid((unsigned)((size_t)p.blocks_per_sample * num));
    if (v4) {
        trace_kernel("augment_label:v4");
        augment_label_kernel<true><<<grid, kLabelBlock, 0, st>>>(block_d, label_d, p);
    } else {
        trace_kernel("augment_label");
        augment_label_kernel<false><<<grid, kLabelBlock, 0, st>>>(block_d, label_d, p);
    }
    KERNEL_CHECK();
    return 0;
}
