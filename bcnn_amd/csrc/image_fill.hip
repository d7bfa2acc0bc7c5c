// image_fill.hip -- the input tensor of a batch from raw uint8 images, on the device: bilinear resize (bip_resize_bilinear's
// fixed-point rule), optional letterbox onto a grey canvas, uint8 -> float conversion with mean / scale / channel swap
// (bcnn_convert_img_to_float), NCHW planes. One host-to-device copy of one staging block and one kernel launch per call.
// The result is bit-identical to the host composition of those two functions: the sampling rule and the blend are the
// host's own (../host/bip_resize_tap.h; the taps are tabulated on the host, the kernel only looks them up), the conversion
// is one fp32 subtract and one fp32 multiply, uncontracted (-ffp-contract=off).
#include "common.h"

#include <cstdint>
#include <cstring>

#include "../host/bip_resize_tap.h"
#include "image_fill.h"
#include "store_run.h"

namespace bcnn_hip {
namespace {

constexpr int kFillBlock = 256;
constexpr int kCanvas = 128;     // the letterbox canvas byte (yolo_example.cc:40-75)

struct FillParams {
    float mean[4];               // per OUTPUT channel: the mean of the source channel it reads
    float norm;
    int swap;                    // read channel 2 - k (c == 3 only)
    int H, W;                    // destination plane
    int runs_per_row, blocks_per_image;
};

// A lane owns kRun consecutive destination pixels of one row of one image and writes them into all C planes.
template <int C>
__global__ __launch_bounds__(kFillBlock) void fill_images_kernel(const uint8_t* __restrict__ stage, float* __restrict__ dst,
                                                                 FillParams p) {
    const int b = blockIdx.x / p.blocks_per_image;
    const int run = (blockIdx.x - b * p.blocks_per_image) * kFillBlock + threadIdx.x;
    const int y = run / p.runs_per_row;
    if (y >= p.H) return;
    const int x0 = (run - y * p.runs_per_row) * kRun;
    const int len = min(kRun, p.W - x0);
    const ImageDesc d = reinterpret_cast<const ImageDesc*>(stage)[b];
    const int2* __restrict__ tapx = reinterpret_cast<const int2*>(stage + d.tapx_off);
    const int2* __restrict__ tapy = reinterpret_cast<const int2*>(stage + d.tapy_off);
    const int row_bytes = d.w * C;
    const int xstep = d.w > 1 ? C : 0, ystep = d.h > 1 ? row_bytes : 0;

    float fill[C];
#pragma unroll
    for (int k = 0; k < C; ++k) fill[k] = ((float)kCanvas - p.mean[k]) * p.norm;
    float v[C][kRun];
    const int ty = y - d.y_off;
    const bool row_inside = ty >= 0 && ty < d.new_h;
    int2 ty_tap = make_int2(0, 0);
    if (row_inside) ty_tap = tapy[ty];
    const uint8_t* __restrict__ r0 = stage + d.data_off + (size_t)ty_tap.x * row_bytes;
    const uint8_t* __restrict__ r1 = r0 + ystep;
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        const int tx = x0 + j - d.x_off;
        if (row_inside && j < len && tx >= 0 && tx < d.new_w) {
            const int2 t = tapx[tx];
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int o = t.x * C + ((C == 3 && p.swap) ? 2 - k : k);
                const uint8_t s = bip_resize_blend(r0[o], r0[o + xstep], r1[o], r1[o + xstep], t.y, ty_tap.y);
                v[k][j] = ((float)s - p.mean[k]) * p.norm;
            }
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) v[k][j] = fill[k];
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k)
        store_run(dst + (((size_t)b * C + k) * p.H + y) * p.W + x0, v[k], len);
}

}  // namespace

// Extent of image iw x ih inside the W x H plane: the plane itself (stretch), or the largest extent of the image's aspect
// ratio that fits, by the reference example's integer rule (yolo_example.cc:40-75). False when an extent comes out 0.
bool fitted_extent(int fit, int W, int H, int iw, int ih, int* new_w, int* new_h) {
    *new_w = W;
    *new_h = H;
    if (fit == BCNN_HIP_IMAGE_FIT_LETTERBOX) {
        if ((float)W / iw < (float)H / ih) {
            *new_h = (int)(((long long)ih * W) / iw);
        } else {
            *new_w = (int)(((long long)iw * H) / ih);
        }
    }
    return *new_w >= 1 && *new_h >= 1 && *new_w <= W && *new_h <= H;
}

size_t stage_taps(uint8_t* stage, size_t tap_at, ImageDesc& d) {
    d.tapx_off = (uint32_t)tap_at;
    int2* tx = reinterpret_cast<int2*>(stage + tap_at);
    const float xs = bip_resize_scale((size_t)d.w, (size_t)d.new_w), ys = bip_resize_scale((size_t)d.h, (size_t)d.new_h);
    for (int x = 0; x < d.new_w; ++x) bip_resize_tap((size_t)x, xs, (size_t)d.w, &tx[x].x, &tx[x].y);
    d.tapy_off = (uint32_t)(tap_at + (size_t)d.new_w * sizeof(int2));
    int2* ty = reinterpret_cast<int2*>(stage + d.tapy_off);
    for (int y = 0; y < d.new_h; ++y) bip_resize_tap((size_t)y, ys, (size_t)d.h, &ty[y].x, &ty[y].y);
    return ((size_t)d.new_w + d.new_h) * sizeof(int2);
}

size_t stage_geometry(uint8_t* stage, size_t tap_at, ImageDesc& d, int fit, int W, int H, int iw, int ih) {
    d.w = iw;
    d.h = ih;
    fitted_extent(fit, W, H, iw, ih, &d.new_w, &d.new_h);
    d.x_off = (W - d.new_w) / 2;
    d.y_off = (H - d.new_h) / 2;
    return stage_taps(stage, tap_at, d);
}

bool fill_grid(int W, int H, int num_images, int* runs_per_row, int* blocks_per_image, long long* blocks) {
    *runs_per_row = ceil_div(W, kRun);
    *blocks_per_image = ceil_div((long long)*runs_per_row * H, kFillBlock);
    *blocks = (long long)*blocks_per_image * num_images;
    return *blocks <= 0x7fffffff;
}

void launch_fill_images(const uint8_t* stage_d, float* dst_d, int c, int H, int W, int num_images, float norm_coeff,
                        int swap_to_bgr, float mean_r, float mean_g, float mean_b, hipStream_t st) {
    FillParams p;
    long long blocks;
    fill_grid(W, H, num_images, &p.runs_per_row, &p.blocks_per_image, &blocks);
    const float m[3] = {mean_r, mean_g, mean_b};
    p.swap = (swap_to_bgr && c == 3) ? 1 : 0;
    for (int k = 0; k < 4; ++k) p.mean[k] = (c == 3 && k < 3) ? m[p.swap ? 2 - k : k] : m[0];
    p.norm = norm_coeff;
    p.H = H;
    p.W = W;
    const dim3 grid((unsigned)blocks);
    switch (c) {
        case 1: fill_images_kernel<1><<<grid, kFillBlock, 0, st>>>(stage_d, dst_d, p); break;
        case 2: fill_images_kernel<2><<<grid, kFillBlock, 0, st>>>(stage_d, dst_d, p); break;
        case 3: fill_images_kernel<3><<<grid, kFillBlock, 0, st>>>(stage_d, dst_d, p); break;
        default: fill_images_kernel<4><<<grid, kFillBlock, 0, st>>>(stage_d, dst_d, p); break;
    }
    KERNEL_CHECK();
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_fill_images(float* dst_d, int n, int c, int h, int w, int num_images, const uint8_t* const* images,
                         const int* widths, const int* heights, const int* strides, int fit, float norm_coeff,
                         int swap_to_bgr, float mean_r, float mean_g, float mean_b) {
    if (!dst_d || !images || !widths || !heights || n < 1 || h < 1 || w < 1 || c < 1 || c > 4 || num_images < 1 ||
        num_images > n || (fit != BCNN_HIP_IMAGE_FIT_STRETCH && fit != BCNN_HIP_IMAGE_FIT_LETTERBOX))
        return 1;
    // ---- every refusal comes before anything is staged or queued
    size_t pixels = 0;
    for (int b = 0; b < num_images; ++b) {
        if (!images[b] || widths[b] < 1 || heights[b] < 1) return 1;
        const long long row = (long long)widths[b] * c;
        if (row > 0x7fffffff || (strides && strides[b] < row)) return 1;
        int new_w, new_h;
        if (!fitted_extent(fit, w, h, widths[b], heights[b], &new_w, &new_h)) return 1;
        pixels += align_up((size_t)row * heights[b], 16);
        if (pixels > (size_t)0x7fffffff) return 1;
    }
    // the staging block: [descriptors][tap tables, room for W + H taps per image][pixels]; its offsets are 32-bit
    const size_t desc_bytes = align_up((size_t)num_images * sizeof(ImageDesc), 16);
    const size_t taps = (size_t)num_images * ((size_t)w + h) * sizeof(int2);
    const size_t total = desc_bytes + taps + pixels;
    int runs_per_row, blocks_per_image;
    long long blocks;
    if (total > (size_t)0x7fffffff || !fill_grid(w, h, num_images, &runs_per_row, &blocks_per_image, &blocks)) return 1;

    uint8_t* stage = host_stage(STAGE_IMAGES, total);
    ImageDesc* desc = reinterpret_cast<ImageDesc*>(stage);
    size_t tap_at = desc_bytes, pix_at = desc_bytes + taps;
    for (int b = 0; b < num_images; ++b) {
        const int iw = widths[b], ih = heights[b];
        ImageDesc& d = desc[b];
        tap_at += stage_geometry(stage, tap_at, d, fit, w, h, iw, ih);
        d.data_off = (uint32_t)pix_at;
        const size_t row = (size_t)iw * c, stride = strides ? (size_t)strides[b] : row;
        if (stride == row) {
            memcpy(stage + pix_at, images[b], row * ih);
        } else {
            for (int y = 0; y < ih; ++y) memcpy(stage + pix_at + y * row, images[b] + y * stride, row);
        }
        pix_at += align_up(row * ih, 16);
    }
    // ---- one copy, one launch
    hipStream_t st = current_stream();
    uint8_t* stage_d = stage_upload(STAGE_IMAGES, SCRATCH_IMAGES, total, total, st);
    launch_fill_images(stage_d, dst_d, c, h, w, num_images, norm_coeff, swap_to_bgr, mean_r, mean_g, mean_b, st);
    return 0;
}

}  // extern "C"
