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
//
// bcnn_hip_augment_jpeg_begin / _run / _cancel make the same batch when some samples are still
// JPEG coefficient blocks: the two kernels of jpeg_pixels.hip decode them behind the uploaded part of the block, and the
// windowed form of the geometry kernel reads every sample through an AugWindow, which is the list loaders' crop to the
// net input. One copy, at most four launches.
//
// bcnn_hip_augment_letterbox_batch makes it when every sample is a decoded image of its own size:
// augment_letterbox_kernel resizes each (bip_resize_bilinear's rule, taps tabulated on the host side of the entry) and
// pastes it on a canvas of 128 behind the uploaded part of the block; the canvases are the raw samples of the two kernels
// above. One copy, three launches.
//
// bcnn_hip_augment_effects_begin / _cancel stage Perlin distortion and random spotlights for the
// next of the three batch calls above, which copies the staged tables into its block (still one copy) and launches
// augment_convert_effects_kernel in place of the convert kernel. cos and exp were called on the host; the kernel's
// arithmetic is ../host/bip_effects.h, which libbip's host functions are written on as well.
#include "common.h"

#include <cstdint>
#include <cstring>

#include <vector>

#include "../host/bip_effects.h"
#include "../host/bip_resize_tap.h"
#include "image_fill.h"
#include "jpeg_pixels.h"
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
    uint32_t win_off;                             // the window table of the windowed geometry kernel
    uint32_t fx_off;                              // the staged effects (FxHeader); 0: none, the plain convert kernel runs
};

// What bcnn_hip_augment_effects_begin lays out and a batch call copies into its block at fx_off, 16-byte aligned:
// [FxHeader][FxSample per sample][FxSpot per spot][per sample with DISTORT: norm_x, norm_y, weight_x, weight_y (floats),
// cell_x, cell_y (int32)][the spots' tables]. Offsets count from the header's first byte.
struct FxHeader { uint32_t spot_off, pad[3]; };
struct FxSample {
    int32_t flags, seed;
    float distortion;
    int32_t first_spot, num_spots;
    uint32_t perlin_off;
};
struct FxSpot { int32_t x0, y0, bw, bh; uint32_t table_off; };

// Where the windowed geometry kernel finds one sample's raw bytes: a wi x hi image at `base` (bytes from the block's first
// byte), of which the sample is the w x h window at (x_ul, y_ul). Outside the image the sample is 0: bip_crop_image onto
// the loader's zeroed buffer.
struct AugWindow { uint32_t base; int wi, hi, x_ul, y_ul; };

// One sample as the stages see it
struct Sample {
    const uint8_t* __restrict__ px;
    const int2* __restrict__ tapx;
    const int2* __restrict__ tapy;
    int w, h, flags, x_ul, y_ul;
    int wi, hi, wx, wy;   // kWin: the image behind px and the window's origin in it
};

// The raw byte of sample pixel (x, y): dense w x h samples, or (kWin) the window of the decoded image. The window sits
// below the flip, so every stage above sees the cropped sample.
template <int C, bool kWin>
__device__ __forceinline__ int32_t raw(const Sample& s, int x, int y, int k) {
    if constexpr (kWin) {
        const long long X = (long long)x + s.wx, Y = (long long)y + s.wy;
        return (X >= 0 && X < s.wi && Y >= 0 && Y < s.hi) ? s.px[((size_t)Y * s.wi + (size_t)X) * C + k] : 0;
    } else {
        return s.px[((size_t)y * s.w + x) * C + k];
    }
}
template <int C, bool kWin>
__device__ __forceinline__ int32_t flipped(const Sample& s, int x, int y, int k) {
    if (s.flags & BCNN_HIP_AUG_FLIP) x = s.w - 1 - x;
    return raw<C, kWin>(s, x, y, k);
}
template <int C, bool kWin>
__device__ __forceinline__ int32_t shifted(const Sample& s, int x, int y, int k) {
    if (!(s.flags & BCNN_HIP_AUG_SHIFT)) return flipped<C, kWin>(s, x, y, k);
    const long long X = (long long)x + s.x_ul, Y = (long long)y + s.y_ul;
    return (X >= 0 && X < s.w && Y >= 0 && Y < s.h) ? flipped<C, kWin>(s, (int)X, (int)Y, k) : kCanvas;
}
template <int C, bool kWin>
__device__ __forceinline__ int32_t scaled(const Sample& s, int x, int y, int k) {
    if (s.flags & BCNN_HIP_AUG_SCALE) {
        const int2 tx = s.tapx[x], ty = s.tapy[y];
        if (tx.x >= 0 && ty.x >= 0) {  // covered by the resized image
            const int x1 = tx.x + (s.w > 1 ? 1 : 0), y1 = ty.x + (s.h > 1 ? 1 : 0);
            return bip_resize_blend(shifted<C, kWin>(s, tx.x, ty.x, k), shifted<C, kWin>(s, x1, ty.x, k),
                                    shifted<C, kWin>(s, tx.x, y1, k), shifted<C, kWin>(s, x1, y1, k), tx.y, ty.y);
        }
    }
    return shifted<C, kWin>(s, x, y, k);
}

// Stages 1 to 4 of every pixel of the batch -> s4, and the channel sums the contrast stage needs. A lane per pixel.
// kWin (bcnn_hip_augment_jpeg_run): the raw bytes of sample b are a window of the image its AugWindow names -- the crop
// of a list image to the net input is this read, not a pass of its own.
template <int C, bool kWin = false>
__global__ __launch_bounds__(kAugBlock) void augment_geometry_kernel(uint8_t* __restrict__ block, AugParams p) {
    const int b = blockIdx.x / p.blocks_per_sample;
    const int pix = (blockIdx.x - b * p.blocks_per_sample) * kAugBlock + threadIdx.x;
    const bcnn_hip_augment_record r = reinterpret_cast<const bcnn_hip_augment_record*>(block + p.rec_off)[b];
    const size_t sample_bytes = (size_t)p.sw * p.sh * C;
    Sample s;
    if constexpr (kWin) {
        const AugWindow win = reinterpret_cast<const AugWindow*>(block + p.win_off)[b];
        s.px = block + win.base;
        s.wi = win.wi;
        s.hi = win.hi;
        s.wx = win.x_ul;
        s.wy = win.y_ul;
    } else {
        s.px = block + p.pix_off + b * sample_bytes;
    }
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
                    const float p00 = (float)scaled<C, kWin>(s, mx, my, k), p01 = (float)scaled<C, kWin>(s, mx + 1, my, k);
                    const float p10 = (float)scaled<C, kWin>(s, mx, my + 1, k);
                    const float p11 = (float)scaled<C, kWin>(s, mx + 1, my + 1, k);
                    const float level = p00 * (1 - fx) * (1 - fy) + p01 * (fx) * (1 - fy) + p10 * (1 - fx) * (fy) +
                                        p11 * (fx) * (fy);
                    sum[k] = (uint8_t)level;
                }
            }  // else 0
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) sum[k] = (uint32_t)scaled<C, kWin>(s, x, y, k);
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

// bcnn_hip_augment_letterbox_batch: a source image of the batch is an ImageDesc (image_fill.h) whose plane is the canvas.
struct LetterboxParams {
    uint32_t desc_off, canvas_off;  // the ImageDescs; the canvases, dense W x H x C each (AugParams::pix_off)
    int W, H;
    int chunks_per_row, blocks_per_sample;
};
constexpr int kChunk = 16;  // canvas bytes per lane: one 16-byte store

// The canvases of the whole batch: 128, and the resized image where it is pasted. A lane owns the part of one canvas row
// that falls into one 16-byte-aligned chunk of the block, so every chunk inside a row goes out as one aligned 16-byte
// store and only the two chunks a row shares with its neighbours are written byte by byte. Integer work only.
template <int C>
__global__ __launch_bounds__(kAugBlock) void augment_letterbox_kernel(uint8_t* __restrict__ block, LetterboxParams p) {
    const int b = blockIdx.x / p.blocks_per_sample;
    const int lane = (blockIdx.x - b * p.blocks_per_sample) * kAugBlock + threadIdx.x;
    const int y = lane / p.chunks_per_row;
    if (y >= p.H) return;
    const int row_bytes = p.W * C;
    const uint32_t row_at = p.canvas_off + (uint32_t)(((size_t)b * p.H + y) * row_bytes);  // below 2 GiB: checked
    const uint32_t chunk_at = (row_at & ~(uint32_t)(kChunk - 1)) + (uint32_t)(lane - y * p.chunks_per_row) * kChunk;
    // bytes [first, last) of the chunk belong to this row; q0 is the row byte of the chunk's byte 0 (may be negative)
    const int q0 = (int)chunk_at - (int)row_at;
    const int first = q0 < 0 ? -q0 : 0, last = min(kChunk, row_bytes - q0);
    if (first >= last) return;
    const ImageDesc d = reinterpret_cast<const ImageDesc*>(block + p.desc_off)[b];
    uint32_t word[kChunk / 4];
#pragma unroll
    for (int i = 0; i < kChunk / 4; ++i) word[i] = 0x01010101u * kCanvas;
    const int yr = y - d.y_off;
    if (yr >= 0 && yr < d.new_h) {
        const int2 ty = reinterpret_cast<const int2*>(block + d.tapy_off)[yr];  // the row's tap, once
        const int2* __restrict__ tapx = reinterpret_cast<const int2*>(block + d.tapx_off);
        const size_t src_row = (size_t)d.w * C;
        const uint8_t* __restrict__ r0 = block + d.data_off + (size_t)ty.x * src_row;
        const uint8_t* __restrict__ r1 = r0 + (d.h > 1 ? src_row : 0);  // a one-row source replicates
        const int step = d.w > 1 ? C : 0;                               // and so does a one-column source
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            const int q = q0 + i;
            if (i < first || i >= last) continue;
            const int x = q / C, k = q - x * C, xr = x - d.x_off;
            if (xr < 0 || xr >= d.new_w) continue;
            const int2 tx = tapx[xr];
            const int at = tx.x * C + k;
            const uint32_t v = bip_resize_blend(r0[at], r0[at + step], r1[at], r1[at + step], tx.y, ty.y);
            word[i / 4] = (word[i / 4] & ~(0xffu << (8 * (i % 4)))) | (v << (8 * (i % 4)));
        }
    }
    uint8_t* __restrict__ out = block + chunk_at;
    if (first == 0 && last == kChunk) {
        *reinterpret_cast<uint4*>(out) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (int i = 0; i < kChunk; ++i)
            if (i >= first && i < last) out[i] = (uint8_t)(word[i / 4] >> (8 * (i % 4)));
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

// The convert kernel of a batch with staged effects (bcnn_hip_augment_effects_begin): stages 5 to 8 of the kernel above
// with Perlin distortion and the spotlights between brightness and crop, in the same pass and with no further image.
// Contrast and brightness are pointwise functions of a rotated byte given the channel sums, so a distorted pixel is the
// reference's four-tap blend of tone(s4[tap]), and the spots are a pointwise chain on top of it. A lane keeps its kRun
// destination pixels and store_run's 16-byte stores; its taps are a byte gather that stays within a few rows of one sample
// (the noise moves a position by at most distortion x extent), which the cache holds. Every table value was made on the
// host with libm; the arithmetic here is bip_effects.h's, uncontracted: no cos, no exp, no division. A sample without a
// flag takes the plain path.
template <int C>
__global__ __launch_bounds__(kAugBlock) void augment_convert_effects_kernel(const uint8_t* __restrict__ block,
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
    const uint8_t* __restrict__ fx = block + p.fx_off;
    const FxSample f = reinterpret_cast<const FxSample*>(fx + sizeof(FxHeader))[b];
    const uint8_t* __restrict__ s4 = block + p.s4_off + (size_t)b * p.sh * p.sw * C;
    const int sy = y + p.cy, sx0 = x0 + p.cx;   // the run in sample coordinates
    int32_t mean[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int ks = (C == 3 && p.swap) ? 2 - k : k;
        mean[k] = contrast ? (int32_t)(sums[ks] / (uint32_t)(p.sw * p.sh)) : 0;
    }
    auto tone = [&](int32_t px, int k) {   // stages 5 and 6 of one byte of channel plane k
        if (contrast) px = clamp_u8((((px - mean[k]) * r.gain + (1 << 11)) >> 12) + mean[k]);
        return clamp_u8(px + r.brightness);
    };
    int32_t v8[C][kRun];
    if (f.flags & BCNN_HIP_AUG_DISTORT) {
        const float* __restrict__ norm_x = reinterpret_cast<const float*>(fx + f.perlin_off);
        const float* __restrict__ norm_y = norm_x + p.sw;
        const float* __restrict__ weight_x = norm_y + p.sh;
        const float* __restrict__ weight_y = weight_x + p.sw;
        const int32_t* __restrict__ cell_x = reinterpret_cast<const int32_t*>(weight_y + p.sh);
        const int32_t* __restrict__ cell_y = cell_x + p.sw;
        const float ny = norm_y[sy], wy = weight_y[sy], fw = (float)p.sw, fh = (float)p.sh;
        const int32_t cy = cell_y[sy];
#pragma unroll
        for (int j = 0; j < kRun; ++j) {
#pragma unroll
            for (int k = 0; k < C; ++k) v8[k][j] = 0;
            if (j >= len) continue;
            const int sx = sx0 + j;
            const float noise = bip_perlin_noise(cell_x[sx], cy, weight_x[sx], wy, f.seed);
            int32_t ix, iy;
            float xd, yd;
            if (!bip_distort_map(norm_x[sx], ny, noise, f.distortion, fw, fh, p.sw, p.sh, &ix, &iy, &xd, &yd)) continue;  // 0
            const uint8_t* __restrict__ t0 = s4 + ((size_t)iy * p.sw + ix) * C;   // ix <= sw - 2, iy <= sh - 2
            const uint8_t* __restrict__ t1 = t0 + (size_t)p.sw * C;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int ks = (C == 3 && p.swap) ? 2 - k : k;
                v8[k][j] = bip_distort_blend((float)tone(t0[ks], k), (float)tone(t0[C + ks], k), (float)tone(t1[ks], k),
                                             (float)tone(t1[C + ks], k), xd, yd);
            }
        }
    } else {
        const uint8_t* __restrict__ row = s4 + ((size_t)sy * p.sw + sx0) * C;
#pragma unroll
        for (int j = 0; j < kRun; ++j) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int ks = (C == 3 && p.swap) ? 2 - k : k;
                v8[k][j] = j < len ? tone(row[j * C + ks], k) : 0;
            }
        }
    }
    if (f.flags & BCNN_HIP_AUG_SPOTS) {   // one after the other: the result of spot i is the input of spot i + 1
        const FxSpot* __restrict__ spots =
            reinterpret_cast<const FxSpot*>(fx + reinterpret_cast<const FxHeader*>(fx)->spot_off) + f.first_spot;
        for (int s = 0; s < f.num_spots; ++s) {
            const FxSpot q = spots[s];
            const int ry = sy - q.y0;
            if (ry < 0 || ry >= q.bh) continue;
            const float* __restrict__ tab = reinterpret_cast<const float*>(fx + q.table_off) + (size_t)ry * q.bw;
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                const int rx = sx0 + j - q.x0;
                if (j >= len || rx < 0 || rx >= q.bw) continue;
                const float val = tab[rx];
#pragma unroll
                for (int k = 0; k < C; ++k) v8[k][j] = bip_spot_add(val, (uint8_t)v8[k][j]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        float v[kRun];
#pragma unroll
        for (int j = 0; j < kRun; ++j) v[j] = ((float)v8[k][j] - 127.5f) * (1 / 127.5f);
        store_run(dst + (((size_t)b * C + k) * p.H + y) * p.W + x0, v, len);
    }
}

// Every entry point below stages its batch in the pinned block of STAGE_AUGMENT (common.h) and sends it up with stage_upload.

// What bcnn_hip_augment_effects_begin staged for this thread's next batch call: the blob that goes into that call's block
// as it is (FxHeader ...), and the batch it was made for.
struct PendingFx {
    bool active = false;
    int num = 0, w = 0, h = 0;
    std::vector<uint8_t> blob;
};
thread_local PendingFx g_fx;

// Every batch call begins with this: what is staged is consumed, whatever the call returns. Bytes of the blob (a multiple
// of 16), 0 when nothing is staged; `mismatch` when it was staged for another batch, which the call then refuses.
size_t take_effects(int num, int w, int h, bool& mismatch) {
    PendingFx& f = g_fx;
    mismatch = false;
    if (!f.active) return 0;
    f.active = false;
    mismatch = f.num != num || f.w != w || f.h != h;
    return mismatch ? 0 : f.blob.size();
}

template <int C, bool kWin = false>
void launch(uint8_t* block_d, float* dst_d, AugParams p, int num, hipStream_t st) {
    p.blocks_per_sample = ceil_div((long long)p.sw * p.sh, kAugBlock);
    augment_geometry_kernel<C, kWin><<<dim3((unsigned)(p.blocks_per_sample * num)), kAugBlock, 0, st>>>(block_d, p);
    KERNEL_CHECK();
    p.runs_per_row = ceil_div(p.W, kRun);
    p.blocks_per_sample = ceil_div((long long)p.runs_per_row * p.H, kAugBlock);
    const dim3 grid((unsigned)(p.blocks_per_sample * num));
    if (p.fx_off) augment_convert_effects_kernel<C><<<grid, kAugBlock, 0, st>>>(block_d, dst_d, p);
    else augment_convert_kernel<C><<<grid, kAugBlock, 0, st>>>(block_d, dst_d, p);
    KERNEL_CHECK();
}

// Every tap index of the samples that scale lies in [-1, max(extent - 2, 0)]: the four reads of the blend stay inside.
bool taps_in_range(const bcnn_hip_augment_record* records, const int32_t* taps, size_t num, int src_w, int src_h) {
    const size_t sample_taps = (size_t)src_w + src_h;
    for (size_t b = 0; b < num; ++b) {
        if (!(records[b].flags & BCNN_HIP_AUG_SCALE)) continue;
        const int32_t* t = taps + b * sample_taps * 2;
        for (size_t i = 0; i < sample_taps; ++i) {
            const int extent = i < (size_t)src_w ? src_w : src_h;
            if (t[2 * i] < -1 || t[2 * i] > (extent >= 2 ? extent - 2 : 0)) return false;
        }
    }
    return true;
}

// What bcnn_hip_augment_jpeg_begin laid out for this thread, until _run or _cancel. Upload part of the block:
// [records][channel sums][taps][windows][plane table][image table][coefficients of every candidate][raw samples of the
// host-decoded ones, as many as _run finds]; behind `device_at`, on the device only: [planes][pixels][rotated samples].
struct PendingJpeg {
    bool active = false;
    uint8_t* stage;
    int device;            // where _begin took the block, and the block's generation then: _run refuses when another
    uint64_t generation;   // call has taken it since (`stage` may point into freed memory)
    int c, h, w, num;
    size_t sum_off, tap_off, win_off, planes_at, images_at, raw_at, device_at, plane_bytes, pixel_bytes, total;
    std::vector<uint32_t> coeff_off;   // per sample; 0: not a candidate
    std::vector<bcnn_hip_jpeg_frame> frames;
};
thread_local PendingJpeg g_jpeg;

}  // namespace
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_augment_batch(float* dst_d, int n, int c, int h, int w, int num_samples, int src_w, int src_h,
                           const uint8_t* pixels, const bcnn_hip_augment_record* records, const int32_t* taps,
                           int swap_to_bgr) {
    bool fx_mismatch;
    const size_t fx_bytes = take_effects(num_samples, src_w, src_h, fx_mismatch);
    if (fx_mismatch) return 1;
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
    const size_t plain = rec_bytes + sum_bytes + tap_bytes + pix_bytes;
    const size_t fx_at = fx_bytes ? align_up(plain, 16) : 0, total = fx_bytes ? fx_at + fx_bytes : plain;
    if (total + pix_bytes > (size_t)0x7fffffff) return 1;
    if (any_scale && !taps_in_range(records, taps, num, src_w, src_h)) return 1;

    // the staging block: [records][channel sums, zero][taps][pixels][staged effects]; behind it on the device, the rotated
    // samples
    uint8_t* stage = host_stage(STAGE_AUGMENT, total);
    AugParams p;
    p.rec_off = 0;
    p.sum_off = (uint32_t)rec_bytes;
    p.tap_off = (uint32_t)(rec_bytes + sum_bytes);
    p.pix_off = (uint32_t)(rec_bytes + sum_bytes + tap_bytes);
    p.s4_off = (uint32_t)total;
    p.fx_off = (uint32_t)fx_at;
    if (fx_bytes) memcpy(stage + fx_at, g_fx.blob.data(), fx_bytes);
    memcpy(stage, records, num * sizeof(bcnn_hip_augment_record));
    memset(stage + p.sum_off, 0, sum_bytes);
    if (any_scale) memcpy(stage + p.tap_off, taps, tap_bytes);
    memcpy(stage + p.pix_off, pixels, num * sample_bytes);
    if (!any_scale)  // no tap table was staged: no record may ask for one
        for (size_t b = 0; b < num; ++b) reinterpret_cast<bcnn_hip_augment_record*>(stage)[b].flags &= ~BCNN_HIP_AUG_SCALE;

    // ---- one copy, two launches
    hipStream_t st = current_stream();
    uint8_t* block_d = stage_upload(STAGE_AUGMENT, SCRATCH_AUGMENT, total, total + pix_bytes, st);

    p.sw = src_w;
    p.sh = src_h;
    p.H = h;
    p.W = w;
    p.cx = (src_w - w) / 2;
    p.cy = (src_h - h) / 2;
    p.swap = (swap_to_bgr && c == 3) ? 1 : 0;
    p.blocks_per_sample = p.runs_per_row = 0;
    p.win_off = 0;
    switch (c) {
        case 1: launch<1>(block_d, dst_d, p, num_samples, st); break;
        case 2: launch<2>(block_d, dst_d, p, num_samples, st); break;
        case 3: launch<3>(block_d, dst_d, p, num_samples, st); break;
        default: launch<4>(block_d, dst_d, p, num_samples, st); break;
    }
    return 0;
}

int bcnn_hip_augment_letterbox_batch(float* dst_d, int n, int c, int h, int w, int num_samples,
                                     const bcnn_hip_letterbox_image* images, const bcnn_hip_augment_record* records,
                                     const int32_t* taps, int swap_to_bgr) {
    bool fx_mismatch;
    const size_t fx_bytes = take_effects(num_samples, w, h, fx_mismatch);
    if (fx_mismatch) return 1;
    if (!dst_d || !images || !records || n < 1 || h < 1 || w < 1 || c < 1 || c > 4 || num_samples < 1 || num_samples > n ||
        (long long)w * h > 0x7fffffff / (c * (long long)num_samples))
        return 1;
    // ---- every refusal comes before anything is staged or queued
    const size_t num = (size_t)num_samples, sample_bytes = (size_t)w * h * c, sample_taps = (size_t)w + h;
    bool any_scale = false;
    size_t lb_tap_bytes = 0, src_bytes = 0;
    for (size_t b = 0; b < num; ++b) {
        const bcnn_hip_letterbox_image& im = images[b];
        if (!im.pixels || im.w < 1 || im.h < 1 || im.new_w < 1 || im.new_w > w || im.new_h < 1 || im.new_h > h ||
            im.x_off < 0 || im.x_off > w - im.new_w || im.y_off < 0 || im.y_off > h - im.new_h ||
            (long long)im.w * im.h > 0x7fffffff / c)
            return 1;
        any_scale = any_scale || (records[b].flags & BCNN_HIP_AUG_SCALE);
        lb_tap_bytes += ((size_t)im.new_w + im.new_h) * sizeof(int2);
        src_bytes += align_up((size_t)im.w * im.h * c, 16);
        if (src_bytes > (size_t)0x7fffffff) return 1;
    }
    if (any_scale && !taps) return 1;
    const size_t rec_bytes = align_up(num * sizeof(bcnn_hip_augment_record), 16), sum_bytes = num * 4 * sizeof(uint32_t);
    const size_t tap_bytes = any_scale ? align_up(num * sample_taps * 2 * sizeof(int32_t), 16) : 0;
    const size_t desc_bytes = align_up(num * sizeof(ImageDesc), 16);
    const size_t canvas_bytes = align_up(num * sample_bytes, 16);
    const size_t desc_at = rec_bytes + sum_bytes + tap_bytes, lb_tap_at = desc_at + desc_bytes;
    const size_t src_at = lb_tap_at + align_up(lb_tap_bytes, 16), fx_at = src_at + src_bytes, total = fx_at + fx_bytes;
    if (total + 2 * canvas_bytes > (size_t)0x7fffffff) return 1;
    if (any_scale && !taps_in_range(records, taps, num, w, h)) return 1;

    // the staging block: [records][channel sums, zero][augmentation taps][descriptors][letterbox taps][source pixels]
    // [staged effects]; behind it on the device, the canvases and the rotated samples
    uint8_t* stage = host_stage(STAGE_AUGMENT, total);
    if (fx_bytes) memcpy(stage + fx_at, g_fx.blob.data(), fx_bytes);
    memcpy(stage, records, num * sizeof(bcnn_hip_augment_record));
    memset(stage + rec_bytes, 0, sum_bytes);
    if (any_scale) memcpy(stage + rec_bytes + sum_bytes, taps, num * sample_taps * 2 * sizeof(int32_t));
    else  // no tap table was staged: no record may ask for one
        for (size_t b = 0; b < num; ++b) reinterpret_cast<bcnn_hip_augment_record*>(stage)[b].flags &= ~BCNN_HIP_AUG_SCALE;
    ImageDesc* desc = reinterpret_cast<ImageDesc*>(stage + desc_at);
    size_t tap_at = lb_tap_at, pix_at = src_at;
    for (size_t b = 0; b < num; ++b) {
        const bcnn_hip_letterbox_image& im = images[b];
        ImageDesc& d = desc[b];
        d.w = im.w; d.h = im.h; d.new_w = im.new_w; d.new_h = im.new_h; d.x_off = im.x_off; d.y_off = im.y_off;
        tap_at += stage_taps(stage, tap_at, d);
        d.data_off = (uint32_t)pix_at;
        memcpy(stage + pix_at, im.pixels, (size_t)im.w * im.h * c);
        pix_at += align_up((size_t)im.w * im.h * c, 16);
    }

    // ---- one copy, three launches
    hipStream_t st = current_stream();
    uint8_t* block_d = stage_upload(STAGE_AUGMENT, SCRATCH_AUGMENT, total, total + 2 * canvas_bytes, st);

    LetterboxParams lp;
    lp.desc_off = (uint32_t)desc_at;
    lp.canvas_off = (uint32_t)total;
    lp.W = w;
    lp.H = h;
    lp.chunks_per_row = (w * c + 2 * (kChunk - 1)) / kChunk;  // a row may begin and end inside a chunk
    lp.blocks_per_sample = ceil_div((long long)lp.chunks_per_row * h, kAugBlock);
    const dim3 grid((unsigned)(lp.blocks_per_sample * num_samples));
    switch (c) {
        case 1: augment_letterbox_kernel<1><<<grid, kAugBlock, 0, st>>>(block_d, lp); break;
        case 2: augment_letterbox_kernel<2><<<grid, kAugBlock, 0, st>>>(block_d, lp); break;
        case 3: augment_letterbox_kernel<3><<<grid, kAugBlock, 0, st>>>(block_d, lp); break;
        default: augment_letterbox_kernel<4><<<grid, kAugBlock, 0, st>>>(block_d, lp); break;
    }
    KERNEL_CHECK();

    AugParams p;
    p.rec_off = 0;
    p.sum_off = (uint32_t)rec_bytes;
    p.tap_off = (uint32_t)(rec_bytes + sum_bytes);
    p.pix_off = (uint32_t)total;
    p.s4_off = (uint32_t)(total + canvas_bytes);
    p.sw = p.W = w;
    p.sh = p.H = h;
    p.cx = p.cy = 0;
    p.swap = (swap_to_bgr && c == 3) ? 1 : 0;
    p.blocks_per_sample = p.runs_per_row = 0;
    p.win_off = 0;
    p.fx_off = fx_bytes ? (uint32_t)fx_at : 0;
    switch (c) {
        case 1: launch<1>(block_d, dst_d, p, num_samples, st); break;
        case 2: launch<2>(block_d, dst_d, p, num_samples, st); break;
        case 3: launch<3>(block_d, dst_d, p, num_samples, st); break;
        default: launch<4>(block_d, dst_d, p, num_samples, st); break;
    }
    return 0;
}

int bcnn_hip_augment_jpeg_begin(int n, int c, int h, int w, int num_samples, const bcnn_hip_jpeg_frame* frames,
                                int16_t** coeff) {
    PendingJpeg& q = g_jpeg;
    q.active = false;
    if (!frames || !coeff || n < 1 || h < 1 || w < 1 || (c != 1 && c != 3) || num_samples < 1 || num_samples > n ||
        (long long)w * h > 0x7fffffff / (c * (long long)num_samples))
        return 1;
    // ---- every refusal comes before anything is staged
    const size_t num = (size_t)num_samples, sample_bytes = (size_t)w * h * c;
    size_t coeff_bytes = 0, plane_bytes = 0, pixel_bytes = 0;
    unsigned long long blocks = 0, runs = 0;
    int candidates = 0;
    for (size_t b = 0; b < num; ++b) {
        coeff[b] = nullptr;
        if (frames[b].ncomp == 0 || !jpeg_frame_ok(frames[b], c)) continue;   // the caller decodes this one
        const JpegFrameSize s = jpeg_frame_size(frames[b], c);
        coeff_bytes += s.coeff;
        plane_bytes += s.planes;
        pixel_bytes += s.pixels;
        blocks += s.blocks;
        runs += s.runs;
        ++candidates;
        if (coeff_bytes + plane_bytes + pixel_bytes > (size_t)0x7fffffff) return 1;
    }
    if (candidates == 0) return 1;
    const size_t rec_bytes = align_up(num * sizeof(bcnn_hip_augment_record), 16), sum_bytes = num * 4 * sizeof(uint32_t);
    const size_t tap_bytes = align_up(num * ((size_t)w + h) * 2 * sizeof(int32_t), 16);
    const size_t win_bytes = align_up(num * sizeof(AugWindow), 16), raw_bytes = align_up(num * sample_bytes, 16);
    q.sum_off = rec_bytes;
    q.tap_off = q.sum_off + sum_bytes;
    q.win_off = q.tap_off + tap_bytes;
    q.planes_at = q.win_off + win_bytes;
    q.images_at = q.planes_at + jpeg_plane_table_bytes(candidates * c);
    const size_t coeff_at = q.images_at + jpeg_image_table_bytes(candidates);
    q.raw_at = coeff_at + coeff_bytes;
    q.device_at = q.raw_at + raw_bytes;
    q.plane_bytes = plane_bytes;
    q.pixel_bytes = pixel_bytes;
    q.total = q.device_at + plane_bytes + pixel_bytes + raw_bytes;
    if (q.total > (size_t)0x7fffffff || blocks > 0x7fffffffull || runs > 0x7fffffffull) return 1;

    q.stage = host_stage(STAGE_AUGMENT, q.device_at);
    q.device = current_device();
    q.generation = stage_generation(STAGE_AUGMENT);
    q.coeff_off.assign(num, 0);
    q.frames.assign(frames, frames + num);
    size_t c_at = coeff_at;
    for (size_t b = 0; b < num; ++b) {
        if (frames[b].ncomp == 0 || !jpeg_frame_ok(frames[b], c)) continue;
        q.coeff_off[b] = (uint32_t)c_at;
        coeff[b] = reinterpret_cast<int16_t*>(q.stage + c_at);
        c_at += jpeg_frame_size(frames[b], c).coeff;
    }
    q.c = c; q.h = h; q.w = w; q.num = num_samples;
    q.active = true;
    return 0;
}

void bcnn_hip_augment_jpeg_cancel(void) { g_jpeg.active = false; }

int bcnn_hip_augment_effects_begin(int num_samples, int src_w, int src_h, const bcnn_hip_augment_effect* effects,
                                   const float* perlin, const int32_t* cells, const bcnn_hip_augment_spot* spots,
                                   int num_spots, const float* spot_tables, size_t num_table_floats) {
    PendingFx& q = g_fx;
    q.active = false;
    if (!effects || num_samples < 1 || src_w < 1 || src_h < 1 || num_spots < 0 || (num_spots > 0 && (!spots || !spot_tables)))
        return 1;
    // ---- every refusal comes before anything is staged
    const size_t num = (size_t)num_samples, axis = (size_t)src_w + src_h;
    size_t distorted = 0;
    for (size_t b = 0; b < num; ++b) {
        const bcnn_hip_augment_effect& e = effects[b];
        if (e.flags & ~(BCNN_HIP_AUG_DISTORT | BCNN_HIP_AUG_SPOTS)) return 1;
        if (e.flags & BCNN_HIP_AUG_DISTORT) {
            if (!perlin || !cells || !(e.distortion >= -3.4028234e38f && e.distortion <= 3.4028234e38f)) return 1;
            ++distorted;
        }
        if ((e.flags & BCNN_HIP_AUG_SPOTS) &&
            (e.first_spot < 0 || e.num_spots < 0 || e.first_spot > num_spots || e.num_spots > num_spots - e.first_spot))
            return 1;
    }
    for (int s = 0; s < num_spots; ++s) {   // the box inside the sample, the table inside spot_tables
        const bcnn_hip_augment_spot& t = spots[s];
        if (t.x0 < 0 || t.y0 < 0 || t.bw < 1 || t.bh < 1 || t.bw > src_w - t.x0 || t.bh > src_h - t.y0 ||
            t.table > num_table_floats || (size_t)t.bw * t.bh > num_table_floats - t.table)
            return 1;
    }
    if (num_table_floats > (size_t)0x7fffffff / sizeof(float) || axis > (size_t)0x7fffffff / (12 * num)) return 1;
    const size_t sample_at = sizeof(FxHeader), spot_at = sample_at + align_up(num * sizeof(FxSample), 16);
    const size_t perlin_at = spot_at + align_up((size_t)num_spots * sizeof(FxSpot), 16);
    const size_t table_at = perlin_at + align_up(distorted * axis * 12, 16);
    const size_t total = table_at + align_up(num_table_floats * sizeof(float), 16);
    if (total > (size_t)0x7fffffff) return 1;

    q.blob.assign(total, 0);
    uint8_t* blob = q.blob.data();
    reinterpret_cast<FxHeader*>(blob)->spot_off = (uint32_t)spot_at;
    FxSample* fs = reinterpret_cast<FxSample*>(blob + sample_at);
    size_t at = perlin_at;
    for (size_t b = 0; b < num; ++b) {
        const bcnn_hip_augment_effect& e = effects[b];
        fs[b].flags = e.flags;
        if (e.flags & BCNN_HIP_AUG_DISTORT) {   // norm and weight (columns, rows), then the cells
            fs[b].seed = e.seed;
            fs[b].distortion = e.distortion;
            fs[b].perlin_off = (uint32_t)at;
            memcpy(blob + at, perlin + b * axis * 2, axis * 2 * sizeof(float));
            memcpy(blob + at + axis * 2 * sizeof(float), cells + b * axis, axis * sizeof(int32_t));
            at += axis * 12;
        }
        if (e.flags & BCNN_HIP_AUG_SPOTS) {
            fs[b].first_spot = e.first_spot;
            fs[b].num_spots = e.num_spots;
        }
    }
    FxSpot* sp = reinterpret_cast<FxSpot*>(blob + spot_at);
    for (int s = 0; s < num_spots; ++s) {
        const FxSpot v = {spots[s].x0, spots[s].y0, spots[s].bw, spots[s].bh,
                          (uint32_t)(table_at + (size_t)spots[s].table * sizeof(float))};
        sp[s] = v;
    }
    if (num_table_floats) memcpy(blob + table_at, spot_tables, num_table_floats * sizeof(float));
    q.num = num_samples;
    q.w = src_w;
    q.h = src_h;
    q.active = true;
    return 0;
}

void bcnn_hip_augment_effects_cancel(void) { g_fx.active = false; }

int bcnn_hip_augment_jpeg_run(float* dst_d, const uint8_t* decoded, const uint8_t* pixels,
                              const bcnn_hip_augment_record* records, const int32_t* taps, const int32_t* origins,
                              int swap_to_bgr) {
    PendingJpeg& q = g_jpeg;
    bool fx_mismatch;
    const size_t fx_bytes = take_effects(q.active ? q.num : 0, q.active ? q.w : 0, q.active ? q.h : 0, fx_mismatch);
    if (!q.active) return 1;
    q.active = false;
    if (current_device() != q.device || stage_generation(STAGE_AUGMENT) != q.generation) return 1;  // the block is another call's
    if (fx_mismatch || !dst_d || !decoded || !pixels || !records || !origins) return 1;
    const size_t num = (size_t)q.num, sample_bytes = (size_t)q.w * q.h * q.c, sample_taps = (size_t)q.w + q.h;
    bool any_scale = false;
    for (size_t b = 0; b < num; ++b) {
        if (decoded[b] && q.coeff_off[b] == 0) return 1;
        any_scale = any_scale || (records[b].flags & BCNN_HIP_AUG_SCALE);
    }
    if (any_scale && (!taps || !taps_in_range(records, taps, num, q.w, q.h))) return 1;
    // staged effects go behind the upload part _begin laid out, and the device-only part moves back by as much
    const size_t fx_at = fx_bytes ? align_up(q.device_at, 16) : 0, device_at = fx_bytes ? fx_at + fx_bytes : q.device_at;
    const size_t total = q.total + (device_at - q.device_at);
    if (total > (size_t)0x7fffffff) return 1;

    uint8_t* stage = q.stage;
    if (fx_bytes) {
        stage = q.stage = host_stage_extend(STAGE_AUGMENT, q.device_at, fx_at + fx_bytes);
        memcpy(stage + fx_at, g_fx.blob.data(), fx_bytes);
    }
    memcpy(stage, records, num * sizeof(bcnn_hip_augment_record));
    memset(stage + q.sum_off, 0, num * 4 * sizeof(uint32_t));
    if (any_scale) memcpy(stage + q.tap_off, taps, num * sample_taps * 2 * sizeof(int32_t));
    else  // the tap table holds nothing: no record may ask for it
        for (size_t b = 0; b < num; ++b) reinterpret_cast<bcnn_hip_augment_record*>(stage)[b].flags &= ~BCNN_HIP_AUG_SCALE;
    AugWindow* win = reinterpret_cast<AugWindow*>(stage + q.win_off);
    JpegCursor cur = {0, device_at, device_at + q.plane_bytes, 0, 0, 0, 0};
    size_t raw_at = q.raw_at;
    for (size_t b = 0; b < num; ++b) {
        if (decoded[b]) {   // a window of the image the colour kernel leaves at cur.pixel_at
            const bcnn_hip_jpeg_frame& f = q.frames[b];
            const AugWindow v = {(uint32_t)cur.pixel_at, f.width, f.height, origins[2 * b], origins[2 * b + 1]};
            win[b] = v;
            cur.coeff_at = q.coeff_off[b];
            jpeg_append_image(stage, q.planes_at, q.images_at, f, q.c, cur);
        } else {            // the caller's cropped sample, whole
            const AugWindow v = {(uint32_t)raw_at, q.w, q.h, 0, 0};
            win[b] = v;
            memcpy(stage + raw_at, pixels + b * sample_bytes, sample_bytes);
            raw_at += sample_bytes;
        }
    }
    jpeg_close_tables(stage, q.planes_at, q.images_at, cur);

    // ---- one copy, four launches
    hipStream_t st = current_stream();
    uint8_t* block_d = stage_upload(STAGE_AUGMENT, SCRATCH_AUGMENT, fx_bytes ? fx_at + fx_bytes : raw_at, total, st);
    launch_jpeg_pixels(block_d, (uint32_t)q.planes_at, (uint32_t)q.images_at, cur, st);

    AugParams p;
    p.rec_off = 0;
    p.sum_off = (uint32_t)q.sum_off;
    p.tap_off = (uint32_t)q.tap_off;
    p.pix_off = 0;
    p.win_off = (uint32_t)q.win_off;
    p.s4_off = (uint32_t)(device_at + q.plane_bytes + q.pixel_bytes);
    p.fx_off = (uint32_t)fx_at;
    p.sw = p.W = q.w;
    p.sh = p.H = q.h;
    p.cx = p.cy = 0;
    p.swap = (swap_to_bgr && q.c == 3) ? 1 : 0;
    p.blocks_per_sample = p.runs_per_row = 0;
    if (q.c == 1) launch<1, true>(block_d, dst_d, p, q.num, st);
    else launch<3, true>(block_d, dst_d, p, q.num, st);
    return 0;
}

}  // extern "C"
