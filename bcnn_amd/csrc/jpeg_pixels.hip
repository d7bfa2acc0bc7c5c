// jpeg_pixels.hip -- the input tensor of a batch from JPEG streams whose entropy decoding the host has done: the pixel
// stage of the decoder on the device. The host (libbcnn.so + libbip.so) leaves every image's dequantised int16 coefficient
// blocks in the pinned staging block; ONE copy sends descriptors, tap tables and coefficients up, THREE kernels follow:
//   jpeg_idct_kernel    coefficient blocks -> uint8 component planes (8 lanes per 8 x 8 block)
//   jpeg_colour_kernel  planes -> interleaved uint8 pixels: chroma upsampling + Y Cb Cr -> R G B (a lane per 8 pixels)
//   fill_images_kernel  pixels -> float NCHW tensor: resize / letterbox / conversion (image_fill.hip, unchanged)
// Planes and pixels live behind the uploaded part of the same device block (SCRATCH_IMAGES), so the fill kernel's
// offsets need no second base; decoded pixels never exist on the host. The arithmetic of the first two kernels is the
// host decoder's own (../host/bip_jpeg_pixels.h): integer, per block / per sample, so the bytes are the host's.
#include "common.h"

#include <cstdint>
#include <cstring>

#include "../host/bip_jpeg_pixels.h"
#include "image_fill.h"
#include "jpeg_pixels.h"

namespace bcnn_hip {
namespace {

constexpr int kIdctThreads = 256, kIdctBlocks = kIdctThreads / 8;   // 8 x 8 blocks per workgroup
constexpr int kTilePitch = 9;                                       // words per tile row: 8 + 1, no bank conflicts
constexpr int kColourThreads = 256, kColourRun = 8;

// One component plane of one image. Blocks first_block .. next record's first_block - 1 of the grid are its
// idct_w x idct_h transformed blocks, row by row; the table ends with a record that only holds the total.
struct JpegPlane {
    uint32_t first_block;
    uint32_t coeff_off, plane_off;   // bytes from the device block's first byte, both multiples of 16
    int idct_w, blocks_w, pitch;
};

struct JpegComp { uint32_t plane_off; int pitch, hs, vs, w_lores, rows; };   // rows: with content
// One image. Runs first_run .. next record's first_run - 1 are its rows of runs_per_row runs of 8 pixels.
struct JpegImage {
    uint32_t first_run, pix_off;
    int width, height, ncomp, runs_per_row;
    JpegComp comp[3];
};

// Index of the last record whose `first` is <= id; first[0] == 0 and first[count] is the total, id < total.
template <class T, uint32_t T::*first>
__device__ int find_record(const T* __restrict__ table, int count, uint32_t id) {
    int lo = 0, hi = count;   // table[lo].first <= id < table[hi].first
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].*first <= id) lo = mid; else hi = mid;
    }
    return lo;
}

// Eight lanes per block. Lane r loads row r of the coefficients (16 bytes); lane x runs the column pass of column x;
// lane y runs the row pass of row y and stores its 8 bytes. The two exchanges go through LDS tiles of 8 rows of 9 words.
__global__ __launch_bounds__(kIdctThreads) void jpeg_idct_kernel(uint8_t* __restrict__ stage, uint32_t planes_off,
                                                                 int num_planes, uint32_t total_blocks) {
    __shared__ int32_t coef[kIdctBlocks][8 * kTilePitch];
    __shared__ int32_t midt[kIdctBlocks][8 * kTilePitch];
    const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const uint32_t g = blockIdx.x * (uint32_t)kIdctBlocks + slot;
    const bool live = g < total_blocks;
    JpegPlane pl = {};
    int bx = 0, by = 0;
    if (live) {
        const JpegPlane* __restrict__ table = reinterpret_cast<const JpegPlane*>(stage + planes_off);
        pl = table[find_record<JpegPlane, &JpegPlane::first_block>(table, num_planes, g)];
        const uint32_t local = g - pl.first_block;
        by = (int)(local / (uint32_t)pl.idct_w);
        bx = (int)(local - (uint32_t)by * pl.idct_w);
        const int4 v = *reinterpret_cast<const int4*>(stage + pl.coeff_off + ((size_t)by * pl.blocks_w + bx) * 128 + lane * 16);
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            coef[slot][lane * kTilePitch + 2 * j] = (int16_t)(w[j] & 0xffff);
            coef[slot][lane * kTilePitch + 2 * j + 1] = (int16_t)(w[j] >> 16);
        }
    }
    __syncthreads();
    if (live) {
        int16_t c[8];
        int32_t mid[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = (int16_t)coef[slot][k * kTilePitch + lane];
        bip_jpeg_idct_column(c, 1, mid);
#pragma unroll
        for (int y = 0; y < 8; ++y) midt[slot][y * kTilePitch + lane] = mid[y];
    }
    __syncthreads();
    if (live) {
        int32_t m[8];
        uint8_t row[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = midt[slot][lane * kTilePitch + j];
        bip_jpeg_idct_row(m, row);
        uint2 out;
        out.x = row[0] | (row[1] << 8) | (row[2] << 16) | ((uint32_t)row[3] << 24);
        out.y = row[4] | (row[5] << 8) | (row[6] << 16) | ((uint32_t)row[7] << 24);
        *reinterpret_cast<uint2*>(stage + pl.plane_off + ((size_t)by * 8 + lane) * pl.pitch + bx * 8) = out;
    }
}

// A lane owns 8 consecutive pixels of one row of one image.
__global__ __launch_bounds__(kColourThreads) void jpeg_colour_kernel(uint8_t* __restrict__ stage, uint32_t images_off,
                                                                     int num_images, uint32_t total_runs) {
    const uint32_t r = blockIdx.x * (uint32_t)kColourThreads + threadIdx.x;
    if (r >= total_runs) return;
    const JpegImage* __restrict__ table = reinterpret_cast<const JpegImage*>(stage + images_off);
    const JpegImage& im = table[find_record<JpegImage, &JpegImage::first_run>(table, num_images, r)];
    const uint32_t local = r - im.first_run;
    const int y = (int)(local / (uint32_t)im.runs_per_row);
    const int x0 = (int)(local - (uint32_t)y * im.runs_per_row) * kColourRun;
    const int width = im.width, ncomp = im.ncomp;
    const int len = min(kColourRun, width - x0);
    uint8_t s[3][kColourRun];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= ncomp) break;
        const JpegComp c = im.comp[k];
        int near_row, far_row;
        bip_jpeg_up_source_rows(y, c.vs, c.rows, &near_row, &far_row);
        const uint8_t* __restrict__ nr = stage + c.plane_off + (size_t)near_row * c.pitch;
        const uint8_t* __restrict__ fr = stage + c.plane_off + (size_t)far_row * c.pitch;
        if (c.hs == 1 && c.vs == 1) {   // full resolution: the 8 samples are 8 aligned bytes inside the plane's pitch
            const uint2 v = *reinterpret_cast<const uint2*>(nr + x0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[k][j] = (uint8_t)(v.x >> (8 * j));
                s[k][4 + j] = (uint8_t)(v.y >> (8 * j));
            }
        } else {
#pragma unroll
            for (int j = 0; j < kColourRun; ++j)
                s[k][j] = j < len ? bip_jpeg_up_sample(nr, fr, c.w_lores, c.hs, c.vs, x0 + j) : (uint8_t)0;
        }
    }
    uint8_t* __restrict__ out = stage + im.pix_off + ((size_t)y * width + x0) * ncomp;
    if (ncomp == 3) {
        uint8_t px[3 * kColourRun];
#pragma unroll
        for (int j = 0; j < kColourRun; ++j) bip_jpeg_ycc_to_rgb(s[0][j], s[1][j], s[2][j], px + 3 * j);
        if (len == kColourRun && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(out);
#pragma unroll
            for (int q = 0; q < 6; ++q)
                o4[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | ((uint32_t)px[4 * q + 3] << 24);
        } else {
            for (int j = 0; j < 3 * len; ++j) out[j] = px[j];
        }
    } else {
        if (len == kColourRun && (reinterpret_cast<uintptr_t>(out) & 7) == 0) {
            uint2 v;
            v.x = s[0][0] | (s[0][1] << 8) | (s[0][2] << 16) | ((uint32_t)s[0][3] << 24);
            v.y = s[0][4] | (s[0][5] << 8) | (s[0][6] << 16) | ((uint32_t)s[0][7] << 24);
            *reinterpret_cast<uint2*>(out) = v;
        } else {
            for (int j = 0; j < len; ++j) out[j] = s[0][j];
        }
    }
}

// What bcnn_hip_jpeg_stage_begin laid out for this thread in the block of STAGE_IMAGES, until _run or _cancel.
struct Pending {
    bool active = false;
    int device;                           // where _begin took the block, and the block's generation then: _run refuses
    uint64_t generation;                  // when another call has taken it since
    int c, h, w;
    size_t upload, total;                 // bytes copied up / of the whole device block
    uint32_t planes_off, images_off;
    JpegCursor cur;                       // behind the last image: the totals
};
thread_local Pending g_pending;

}  // namespace

// A frame the kernels can run on without leaving its planes: what bip_jpeg_frame_info reports, checked again here
// because every bound of the two kernels follows from these numbers.
bool jpeg_frame_ok(const bcnn_hip_jpeg_frame& f, int c) {
    if (f.ncomp != c || (c != 1 && c != 3) || f.width < 1 || f.height < 1 || f.hmax < 1 || f.hmax > 4 || f.vmax < 1 ||
        f.vmax > 4 || (long long)f.width * f.height * c > (1ll << 30))
        return false;
    for (int k = 0; k < c; ++k) {
        const bcnn_hip_jpeg_component& p = f.comp[k];
        if (p.h < 1 || p.v < 1 || f.hmax % p.h || f.vmax % p.v) return false;
        const int hs = f.hmax / p.h, vs = f.vmax / p.v;
        if (p.blocks_w < 1 || p.blocks_h < 1 || p.blocks_w > (1 << 16) || p.blocks_h > (1 << 16) ||
            p.pitch != 8 * p.blocks_w || p.rows != 8 * p.blocks_h || p.idct_w < 1 || p.idct_h < 1 ||
            p.idct_w > p.blocks_w || p.idct_h > p.blocks_h)
            return false;
        // the samples the colour kernel reads: columns 0 .. ceil(width / hs) - 1 (rounded up to 8 for a full-resolution
        // component), rows 0 .. height - 1 of the content, all of them inside the transformed blocks
        const int w_lores = (f.width + hs - 1) / hs;
        if (p.width != w_lores || p.height != (f.height + vs - 1) / vs || p.height < 1 || w_lores > 8 * p.idct_w ||
            p.height > 8 * p.idct_h)
            return false;
    }
    return true;
}

JpegFrameSize jpeg_frame_size(const bcnn_hip_jpeg_frame& f, int c) {
    JpegFrameSize s = {0, 0, align_up((size_t)f.width * f.height * c, 16), 0,
                       (unsigned long long)ceil_div(f.width, kColourRun) * f.height};
    for (int k = 0; k < c; ++k) {
        const bcnn_hip_jpeg_component& p = f.comp[k];
        s.coeff += (size_t)p.blocks_w * p.blocks_h * 128;
        s.planes += (size_t)p.pitch * p.rows;
        s.blocks += (unsigned long long)p.idct_w * p.idct_h;
    }
    return s;
}

size_t jpeg_plane_table_bytes(int num_planes) { return align_up(((size_t)num_planes + 1) * sizeof(JpegPlane), 16); }
size_t jpeg_image_table_bytes(int num_images) { return align_up(((size_t)num_images + 1) * sizeof(JpegImage), 16); }

void jpeg_append_image(uint8_t* stage, size_t planes_at, size_t images_at, const bcnn_hip_jpeg_frame& f, int c,
                       JpegCursor& cur) {
    JpegPlane* plane = reinterpret_cast<JpegPlane*>(stage + planes_at);
    JpegImage& im = reinterpret_cast<JpegImage*>(stage + images_at)[cur.images];
    memset(&im, 0, sizeof(im));
    im.first_run = cur.run_at;
    im.pix_off = (uint32_t)cur.pixel_at;
    im.width = f.width;
    im.height = f.height;
    im.ncomp = c;
    im.runs_per_row = ceil_div(f.width, kColourRun);
    for (int k = 0; k < c; ++k) {
        const bcnn_hip_jpeg_component& p = f.comp[k];
        JpegPlane& pl = plane[cur.planes++];
        pl.first_block = cur.block_at;
        pl.coeff_off = (uint32_t)cur.coeff_at;
        pl.plane_off = (uint32_t)cur.plane_at;
        pl.idct_w = p.idct_w;
        pl.blocks_w = p.blocks_w;
        pl.pitch = p.pitch;
        im.comp[k].plane_off = (uint32_t)cur.plane_at;
        im.comp[k].pitch = p.pitch;
        im.comp[k].hs = f.hmax / p.h;
        im.comp[k].vs = f.vmax / p.v;
        im.comp[k].w_lores = p.width;
        im.comp[k].rows = p.height;
        cur.block_at += (uint32_t)(p.idct_w * p.idct_h);
        cur.coeff_at += (size_t)p.blocks_w * p.blocks_h * 128;
        cur.plane_at += (size_t)p.pitch * p.rows;
    }
    cur.run_at += (uint32_t)(im.runs_per_row * f.height);
    cur.pixel_at += align_up((size_t)f.width * f.height * c, 16);
    ++cur.images;
}

void jpeg_close_tables(uint8_t* stage, size_t planes_at, size_t images_at, const JpegCursor& cur) {
    JpegPlane& pl = reinterpret_cast<JpegPlane*>(stage + planes_at)[cur.planes];
    memset(&pl, 0, sizeof(JpegPlane));
    pl.first_block = cur.block_at;
    JpegImage& im = reinterpret_cast<JpegImage*>(stage + images_at)[cur.images];
    memset(&im, 0, sizeof(JpegImage));
    im.first_run = cur.run_at;
}

void launch_jpeg_pixels(uint8_t* stage_d, uint32_t planes_off, uint32_t images_off, const JpegCursor& cur, hipStream_t st) {
    if (cur.images < 1) return;
    jpeg_idct_kernel<<<dim3((unsigned)ceil_div(cur.block_at, kIdctBlocks)), kIdctThreads, 0, st>>>(
        stage_d, planes_off, cur.planes, cur.block_at);
    KERNEL_CHECK();
    jpeg_colour_kernel<<<dim3((unsigned)ceil_div(cur.run_at, kColourThreads)), kColourThreads, 0, st>>>(
        stage_d, images_off, cur.images, cur.run_at);
    KERNEL_CHECK();
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_jpeg_stage_begin(int n, int c, int h, int w, int num_images, const bcnn_hip_jpeg_frame* frames, int fit,
                              int16_t** coeff, int* failed_image) {
    if (failed_image) *failed_image = -1;
    g_pending.active = false;
    if (!frames || !coeff || n < 1 || h < 1 || w < 1 || (c != 1 && c != 3) || num_images < 1 || num_images > n ||
        (fit != BCNN_HIP_IMAGE_FIT_STRETCH && fit != BCNN_HIP_IMAGE_FIT_LETTERBOX))
        return 1;
    // ---- every refusal comes before anything is staged
    size_t coeff_bytes = 0, plane_bytes = 0, pixel_bytes = 0;
    unsigned long long blocks = 0, runs = 0;
    for (int b = 0; b < num_images; ++b) {
        const bcnn_hip_jpeg_frame& f = frames[b];
        int new_w, new_h;
        if (!jpeg_frame_ok(f, c) || !fitted_extent(fit, w, h, f.width, f.height, &new_w, &new_h)) {
            if (failed_image) *failed_image = b;
            return 1;
        }
        const JpegFrameSize s = jpeg_frame_size(f, c);
        coeff_bytes += s.coeff;
        plane_bytes += s.planes;
        pixel_bytes += s.pixels;
        blocks += s.blocks;
        runs += s.runs;
        if (coeff_bytes + plane_bytes + pixel_bytes > (size_t)0x7fffffff) {
            if (failed_image) *failed_image = b;
            return 1;
        }
    }
    // the device block: [image records][tap tables, room for W + H taps per image][plane table][image table]
    // [coefficients] -- so far it is the pinned block too and goes up -- [planes][pixels]; its offsets are 32-bit
    const size_t desc_bytes = align_up((size_t)num_images * sizeof(ImageDesc), 16);
    const size_t taps = align_up((size_t)num_images * ((size_t)w + h) * sizeof(int2), 16);
    const size_t planes_at = desc_bytes + taps;
    const size_t images_at = planes_at + jpeg_plane_table_bytes(num_images * c);
    const size_t coeff_at = images_at + jpeg_image_table_bytes(num_images);
    const size_t upload = coeff_at + coeff_bytes, total = upload + plane_bytes + pixel_bytes;
    int runs_per_row, blocks_per_image;
    long long fill_blocks;
    if (total > (size_t)0x7fffffff || blocks > 0x7fffffffull || runs > 0x7fffffffull ||
        !fill_grid(w, h, num_images, &runs_per_row, &blocks_per_image, &fill_blocks)) {
        if (failed_image) *failed_image = num_images - 1;
        return 1;
    }

    uint8_t* stage = host_stage(STAGE_IMAGES, upload);
    ImageDesc* desc = reinterpret_cast<ImageDesc*>(stage);
    size_t tap_at = desc_bytes;
    JpegCursor cur = {coeff_at, upload, upload + plane_bytes, 0, 0, 0, 0};
    for (int b = 0; b < num_images; ++b) {
        const bcnn_hip_jpeg_frame& f = frames[b];
        tap_at += stage_geometry(stage, tap_at, desc[b], fit, w, h, f.width, f.height);
        desc[b].data_off = (uint32_t)cur.pixel_at;
        coeff[b] = reinterpret_cast<int16_t*>(stage + cur.coeff_at);
        jpeg_append_image(stage, planes_at, images_at, f, c, cur);
    }
    jpeg_close_tables(stage, planes_at, images_at, cur);

    Pending& q = g_pending;
    q.active = true;
    q.device = current_device();
    q.generation = stage_generation(STAGE_IMAGES);
    q.c = c; q.h = h; q.w = w;
    q.upload = upload; q.total = total;
    q.planes_off = (uint32_t)planes_at; q.images_off = (uint32_t)images_at;
    q.cur = cur;
    return 0;
}

void bcnn_hip_jpeg_stage_cancel(void) { g_pending.active = false; }

int bcnn_hip_jpeg_stage_run(float* dst_d, float norm_coeff, int swap_to_bgr, float mean_r, float mean_g, float mean_b) {
    Pending& q = g_pending;
    if (!q.active || !dst_d) return 1;
    q.active = false;
    if (current_device() != q.device || stage_generation(STAGE_IMAGES) != q.generation) return 1;  // the block is another call's
    // ---- one copy, three launches
    hipStream_t st = current_stream();
    uint8_t* stage_d = stage_upload(STAGE_IMAGES, SCRATCH_IMAGES, q.upload, q.total, st);
    launch_jpeg_pixels(stage_d, q.planes_off, q.images_off, q.cur, st);
    launch_fill_images(stage_d, dst_d, q.c, q.h, q.w, q.cur.images, norm_coeff, swap_to_bgr, mean_r, mean_g, mean_b, st);
    return 0;
}

}  // extern "C"
