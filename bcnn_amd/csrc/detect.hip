// detect.hip -- the graph nodes a Darknet detector (yolov3-tiny) needs besides convolution / batch-norm / pooling:
// concat ([route]), nearest-neighbour upsample and the activation of the YOLOv3 head. All three are copies or single
// adds, HBM-bound; every kernel moves 16 bytes per access where the alignment of the slice allows it.
#include "common.h"

namespace bcnn_hip {

// ---- concat ---------------------------------------------------------------------------------------------------------
// Reference bcnn_concat_layer.c:113-146: per image j, source i occupies dst[j * dst_sz + off_i, + src_sz_i). Here one
// launch covers every (source, image) slice: blockIdx.y = slice, the x dimension strides over the slice's elements.
constexpr int kConcatMax = 16;  // sources per launch (more: the host side splits the table)
struct ConcatTable {
    const float* src[kConcatMax];  // forward: source data; backward: unused
    float* grad[kConcatMax];       // backward: source gradients (never NULL inside a table)
    int size[kConcatMax];          // size3d of the source
    int offset[kConcatMax];        // its channel-slice offset inside one image of dst (floats)
};

// one slice copy / add: dst[k] (op)= src[k], k < n. 16-byte accesses when src and dst share their alignment mod 16
// (scalar head up to the first aligned element, scalar tail); otherwise scalar throughout. ADD: dst[k] = dst[k] + src[k].
template <bool ADD>
__device__ __forceinline__ void slice_op(const float* __restrict__ src, float* __restrict__ dst, size_t n, size_t t0,
                                         size_t nt) {
    const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
    if (((as ^ ad) & 15) == 0) {
        size_t head = ((16 - (ad & 15)) & 15) / 4;
        if (head > n) head = n;
        if (t0 < head) dst[t0] = ADD ? dst[t0] + src[t0] : src[t0];
        const size_t nv = (n - head) / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src + head);
        float4* d4 = reinterpret_cast<float4*>(dst + head);
        for (size_t v = t0; v < nv; v += nt) {
            float4 x = s4[v];
            if (ADD) {
                const float4 y = d4[v];
                x.x = y.x + x.x; x.y = y.y + x.y; x.z = y.z + x.z; x.w = y.w + x.w;
            }
            d4[v] = x;
        }
        const size_t k = head + nv * 4 + t0;
        if (k < n) dst[k] = ADD ? dst[k] + src[k] : src[k];
    } else {
        for (size_t k = t0; k < n; k += nt) dst[k] = ADD ? dst[k] + src[k] : src[k];
    }
}

__global__ __launch_bounds__(256) void concat_fwd_kernel(ConcatTable tab, int nsrc, float* __restrict__ dst,
                                                         int dst_size) {
    const int i = blockIdx.y % nsrc, j = blockIdx.y / nsrc;
    const size_t n = (size_t)tab.size[i];
    slice_op<false>(tab.src[i] + (size_t)j * n, dst + (size_t)j * dst_size + tab.offset[i], n,
                    (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void concat_bwd_kernel(ConcatTable tab, int nsrc, const float* __restrict__ dgrad,
                                                         int dst_size) {
    const int i = blockIdx.y % nsrc, j = blockIdx.y / nsrc;
    const size_t n = (size_t)tab.size[i];
    slice_op<true>(dgrad + (size_t)j * dst_size + tab.offset[i], tab.grad[i] + (size_t)j * n, n,
                   (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// x blocks for slices of up to max_size floats: one float4 per lane, capped (the kernels stride)
static int concat_grid_x(int max_size, int slices) {
    int gx = ceil_div((long long)max_size, 4 * 256);
    const int cap = (kCUs * STREAM_GRID_PER_CU * 4 + slices - 1) / slices;
    if (gx > cap) gx = cap;
    return gx < 1 ? 1 : gx;
}

// ---- upsample (nearest neighbour, integer factor s) -------------------------------------------------------------------
// Reference bcnn_upsample_layer.c:84-110 (forward), :120-147 (backward, the CPU code: a serial += over the output in
// row-major order). Planes = n * c; source plane h x w, output plane (h s) x (w s).

// s == 2, even w: a lane owns two neighbouring source elements (float2) and writes their 2 x 4 output block as two
// float4 stores (output rows 2y and 2y + 1, columns 4 * (x / 2) ..).
__global__ __launch_bounds__(256) void upsample2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int w,
                                                            size_t pairs) {
    const int wp = w >> 1;
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < pairs; t += gs) {
        const size_t row = t / (unsigned)wp;  // plane * h + yrow
        const int xp = (int)(t - row * wp);
        const float2 v = reinterpret_cast<const float2*>(x)[t];
        const float4 o = make_float4(v.x, v.x, v.y, v.y);
        float4* out = reinterpret_cast<float4*>(y + row * 4 * (size_t)w) + xp;  // row 2 yrow of the plane
        out[0] = o;
        out[wp] = o;                                                           // row 2 yrow + 1 (2 w floats on)
    }
}

// any s, any w: a lane per source element, its s x s block stored row by row
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int w,
                                                           int s, size_t total) {
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    const size_t ow = (size_t)w * s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gs) {
        const size_t row = t / (unsigned)w;
        const int xc = (int)(t - row * w);
        const float v = x[t];
        float* out = y + row * s * ow + (size_t)xc * s;
        for (int r = 0; r < s; ++r)
            for (int c = 0; c < s; ++c) out[r * ow + c] = v;
    }
}

// Backward is a gather: a lane owns dx elements and adds its s x s dy block in the order the reference's serial loop
// reaches them -- start from the current dx, rows top to bottom, left to right within a row -- so every dx is the same
// chain of float additions as there (bit-exact, deterministic, no atomics).
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(float* __restrict__ dx, const float* __restrict__ dy, int w,
                                                            size_t pairs) {
    const int wp = w >> 1;
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < pairs; t += gs) {
        const size_t row = t / (unsigned)wp;
        const int xp = (int)(t - row * wp);
        const float4* in = reinterpret_cast<const float4*>(dy + row * 4 * (size_t)w) + xp;
        const float4 a = in[0], b = in[wp];
        float2 g = reinterpret_cast<float2*>(dx)[t];
        g.x = g.x + a.x; g.x = g.x + a.y; g.x = g.x + b.x; g.x = g.x + b.y;
        g.y = g.y + a.z; g.y = g.y + a.w; g.y = g.y + b.z; g.y = g.y + b.w;
        reinterpret_cast<float2*>(dx)[t] = g;
    }
}

__global__ __launch_bounds__(256) void upsample_bwd_kernel(float* __restrict__ dx, const float* __restrict__ dy, int w,
                                                           int s, size_t total) {
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    const size_t ow = (size_t)w * s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gs) {
        const size_t row = t / (unsigned)w;
        const int xc = (int)(t - row * w);
        const float* in = dy + row * s * ow + (size_t)xc * s;
        float g = dx[t];
        for (int r = 0; r < s; ++r)
            for (int c = 0; c < s; ++c) g = g + in[r * ow + c];
        dx[t] = g;
    }
}

// ---- YOLOv3 head ----------------------------------------------------------------------------------------------------
// Reference bcnn_yolo.c:417-440: y = x, then the logistic over entries [0, 2) and [coords, coords + classes + 1) of every
// box (entry_index, :207-215: channel = box * (coords + classes + 1) + entry). The two ranges are applied one after the
// other there, so an entry in both (coords < 2) gets the function twice; so it does here.
__device__ __forceinline__ float yolo_entry(float v, int ch, int per_box, int coords) {
    const int e = ch % per_box;
    if (e < 2) v = act_fwd(v, BCNN_HIP_ACT_LOGISTIC, 0.f);
    if (e >= coords) v = act_fwd(v, BCNN_HIP_ACT_LOGISTIC, 0.f);
    return v;
}

__global__ __launch_bounds__(256) void yolo_activate_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            int hw, int channels, int per_box, int coords,
                                                            size_t total, int vec) {
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    if (vec) {  // x, y 16-byte aligned: four consecutive elements per lane (they may straddle two channels)
        const size_t nv = total / 4;
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nv; t += gs) {
            float4 v = reinterpret_cast<const float4*>(x)[t];
            const size_t k = t * 4;
            v.x = yolo_entry(v.x, (int)((k / hw) % channels), per_box, coords);
            v.y = yolo_entry(v.y, (int)(((k + 1) / hw) % channels), per_box, coords);
            v.z = yolo_entry(v.z, (int)(((k + 2) / hw) % channels), per_box, coords);
            v.w = yolo_entry(v.w, (int)(((k + 3) / hw) % channels), per_box, coords);
            reinterpret_cast<float4*>(y)[t] = v;
        }
        const size_t k = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (k < total) y[k] = yolo_entry(x[k], (int)((k / hw) % channels), per_box, coords);
        return;
    }
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gs)
        y[k] = yolo_entry(x[k], (int)((k / hw) % channels), per_box, coords);
}

// ---- detections of a batch ------------------------------------------------------------------------------------------
// Reference bcnn_yolo.c:470-639 (one image per call, on the host, after reading every head back). Here: one candidate
// launch and one NMS launch for the whole batch; a few thousand lanes per image, launch-bound work.
constexpr int kDetBlock = 1024;        // lanes per workgroup of both kernels (16 waves)
constexpr int kDetWaves = kDetBlock / kWave;
constexpr int kRecHead = BCNN_HIP_YOLO_RECORD_HEAD;  // x, y, w, h, objectness, candidate index; prob follows
// Boxes per image the NMS kernel holds in LDS: 16 B box + 4 B key + 4 B slot + 1 B live flag = 25 B each, 50 KB.
constexpr int kNmsCapacity = 2048;

struct YoloTable {
    bcnn_hip_yolo_head head[BCNN_HIP_YOLO_MAX_HEADS];
    int first[BCNN_HIP_YOLO_MAX_HEADS + 1];  // candidate index of a head's (cell 0, anchor 0); [nheads] = candidates per image
};

// head of candidate g, and g's index inside it (cell * num + anchor)
__device__ __forceinline__ int yolo_locate(const YoloTable& tab, int nheads, int g, int* local) {
    int k = 0;
    while (k + 1 < nheads && g >= tab.first[k + 1]) ++k;
    *local = g - tab.first[k];
    return k;
}

// entry_index of bcnn_yolo.c:207-215: image b, anchor a, entry e, cell
__device__ __forceinline__ size_t yolo_entry_index(const bcnn_hip_yolo_head& hd, int b, int a, int e, int cell) {
    const int hw = hd.h * hd.w;
    return ((size_t)(b * hd.num + a) * (hd.coords + hd.classes + 1) + e) * hw + cell;
}

__device__ __forceinline__ float yolo_objectness(const YoloTable& tab, int nheads, int b, int g) {
    int local;
    const bcnn_hip_yolo_head& hd = tab.head[yolo_locate(tab, nheads, g, &local)];
    return hd.out_d[yolo_entry_index(hd, b, local % hd.num, hd.coords, local / hd.num)];
}

// grid (chunks of kDetBlock candidates, images). A workgroup counts the survivors of the chunks in front of its own
// (objectness only: at most a few reads per lane), then ranks its own survivors by wave ballot + wave offsets.
__global__ __launch_bounds__(kDetBlock) void yolo_candidates_kernel(YoloTable tab, int nheads,
                                                                     const int4* __restrict__ geom, int in_w, int in_h,
                                                                     int netw, int neth, float thresh, int relative,
                                                                     int cap, int stride, int* __restrict__ count,
                                                                     float* __restrict__ records) {
    __shared__ int wave_before[kDetWaves], wave_own[kDetWaves];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int total = tab.first[nheads];
    const int g0 = blockIdx.x * kDetBlock;  // < total by the launch shape

    int before = 0;  // this wave's share of the survivors in [0, g0): wave-uniform
    for (int g = tid; g < g0; g += kDetBlock)
        before += __popcll(__ballot(yolo_objectness(tab, nheads, b, g) > thresh));

    const int g = g0 + tid;
    float objectness = 0.f;
    if (g < total) objectness = yolo_objectness(tab, nheads, b, g);
    const bool keep = g < total && objectness > thresh;
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) {
        wave_before[wid] = before;
        wave_own[wid] = __popcll(vote);
    }
    __syncthreads();
    int pos = 0, all = 0;
    for (int w = 0; w < kDetWaves; ++w) {
        pos += wave_before[w] + (w < wid ? wave_own[w] : 0);
        all += wave_before[w] + wave_own[w];
    }
    pos += __popcll(vote & ((1ull << lane) - 1ull));
    if (blockIdx.x == gridDim.x - 1 && tid == 0) count[b] = all;  // the true count, whatever cap is
    if (!keep || pos >= cap) return;

    int local;
    const bcnn_hip_yolo_head& hd = tab.head[yolo_locate(tab, nheads, g, &local)];
    const int a = local % hd.num, cell = local / hd.num, hw = hd.h * hd.w;
    const int row = cell / hd.w, col = cell % hd.w;
    const float* x = hd.out_d + yolo_entry_index(hd, b, a, 0, cell);
    // get_yolo_box, bcnn_yolo.c:137-145
    float bx = ((float)col + x[0]) / (float)hd.w;
    float by = ((float)row + x[hw]) / (float)hd.h;
    float bw = expf(x[2 * hw]) * hd.anchor_w[a] / (float)in_w;
    float bh = expf(x[3 * hw]) * hd.anchor_h[a] / (float)in_h;
    // correct_region_boxes, bcnn_yolo.c:99-128: the offsets are double there, the scales float
    const int4 gm = geom[b];  // w, h, new_w, new_h
    bx = (float)(((double)bx - (double)(netw - gm.z) / 2. / (double)netw) / (double)((float)gm.z / (float)netw));
    by = (float)(((double)by - (double)(neth - gm.w) / 2. / (double)neth) / (double)((float)gm.w / (float)neth));
    bw = bw * ((float)netw / (float)gm.z);
    bh = bh * ((float)neth / (float)gm.w);
    if (!relative) {
        bx = bx * (float)gm.x;
        bw = bw * (float)gm.x;
        by = by * (float)gm.y;
        bh = bh * (float)gm.y;
    }
    float* r = records + ((size_t)b * cap + pos) * stride;
    r[0] = bx;
    r[1] = by;
    r[2] = bw;
    r[3] = bh;
    r[4] = objectness;
    r[5] = __int_as_float(g);
    const float* cls = x + (size_t)(hd.coords + 1) * hw;
    for (int j = 0; j < hd.classes; ++j) {
        const float p = objectness * cls[(size_t)j * hw];
        r[kRecHead + j] = p > thresh ? p : 0.f;
    }
    for (int j = kRecHead + hd.classes; j < stride; ++j) r[j] = 0.f;
}

// overlap / box_iou of bcnn_yolo.c:15-53, operation for operation (contraction is off for this library)
__device__ __forceinline__ float yolo_overlap(float x1, float w1, float x2, float w2) {
    const float l1 = x1 - w1 / 2, l2 = x2 - w2 / 2;
    const float left = l1 > l2 ? l1 : l2;
    const float r1 = x1 + w1 / 2, r2 = x2 + w2 / 2;
    const float right = r1 < r2 ? r1 : r2;
    return right - left;
}
__device__ __forceinline__ float yolo_box_iou(float4 a, float4 b) {  // (x, y, z, w) = box (x, y, w, h)
    const float w = yolo_overlap(a.x, a.z, b.x, b.z), h = yolo_overlap(a.y, a.w, b.y, b.w);
    const float inter = (w < 0 || h < 0) ? 0 : w * h;
    return inter / (a.z * a.w + b.z * b.w - inter);
}

// (objectness descending, slot ascending): the slot order is the candidate order
__device__ __forceinline__ bool det_before(float ka, int ia, float kb, int ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// One workgroup per image. Bitonic sort of the keys on the power-of-two padding, then the greedy walk: one barrier per
// box, the lanes behind a live box i test it against the boxes j > i.
__global__ __launch_bounds__(kDetBlock) void yolo_nms_kernel(const int* __restrict__ count, int cap, int nms_cap,
                                                              int stride, float nms_thresh, int* __restrict__ order,
                                                              float* __restrict__ records) {
    __shared__ float4 box[kNmsCapacity];
    __shared__ float key[kNmsCapacity];
    __shared__ int slot[kNmsCapacity];
    __shared__ unsigned char live[kNmsCapacity];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = count[b];
    if (cnt <= 0 || cnt > cap || cnt > nms_cap) return;  // nothing to do / the pass is run again / the caller's NMS
    float* rec = records + (size_t)b * cap * stride;
    int padded = 1;
    while (padded < cnt) padded <<= 1;  // <= kNmsCapacity, a power of two: cnt <= nms_cap <= kNmsCapacity
    for (int t = tid; t < padded; t += kDetBlock) {
        key[t] = t < cnt ? rec[(size_t)t * stride + 4] : -INFINITY;
        slot[t] = t < cnt ? t : 0x7fffffff;
    }
    __syncthreads();
    for (int k = 2; k <= padded; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < padded; t += kDetBlock) {
                const int u = t ^ j;
                if (u > t) {
                    const float kt = key[t], ku = key[u];
                    const int it = slot[t], iu = slot[u];
                    const bool swap = (t & k) == 0 ? det_before(ku, iu, kt, it) : det_before(kt, it, ku, iu);
                    if (swap) {
                        key[t] = ku; key[u] = kt;
                        slot[t] = iu; slot[u] = it;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < cnt; t += kDetBlock) {
        const float* r = rec + (size_t)slot[t] * stride;
        box[t] = make_float4(r[0], r[1], r[2], r[3]);
        live[t] = key[t] != 0.f;  // do_nms_obj: a box without objectness neither suppresses nor is suppressed
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
        if (live[i]) {  // the same value in every lane: written before the barrier that ended step i - 1
            const float4 a = box[i];
            for (int j = i + 1 + tid; j < cnt; j += kDetBlock)
                if (live[j] && yolo_box_iou(a, box[j]) > nms_thresh) live[j] = 0;
        }
        __syncthreads();
    }
    for (int t = tid; t < cnt; t += kDetBlock) {
        const int s = slot[t];
        if (!live[t]) {
            float* r = rec + (size_t)s * stride;
            r[4] = 0.f;
            for (int j = kRecHead; j < stride; ++j) r[j] = 0.f;
        }
        order[(size_t)b * cap + t] = live[t] ? s : (int)(0x80000000u | (unsigned)s);
    }
}

// ---- training loss of the head ---------------------------------------------------------------------------------------
// Reference bcnn_yolo.c:250-415 (a host loop there, after a read-back of the head, in the CUDA build too). Three stages
// on the launch stream; every sum is a fixed-order tree, nothing is an atomic: the same inputs give the same bits.
constexpr int kTrainBlock = 256;
constexpr int kTruthFloats = BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS * 5;  // truth = x, y, w, h, class (coords == 4)
constexpr int kCostBlocksMax = 1024;
constexpr int kStatsPerImage = 6;  // avg_iou, avg_cat, avg_obj, recall, recall75, count

// get_yolo_box, bcnn_yolo.c:137-145: v = the four ACTIVATED box entries
__device__ __forceinline__ float4 yolo_train_box(const float v[4], int col, int row, int lw, int lh, float aw, float ah,
                                                 int in_w, int in_h) {
    float4 b;
    b.x = ((float)col + v[0]) / (float)lw;
    b.y = ((float)row + v[1]) / (float)lh;
    b.z = expf(v[2]) * aw / (float)in_w;
    b.w = expf(v[3]) * ah / (float)in_h;
    return b;
}

// the label row of image b into LDS (label_stride >= kTruthFloats floats per image)
__device__ __forceinline__ void yolo_stage_truths(float* truths, const float* __restrict__ label, int label_stride, int b) {
    for (int t = threadIdx.x; t < kTruthFloats; t += blockDim.x) truths[t] = label[(size_t)b * label_stride + t];
    __syncthreads();
}

// (a) grid (ceil(num * hw / kTrainBlock), n): a lane owns one predicted box. Writes y and EVERY element of the box's
// gradient (the reference's memset + the no-object delta), leaves the block's sum of objectness in anyobj_part.
__global__ __launch_bounds__(kTrainBlock) void yolo_train_forward_kernel(bcnn_hip_yolo_train_head hd,
                                                                         const float* __restrict__ x,
                                                                         const float* __restrict__ label,
                                                                         float* __restrict__ y, float* __restrict__ grad,
                                                                         float* __restrict__ anyobj_part) {
    __shared__ float truths[kTruthFloats];
    __shared__ float red[kTrainBlock / kWave];
    const int b = blockIdx.y, hw = hd.h * hd.w, per_box = hd.coords + hd.classes + 1;
    yolo_stage_truths(truths, label, hd.label_stride, b);
    const int p = blockIdx.x * kTrainBlock + threadIdx.x;
    float obj = 0.f;
    if (p < hd.num * hw) {
        const int a = p / hw, cell = p - a * hw;
        const size_t base = ((size_t)(b * hd.num + a) * per_box) * hw + cell;
        float v[4];
        for (int e = 0; e < 4; ++e) {  // coords == 4 (checked by the launcher)
            v[e] = yolo_entry(x[base + (size_t)e * hw], e, per_box, hd.coords);
            y[base + (size_t)e * hw] = v[e];
            grad[base + (size_t)e * hw] = 0.f;
        }
        const float4 pred = yolo_train_box(v, cell % hd.w, cell / hd.w, hd.w, hd.h, hd.biases[2 * hd.mask[a]],
                                           hd.biases[2 * hd.mask[a] + 1], hd.in_w, hd.in_h);
        float best_iou = 0.f;
        for (int t = 0; t < BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS; ++t) {
            const float* tr = truths + 5 * t;
            if (!tr[0]) break;
            const float iou = yolo_box_iou(pred, make_float4(tr[0], tr[1], tr[2], tr[3]));
            if (iou > best_iou) best_iou = iou;
        }
        obj = yolo_entry(x[base + (size_t)hd.coords * hw], hd.coords, per_box, hd.coords);
        y[base + (size_t)hd.coords * hw] = obj;
        grad[base + (size_t)hd.coords * hw] = best_iou > 0.5f ? 0.f : obj;
        for (int e = hd.coords + 1; e < per_box; ++e) {
            y[base + (size_t)e * hw] = yolo_entry(x[base + (size_t)e * hw], e, per_box, hd.coords);
            grad[base + (size_t)e * hw] = 0.f;
        }
    }
    const float s = block_sum(obj, red);
    if (threadIdx.x == 0) anyobj_part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// (b) grid n, one wave per image: the truths of the image IN ORDER (two truths of one (cell, anchor) overwrite each
// other's deltas, and delta_yolo_class branches on what the earlier one left). Every lane follows the same control flow;
// lane 0 writes the box / objectness deltas and keeps the statistics, the lanes run over the classes.
__global__ __launch_bounds__(kWave) void yolo_train_truths_kernel(bcnn_hip_yolo_train_head hd,
                                                                  const float* __restrict__ label,
                                                                  const float* __restrict__ y, float* grad,
                                                                  float* __restrict__ stats_part) {
    __shared__ float truths[kTruthFloats];
    const int b = blockIdx.x, lane = threadIdx.x, hw = hd.h * hd.w, per_box = hd.coords + hd.classes + 1;
    yolo_stage_truths(truths, label, hd.label_stride, b);
    float avg_iou = 0.f, avg_cat = 0.f, avg_obj = 0.f, recall = 0.f, recall75 = 0.f;
    int count = 0;
    for (int t = 0; t < BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS; ++t) {
        const float* tr = truths + 5 * t;
        if (!tr[0]) break;
        const float4 truth = make_float4(tr[0], tr[1], tr[2], tr[3]);
        // i = (int)(truth.x * w), j = (int)(truth.y * h), class = (int)label: a truth whose cell or class falls outside
        // the head is skipped as a whole (the reference writes out of bounds there)
        const float fi = truth.x * (float)hd.w, fj = truth.y * (float)hd.h, fc = tr[4];
        if (!(fi > -1.f && fi < (float)hd.w && fj > -1.f && fj < (float)hd.h && fc > -1.f && fc < (float)hd.classes))
            continue;
        const int i = (int)fi, j = (int)fj, cls = (int)fc;
        float best_iou = 0.f;
        int best_n = 0;
        const float4 shifted = make_float4(0.f, 0.f, truth.z, truth.w);
        for (int n = 0; n < hd.total; ++n) {
            const float4 anchor = make_float4(0.f, 0.f, hd.biases[2 * n] / (float)hd.in_w, hd.biases[2 * n + 1] / (float)hd.in_h);
            const float iou = yolo_box_iou(anchor, shifted);
            if (iou > best_iou) {
                best_iou = iou;
                best_n = n;
            }
        }
        int mask_n = -1;
        for (int k = 0; k < hd.num; ++k)
            if (hd.mask[k] == best_n) {
                mask_n = k;
                break;
            }
        if (mask_n < 0) continue;
        const size_t base = ((size_t)(b * hd.num + mask_n) * per_box) * hw + (size_t)j * hd.w + i;
        const size_t obj_index = base + (size_t)hd.coords * hw, class_index = obj_index + hw;
        if (lane == 0) {  // delta_yolo_box, bcnn_yolo.c:147-175, and the objectness delta
            const float v[4] = {y[base], y[base + hw], y[base + 2 * (size_t)hw], y[base + 3 * (size_t)hw]};
            const float aw = hd.biases[2 * best_n], ah = hd.biases[2 * best_n + 1];
            const float iou = yolo_box_iou(yolo_train_box(v, i, j, hd.w, hd.h, aw, ah, hd.in_w, hd.in_h), truth);
            const float scale = 2 - truth.z * truth.w;
            const float tx = truth.x * (float)hd.w - (float)i, ty = truth.y * (float)hd.h - (float)j;
            const float tw = logf(truth.z * (float)hd.in_w / aw), th = logf(truth.w * (float)hd.in_h / ah);
            grad[base] = -scale * (tx - v[0]);
            grad[base + hw] = -scale * (ty - v[1]);
            grad[base + 2 * (size_t)hw] = -scale * (tw - v[2]);
            grad[base + 3 * (size_t)hw] = -scale * (th - v[3]);
            avg_obj += y[obj_index];
            grad[obj_index] = y[obj_index] - 1;
            ++count;
            if (iou > 0.5f) recall += 1;
            if (iou > 0.75f) recall75 += 1;
            avg_iou += iou;
        }
        // delta_yolo_class, bcnn_yolo.c:185-205: what an earlier truth of this image left at class 0 of the slot decides
        if (grad[class_index]) {
            if (lane == 0) {
                const float out = y[class_index + (size_t)cls * hw];
                grad[class_index + (size_t)cls * hw] = out - 1;
                avg_cat += out;
            }
        } else {
            for (int c = lane; c < hd.classes; c += kWave) {
                const float out = y[class_index + (size_t)c * hw];
                grad[class_index + (size_t)c * hw] = out - (c == cls ? 1 : 0);
                if (c == cls) avg_cat += out;  // one lane per truth: gathered below
            }
        }
        __syncthreads();  // the wave's stores are in place before the next truth reads class 0 of its slot
    }
    // avg_cat lives in whichever lane owned the class: every lane added at most its own terms, in truth order; the
    // wave tree over them is fixed
    avg_cat = wave_sum(avg_cat);
    if (lane == 0) {
        float* s = stats_part + (size_t)b * kStatsPerImage;
        s[0] = avg_iou;
        s[1] = avg_cat;
        s[2] = avg_obj;
        s[3] = recall;
        s[4] = recall75;
        s[5] = (float)count;  // <= 50: exact
    }
}

// (c) cost = sum of grad^2: kCost blocks leave one partial each ...
__global__ __launch_bounds__(kTrainBlock) void yolo_train_cost_kernel(const float* __restrict__ grad, size_t total,
                                                                      float* __restrict__ cost_part) {
    __shared__ float red[kTrainBlock / kWave];
    const size_t gs = (size_t)gridDim.x * kTrainBlock;
    float s = 0.f;
    for (size_t k = (size_t)blockIdx.x * kTrainBlock + threadIdx.x; k < total; k += gs) s += grad[k] * grad[k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) cost_part[blockIdx.x] = s;
}

// ... and one block folds them, the objectness partials of (a) and the per-image statistics of (b) into the record
__global__ __launch_bounds__(kTrainBlock) void yolo_train_record_kernel(const float* __restrict__ cost_part, int cost_blocks,
                                                                        const float* __restrict__ anyobj_part, int anyobj_parts,
                                                                        const float* __restrict__ stats_part, int n,
                                                                        bcnn_hip_yolo_train_record* __restrict__ rec) {
    __shared__ float red[kTrainBlock / kWave];
    __shared__ float stats[kStatsPerImage];
    float c = 0.f, a = 0.f;
    for (int k = threadIdx.x; k < cost_blocks; k += kTrainBlock) c += cost_part[k];
    for (int k = threadIdx.x; k < anyobj_parts; k += kTrainBlock) a += anyobj_part[k];
    c = block_sum(c, red);
    a = block_sum(a, red);
    if (threadIdx.x < kStatsPerImage) {
        float s = 0.f;
        for (int b = 0; b < n; ++b) s += stats_part[(size_t)b * kStatsPerImage + threadIdx.x];
        stats[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rec->cost = c;
        rec->avg_iou = stats[0];
        rec->avg_cat = stats[1];
        rec->avg_obj = stats[2];
        rec->avg_anyobj = a;
        rec->recall = stats[3];
        rec->recall75 = stats[4];
        rec->count = (int)stats[5];
    }
}

static bool yolo_train_head_ok(const bcnn_hip_yolo_train_head* hd) {
    if (!hd || hd->n < 1 || hd->n > 65535 || hd->h < 1 || hd->w < 1 || hd->num < 1 || hd->num > BCNN_HIP_YOLO_MAX_ANCHORS ||
        hd->coords != 4 || hd->classes < 0 || hd->total < 1 || hd->total > BCNN_HIP_YOLO_TRAIN_MAX_TOTAL || hd->in_w < 1 ||
        hd->in_h < 1 || hd->label_stride < kTruthFloats)
        return false;
    for (int k = 0; k < hd->num; ++k)
        if (hd->mask[k] < 0 || hd->mask[k] >= hd->total) return false;
    const long long total = (long long)hd->n * hd->num * (hd->coords + hd->classes + 1) * hd->h * hd->w;
    return total <= (1ll << 31) - 1;
}

static int yolo_train_cost_blocks(size_t total) {
    const int need = ceil_div((long long)total, 4 * kTrainBlock);
    return need < 1 ? 1 : (need > kCostBlocksMax ? kCostBlocksMax : need);
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" {

void bcnn_hip_concat_forward(int num_src, const float* const* src_d, const int* src_size3d, float* dst_d,
                             int dst_size3d, int n) {
    if (num_src <= 0 || n <= 0) return;
    int offset = 0;
    for (int base = 0; base < num_src; base += kConcatMax) {
        ConcatTable tab = {};
        int cnt = 0, max_size = 0;
        for (int i = base; i < num_src && cnt < kConcatMax; ++i) {
            if (src_size3d[i] > 0) {
                tab.src[cnt] = src_d[i];
                tab.size[cnt] = src_size3d[i];
                tab.offset[cnt] = offset;
                if (src_size3d[i] > max_size) max_size = src_size3d[i];
                ++cnt;
            }
            offset += src_size3d[i];
        }
        if (!cnt) continue;
        const dim3 grid(concat_grid_x(max_size, cnt * n), cnt * n);
        concat_fwd_kernel<<<grid, 256, 0, current_stream()>>>(tab, cnt, dst_d, dst_size3d);
        KERNEL_CHECK();
    }
}

void bcnn_hip_concat_backward(int num_src, float* const* src_grad_d, const int* src_size3d, const float* dst_grad_d,
                              int dst_size3d, int n) {
    if (num_src <= 0 || n <= 0 || !dst_grad_d) return;
    int offset = 0, i = 0;
    while (i < num_src) {
        ConcatTable tab = {};
        int cnt = 0, max_size = 0;
        for (; i < num_src && cnt < kConcatMax; ++i) {
            if (src_grad_d[i] && src_size3d[i] > 0) {
                tab.grad[cnt] = src_grad_d[i];
                tab.size[cnt] = src_size3d[i];
                tab.offset[cnt] = offset;
                if (src_size3d[i] > max_size) max_size = src_size3d[i];
                ++cnt;
            }
            offset += src_size3d[i];
        }
        if (!cnt) continue;
        const dim3 grid(concat_grid_x(max_size, cnt * n), cnt * n);
        concat_bwd_kernel<<<grid, 256, 0, current_stream()>>>(tab, cnt, dst_grad_d, dst_size3d);
        KERNEL_CHECK();
    }
}

void bcnn_hip_upsample_forward(const float* x_d, float* y_d, int n, int c, int h, int w, int size) {
    const size_t total = (size_t)n * c * h * w;
    if (!total || size <= 0) return;
    if (size == 2 && (w & 1) == 0 && aligned_to(x_d, 8) && aligned_to(y_d, 16)) {
        upsample2_fwd_kernel<<<stream_grid(total / 2, 256), 256, 0, current_stream()>>>(x_d, y_d, w, total / 2);
    } else {
        upsample_fwd_kernel<<<stream_grid(total, 256), 256, 0, current_stream()>>>(x_d, y_d, w, size, total);
    }
    KERNEL_CHECK();
}

void bcnn_hip_upsample_backward(float* dx_d, const float* dy_d, int n, int c, int h, int w, int size) {
    const size_t total = (size_t)n * c * h * w;
    if (!total || size <= 0 || !dx_d || !dy_d) return;
    if (size == 2 && (w & 1) == 0 && aligned_to(dx_d, 8) && aligned_to(dy_d, 16)) {
        upsample2_bwd_kernel<<<stream_grid(total / 2, 256), 256, 0, current_stream()>>>(dx_d, dy_d, w, total / 2);
    } else {
        upsample_bwd_kernel<<<stream_grid(total, 256), 256, 0, current_stream()>>>(dx_d, dy_d, w, size, total);
    }
    KERNEL_CHECK();
}

void bcnn_hip_yolo_activate(const float* x_d, float* y_d, int n, int num, int coords, int classes, int hw) {
    const int per_box = coords + classes + 1;
    const size_t total = (size_t)n * num * per_box * hw;
    if (!total) return;
    const int vec = aligned_to(x_d, 16) && aligned_to(y_d, 16);
    yolo_activate_kernel<<<stream_grid(vec ? total / 4 + 1 : total, 256), 256, 0, current_stream()>>>(
        x_d, y_d, hw, num * per_box, per_box, coords, total, vec);
    KERNEL_CHECK();
}

// workspace: [cost partials][objectness partials n x blocks of (a)][statistics n x 6]
size_t bcnn_hip_yolo_train_workspace_size(const bcnn_hip_yolo_train_head* hd) {
    if (!yolo_train_head_ok(hd)) return 0;
    const int gx = ceil_div((long long)hd->num * hd->h * hd->w, kTrainBlock);
    return (size_t)kCostBlocksMax + (size_t)hd->n * gx + (size_t)hd->n * kStatsPerImage;
}

int bcnn_hip_yolo_train_forward(const bcnn_hip_yolo_train_head* hd, const float* x_d, const float* label_d, float* y_d,
                                float* grad_d, bcnn_hip_yolo_train_record* record_d, float* workspace_d) {
    if (!yolo_train_head_ok(hd) || !x_d || !label_d || !y_d || !grad_d || !record_d || !workspace_d) return 1;
    const int hw = hd->h * hd->w, gx = ceil_div((long long)hd->num * hw, kTrainBlock);
    const size_t total = (size_t)hd->n * hd->num * (hd->coords + hd->classes + 1) * hw;
    float* cost_part = workspace_d;
    float* anyobj_part = cost_part + kCostBlocksMax;
    float* stats_part = anyobj_part + (size_t)hd->n * gx;
    const int cost_blocks = yolo_train_cost_blocks(total);
    hipStream_t st = current_stream();
    yolo_train_forward_kernel<<<dim3(gx, hd->n), kTrainBlock, 0, st>>>(*hd, x_d, label_d, y_d, grad_d, anyobj_part);
    KERNEL_CHECK();
    yolo_train_truths_kernel<<<hd->n, kWave, 0, st>>>(*hd, label_d, y_d, grad_d, stats_part);
    KERNEL_CHECK();
    yolo_train_cost_kernel<<<cost_blocks, kTrainBlock, 0, st>>>(grad_d, total, cost_part);
    KERNEL_CHECK();
    yolo_train_record_kernel<<<1, kTrainBlock, 0, st>>>(cost_part, cost_blocks, anyobj_part, hd->n * gx, stats_part, hd->n,
                                                        record_d);
    KERNEL_CHECK();
    return 0;
}

int bcnn_hip_yolo_nms_capacity(void) { return kNmsCapacity; }

size_t bcnn_hip_yolo_detect_result_words(int n, int record_cap, int max_classes) {
    if (n <= 0 || record_cap <= 0 || max_classes < 0) return 0;
    return (size_t)n + (size_t)n * record_cap * (1 + kRecHead + max_classes);
}

int bcnn_hip_yolo_detect_batch(const bcnn_hip_yolo_head* heads, int num_heads, int n, const int* image_geom, int in_w,
                               int in_h, int netw, int neth, float thresh, int relative, float nms_thresh,
                               int record_cap, int nms_cap, void* result_host) {
    if (!heads || !image_geom || !result_host || num_heads < 1 || num_heads > BCNN_HIP_YOLO_MAX_HEADS || n < 1 || n > 65535 ||
        record_cap < 1 || in_w < 1 || in_h < 1 || netw < 1 || neth < 1)
        return 1;
    YoloTable tab = {};
    int max_classes = 0;
    long long total = 0;
    for (int k = 0; k < num_heads; ++k) {
        const bcnn_hip_yolo_head& hd = heads[k];
        if (!hd.out_d || hd.h < 1 || hd.w < 1 || hd.num < 1 || hd.num > BCNN_HIP_YOLO_MAX_ANCHORS || hd.coords < 4 ||
            hd.classes < 0)
            return 1;
        tab.head[k] = hd;
        tab.first[k] = (int)total;
        total += (long long)hd.h * hd.w * hd.num;
        if (total > (1ll << 30)) return 1;
        if (hd.classes > max_classes) max_classes = hd.classes;
    }
    for (int k = num_heads; k <= BCNN_HIP_YOLO_MAX_HEADS; ++k) tab.first[k] = (int)total;
    for (int b = 0; b < n; ++b)
        if (image_geom[4 * b] < 1 || image_geom[4 * b + 1] < 1) return 1;
    if (nms_cap <= 0 || nms_cap > kNmsCapacity) nms_cap = kNmsCapacity;
    const int stride = kRecHead + max_classes;
    const size_t result_words = bcnn_hip_yolo_detect_result_words(n, record_cap, max_classes);
    if ((size_t)n * record_cap > (size_t)0x7fffffff) return 1;
    // [geom n x 4][count n][order n x cap][records n x cap x stride]; the last three are the result, copied as one block
    float* base = scratch(SCRATCH_DETECT, (size_t)4 * n + result_words);
    int4* geom_d = reinterpret_cast<int4*>(base);
    int* count_d = reinterpret_cast<int*>(base) + (size_t)4 * n;
    int* order_d = count_d + n;
    float* records_d = reinterpret_cast<float*>(order_d + (size_t)n * record_cap);
    hipStream_t st = current_stream();
    HIP_CHECK(hipMemcpyAsync(geom_d, image_geom, (size_t)4 * n * sizeof(int), hipMemcpyHostToDevice, st));
    const dim3 grid(ceil_div(total, kDetBlock), n);
    yolo_candidates_kernel<<<grid, kDetBlock, 0, st>>>(tab, num_heads, geom_d, in_w, in_h, netw, neth, thresh,
                                                       relative, record_cap, stride, count_d, records_d);
    KERNEL_CHECK();
    yolo_nms_kernel<<<n, kDetBlock, 0, st>>>(count_d, record_cap, nms_cap, stride, nms_thresh, order_d, records_d);
    KERNEL_CHECK();
    HIP_CHECK(hipMemcpyAsync(result_host, count_d, result_words * sizeof(float), hipMemcpyDeviceToHost, st));
    return 0;
}

}  // extern "C"
