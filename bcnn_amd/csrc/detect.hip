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

}  // extern "C"
