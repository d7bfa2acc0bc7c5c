// lrn_dropout.hip -- local response normalisation across channels and dropout. Both are HBM-bound streams.
//
// LRN (NCHW, channel stride H*W): one lane owns one (image, pixel) column -- four consecutive pixels with 16-byte
// accesses when H*W % 4 == 0 and the pointers allow it -- and marches over the channels, keeping the inputs of the
// current window in a register ring. Each s_c is the direct window sum in ascending channel order (no running
// add / subtract), so its value does not depend on where a march starts: a column split into channel chunks with an
// (n - 1) halo gives the same bits as one march. The backward recomputes s and y from x (no saved scale tensor).
//
// Dropout: the mask is drawn by a counter-based Philox4x32-10 in the kernel (include/bcnn_hip.h defines it element
// by element), so the backward regenerates it from (key, step) and nothing is stored.
#include "common.h"

namespace bcnn_hip {

// ---- LRN ------------------------------------------------------------------------------------------------------------
// window of channel c: [c - (N-1)/2, c + N/2] clipped to [0, C); s_c = k + alpha/N * sum x^2; y_c = x_c * s_c^-beta
struct LrnArgs {
    int C, hw, cols;   // cols: lanes per chunk row (images * hw / V)
    int chunk;         // channels per chunk (blockIdx.y)
    float alpha_n, beta, k, ratio;  // ratio = 2 alpha beta / N
    int overwrite;
};

template <int V> struct VecT;
template <> struct VecT<1> { using T = float; };
template <> struct VecT<4> { using T = float4; };

template <int V> __device__ __forceinline__ float lane_get(const typename VecT<V>::T& v, int e);
template <> __device__ __forceinline__ float lane_get<1>(const float& v, int) { return v; }
template <> __device__ __forceinline__ float lane_get<4>(const float4& v, int e) {
    return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
}
template <int V> __device__ __forceinline__ void lane_set(typename VecT<V>::T& v, int e, float f);
template <> __device__ __forceinline__ void lane_set<1>(float& v, int, float f) { v = f; }
template <> __device__ __forceinline__ void lane_set<4>(float4& v, int e, float f) {
    if (e == 0) v.x = f; else if (e == 1) v.y = f; else if (e == 2) v.z = f; else v.w = f;
}

// s^-beta as powf computes it for s >= 0 (beta == 0 gives 1 also for s == 0)
__device__ __forceinline__ float lrn_pow(float s, float beta) {
    return beta == 0.f ? 1.f : exp2f(-beta * log2f(s));
}

// offset of the first element of lane g's column (V consecutive pixels of one image)
__device__ __forceinline__ size_t lrn_col_base(int g, int hw, int C, int V) {
    const int per_img = hw / V;
    const int img = g / per_img, p = (g - img * per_img) * V;
    return (size_t)img * C * hw + p;
}

template <int N, int V>
__global__ __launch_bounds__(256) void lrn_fwd_ring(const float* __restrict__ x, float* __restrict__ y, LrnArgs a) {
    using T = typename VecT<V>::T;
    constexpr int LO = (N - 1) / 2, HI = N / 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.cols) return;
    const size_t base = lrn_col_base(g, a.hw, a.C, V);
    const T* xp = reinterpret_cast<const T*>(x + base);
    T* yp = reinterpret_cast<T*>(y + base);
    const size_t cs = (size_t)a.hw / V;  // channel stride in T units
    const int c0 = blockIdx.y * a.chunk, c1 = min(a.C, c0 + a.chunk);
    T r[N];  // r[j] = x of channel c - LO + j (zero outside [0, C))
    T zero;
#pragma unroll
    for (int e = 0; e < V; ++e) lane_set<V>(zero, e, 0.f);
    r[0] = zero;
#pragma unroll
    for (int j = 1; j < N; ++j) {
        const int ch = c0 - 1 - LO + j;
        r[j] = (ch >= 0 && ch < a.C) ? xp[(size_t)ch * cs] : zero;
    }
    for (int c = c0; c < c1; ++c) {
#pragma unroll
        for (int j = 0; j < N - 1; ++j) r[j] = r[j + 1];
        const int ch = c + HI;
        r[N - 1] = ch < a.C ? xp[(size_t)ch * cs] : zero;
        T out;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float v = lane_get<V>(r[j], e);
                sum = sum + v * v;
            }
            const float s = a.k + a.alpha_n * sum;
            lane_set<V>(out, e, lane_get<V>(r[LO], e) * lrn_pow(s, a.beta));
        }
        yp[(size_t)c * cs] = out;
    }
}

// dx_j = dy_j s_j^-beta - ratio x_j sum_{c in [j - HI, j + LO]} dy_c x_c s_c^(-beta) / s_c. The march runs a lead
// channel c from c0 - HI to c1 - 1 + LO; at each step it forms t_c = dy_c y_c / s_c and finishes channel j = c - LO.
template <int N, int V>
__global__ __launch_bounds__(256) void lrn_bwd_ring(const float* __restrict__ x, const float* __restrict__ dy,
                                                    float* __restrict__ dx, LrnArgs a) {
    using T = typename VecT<V>::T;
    constexpr int LO = (N - 1) / 2, HI = N / 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.cols) return;
    const size_t base = lrn_col_base(g, a.hw, a.C, V);
    const T* xp = reinterpret_cast<const T*>(x + base);
    const T* dyp = reinterpret_cast<const T*>(dy + base);
    T* dxp = reinterpret_cast<T*>(dx + base);
    const size_t cs = (size_t)a.hw / V;
    const int c0 = blockIdx.y * a.chunk, c1 = min(a.C, c0 + a.chunk);
    T zero;
#pragma unroll
    for (int e = 0; e < V; ++e) lane_set<V>(zero, e, 0.f);
    T r[N];        // x of channels c - LO .. c + HI
    T t[N];        // t of channels c - N + 1 .. c
    T dyr[LO + 1]; // dy of channels c - LO .. c
    T pr[LO + 1];  // s^-beta of channels c - LO .. c
    const int cstart = c0 - HI;
    r[0] = zero;
#pragma unroll
    for (int j = 1; j < N; ++j) {
        const int ch = cstart - 1 - LO + j;
        r[j] = (ch >= 0 && ch < a.C) ? xp[(size_t)ch * cs] : zero;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = zero;
#pragma unroll
    for (int j = 0; j <= LO; ++j) { dyr[j] = zero; pr[j] = zero; }
    for (int c = cstart; c < c1 + LO; ++c) {
#pragma unroll
        for (int j = 0; j < N - 1; ++j) { r[j] = r[j + 1]; t[j] = t[j + 1]; }
#pragma unroll
        for (int j = 0; j < LO; ++j) { dyr[j] = dyr[j + 1]; pr[j] = pr[j + 1]; }
        const int ch = c + HI;
        r[N - 1] = (ch >= 0 && ch < a.C) ? xp[(size_t)ch * cs] : zero;
        const bool live = c >= 0 && c < a.C;
        const T dyc = live ? dyp[(size_t)c * cs] : zero;
        T tc, pc;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float v = lane_get<V>(r[j], e);
                sum = sum + v * v;
            }
            const float s = a.k + a.alpha_n * sum;
            const float p = lrn_pow(s, a.beta);
            lane_set<V>(pc, e, p);
            lane_set<V>(tc, e, live ? lane_get<V>(dyc, e) * (lane_get<V>(r[LO], e) * p) / s : 0.f);
        }
        t[N - 1] = tc;
        dyr[LO] = dyc;
        pr[LO] = pc;
        const int jc = c - LO;  // the channel finished at this step; x_jc = r[0]
        if (jc >= c0) {
            T out;
            const T old = a.overwrite ? zero : dxp[(size_t)jc * cs];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < N; ++j) acc = acc + lane_get<V>(t[j], e);
                const float v = lane_get<V>(dyr[0], e) * lane_get<V>(pr[0], e) -
                                a.ratio * (lane_get<V>(r[0], e) * acc);
                lane_set<V>(out, e, a.overwrite ? v : lane_get<V>(old, e) + v);
            }
            dxp[(size_t)jc * cs] = out;
        }
    }
}

// any window size: one thread per element, windows read straight from memory (sum order as in the ring kernels)
__device__ __forceinline__ float lrn_scale_at(const float* __restrict__ xc, int c, int n, const LrnArgs& a) {
    const int lo = (n - 1) / 2, hi = n / 2;
    float sum = 0.f;
    for (int q = max(0, c - lo); q <= min(a.C - 1, c + hi); ++q) {
        const float v = xc[(size_t)q * a.hw];
        sum = sum + v * v;
    }
    return a.k + a.alpha_n * sum;
}

__global__ __launch_bounds__(256) void lrn_fwd_generic(const float* __restrict__ x, float* __restrict__ y, int n,
                                                       size_t total, LrnArgs a) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t img = i / ((size_t)a.C * a.hw), rem = i - img * a.C * a.hw;
        const int c = (int)(rem / a.hw), p = (int)(rem - (size_t)c * a.hw);
        const float* xc = x + img * a.C * a.hw + p;
        y[i] = x[i] * lrn_pow(lrn_scale_at(xc, c, n, a), a.beta);
    }
}

__global__ __launch_bounds__(256) void lrn_bwd_generic(const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx, int n, size_t total, LrnArgs a) {
    const int lo = (n - 1) / 2, hi = n / 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t img = i / ((size_t)a.C * a.hw), rem = i - img * a.C * a.hw;
        const int j = (int)(rem / a.hw), p = (int)(rem - (size_t)j * a.hw);
        const size_t col = img * a.C * a.hw + p;
        const float* xc = x + col;
        float acc = 0.f;
        for (int c = j - hi; c <= j + lo; ++c) {
            if (c < 0 || c >= a.C) continue;
            const float s = lrn_scale_at(xc, c, n, a);
            acc = acc + dy[col + (size_t)c * a.hw] * (xc[(size_t)c * a.hw] * lrn_pow(s, a.beta)) / s;
        }
        const float v = dy[i] * lrn_pow(lrn_scale_at(xc, j, n, a), a.beta) - a.ratio * (x[i] * acc);
        dx[i] = a.overwrite ? v : dx[i] + v;
    }
}

// ---- dropout --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * ctr.x, hi0 = __umulhi(0xD2511F53u, ctr.x);
        const uint32_t lo1 = 0xCD9E8D57u * ctr.z, hi1 = __umulhi(0xCD9E8D57u, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0);
    }
    return ctr;
}

__device__ __forceinline__ float dropout_one(float v, uint32_t word, float rate, float scale) {
    return (float)(word >> 8) * 5.9604644775390625e-08f < rate ? 0.f : v * scale;
}

// x[i] <- mask_i ? 0 : x[i] * scale; lane q owns elements 4q .. 4q + 3 and draws one Philox block for them
__global__ __launch_bounds__(256) void dropout_kernel(float* __restrict__ x, size_t size, float rate, float scale,
                                                      uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, int vec) {
    const size_t quads = (size + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), s0, s1), k0, k1);
        const size_t i = q * 4;
        if (vec && i + 4 <= size) {
            float4 v = reinterpret_cast<float4*>(x)[q];
            v.x = dropout_one(v.x, w.x, rate, scale);
            v.y = dropout_one(v.y, w.y, rate, scale);
            v.z = dropout_one(v.z, w.z, rate, scale);
            v.w = dropout_one(v.w, w.w, rate, scale);
            reinterpret_cast<float4*>(x)[q] = v;
        } else {
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            for (int e = 0; e < 4 && i + e < size; ++e) x[i + e] = dropout_one(x[i + e], ws[e], rate, scale);
        }
    }
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// lanes wanted in flight before the channels are split into chunks (4 blocks of 256 per CU)
static constexpr int kLrnLanes = kCUs * 4 * 256;

// chunk length for `cols` lanes per chunk row: split C only while the chip is not full, and keep the halo (n - 1
// channels re-read per chunk) at most a quarter of a chunk's own channels
static int lrn_chunk(int C, int n, int cols) {
    if (cols >= kLrnLanes) return C;
    const int want = ceil_div(kLrnLanes, cols);
    const int min_len = 4 * (n > 1 ? n - 1 : 1);
    int len = ceil_div(C, want);
    if (len < min_len) len = min_len;
    return len < C ? len : C;
}

template <int N>
static void lrn_launch_n(bool fwd, bool vec, const float* x, const float* dy, float* out, const LrnArgs& a) {
    const dim3 grid(ceil_div(a.cols, 256), ceil_div(a.C, a.chunk));
    if (fwd) {
        if (vec) lrn_fwd_ring<N, 4><<<grid, 256, 0, current_stream()>>>(x, out, a);
        else lrn_fwd_ring<N, 1><<<grid, 256, 0, current_stream()>>>(x, out, a);
    } else {
        if (vec) lrn_bwd_ring<N, 4><<<grid, 256, 0, current_stream()>>>(x, dy, out, a);
        else lrn_bwd_ring<N, 1><<<grid, 256, 0, current_stream()>>>(x, dy, out, a);
    }
}

// the 16-byte form keeps 4 lanes of every ring entry: up to n = 7 (backward: ~90 VGPRs of rings)
static constexpr int kLrnVecMax = 7;
static constexpr int kLrnRingMax = 15;

static void lrn_run(bool fwd, const float* x, const float* dy, float* out, int n, int c, int h, int w, int local_size,
                    float alpha, float beta, float k, int overwrite) {
    const int hw = h * w;
    const size_t total = (size_t)n * c * hw;
    if (!total || local_size < 1 || !x || !out || (!fwd && !dy)) return;
    LrnArgs a;
    a.C = c;
    a.hw = hw;
    a.alpha_n = alpha / (float)local_size;
    a.beta = beta;
    a.k = k;
    a.ratio = 2.f * alpha * beta / (float)local_size;
    a.overwrite = overwrite;
    if (local_size > kLrnRingMax) {
        if (fwd) lrn_fwd_generic<<<stream_grid(total, 256), 256, 0, current_stream()>>>(x, out, local_size, total, a);
        else lrn_bwd_generic<<<stream_grid(total, 256), 256, 0, current_stream()>>>(x, dy, out, local_size, total, a);
        KERNEL_CHECK();
        return;
    }
    const bool vec = local_size <= kLrnVecMax && hw % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 16) &&
                     (fwd || aligned_to(dy, 16));
    const long long cols = (long long)n * (hw / (vec ? 4 : 1));
    if (cols > 0x7fffffffLL) return;  // > 2^31 columns: not a tensor this library allocates
    a.cols = (int)cols;
    a.chunk = lrn_chunk(c, local_size, a.cols);
    switch (local_size) {
        case 1: lrn_launch_n<1>(fwd, vec, x, dy, out, a); break;
        case 2: lrn_launch_n<2>(fwd, vec, x, dy, out, a); break;
        case 3: lrn_launch_n<3>(fwd, vec, x, dy, out, a); break;
        case 4: lrn_launch_n<4>(fwd, vec, x, dy, out, a); break;
        case 5: lrn_launch_n<5>(fwd, vec, x, dy, out, a); break;
        case 6: lrn_launch_n<6>(fwd, vec, x, dy, out, a); break;
        case 7: lrn_launch_n<7>(fwd, vec, x, dy, out, a); break;
        case 8: lrn_launch_n<8>(fwd, false, x, dy, out, a); break;
        case 9: lrn_launch_n<9>(fwd, false, x, dy, out, a); break;
        case 10: lrn_launch_n<10>(fwd, false, x, dy, out, a); break;
        case 11: lrn_launch_n<11>(fwd, false, x, dy, out, a); break;
        case 12: lrn_launch_n<12>(fwd, false, x, dy, out, a); break;
        case 13: lrn_launch_n<13>(fwd, false, x, dy, out, a); break;
        case 14: lrn_launch_n<14>(fwd, false, x, dy, out, a); break;
        default: lrn_launch_n<15>(fwd, false, x, dy, out, a); break;
    }
    KERNEL_CHECK();
}

static void dropout_run(float* x_d, size_t size, float rate, uint64_t key, uint64_t step) {
    if (!x_d || !size || !(rate > 0.f)) return;  // rate 0 keeps every element and scales by exactly 1
    const float scale = 1.f / (1.f - rate);
    const size_t quads = (size + 3) / 4;
    dropout_kernel<<<stream_grid(quads, 256), 256, 0, current_stream()>>>(
        x_d, size, rate, scale, (uint32_t)key, (uint32_t)(key >> 32), (uint32_t)step, (uint32_t)(step >> 32),
        aligned_to(x_d, 16) ? 1 : 0);
    KERNEL_CHECK();
}

extern "C" {

void bcnn_hip_lrn_forward(const float* x_d, float* y_d, int n, int c, int h, int w, int local_size, float alpha,
                          float beta, float k) {
    lrn_run(true, x_d, nullptr, y_d, n, c, h, w, local_size, alpha, beta, k, 1);
}

void bcnn_hip_lrn_backward(const float* x_d, const float* dy_d, float* dx_d, int n, int c, int h, int w,
                           int local_size, float alpha, float beta, float k, int overwrite) {
    lrn_run(false, x_d, dy_d, dx_d, n, c, h, w, local_size, alpha, beta, k, overwrite);
}

void bcnn_hip_dropout_forward(float* x_d, size_t size, float rate, uint64_t key, uint64_t step) {
    dropout_run(x_d, size, rate, key, step);
}

void bcnn_hip_dropout_backward(float* dx_d, size_t size, float rate, uint64_t key, uint64_t step) {
    dropout_run(dx_d, size, rate, key, step);
}

}  // extern "C"
