// pool2d.hip -- windowed max / average pooling with symmetric leading padding (the pool2d node). HBM-bound.
//
// Semantics: torch.nn.functional.max_pool2d / avg_pool2d (Caffe's rules), include/bcnn_hip.h. Window (i, j) covers rows
// i*stride - pad .. + size - 1 and the same columns, clipped to the input; pad <= size / 2, so every window holds a real
// element. Max: rows outer / columns inner, replace only on `>` (the first maximum wins, a NaN never wins, padding never
// wins), index = int32 flat offset into the whole source tensor -- the format of pool.hip, whose kernels stay as they are.
// Average: sum of the real elements / divisor, a true division.
//
// Every kernel is a grid-stride loop over a capped 1-D grid: plane counts and element counts are bounded only by the
// int32 index format (fewer than 2^31 elements per tensor). The two or three index divisions per work item are
// multiply-high by constants from the host (FastDiv); everything that depends only on the window row or column (clip
// bounds, divisor factors) is computed once per item, not per tap.
#include <cfloat>
#include <cstdint>

#include "common.h"

namespace bcnn_hip {

enum { POOL_MAX = BCNN_HIP_POOL2D_MAX, POOL_AVG = BCNN_HIP_POOL2D_AVG };

struct Pool2dGeom {
    int H, W, OH, OW, size, stride, pad, include_pad;
};

// window extent along one axis: [lo, hi) clipped to the input, and the divisor factor of the average
__device__ __forceinline__ void window_axis(int o, int in, int size, int stride, int pad, int include_pad, int& lo, int& hi,
                                            int& cnt) {
    const int start = o * stride - pad;
    const int end_p = min(start + size, in + pad);  // may reach into the trailing padding, never past it
    lo = max(start, 0);
    hi = min(end_p, in);
    cnt = include_pad ? end_p - start : hi - lo;
}

// ---- forward, any geometry: one thread per output element, consecutive lanes on consecutive columns ----------------------
template <int KIND>
__global__ __launch_bounds__(256) void pool2d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         int* __restrict__ idx, const Pool2dGeom g, const FastDiv dow,
                                                         const FastDiv doh, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gstride) {
        const unsigned t = fdiv(o, dow), j = o - t * dow.d;
        const unsigned plane = fdiv(t, doh), i = t - plane * doh.d;
        int h0, h1, hc, w0, w1, wc;
        window_axis((int)i, g.H, g.size, g.stride, g.pad, g.include_pad, h0, h1, hc);
        window_axis((int)j, g.W, g.size, g.stride, g.pad, g.include_pad, w0, w1, wc);
        const int base = (int)plane * g.H * g.W;
        if (KIND == POOL_MAX) {
            float best = -FLT_MAX;
            int bi = -1;
            for (int hh = h0; hh < h1; ++hh) {
                const int rb = base + hh * g.W;
                for (int ww = w0; ww < w1; ++ww) {
                    const float v = x[rb + ww];
                    if (v > best) { best = v; bi = rb + ww; }
                }
            }
            y[o] = best;
            if (idx) idx[o] = bi;
        } else {
            float s = 0.f;
            for (int hh = h0; hh < h1; ++hh) {
                const int rb = base + hh * g.W;
                for (int ww = w0; ww < w1; ++ww) s += x[rb + ww];
            }
            y[o] = s / (float)(hc * wc);
        }
    }
}

// ---- forward, stride 2 with size 2 / pad 0 or size 3 / pad 1 (the DenseNet, ResNet and ShuffleNet pools) -----------------
// One thread per FOUR consecutive outputs of a row. Their windows span source columns 8q - PAD .. 8q + 7: two aligned
// 16-byte loads per window row (plus the one column to the left for size 3) instead of 4 x SIZE scalar loads, and one
// 16-byte store per output tensor where VEC (out_w % 4 == 0, aligned pointers). Rows and columns outside the input are
// flagged once per item and read as -FLT_MAX (max: never wins against the strict `>`) or 0 (average). Scan order, strict
// `>` and the index are those of the kernel above.
template <int KIND, int SIZE, bool VEC>
__global__ __launch_bounds__(256) void pool2d_fwd_s2x4_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              int* __restrict__ idx, const Pool2dGeom g, const FastDiv dq,
                                                              const FastDiv doh, unsigned total_items) {
    constexpr int PAD = SIZE == 3 ? 1 : 0;
    const float fill = KIND == POOL_MAX ? -FLT_MAX : 0.f;
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total_items; t += gstride) {
        const unsigned rowid = fdiv(t, dq), q = t - rowid * dq.d;
        const unsigned plane = fdiv(rowid, doh), i = rowid - plane * doh.d;
        const int base = (int)plane * g.H * g.W;
        const int c8 = (int)q * 8;
        const bool ok_a = c8 < g.W, ok_b = c8 + 4 < g.W, ok_l = PAD && q > 0;  // W % 4 == 0: a 16-byte load is in or out as a whole
        float best[4] = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}, sum[4] = {0.f, 0.f, 0.f, 0.f};
        int bi[4] = {-1, -1, -1, -1};
#pragma unroll
        for (int r = 0; r < SIZE; ++r) {
            const int hh = (int)i * 2 - PAD + r;
            if (hh < 0 || hh >= g.H) continue;  // padding rows never win and add nothing
            const int rb = base + hh * g.W + c8 - PAD;  // flat offset of v[0]
            const float4 a = ok_a ? *reinterpret_cast<const float4*>(x + rb + PAD) : make_float4(fill, fill, fill, fill);
            const float4 b = ok_b ? *reinterpret_cast<const float4*>(x + rb + PAD + 4) : make_float4(fill, fill, fill, fill);
            float v[9];
            v[0] = ok_l ? x[rb] : fill;  // size 3 only
            v[PAD + 0] = a.x; v[PAD + 1] = a.y; v[PAD + 2] = a.z; v[PAD + 3] = a.w;
            v[PAD + 4] = b.x; v[PAD + 5] = b.y; v[PAD + 6] = b.z; v[PAD + 7] = b.w;
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int c = 0; c < SIZE; ++c) {
                    const int k = 2 * o + c;  // v[k] is column 8q - PAD + k; k <= 6 + SIZE - 1 <= 7 + PAD
                    if (KIND == POOL_MAX) {
                        if (v[k] > best[o]) { best[o] = v[k]; bi[o] = rb + k; }
                    } else {
                        sum[o] += v[k];
                    }
                }
        }
        float res[4];
        if (KIND == POOL_MAX) {
#pragma unroll
            for (int o = 0; o < 4; ++o) res[o] = best[o];
        } else {
            int h0, h1, hc;
            window_axis((int)i, g.H, SIZE, 2, PAD, g.include_pad, h0, h1, hc);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                int w0, w1, wc;
                window_axis((int)q * 4 + o, g.W, SIZE, 2, PAD, g.include_pad, w0, w1, wc);
                res[o] = sum[o] / (float)(hc * max(wc, 1));  // wc < 1 only for outputs past out_w, which are not stored
            }
        }
        const unsigned out = rowid * (unsigned)g.OW + q * 4;
        if (VEC) {
            *reinterpret_cast<float4*>(y + out) = make_float4(res[0], res[1], res[2], res[3]);
            if (KIND == POOL_MAX && idx) *reinterpret_cast<int4*>(idx + out) = make_int4(bi[0], bi[1], bi[2], bi[3]);
        } else {
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if ((int)q * 4 + o < g.OW) {
                    y[out + o] = res[o];
                    if (KIND == POOL_MAX && idx) idx[out + o] = bi[o];
                }
        }
    }
}

// ---- backward: gather form, no atomics -----------------------------------------------------------------------------------
// first / last window index along one axis whose extent covers source position p
__device__ __forceinline__ void cover_axis(int p, int outs, int size, int stride, int pad, int& o0, int& o1) {
    const int a = p + pad - size + 1;  // the lowest window start that still reaches p, in padded coordinates
    o0 = a <= 0 ? 0 : (a + stride - 1) / stride;
    o1 = min((p + pad) / stride, outs - 1);
}
// the average's divisor factor of window o along one axis (window_axis' cnt)
__device__ __forceinline__ int axis_count(int o, int in, int size, int stride, int pad, int include_pad) {
    int lo, hi, cnt;
    window_axis(o, in, size, stride, pad, include_pad, lo, hi, cnt);
    return cnt;
}

// One thread per SOURCE element visits the (at most ceil(size/stride)^2) windows that cover it, in ascending output
// order, and adds dy[o] where the stored index selects it (max) or dy[o] / divisor(o) (average). OVERWRITE: start from 0
// and always store (this node is the gradient's only writer and its zero fill was skipped); an element no window covers
// (stride > size) then becomes 0 and otherwise keeps its value.
template <int KIND, bool OVERWRITE>
__global__ __launch_bounds__(256) void pool2d_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                         float* __restrict__ dx, const Pool2dGeom g, const FastDiv dw,
                                                         const FastDiv dh, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gstride) {
        const unsigned t = fdiv(s, dw), w = s - t * dw.d;
        const unsigned plane = fdiv(t, dh), h = t - plane * dh.d;
        int i0, i1, j0, j1;
        cover_axis((int)h, g.OH, g.size, g.stride, g.pad, i0, i1);
        cover_axis((int)w, g.OW, g.size, g.stride, g.pad, j0, j1);
        float acc = OVERWRITE ? 0.f : dx[s];
        bool hit = OVERWRITE;
        const int obase = (int)plane * g.OH * g.OW;
        for (int i = i0; i <= i1; ++i) {
            const int hc = KIND == POOL_AVG ? axis_count(i, g.H, g.size, g.stride, g.pad, g.include_pad) : 0;
            for (int j = j0; j <= j1; ++j) {
                const int o = obase + i * g.OW + j;
                if (KIND == POOL_MAX) {
                    if (idx[o] == (int)s) { acc += dy[o]; hit = true; }
                } else {
                    acc += dy[o] / (float)(hc * axis_count(j, g.W, g.size, g.stride, g.pad, g.include_pad));
                    hit = true;
                }
            }
        }
        if (hit) dx[s] = acc;
    }
}

// The same gather, one thread per 4 consecutive source pixels of a row: a 16-byte read-modify-write of dx (a 16-byte
// store alone in the OVERWRITE form). The windows covering the 4 pixels are visited in ascending output order, so every
// element sees its additions in the order of the kernel above: same bits.
// CS / CSTRIDE / CPAD > 0 (CPAD >= 0) fix the geometry at compile time: the NI x NJ (index, gradient) pairs that can
// cover the group are then loaded up front from clamped addresses -- independent loads in flight instead of a
// load -> compare -> load chain per window -- and applied in the same order. CS == 0: run-time geometry, plain loops.
template <int KIND>
__device__ __forceinline__ void bwd_apply(float (&v)[4], bool& hit, float gval, int id, int s0, int w0, int j, int size,
                                          int stride, int pad, int divisor) {
    if (KIND == POOL_MAX) {
        const unsigned d = (unsigned)(id - s0);
        if (d < 4u) {
            if (d == 0) v[0] += gval; else if (d == 1) v[1] += gval; else if (d == 2) v[2] += gval; else v[3] += gval;
            hit = true;
        }
    } else {
        const float q = gval / (float)divisor;
        const int lo = j * stride - pad - w0, hi = lo + size;  // the window's columns relative to the group: [lo, hi)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e >= lo && e < hi) { v[e] += q; hit = true; }
    }
}

template <int KIND, bool OVERWRITE, int CS, int CSTRIDE, int CPAD>
__global__ __launch_bounds__(256) void pool2d_bwd_vec4_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                              float* __restrict__ dx, const Pool2dGeom g, const FastDiv dw4,
                                                              const FastDiv dh, unsigned total_groups) {
    const int size = CS ? CS : g.size, stride = CS ? CSTRIDE : g.stride, pad = CS ? CPAD : g.pad;
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total_groups; t += gstride) {
        const unsigned rowid = fdiv(t, dw4), k = t - rowid * dw4.d;
        const unsigned plane = fdiv(rowid, dh), h = rowid - plane * dh.d;
        const int w0 = (int)k * 4;
        const int s0 = (int)rowid * g.W + w0;
        int i0, i1, j0, j1, jx;
        cover_axis((int)h, g.OH, size, stride, pad, i0, i1);
        cover_axis(w0, g.OW, size, stride, pad, j0, jx);
        j1 = min((w0 + 3 + pad) / stride, g.OW - 1);
        const int obase = (int)plane * g.OH * g.OW;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (!OVERWRITE) {
            const float4 c = *reinterpret_cast<const float4*>(dx + s0);
            v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
        }
        bool hit = OVERWRITE;
        if (CS) {
            constexpr int S = CS ? CS : 1, ST = CS ? CSTRIDE : 1;
            constexpr int NI = (S + ST - 1) / ST, NJ = (S + 3 + ST - 1) / ST;
            int id[NI][NJ];
            float gv[NI][NJ];
#pragma unroll
            for (int a = 0; a < NI; ++a)
#pragma unroll
                for (int b = 0; b < NJ; ++b) {
                    const int o = obase + min(max(i0 + a, 0), g.OH - 1) * g.OW + min(max(j0 + b, 0), g.OW - 1);
                    id[a][b] = KIND == POOL_MAX ? idx[o] : 0;
                    gv[a][b] = dy[o];
                }
#pragma unroll
            for (int a = 0; a < NI; ++a) {
                const int i = i0 + a;
                const int hc = KIND == POOL_AVG ? axis_count(i, g.H, size, stride, pad, g.include_pad) : 0;
#pragma unroll
                for (int b = 0; b < NJ; ++b) {
                    const int j = j0 + b;
                    if (i > i1 || j > j1) continue;
                    const int dv = KIND == POOL_AVG ? hc * axis_count(j, g.W, size, stride, pad, g.include_pad) : 1;
                    bwd_apply<KIND>(v, hit, gv[a][b], id[a][b], s0, w0, j, size, stride, pad, dv);
                }
            }
        } else {
            for (int i = i0; i <= i1; ++i) {
                const int hc = KIND == POOL_AVG ? axis_count(i, g.H, size, stride, pad, g.include_pad) : 0;
                const int o = obase + i * g.OW;
                for (int j = j0; j <= j1; ++j) {
                    const int dv = KIND == POOL_AVG ? hc * axis_count(j, g.W, size, stride, pad, g.include_pad) : 1;
                    bwd_apply<KIND>(v, hit, dy[o + j], KIND == POOL_MAX ? idx[o + j] : 0, s0, w0, j, size, stride, pad, dv);
                }
            }
        }
        if (hit) *reinterpret_cast<float4*>(dx + s0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// 3x3 / s2 / p1 with out_w == w / 2 (the centred ResNet stem pool, 112 -> 56): the three window columns that cover the
// pixels 4k .. 4k+3 of thread k are 2k, 2k+1 and 2k+2. The pair (2k, 2k+1) is ONE aligned 8-byte load per window row and
// tensor, contiguous over the wave, and column 2k+2 is the next lane's first element: one DPP move (the last lane of a
// wave fetches it itself) -- 4 + 4 memory instructions instead of 12 stride-2 gathers. Column 2k reaches pixels 4k-1 ..
// 4k+1, column 2k+1 pixels 4k+1 .. 4k+3 and column 2k+2 pixels 4k+3 .. 4k+5, so only 2 x 6 (window, pixel) pairs can
// hit; they are applied rows ascending, columns ascending: the order of the kernels above, the same bits. A miss
// selects the old value (not `+ 0.f`: the add form may start from -0.0f). Every lane of a wave runs the loop the same
// number of times, on a clamped item past the end, because the DPP move wants its neighbour alive.
template <typename T>
__device__ __forceinline__ T dpp_from_next_lane(T own_fetch, T v) {  // lane i takes lane i + 1's v; lane 63 keeps own_fetch
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, own_fetch), __builtin_bit_cast(int, v),
                                                             0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

template <int KIND, bool OVERWRITE>
__global__ __launch_bounds__(256) void pool2d_bwd_k3s2p1_pair_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                                     float* __restrict__ dx, const Pool2dGeom g,
                                                                     const FastDiv dw4, const FastDiv dh, unsigned total_groups) {
    const unsigned gstride = gridDim.x * blockDim.x, lane = threadIdx.x & 63u;
    for (unsigned wbase = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < total_groups; wbase += gstride) {  // wave-uniform
        const unsigned t0 = wbase + lane;
        const bool live = t0 < total_groups;
        const unsigned t = live ? t0 : total_groups - 1u;
        const unsigned rowid = fdiv(t, dw4), k = t - rowid * dw4.d;
        const unsigned plane = fdiv(rowid, dh), h = rowid - plane * dh.d;
        const int s0 = (int)rowid * g.W + (int)k * 4;
        const int i0 = (int)h >> 1;                         // windows 2i - 1 <= h <= 2i + 1: i0 and, for odd h, i0 + 1
        const int i1 = min(((int)h + 1) >> 1, g.OH - 1);
        const bool need_right = k + 1 < dw4.d;              // window column 2k + 2 exists (out_w == w / 2) and is the next lane's
        const bool fetch_right = need_right && lane == 63u;
        int id[2][3];
        float gv[2][3];
        bool ok[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int i = i0 + a;
            ok[a] = i <= i1;
            const int o = ((int)plane * g.OH + min(i, g.OH - 1)) * g.OW + 2 * (int)k;
            const float2 gp = *reinterpret_cast<const float2*>(dy + o);
            int2 ip = make_int2(0, 0);
            if (KIND == POOL_MAX) ip = *reinterpret_cast<const int2*>(idx + o);
            float ge = 0.f;
            int ie = -1;
            if (fetch_right) {
                ge = dy[o + 2];
                if (KIND == POOL_MAX) ie = idx[o + 2];
            }
            gv[a][0] = gp.x; gv[a][1] = gp.y;
            gv[a][2] = dpp_from_next_lane(ge, gp.x);
            id[a][0] = ip.x; id[a][1] = ip.y;
            id[a][2] = KIND == POOL_MAX ? dpp_from_next_lane(ie, ip.x) : 0;
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (!OVERWRITE) {
            const float4 c = *reinterpret_cast<const float4*>(dx + s0);
            v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const bool on[3] = {ok[a], ok[a], ok[a] && need_right};
            if (KIND == POOL_MAX) {
                v[0] = on[0] && id[a][0] == s0 ? v[0] + gv[a][0] : v[0];
                v[1] = on[0] && id[a][0] == s0 + 1 ? v[1] + gv[a][0] : v[1];
                v[1] = on[1] && id[a][1] == s0 + 1 ? v[1] + gv[a][1] : v[1];
                v[2] = on[1] && id[a][1] == s0 + 2 ? v[2] + gv[a][1] : v[2];
                v[3] = on[1] && id[a][1] == s0 + 3 ? v[3] + gv[a][1] : v[3];
                v[3] = on[2] && id[a][2] == s0 + 3 ? v[3] + gv[a][2] : v[3];
            } else {
                const int hc = axis_count(i0 + a, g.H, 3, 2, 1, g.include_pad);
                float q[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) q[b] = gv[a][b] / (float)(hc * axis_count(2 * (int)k + b, g.W, 3, 2, 1, g.include_pad));
                v[0] = on[0] ? v[0] + q[0] : v[0];
                v[1] = on[0] ? v[1] + q[0] : v[1];
                v[1] = on[1] ? v[1] + q[1] : v[1];
                v[2] = on[1] ? v[2] + q[1] : v[2];
                v[3] = on[1] ? v[3] + q[1] : v[3];
                v[3] = on[2] ? v[3] + q[2] : v[3];
            }
        }
        if (live) *reinterpret_cast<float4*>(dx + s0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

static int pool2d_extent(const bcnn_hip_pool2d_desc* d, int in) {
    if (!d || (d->kind != POOL_MAX && d->kind != POOL_AVG) || d->size < 1 || d->stride < 1 || d->pad < 0 ||
        d->pad > d->size / 2 || in < 1 || (long long)in + 2LL * d->pad < d->size)
        return 0;
    const long long span = (long long)in + 2LL * d->pad - d->size;
    long long out = (d->ceil_mode ? (span + d->stride - 1) / d->stride : span / d->stride) + 1;
    // ceil mode: the last window must start inside the input or its leading padding
    if (d->ceil_mode && (out - 1) * d->stride >= (long long)in + d->pad) --out;
    return out > 0 && out < 0x7fffffffLL ? (int)out : 0;
}

// geometry and the limits of the int32 index format; exits like every other entry point handed a shape it cannot run
static Pool2dGeom pool2d_geom(const char* who, const bcnn_hip_pool2d_desc* d, int n, int c, int h, int w, long long& in_total,
                              long long& out_total) {
    Pool2dGeom g{};
    const int oh = pool2d_extent(d, h), ow = pool2d_extent(d, w);
    in_total = (long long)n * c * h * w;
    out_total = (long long)n * c * oh * ow;
    if (n < 0 || c < 0 || oh < 1 || ow < 1 || in_total >= 0x7fffffffLL || out_total >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] %s: invalid pooling parameters, or a tensor of 2^31 elements or more "
                        "(ask bcnn_hip_pool2d_out_extent)\n", who);
        exit(1);
    }
    g.H = h; g.W = w; g.OH = oh; g.OW = ow;
    g.size = d->size; g.stride = d->stride; g.pad = d->pad;
    g.include_pad = d->kind == POOL_AVG && d->count_include_pad;
    return g;
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_pool2d_out_extent(const bcnn_hip_pool2d_desc* desc, int in) { return pool2d_extent(desc, in); }

void bcnn_hip_pool2d_forward(const bcnn_hip_pool2d_desc* desc, const float* x, float* y, int* indexes, int n, int c, int h,
                             int w) {
    long long in_total, total;
    const Pool2dGeom g = pool2d_geom("bcnn_hip_pool2d_forward", desc, n, c, h, w, in_total, total);
    if (!total) return;
    const bool is_max = desc->kind == POOL_MAX;
    if (!is_max) indexes = nullptr;
    const FastDiv doh = make_fdiv((unsigned)g.OH, (unsigned long long)n * c * g.OH);
    const bool s2 = g.stride == 2 && ((g.size == 2 && g.pad == 0) || (g.size == 3 && g.pad == 1));
    if (s2 && (w & 3) == 0 && al16(x)) {
        const unsigned qpr = (unsigned)(g.OW + 3) / 4;  // items per output row
        const long long items = (long long)n * c * g.OH * qpr;
        const FastDiv dq = make_fdiv(qpr, (unsigned long long)items);
        const bool vec = (g.OW & 3) == 0 && al16(y) && al16(indexes);
        const int grid = stream_grid((size_t)items, 256);
#define BCNN_POOL2D_FWD_S2(KIND, SIZE, NAME)                                                                              \
    do {                                                                                                                  \
        trace_kernel(vec ? NAME ":v4" : NAME);                                                                            \
        if (vec) pool2d_fwd_s2x4_kernel<KIND, SIZE, true><<<grid, 256, 0, current_stream()>>>(x, y, indexes, g, dq, doh, (unsigned)items); \
        else pool2d_fwd_s2x4_kernel<KIND, SIZE, false><<<grid, 256, 0, current_stream()>>>(x, y, indexes, g, dq, doh, (unsigned)items);    \
    } while (0)
        if (is_max && g.size == 3) BCNN_POOL2D_FWD_S2(POOL_MAX, 3, "pool2d_fwd_s2x4_kernel<max,3>");
        else if (is_max) BCNN_POOL2D_FWD_S2(POOL_MAX, 2, "pool2d_fwd_s2x4_kernel<max,2>");
        else if (g.size == 3) BCNN_POOL2D_FWD_S2(POOL_AVG, 3, "pool2d_fwd_s2x4_kernel<avg,3>");
        else BCNN_POOL2D_FWD_S2(POOL_AVG, 2, "pool2d_fwd_s2x4_kernel<avg,2>");
#undef BCNN_POOL2D_FWD_S2
        KERNEL_CHECK();
        return;
    }
    const FastDiv dow = make_fdiv((unsigned)g.OW, (unsigned long long)total);
    const int grid = stream_grid((size_t)total, 256);
    trace_kernel(is_max ? "pool2d_fwd_kernel<max>" : "pool2d_fwd_kernel<avg>");
    if (is_max) pool2d_fwd_kernel<POOL_MAX><<<grid, 256, 0, current_stream()>>>(x, y, indexes, g, dow, doh, (unsigned)total);
    else pool2d_fwd_kernel<POOL_AVG><<<grid, 256, 0, current_stream()>>>(x, y, indexes, g, dow, doh, (unsigned)total);
    KERNEL_CHECK();
}

void bcnn_hip_pool2d_backward(const bcnn_hip_pool2d_desc* desc, const float* dy, const int* indexes, float* dx, int n, int c,
                              int h, int w, int overwrite) {
    long long total, out_total;
    const Pool2dGeom g = pool2d_geom("bcnn_hip_pool2d_backward", desc, n, c, h, w, total, out_total);
    if (!total) return;
    const bool is_max = desc->kind == POOL_MAX;
    if (is_max && !indexes) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_pool2d_backward: max pooling needs the indexes its forward stored\n");
        exit(1);
    }
    const FastDiv dh = make_fdiv((unsigned)h, (unsigned long long)n * c * h);
    if ((w & 3) == 0 && al16(dx)) {
        const long long groups = total / 4;
        const FastDiv dw4 = make_fdiv((unsigned)(w / 4), (unsigned long long)groups);
        const int grid = stream_grid((size_t)groups, 256);
#define BCNN_POOL2D_BWD_V4(KIND, CS, CST, CP, NAME)                                                                       \
    do {                                                                                                                  \
        trace_kernel(overwrite ? NAME ":overwrite" : NAME);                                                               \
        if (overwrite) pool2d_bwd_vec4_kernel<KIND, true, CS, CST, CP><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups); \
        else pool2d_bwd_vec4_kernel<KIND, false, CS, CST, CP><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups);          \
    } while (0)
        const bool k3 = g.size == 3 && g.stride == 2 && g.pad == 1, k2 = g.size == 2 && g.stride == 2 && g.pad == 0;
        const bool al8 = ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(indexes)) & 7) == 0;
        if (k3 && g.OW * 2 == w && al8) {  // out_w even: every pair starts on an 8-byte boundary
            trace_kernel(is_max ? (overwrite ? "pool2d_bwd_k3s2p1_pair_kernel<max>:overwrite" : "pool2d_bwd_k3s2p1_pair_kernel<max>")
                                : (overwrite ? "pool2d_bwd_k3s2p1_pair_kernel<avg>:overwrite" : "pool2d_bwd_k3s2p1_pair_kernel<avg>"));
            if (is_max && overwrite) pool2d_bwd_k3s2p1_pair_kernel<POOL_MAX, true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups);
            else if (is_max) pool2d_bwd_k3s2p1_pair_kernel<POOL_MAX, false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups);
            else if (overwrite) pool2d_bwd_k3s2p1_pair_kernel<POOL_AVG, true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups);
            else pool2d_bwd_k3s2p1_pair_kernel<POOL_AVG, false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw4, dh, (unsigned)groups);
        } else if (is_max && k3) BCNN_POOL2D_BWD_V4(POOL_MAX, 3, 2, 1, "pool2d_bwd_vec4_kernel<max,3,2,1>");
        else if (is_max && k2) BCNN_POOL2D_BWD_V4(POOL_MAX, 2, 2, 0, "pool2d_bwd_vec4_kernel<max,2,2,0>");
        else if (is_max) BCNN_POOL2D_BWD_V4(POOL_MAX, 0, 0, 0, "pool2d_bwd_vec4_kernel<max>");
        else if (k3) BCNN_POOL2D_BWD_V4(POOL_AVG, 3, 2, 1, "pool2d_bwd_vec4_kernel<avg,3,2,1>");
        else if (k2) BCNN_POOL2D_BWD_V4(POOL_AVG, 2, 2, 0, "pool2d_bwd_vec4_kernel<avg,2,2,0>");
        else BCNN_POOL2D_BWD_V4(POOL_AVG, 0, 0, 0, "pool2d_bwd_vec4_kernel<avg>");
#undef BCNN_POOL2D_BWD_V4
        KERNEL_CHECK();
        return;
    }
    const FastDiv dw = make_fdiv((unsigned)w, (unsigned long long)total);
    const int grid = stream_grid((size_t)total, 256);
    if (is_max) {
        trace_kernel(overwrite ? "pool2d_bwd_kernel<max>:overwrite" : "pool2d_bwd_kernel<max>");
        if (overwrite) pool2d_bwd_kernel<POOL_MAX, true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw, dh, (unsigned)total);
        else pool2d_bwd_kernel<POOL_MAX, false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw, dh, (unsigned)total);
    } else {
        trace_kernel(overwrite ? "pool2d_bwd_kernel<avg>:overwrite" : "pool2d_bwd_kernel<avg>");
        if (overwrite) pool2d_bwd_kernel<POOL_AVG, true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw, dh, (unsigned)total);
        else pool2d_bwd_kernel<POOL_AVG, false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, g, dw, dh, (unsigned)total);
    }
    KERNEL_CHECK();
}

}  // extern "C"
