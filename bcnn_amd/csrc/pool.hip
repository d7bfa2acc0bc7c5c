// pool.hip -- max pooling (bit-exact indices) and global average pooling. HBM-bound.
//
// Reference semantics: src/layers/bcnn_maxpool_layer.c:145-191 (forward), :258-273 (backward),
// src/layers/bcnn_avgpool_layer.c:82-99, 109-125.
#include <cfloat>

#include "batchnorm.h"
#include "bn_math.h"

namespace bcnn_hip {

// One thread per output element; consecutive lanes take consecutive output columns, so the window
// rows they read are contiguous (stride `stride` floats) and the value/index stores are coalesced.
// Window origin (i*stride, j*stride): padding exists only at the bottom/right; out-of-range taps
// read as -FLT_MAX; scan rows outer / cols inner; replace only on `>`: the first maximum wins and a
// NaN never wins. The index is the flat offset into the WHOLE source tensor (int32), as stored by
// the reference -- compared bit-for-bit in tests.
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          int* __restrict__ idx, int planes, int H, int W,
                                                          int OH, int OW, int size, int stride,
                                                          unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gstride) {
        const unsigned j = o % (unsigned)OW, t = o / (unsigned)OW;
        const unsigned i = t % (unsigned)OH, plane = t / (unsigned)OH;
        const int base = (int)plane * H * W;
        float best = -FLT_MAX;
        int bi = -1;
        for (int r = 0; r < size; ++r) {
            const int hh = (int)i * stride + r;
            for (int q = 0; q < size; ++q) {
                const int ww = (int)j * stride + q;
                const int si = base + hh * W + ww;
                const bool ok = hh < H && ww < W;
                const float v = ok ? x[si] : -FLT_MAX;
                if (v > best) { best = v; bi = si; }
            }
        }
        y[o] = best;
        idx[o] = bi;
    }
}

// Stride-2 windows of size 2 or 3 (the ResNet / LeNet pools): one thread per TWO consecutive outputs of a row.
// Their windows span source columns 4q .. 4q+3 (+1 for size 3): one aligned 16-byte load (+ one scalar) per
// window row instead of 2 x SIZE scalar loads, one pair of divisions per two outputs. Scan order, strict
// `>` and the flat int32 index are those of the generic kernel (bit-exact).
template <int SIZE>
__global__ __launch_bounds__(256) void maxpool_fwd_s2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             int* __restrict__ idx, int H, int W, int OH, int OW,
                                                             unsigned total_pairs) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total_pairs) return;
    const unsigned ppr = (unsigned)(OW + 1) >> 1;  // output pairs per row
    const unsigned rowid = t / ppr, q = t - rowid * ppr;
    const unsigned plane = rowid / (unsigned)OH, i = rowid - plane * (unsigned)OH;
    const int base = (int)plane * H * W;
    const int w0 = (int)q * 4;  // first source column of the pair (W % 4 == 0 => the 16-byte load is in range)
    float best[2] = {-FLT_MAX, -FLT_MAX};
    int bi[2] = {-1, -1};
#pragma unroll
    for (int r = 0; r < SIZE; ++r) {
        const int hh = (int)i * 2 + r;
        if (hh >= H) continue;  // bottom padding: every tap of the row reads as -FLT_MAX and never wins
        const int rb = base + hh * W + w0;
        const float4 v4 = *reinterpret_cast<const float4*>(x + rb);
        const float v[5] = {v4.x, v4.y, v4.z, v4.w, (SIZE == 3 && w0 + 4 < W) ? x[rb + 4] : -FLT_MAX};
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int c = 0; c < SIZE; ++c) {
                const float val = v[2 * o + c];
                if (val > best[o]) { best[o] = val; bi[o] = rb + 2 * o + c; }
            }
    }
    const unsigned out = rowid * (unsigned)OW + q * 2;
    y[out] = best[0];
    idx[out] = bi[0];
    if ((int)(q * 2 + 1) < OW) {
        y[out + 1] = best[1];
        idx[out + 1] = bi[1];
    }
}

// The same windows over act(batch-norm(x)) computed on the fly: the pooling node behind a convolution node with batch-norm
// whose pre-normalisation output x is kept anyway (the ResNet stem). The normalised tensor -- four times the size of the
// pooled one -- is then never written nor read back. Values, scan order and indexes are those of bn apply + the kernel
// above (same bn_one arithmetic per element).
#ifdef BCNN_HIP_EXPERIMENT  // reachable with BCNN_HIP_POOL_PAIR_V1: the reference of the second generation below
template <int SIZE, int R>  // R consecutive output rows per thread: their 2R + SIZE - 2 source rows are normalised once each
__global__ __launch_bounds__(256) void maxpool_fwd_s2_bn_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                int* __restrict__ idx, int C, int H, int W, int OH, int OW,
                                                                unsigned total_items, const float* __restrict__ mean,
                                                                const float* __restrict__ var, const float* __restrict__ scale,
                                                                const float* __restrict__ bias, int act,
                                                                float* __restrict__ raw_at_max) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total_items) return;
    const unsigned ppr = (unsigned)(OW + 1) >> 1;       // output pairs per row
    const unsigned rgs = (unsigned)(OH + R - 1) / R;    // row groups per plane
    const unsigned rowid = t / ppr, q = t - rowid * ppr;
    const unsigned plane = rowid / rgs, i0 = (rowid - plane * rgs) * R;
    const int ch = (int)(plane % (unsigned)C);
    const float m = mean[ch], sc = scale[ch], b = bias[ch];
    const BnDiv rs = bn_divisor(sqrtf(var[ch] + 0.000001f));
    const int base = (int)plane * H * W;
    const int w0 = (int)q * 4;
    float best[R][2], braw[R][2];
    int bi[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r][0] = best[r][1] = -FLT_MAX; bi[r][0] = bi[r][1] = -1; braw[r][0] = braw[r][1] = 0.f; }
    float dummy;
    const bool tail = SIZE == 3 && w0 + 4 < W;
    const bool keep = raw_at_max != nullptr;  // uniform
#pragma unroll
    for (int rr = 0; rr < 2 * R + SIZE - 2; ++rr) {
        const int hh = (int)i0 * 2 + rr;
        if (hh >= H) continue;  // bottom padding: the row never wins
        const int rb = base + hh * W + w0;
        const float4 v4 = *reinterpret_cast<const float4*>(x + rb);
        const float raw[5] = {v4.x, v4.y, v4.z, v4.w, tail ? x[rb + 4] : 0.f};
        const float v[5] = {bn_one(raw[0], m, rs, sc, b, 0, act, &dummy), bn_one(raw[1], m, rs, sc, b, 0, act, &dummy),
                            bn_one(raw[2], m, rs, sc, b, 0, act, &dummy), bn_one(raw[3], m, rs, sc, b, 0, act, &dummy),
                            tail ? bn_one(raw[4], m, rs, sc, b, 0, act, &dummy) : -FLT_MAX};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = rr - 2 * r;  // window row of output row i0 + r; ascending rr == ascending k: the scan order
            if (k < 0 || k >= SIZE) continue;
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int c = 0; c < SIZE; ++c) {
                    const float val = v[2 * o + c];
                    if (val > best[r][o]) {
                        best[r][o] = val;
                        bi[r][o] = rb + 2 * o + c;
                        if (keep) braw[r][o] = raw[2 * o + c];
                    }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if ((int)(i0 + r) >= OH) break;
        const unsigned out = (plane * (unsigned)OH + i0 + r) * (unsigned)OW + q * 2;
        y[out] = best[r][0];
        idx[out] = bi[r][0];
        // the pre-normalisation value that won: what the backward pass needs of x at the only places where the pooled
        // gradient lands (bcnn_hip_maxpool_bn_backward)
        if (keep) raw_at_max[out] = braw[r][0];
        if ((int)(q * 2 + 1) < OW) {
            y[out + 1] = best[r][1];
            idx[out + 1] = bi[r][1];
            if (keep) raw_at_max[out + 1] = braw[r][1];
        }
    }
}
#endif

// ---- the same kernel, second generation: bound by memory instead of the vector ALU -----------------------------------------------
// What changed against maxpool_fwd_s2_bn_kernel (kept in the experiment build as the bit-for-bit reference):
//  * a row's fifth column (size 3) is the NEXT thread's first column: its raw and normalised values come over a DPP wave shift
//    instead of a second load and a fifth bn_one. A wave therefore carries 63 items; lane 63 repeats the next wave's first
//    item only to feed lane 62 and stores nothing (an instruction issued for one lane costs what it costs for 64, so a
//    fetched fallback in lane 63 would give the saving back);
//  * the activation is a template parameter, and the bcnn_scal / bcnn_add_scalar quirks are classified once per wave: unless
//    a lane's channel has scale 0 or bias 1 the element is mul + add (x * 1.0f and x + -0.0f are identities bit for bit, so
//    scale 1 and bias 0 need no select), otherwise the whole wave runs bn_one as before;
//  * the three index divisions are multiply-high by constants from the host; 8-byte stores where the pairs are aligned.
struct BnFwdCoef {
    float m, sc, b, badd;  // badd: b, or -0.0f for b == 0 (the add the reference skips)
    BnDiv rs;
};
template <int ACT, bool QUIRK>  // ACT < 0: the run-time `act`
__device__ __forceinline__ float bn_fwd_t(float x, const BnFwdCoef& k, int act) {
    const int a = ACT >= 0 ? ACT : act;
    if (QUIRK) {
        float dummy;
        return bn_one(x, k.m, k.rs, k.sc, k.b, 0, a, &dummy);
    }
    const float v = __fadd_rn(__fmul_rn(bn_div(__fsub_rn(x, k.m), k.rs), k.sc), k.badd);
    return act_fwd_cheap(v, a, 0.f);
}
// a / d by multiply-high with magic = ceil(2^32 / d): exact while a * d < 2^32; the host passes 0 where that does not hold
__device__ __forceinline__ unsigned div_by(unsigned a, unsigned d, unsigned magic) { return magic ? __umulhi(a, magic) : a / d; }
__device__ __forceinline__ float dpp_shl1(float old, float v) {  // lane i takes lane i + 1's value; lane 63 keeps `old`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                                 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

struct PoolBnFwdArgs {
    const float* x; float* y; int* idx; float* raw_at_max;
    const float *mean, *var, *scale, *bias;
    int C, H, W, OH, OW, act, vec2;
    unsigned total_items, ppr, rgs, ppr_magic, rgs_magic, c_magic;
};

template <int SIZE, int R, int ACT, bool QUIRK>
__device__ __forceinline__ void maxpool_fwd_s2_bn_body(const PoolBnFwdArgs& a, const BnFwdCoef& k, int base, int w0, unsigned i0,
                                                       unsigned q, unsigned out0, bool tail, bool self_tail, bool any_self, bool store,
                                                       const float4 (&rows)[2 * R + SIZE - 2]) {
    const float* __restrict__ x = a.x;
    const int H = a.H, W = a.W;
    const bool keep = a.raw_at_max != nullptr;  // uniform
    float best[R][2], braw[R][2];
    int bi[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r][0] = best[r][1] = -FLT_MAX; bi[r][0] = bi[r][1] = -1; braw[r][0] = braw[r][1] = 0.f; }
#pragma unroll
    for (int rr = 0; rr < 2 * R + SIZE - 2; ++rr) {
        const int hh = (int)i0 * 2 + rr;
        if (hh >= H) continue;  // bottom padding: the row never wins (a thread and its right neighbour agree on this)
        const int rb = base + hh * W + w0;
        const float4 v4 = rows[rr];
        float raw[5] = {v4.x, v4.y, v4.z, v4.w, 0.f};
        float v[5] = {bn_fwd_t<ACT, QUIRK>(raw[0], k, a.act), bn_fwd_t<ACT, QUIRK>(raw[1], k, a.act),
                      bn_fwd_t<ACT, QUIRK>(raw[2], k, a.act), bn_fwd_t<ACT, QUIRK>(raw[3], k, a.act), -FLT_MAX};
        if (SIZE == 3) {
            float n4 = dpp_shl1(v[0], v[0]);
            if (keep) raw[4] = dpp_shl1(raw[0], raw[0]);
            if (any_self) {  // uniform; a pair that needs a fifth column but ends its row (out_w below the natural size)
                if (self_tail) {
                    raw[4] = x[rb + 4];
                    n4 = bn_fwd_t<ACT, QUIRK>(raw[4], k, a.act);
                }
            }
            v[4] = tail ? n4 : -FLT_MAX;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int kr = rr - 2 * r;  // window row of output row i0 + r; ascending rr == ascending kr: the scan order
            if (kr < 0 || kr >= SIZE) continue;
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int c = 0; c < SIZE; ++c) {
                    const float val = v[2 * o + c];
                    if (val > best[r][o]) {
                        best[r][o] = val;
                        bi[r][o] = rb + 2 * o + c;
                        if (keep) braw[r][o] = raw[2 * o + c];
                    }
                }
        }
    }
    if (!store) return;
    const bool second = (int)(q * 2 + 1) < a.OW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if ((int)(i0 + r) >= a.OH) break;
        const unsigned out = out0 + (unsigned)r * (unsigned)a.OW;
        if (a.vec2) {
            *reinterpret_cast<float2*>(a.y + out) = make_float2(best[r][0], best[r][1]);
            *reinterpret_cast<int2*>(a.idx + out) = make_int2(bi[r][0], bi[r][1]);
            // the pre-normalisation value that won: what the backward pass needs of x at the only places where the pooled
            // gradient lands (bcnn_hip_maxpool_bn_backward)
            if (keep) *reinterpret_cast<float2*>(a.raw_at_max + out) = make_float2(braw[r][0], braw[r][1]);
        } else {
            a.y[out] = best[r][0];
            a.idx[out] = bi[r][0];
            if (keep) a.raw_at_max[out] = braw[r][0];
            if (second) {
                a.y[out + 1] = best[r][1];
                a.idx[out + 1] = bi[r][1];
                if (keep) a.raw_at_max[out + 1] = braw[r][1];
            }
        }
    }
}

template <int SIZE, int R, int ACT>
__global__ __launch_bounds__(256) void maxpool_fwd_s2_bn_v2_kernel(const PoolBnFwdArgs a) {
    constexpr unsigned LANES = SIZE == 3 ? 63u : 64u;  // items per wave
    const unsigned lane = threadIdx.x & 63u;
    const unsigned t = (blockIdx.x * 4u + (threadIdx.x >> 6)) * LANES + lane;
    const bool store = lane < LANES && t < a.total_items;
    const unsigned tt = t < a.total_items ? t : a.total_items - 1u;  // no early return: the wave shift wants every lane
    const unsigned rowid = div_by(tt, a.ppr, a.ppr_magic), q = tt - rowid * a.ppr;
    const unsigned plane = div_by(rowid, a.rgs, a.rgs_magic), i0 = (rowid - plane * a.rgs) * R;
    const int ch = (int)(plane - div_by(plane, (unsigned)a.C, a.c_magic) * (unsigned)a.C);
    BnFwdCoef k;
    k.m = a.mean[ch]; k.sc = a.scale[ch]; k.b = a.bias[ch];
    k.badd = k.b == 0.0f ? -0.0f : k.b;
    k.rs = bn_divisor(sqrtf(a.var[ch] + 0.000001f));
    const int base = (int)plane * a.H * a.W;
    const int w0 = (int)q * 4;
    const bool tail = SIZE == 3 && w0 + 4 < a.W;
    const bool self_tail = tail && q + 1 >= a.ppr;  // the next thread is not this row's next pair
    const bool any_self = __ballot(self_tail) != 0;
    const bool quirk = k.sc == 0.0f || k.b == 1.0f;
    const unsigned out0 = (plane * (unsigned)a.OH + i0) * (unsigned)a.OW + q * 2;
    // every source row's 16 bytes first, from row-clamped addresses and ahead of the branch on the channel's constants: behind
    // the per-row `hh >= H` test each load would wait for the row before it -- 2R + SIZE - 2 memory round trips in a chain
    // instead of as many loads in flight
    float4 rows[2 * R + SIZE - 2];
#pragma unroll
    for (int rr = 0; rr < 2 * R + SIZE - 2; ++rr) {
        const int hh = (int)i0 * 2 + rr;
        rows[rr] = *reinterpret_cast<const float4*>(a.x + base + (hh < a.H ? hh : a.H - 1) * a.W + w0);
    }
    if (__ballot(quirk) != 0) maxpool_fwd_s2_bn_body<SIZE, R, ACT, true>(a, k, base, w0, i0, q, out0, tail, self_tail, any_self, store, rows);
    else maxpool_fwd_s2_bn_body<SIZE, R, ACT, false>(a, k, base, w0, i0, q, out0, tail, self_tail, any_self, store, rows);
}

// Gather form of `dx[idx[o]] += dy[o]`: one thread per SOURCE element visits the (at most
// ceil(size/stride)^2) outputs whose window covers it, in ascending output order, and adds those
// that selected it. Same per-element addition order as the reference's ascending-o loop, no atomics.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                          float* __restrict__ dx, int H, int W, int OH, int OW,
                                                          int size, int stride, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gstride) {
        const unsigned w = s % (unsigned)W, t = s / (unsigned)W;
        const unsigned h = t % (unsigned)H, plane = t / (unsigned)H;
        // outputs i with i*stride <= h <= i*stride + size - 1
        int i0 = ((int)h - size + stride) / stride; if ((int)h - size + 1 <= 0) i0 = 0;
        int j0 = ((int)w - size + stride) / stride; if ((int)w - size + 1 <= 0) j0 = 0;
        int i1 = (int)h / stride; if (i1 > OH - 1) i1 = OH - 1;
        int j1 = (int)w / stride; if (j1 > OW - 1) j1 = OW - 1;
        float acc = dx[s];
        bool hit = false;
        const int obase = (int)plane * OH * OW;
        for (int i = i0; i <= i1; ++i)
            for (int j = j0; j <= j1; ++j) {
                const int o = obase + i * OW + j;
                if (idx[o] == (int)s) { acc += dy[o]; hit = true; }
            }
        if (hit) dx[s] = acc;
    }
}

// Same gather, vectorised: one thread per 4 consecutive source pixels of a row (16-byte read-modify-write of
// dx, one division per 4 elements). The windows covering the 4 pixels are visited
// in ascending output order, so every dx element still sees its additions in the reference's order.
// OVERWRITE: dx is known to hold zeros semantically (the executor proved this node is its only writer and skipped
// the zero fill): start from 0.f instead of loading, store always -- same sums bit for bit, a third of the traffic.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void maxpool_bwd_vec4_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                               float* __restrict__ dx, int H, int W, int OH, int OW,
                                                               int size, int stride) {
    const int W4 = W >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;  // (row, group of 4) within the plane
    const int plane = blockIdx.y;
    if (t >= H * W4) return;
    const int h = t / W4, w0 = (t - h * W4) * 4;
    const int s0 = (plane * H + h) * W + w0;
    int i0 = (h - size + stride) / stride; if (h - size + 1 <= 0) i0 = 0;
    int j0 = (w0 - size + stride) / stride; if (w0 - size + 1 <= 0) j0 = 0;
    int i1 = h / stride; if (i1 > OH - 1) i1 = OH - 1;
    int j1 = (w0 + 3) / stride; if (j1 > OW - 1) j1 = OW - 1;
    float4 v = OVERWRITE ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(dx + s0);
    bool hit = OVERWRITE;
    for (int i = i0; i <= i1; ++i) {
        const int o = (plane * OH + i) * OW;
        for (int j = j0; j <= j1; ++j) {
            const unsigned d = (unsigned)(idx[o + j] - s0);
            if (d < 4u) {
                const float g = dy[o + j];
                if (d == 0) v.x += g; else if (d == 1) v.y += g; else if (d == 2) v.z += g; else v.w += g;
                hit = true;
            }
        }
    }
    if (hit) *reinterpret_cast<float4*>(dx + s0) = v;
}

// 3x3 / stride 2 (the ResNet stem pool): at most 2 window rows x 3 window columns cover a group of 4 pixels.
// All six (index, gradient) pairs are loaded up front from clamped addresses -- twelve independent loads in flight
// instead of a load -> compare -> load chain per window -- and applied in the same (row, column) order as above,
// so the sums are bit-identical.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void maxpool_bwd_vec4_k3s2_kernel(const float* __restrict__ dy,
                                                                    const int* __restrict__ idx,
                                                                    float* __restrict__ dx, int H, int W, int OH,
                                                                    int OW) {
    const int W4 = W >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    if (t >= H * W4) return;
    const int h = t / W4, w0 = (t - h * W4) * 4;
    const int s0 = (plane * H + h) * W + w0;
    const int i0 = h >= 2 ? (h - 1) >> 1 : 0, j0 = w0 >= 2 ? (w0 - 1) >> 1 : 0;
    int i1 = h >> 1; if (i1 > OH - 1) i1 = OH - 1;
    int j1 = (w0 + 3) >> 1; if (j1 > OW - 1) j1 = OW - 1;
    int id[2][3];
    float g[2][3];
    bool ok[2][3];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int i = i0 + a, j = j0 + b;
            ok[a][b] = i <= i1 && j <= j1;
            const int o = (plane * OH + (i <= i1 ? i : i1)) * OW + (j <= j1 ? j : j1);
            id[a][b] = idx[o];
            g[a][b] = dy[o];
        }
    float4 v = OVERWRITE ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(dx + s0);
    bool hit = OVERWRITE;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const unsigned d = (unsigned)(id[a][b] - s0);
            if (ok[a][b] && d < 4u) {
                const float gg = g[a][b];
                if (d == 0) v.x += gg; else if (d == 1) v.y += gg; else if (d == 2) v.z += gg; else v.w += gg;
                hit = true;
            }
        }
    if (hit) *reinterpret_cast<float4*>(dx + s0) = v;
}

// The same for OW == W / 2 (the "same"-padded stem pool: 112 -> 56): the three window columns of thread k are 2k-1, 2k and
// 2k+1, so the pair (2k, 2k+1) is ONE aligned 8-byte load per row and tensor -- contiguous over the wave -- and column
// 2k-1 is the previous lane's second element (one DPP move; lane 0 of a wave fetches it itself). 4 + 4 memory
// instructions instead of 12 stride-2 gathers; same additions in the same order.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void maxpool_bwd_vec4_k3s2_pair_kernel(const float* __restrict__ dy,
                                                                         const int* __restrict__ idx,
                                                                         float* __restrict__ dx, int H, int W, int OH,
                                                                         int OW) {
    const int W4 = W >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    const bool live = t < H * W4;
    const int tt = live ? t : 0;
    const int h = tt / W4, k = tt - h * W4, w0 = k * 4;
    const int s0 = (plane * H + h) * W + w0;
    const int i0 = h >= 2 ? (h - 1) >> 1 : 0;
    int i1 = h >> 1; if (i1 > OH - 1) i1 = OH - 1;
    const bool need_left = k > 0, fetch_left = need_left && (threadIdx.x & 63) == 0;
    int id[2][3];
    float g[2][3];
    bool ok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 + a;
        ok[a] = live && i <= i1;
        const int o = (plane * OH + (i <= i1 ? i : i1)) * OW + 2 * k;
        const int2 ip = *reinterpret_cast<const int2*>(idx + o);
        const float2 gp = *reinterpret_cast<const float2*>(dy + o);
        const int ie = idx[fetch_left ? o - 1 : o];
        const float ge = dy[fetch_left ? o - 1 : o];
        id[a][0] = __builtin_amdgcn_update_dpp(ie, ip.y, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        g[a][0] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ge), __builtin_bit_cast(int, gp.y),
                                                                        0x138, 0xf, 0xf, false));
        id[a][1] = ip.x; g[a][1] = gp.x;
        id[a][2] = ip.y; g[a][2] = gp.y;
    }
    if (!live) return;
    float4 v = OVERWRITE ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(dx + s0);
    bool hit = OVERWRITE;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const unsigned d = (unsigned)(id[a][b] - s0);
            if (ok[a] && (b > 0 || need_left) && d < 4u) {
                const float gg = g[a][b];
                if (d == 0) v.x += gg; else if (d == 1) v.y += gg; else if (d == 2) v.z += gg; else v.w += gg;
                hit = true;
            }
        }
    if (hit) *reinterpret_cast<float4*>(dx + s0) = v;
}

// The pair kernel for a pooling node behind a convolution node with batch-norm (the ResNet stem), with that node's
// batch-norm backward apply step (bcnn_batchnorm_layer.c:292-296 behind the activation backward) on the four gradient
// values while they are in registers: dx[s] = bn_bwd(sum of the pooled gradients that selected s) is written straight into
// the convolution node's output-gradient tensor, which is then never written and re-read in its pooled-gradient form. The
// coefficients (dmean, dvar) come from sums taken over the POOLED tensors (bcnn_hip_maxpool_bn_backward below).
#ifdef BCNN_HIP_EXPERIMENT  // reachable with BCNN_HIP_POOL_PAIR_V1
__global__ __launch_bounds__(256) void maxpool_bwd_pair_bn_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                                  const float* __restrict__ raw, float* __restrict__ dx,
                                                                  int C, int H, int W, int OH, int OW,
                                                                  const float4* __restrict__ consts, unsigned w4_magic,
                                                                  float fM, float rfM, int act) {
    const int W4 = W >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    const bool live = t < H * W4;
    const int tt = live ? t : 0;
    // tt / W4 by multiply-high with ceil(2^32 / W4) (exact: tt * W4 < 2^32, checked by the launcher)
    const int h = W4 > 1 ? (int)__umulhi((unsigned)tt, w4_magic) : tt, k = tt - h * W4, w0 = k * 4;
    const int s0 = (plane * H + h) * W + w0;
    const int i0 = h >= 2 ? (h - 1) >> 1 : 0;
    int i1 = h >> 1; if (i1 > OH - 1) i1 = OH - 1;
    const bool need_left = k > 0, fetch_left = need_left && (threadIdx.x & 63) == 0;
    const float4 xv = *reinterpret_cast<const float4*>(raw + s0);
    int id[2][3];
    float g[2][3];
    bool ok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 + a;
        ok[a] = live && i <= i1;
        const int o = (plane * OH + (i <= i1 ? i : i1)) * OW + 2 * k;
        const int2 ip = *reinterpret_cast<const int2*>(idx + o);
        const float2 gp = *reinterpret_cast<const float2*>(dy + o);
        const int ie = idx[fetch_left ? o - 1 : o];
        const float ge = dy[fetch_left ? o - 1 : o];
        id[a][0] = __builtin_amdgcn_update_dpp(ie, ip.y, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        g[a][0] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ge), __builtin_bit_cast(int, gp.y),
                                                                        0x138, 0xf, 0xf, false));
        id[a][1] = ip.x; g[a][1] = gp.x;
        id[a][2] = ip.y; g[a][2] = gp.y;
    }
    if (!live) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const unsigned d = (unsigned)(id[a][b] - s0);
            if (ok[a] && (b > 0 || need_left) && d < 4u) {
                const float gg = g[a][b];
                if (d == 0) v.x += gg; else if (d == 1) v.y += gg; else if (d == 2) v.z += gg; else v.w += gg;
            }
        }
    // per-channel constants: the table bn_bwd_finalize_kernel left (wave-uniform: scalar loads). Four IEEE divisions and two
    // square roots per thread -- for four elements -- had made this kernel vector-ALU bound (profiles/r04_sq_step_resnet18.txt)
    const int ch = plane % C;
    const float4 k0 = consts[3 * ch], k1 = consts[3 * ch + 1], k2 = consts[3 * ch + 2];
    const float m = k0.x, sc = k0.y, bb = k1.z, dmm = k1.w, dv = k2.x;
    const BnDiv rs{k0.z, k0.w}, rs_fwd{k1.x, k1.y}, fMd{fM, rfM};
    float dummy;
    float4 o;
    o.x = bn_bwd_one(v.x, bn_one(xv.x, m, rs_fwd, sc, bb, 0, act, &dummy), xv.x, m, rs, sc, dmm, dv, fMd, act);
    o.y = bn_bwd_one(v.y, bn_one(xv.y, m, rs_fwd, sc, bb, 0, act, &dummy), xv.y, m, rs, sc, dmm, dv, fMd, act);
    o.z = bn_bwd_one(v.z, bn_one(xv.z, m, rs_fwd, sc, bb, 0, act, &dummy), xv.z, m, rs, sc, dmm, dv, fMd, act);
    o.w = bn_bwd_one(v.w, bn_one(xv.w, m, rs_fwd, sc, bb, 0, act, &dummy), xv.w, m, rs, sc, dmm, dv, fMd, act);
    *reinterpret_cast<float4*>(dx + s0) = o;
}
#endif

// ---- the same kernel, second generation (maxpool_bwd_pair_bn_kernel stays in the experiment build as the reference) ----------------
//  * scatter: window column 2k-1 covers source columns 4k-2 .. 4k, column 2k covers 4k .. 4k+2 and column 2k+1 covers
//    4k+2 .. 4k+4, so of the 6 x 4 (window, component) pairs only 2 x 6 can hit -- given indexes that lie inside their own
//    windows, which is what every forward kernel here writes. Each is one compare, one select and one add: `v + +0.f` is v bit
//    for bit (v starts at +0 and a sum is -0 only if both terms are), so a miss adds +0 instead of branching. Rows and
//    neighbours that do not count are masked once, on the index (-1 matches no source element);
//  * the channel is blockIdx.y: the activation is a template parameter and the bcnn_scal / bcnn_add_scalar quirks a uniform
//    branch (scale 0 or bias 1 run the reference expression as before; `g * 1.0f` and `x + -0.0f` are identities);
//  * ReLU and leaky ReLU: act'(y) asks only whether y > 0, and y > 0 exactly where the pre-activation value is > 0 (0.1f * v
//    never rounds across zero), so the activation itself is not evaluated; no activation: no forward value at all.
template <int ACT>  // ACT < 0: the run-time `act`
__global__ __launch_bounds__(256) void maxpool_bwd_pair_bn_v2_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                                     const float* __restrict__ raw, float* __restrict__ dx,
                                                                     int C, int H, int W, int OH, int OW,
                                                                     const float4* __restrict__ consts, unsigned w4_magic,
                                                                     float fM, float rfM, int act_rt) {
    const int act = ACT >= 0 ? ACT : act_rt;
    const int W4 = W >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    if ((int)(blockIdx.x * 256 + (threadIdx.x & ~63u)) >= H * W4) return;  // a whole wave past the plane (uniform)
    const bool live = t < H * W4;
    const int tt = live ? t : 0;
    // tt / W4 by multiply-high with ceil(2^32 / W4) (exact: tt * W4 < 2^32, checked by the launcher)
    const int h = W4 > 1 ? (int)__umulhi((unsigned)tt, w4_magic) : tt, k = tt - h * W4, w0 = k * 4;
    const int s0 = (plane * H + h) * W + w0;
    const int i0 = h >= 2 ? (h - 1) >> 1 : 0;
    int i1 = h >> 1; if (i1 > OH - 1) i1 = OH - 1;
    const bool need_left = k > 0, fetch_left = need_left && (threadIdx.x & 63) == 0;
    const float4 xv = *reinterpret_cast<const float4*>(raw + s0);
    int id[2][3], o[2], ie[2] = {-1, -1};
    float g[2][3], ge[2] = {0.f, 0.f};
    int2 ip[2];
    float2 gp[2];
    bool ok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 + a;
        ok[a] = live && i <= i1;
        o[a] = (plane * OH + (i <= i1 ? i : i1)) * OW + 2 * k;
        ip[a] = *reinterpret_cast<const int2*>(idx + o[a]);
        gp[a] = *reinterpret_cast<const float2*>(dy + o[a]);
    }
    // window column 2k-1 of a wave's first lane: nobody to shift it from. One branch for both rows and ahead of the shifts, so
    // that these loads go out with the others; the other lanes load nothing
    if (fetch_left) {
        ie[0] = idx[o[0] - 1]; ge[0] = dy[o[0] - 1];
        ie[1] = idx[o[1] - 1]; ge[1] = dy[o[1] - 1];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        // rows that do not count, masked on the index; the left neighbour is on this row: the same `ok`
        ip[a].x = ok[a] ? ip[a].x : -1; ip[a].y = ok[a] ? ip[a].y : -1; ie[a] = ok[a] ? ie[a] : -1;
        const int il = __builtin_amdgcn_update_dpp(ie[a], ip[a].y, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        id[a][0] = need_left ? il : -1;
        g[a][0] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ge[a]), __builtin_bit_cast(int, gp[a].y),
                                                                        0x138, 0xf, 0xf, false));
        id[a][1] = ip[a].x; g[a][1] = gp[a].x;
        id[a][2] = ip[a].y; g[a][2] = gp[a].y;
    }
    // no early return: behind one, the loads that feed no wave shift sink past the branch and queue up behind the first batch
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < 2; ++a) {  // per component: rows ascending, columns ascending -- the order of the gather kernels above
        v.x += id[a][0] == s0 ? g[a][0] : 0.f;
        v.x += id[a][1] == s0 ? g[a][1] : 0.f;
        v.y += id[a][1] == s0 + 1 ? g[a][1] : 0.f;
        v.z += id[a][1] == s0 + 2 ? g[a][1] : 0.f;
        v.z += id[a][2] == s0 + 2 ? g[a][2] : 0.f;
        v.w += id[a][2] == s0 + 3 ? g[a][2] : 0.f;
    }
    // per-channel constants: the table bn_bwd_finalize_kernel left (wave-uniform: scalar loads)
    const int ch = plane % C;
    const float4 k0 = consts[3 * ch], k1 = consts[3 * ch + 1], k2 = consts[3 * ch + 2];
    const float m = k0.x, sc = k0.y, bb = k1.z, dmm = k1.w, dv = k2.x;
    const BnDiv rs{k0.z, k0.w}, rs_fwd{k1.x, k1.y}, fMd{fM, rfM};
    const float vin[4] = {v.x, v.y, v.z, v.w}, xin[4] = {xv.x, xv.y, xv.z, xv.w};
    float out[4];
    const bool fast_act = ACT == BCNN_HIP_ACT_NONE || ACT == BCNN_HIP_ACT_RELU || ACT == BCNN_HIP_ACT_LRELU;
    if (!fast_act || sc == 0.0f || (ACT != BCNN_HIP_ACT_NONE && bb == 1.0f)) {  // uniform
        float dummy;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[e] = bn_bwd_one(vin[e], bn_one(xin[e], m, rs_fwd, sc, bb, 0, act, &dummy), xin[e], m, rs, sc, dmm, dv, fMd, act);
    } else {
        const float dv2 = __fmul_rn(dv, 2.0f), badd = bb == 0.0f ? -0.0f : bb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xm = __fsub_rn(xin[e], m);
            float gg = vin[e];
            if (ACT != BCNN_HIP_ACT_NONE) {
                const float pre = __fadd_rn(__fmul_rn(bn_div(xm, rs_fwd), sc), badd);
                gg *= ACT == BCNN_HIP_ACT_RELU ? (float)(pre > 0) : (pre > 0 ? 1.0f : 0.1f);
            }
            gg = __fmul_rn(gg, sc);
            out[e] = __fadd_rn(__fadd_rn(bn_div(gg, rs), bn_div(__fmul_rn(dv2, xm), fMd)), dmm);
        }
    }
    if (live) *reinterpret_cast<float4*>(dx + s0) = make_float4(out[0], out[1], out[2], out[3]);
}

// Global average pooling: one wave64 per (n,c) plane, shuffle reduction, then / (H*W).
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          int planes, int HW) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int p = wave; p < planes; p += nwaves) {
        const float* src = x + (long long)p * HW;
        float s = 0.f;
        for (int i = lane; i < HW; i += 64) s += src[i];
        s = wave_sum(s);
        if (lane == 0) y[p] = s / (float)HW;
    }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                          int HW, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const unsigned p = i / (unsigned)HW;
        dx[i] += dy[p] / (float)HW;  // dst.grad / (h*w), int divisor promoted (bcnn_avgpool_layer.c:118-120)
    }
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

void bcnn_hip_maxpool_forward(const float* x, float* y, int* indexes, int n, int c, int h, int w, int out_h,
                              int out_w, int size, int stride) {
    const long long total = (long long)n * c * out_h * out_w;
    if (!total) return;
    // two outputs per thread need both windows inside the 16-byte load: out_w = ceil(w / 2) covers it when w % 4 == 0
    if (stride == 2 && (size == 2 || size == 3) && (w & 3) == 0 && out_w * 2 <= w + 1 &&
        (long long)n * c * h * w < 0x7fffffffLL && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const long long pairs = (long long)n * c * out_h * ((out_w + 1) / 2);
        const unsigned blocks = (unsigned)((pairs + 255) / 256);
        trace_kernel(size == 2 ? "maxpool_fwd_s2_kernel<2>" : "maxpool_fwd_s2_kernel<3>");
        if (size == 2) maxpool_fwd_s2_kernel<2><<<blocks, 256, 0, current_stream()>>>(x, y, indexes, h, w, out_h, out_w, (unsigned)pairs);
        else maxpool_fwd_s2_kernel<3><<<blocks, 256, 0, current_stream()>>>(x, y, indexes, h, w, out_h, out_w, (unsigned)pairs);
        KERNEL_CHECK();
        return;
    }
    trace_kernel("maxpool_fwd_kernel");
    maxpool_fwd_kernel<<<stream_grid((size_t)total, 256), 256, 0, current_stream()>>>(
        x, y, indexes, n * c, h, w, out_h, out_w, size, stride, (unsigned)total);
    KERNEL_CHECK();
}

int bcnn_hip_maxpool_bn_fusable(int n, int c, int h, int w, int out_h, int out_w, int size, int stride, int act,
                                 const float* x) {
    return stride == 2 && (size == 2 || size == 3) && (w & 3) == 0 && out_w * 2 <= w + 1 &&
           (long long)n * c * h * w < 0x7fffffffLL && x && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && act_is_cheap(act) &&
           act != BCNN_HIP_ACT_PRELU;
}

void bcnn_hip_maxpool_forward_bn_keep(const float* x, float* y, int* indexes, int n, int c, int h, int w, int out_h, int out_w,
                                      int size, int stride, const float* scales, const float* bias, const float* mean,
                                      const float* var, int act, float* raw_at_max) {
    const long long total = (long long)n * c * out_h * out_w;
    if (!total) return;
    if (!bcnn_hip_maxpool_bn_fusable(n, c, h, w, out_h, out_w, size, stride, act, x)) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_maxpool_forward_bn: not fusable (ask bcnn_hip_maxpool_bn_fusable)\n");
        exit(1);
    }
    // raw in; pooled values, indexes and (when kept) the raw values that won out
    KTimer kt(K_POOL, 0.0, 4.0 * ((double)n * c * h * w + (raw_at_max ? 3.0 : 2.0) * (double)total));
    constexpr int R = 4;
    const long long items = (long long)n * c * ((out_h + R - 1) / R) * ((out_w + 1) / 2);
#ifdef BCNN_HIP_EXPERIMENT
    if (BCNN_EXP_ENV("BCNN_HIP_POOL_PAIR_V1")) {
        trace_kernel("maxpool_fwd_s2_bn_kernel:v1");
        const unsigned blocks = (unsigned)((items + 255) / 256);
        if (size == 2)
            maxpool_fwd_s2_bn_kernel<2, R><<<blocks, 256, 0, current_stream()>>>(x, y, indexes, c, h, w, out_h, out_w,
                                                                                 (unsigned)items, mean, var, scales, bias, act,
                                                                                 raw_at_max);
        else
            maxpool_fwd_s2_bn_kernel<3, R><<<blocks, 256, 0, current_stream()>>>(x, y, indexes, c, h, w, out_h, out_w,
                                                                                 (unsigned)items, mean, var, scales, bias, act,
                                                                                 raw_at_max);
        KERNEL_CHECK();
        return;
    }
#endif
    trace_kernel("maxpool_fwd_s2_bn_kernel");  // the family name: both generations
    PoolBnFwdArgs a;
    a.x = x; a.y = y; a.idx = indexes; a.raw_at_max = raw_at_max;
    a.mean = mean; a.var = var; a.scale = scales; a.bias = bias;
    a.C = c; a.H = h; a.W = w; a.OH = out_h; a.OW = out_w; a.act = act;
    const uintptr_t p8 = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(indexes) | reinterpret_cast<uintptr_t>(raw_at_max);
    a.vec2 = (out_w & 1) == 0 && (p8 & 7) == 0;
    a.total_items = (unsigned)items;
    a.ppr = (unsigned)((out_w + 1) / 2);
    a.rgs = (unsigned)((out_h + R - 1) / R);
    // multiply-high division (the kernel's div_by): exact while dividend * divisor < 2^32; every dividend is below `items`
    auto magic = [items](unsigned d) {
        return d > 1 && items * (long long)d < (1LL << 32) ? (unsigned)((0x100000000ULL + d - 1) / d) : 0u;
    };
    a.ppr_magic = magic(a.ppr); a.rgs_magic = magic(a.rgs); a.c_magic = magic((unsigned)c);
    const unsigned per_block = size == 3 ? 4u * 63u : 256u;  // size 3: 63 items per wave (see the kernel)
    const unsigned blocks = (unsigned)((items + per_block - 1) / per_block);
#define BCNN_POOL_FWD_V2(SIZE, ACT) maxpool_fwd_s2_bn_v2_kernel<SIZE, R, ACT><<<blocks, 256, 0, current_stream()>>>(a)
#define BCNN_POOL_FWD_V2_ACT(ACT) do { if (size == 2) BCNN_POOL_FWD_V2(2, ACT); else BCNN_POOL_FWD_V2(3, ACT); } while (0)
    switch (act) {
        case BCNN_HIP_ACT_NONE: BCNN_POOL_FWD_V2_ACT(BCNN_HIP_ACT_NONE); break;
        case BCNN_HIP_ACT_RELU: BCNN_POOL_FWD_V2_ACT(BCNN_HIP_ACT_RELU); break;
        case BCNN_HIP_ACT_LRELU: BCNN_POOL_FWD_V2_ACT(BCNN_HIP_ACT_LRELU); break;
        default: BCNN_POOL_FWD_V2_ACT(-1); break;
    }
#undef BCNN_POOL_FWD_V2_ACT
#undef BCNN_POOL_FWD_V2
    KERNEL_CHECK();
}

void bcnn_hip_maxpool_forward_bn(const float* x, float* y, int* indexes, int n, int c, int h, int w, int out_h, int out_w,
                                 int size, int stride, const float* scales, const float* bias, const float* mean,
                                 const float* var, int act) {
    bcnn_hip_maxpool_forward_bn_keep(x, y, indexes, n, c, h, w, out_h, out_w, size, stride, scales, bias, mean, var, act, nullptr);
}

int bcnn_hip_maxpool_bn_backward_fusable(int n, int c, int h, int w, int out_h, int out_w, int size, int stride, int act,
                                         const float* raw, const float* dpool, const int* indexes, const float* dx) {
    const uintptr_t p16 = reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(dx);
    const uintptr_t p8 = reinterpret_cast<uintptr_t>(dpool) | reinterpret_cast<uintptr_t>(indexes);
    return size == 3 && stride == 2 && (w & 3) == 0 && out_w * 2 == w && out_h * out_w > 0 &&
           (long long)n * c * h * w < 0x7fffffffLL && (long long)n * c <= 65535 && raw && dx && (p16 & 15) == 0 && (p8 & 7) == 0 &&
           (long long)h * (w / 4) * (w / 4) < (1LL << 32) &&  // the kernel's t / (W / 4) by multiply-high is exact only while t * (W / 4) < 2^32
           act_is_cheap(act) && act_bwd_is_cheap(act) && act != BCNN_HIP_ACT_PRELU;
}

void bcnn_hip_maxpool_bn_backward(const float* dpool, const int* indexes, const float* raw_at_max, const float* raw, float* dx,
                                  int n, int c, int h, int w, int out_h, int out_w, int size, int stride, const float* scales,
                                  float* dscales, const float* bias, float* dbias, const float* mean, const float* var,
                                  float* dmean, float* dvar, int act) {
    const long long total = (long long)n * c * h * w, ptotal = (long long)n * c * out_h * out_w;
    if (!total) return;
    if (!bcnn_hip_maxpool_bn_backward_fusable(n, c, h, w, out_h, out_w, size, stride, act, raw, dpool, indexes, dx) || !raw_at_max) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_maxpool_bn_backward: not fusable (ask bcnn_hip_maxpool_bn_backward_fusable)\n");
        exit(1);
    }
    float4* consts = scratch_f4(SCRATCH_BN_CONSTS, (size_t)c * 3);  // the per-channel constants the backward finalize leaves
    const float fM = (float)((long long)n * h * w);  // the un-pooled element count divides dmean and the dvar term
    // S1 = sum g act'(y), S2 = sum g act'(y) (x - mean) of the batch-norm backward: the gradient of the un-pooled tensor is
    // zero except where a window's maximum sits, and there it is the sum of the pooled gradients that selected the place --
    // so both sums are sums over the POOLED gradient against the pre-normalisation values that won (a quarter of the data;
    // the divisor of dmean / M and of the dvar term stays the un-pooled element count)
    {
        KTimer kt(K_BN_BWD, 0.0, 4.0 * 2.0 * (double)ptotal);
        BnBwdCall b{};
        b.dout = dpool; b.workspace = raw_at_max; b.act = act; b.e.n = n; b.e.c = c; b.e.hw = out_h * out_w;
        b.p.scales = scales; b.p.bias = act != BCNN_HIP_ACT_NONE ? bias : nullptr; b.s.mean = mean; b.s.var = var;
        b.g.dscales = dscales; b.g.dbias = dbias; b.g.dmean = dmean; b.g.dvar = dvar; b.consts = consts; b.consts_fM = fM;
        batchnorm_backward_sums(b);
    }
    KTimer kt(K_POOL, 0.0, 4.0 * (2.0 * (double)total + 2.0 * (double)ptotal));
    dim3 grid((unsigned)ceil_div(h * (w / 4), 256), (unsigned)(n * c));
    const unsigned w4 = (unsigned)(w / 4);
    const unsigned w4m = w4 > 1 ? (unsigned)((0x100000000ULL + w4 - 1) / w4) : 0u;
#ifdef BCNN_HIP_EXPERIMENT
    if (BCNN_EXP_ENV("BCNN_HIP_POOL_PAIR_V1")) {
        trace_kernel("maxpool_bwd_pair_bn_kernel:v1");
        maxpool_bwd_pair_bn_kernel<<<grid, 256, 0, current_stream()>>>(dpool, indexes, raw, dx, c, h, w, out_h, out_w, consts, w4m,
                                                                       fM, 1.0f / fM, act);
        KERNEL_CHECK();
        return;
    }
#endif
    trace_kernel("maxpool_bwd_pair_bn_kernel");  // the family name: both generations
#define BCNN_POOL_BWD_V2(ACT) \
    maxpool_bwd_pair_bn_v2_kernel<ACT><<<grid, 256, 0, current_stream()>>>(dpool, indexes, raw, dx, c, h, w, out_h, out_w, consts, \
                                                                            w4m, fM, 1.0f / fM, act)
    switch (act) {
        case BCNN_HIP_ACT_NONE: BCNN_POOL_BWD_V2(BCNN_HIP_ACT_NONE); break;
        case BCNN_HIP_ACT_RELU: BCNN_POOL_BWD_V2(BCNN_HIP_ACT_RELU); break;
        case BCNN_HIP_ACT_LRELU: BCNN_POOL_BWD_V2(BCNN_HIP_ACT_LRELU); break;
        default: BCNN_POOL_BWD_V2(-1); break;
    }
#undef BCNN_POOL_BWD_V2
    KERNEL_CHECK();
}

void bcnn_hip_maxpool_backward(const float* dy, const int* indexes, float* dx, int n, int c, int h, int w,
                               int out_h, int out_w, int size, int stride, int overwrite) {
    const long long total = (long long)n * c * h * w;
    if (!total) return;
    if (!(out_h * out_w)) {
        if (overwrite) bcnn_hip_fill_f32(dx, (size_t)total, 0.f);
        return;
    }
    if ((w & 3) == 0 && total < 0x7fffffffLL && (long long)n * c <= 65535 &&
        (reinterpret_cast<uintptr_t>(dx) & 15) == 0) {
        dim3 grid((unsigned)ceil_div(h * (w / 4), 256), (unsigned)(n * c));
        const bool pairs = size == 3 && stride == 2 && out_w * 2 == w &&
                           ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(indexes)) & 7) == 0;
        if (pairs) {
            trace_kernel(overwrite ? "maxpool_bwd_vec4_k3s2_pair_kernel:overwrite" : "maxpool_bwd_vec4_k3s2_pair_kernel");
            if (overwrite) maxpool_bwd_vec4_k3s2_pair_kernel<true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w);
            else maxpool_bwd_vec4_k3s2_pair_kernel<false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w);
        } else if (size == 3 && stride == 2) {
            trace_kernel(overwrite ? "maxpool_bwd_vec4_k3s2_kernel:overwrite" : "maxpool_bwd_vec4_k3s2_kernel");
            if (overwrite) maxpool_bwd_vec4_k3s2_kernel<true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w);
            else maxpool_bwd_vec4_k3s2_kernel<false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w);
        } else {
            trace_kernel(overwrite ? "maxpool_bwd_vec4_kernel:overwrite" : "maxpool_bwd_vec4_kernel");
            if (overwrite) maxpool_bwd_vec4_kernel<true><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w, size, stride);
            else maxpool_bwd_vec4_kernel<false><<<grid, 256, 0, current_stream()>>>(dy, indexes, dx, h, w, out_h, out_w, size, stride);
        }
        KERNEL_CHECK();
        return;
    }
    if (overwrite) bcnn_hip_fill_f32(dx, (size_t)total, 0.f);
    trace_kernel(overwrite ? "maxpool_bwd_kernel:overwrite" : "maxpool_bwd_kernel");
    maxpool_bwd_kernel<<<stream_grid((size_t)total, 256), 256, 0, current_stream()>>>(
        dy, indexes, dx, h, w, out_h, out_w, size, stride, (unsigned)total);
    KERNEL_CHECK();
}

void bcnn_hip_avgpool_forward(const float* x, float* y, int n, int c, int h, int w) {
    const int planes = n * c;
    if (!planes) return;
    const int grid = stream_grid((size_t)planes * 64, 256);
    trace_kernel("avgpool_fwd_kernel");
    avgpool_fwd_kernel<<<grid, 256, 0, current_stream()>>>(x, y, planes, h * w);
    KERNEL_CHECK();
}

void bcnn_hip_avgpool_backward(const float* dy, float* dx, int n, int c, int h, int w) {
    const long long total = (long long)n * c * h * w;
    if (!total) return;
    trace_kernel("avgpool_bwd_kernel");
    avgpool_bwd_kernel<<<stream_grid((size_t)total, 256), 256, 0, current_stream()>>>(dy, dx, h * w, (unsigned)total);
    KERNEL_CHECK();
}

}  // extern "C"
