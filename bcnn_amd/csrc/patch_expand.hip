// patch_expand.hip -- the patch-expanding node (Swin-UNet's decoder step, depth-to-space, torch's PixelShuffle): the channels of
// src [N, P^2 c, H, W] move to the positions, dst [N, c, P H, P W] with P = 2 or 4: dst[n, ch, P h + p1, P w + p2] takes
// src[n, plane(ch, p1, p2), h, w]. Two orders of the source planes:
//   blocks  : plane = (p1 P + p2) c + ch -- einops 'b h w (p1 p2 c) -> b (h p1) (w p2) c', Swin-UNet's PatchExpand and
//             FinalPatchExpand_X4, TensorFlow / ONNX-DCR depth-to-space;
//   channels: plane = ch P^2 + p1 P + p2 -- torch.nn.PixelShuffle, ONNX CRD.
// The block index is ROW-MAJOR (p1 P + p2), as those models have it; patch merging's (patch_merge.hip) is 2 dx + dy, as Swin's
// encoder has it. Each follows the model it serves, so for P = 2 `blocks` is not the inverse of patch merging's rearrangement
// (INTEGRATION.md gives the permutation). With a norm every OUTPUT position is then normalised over its c values and mapped
// through scales[c], b[c], in the same launch: the rearranged tensor never exists in memory un-normalised.
//   forward : s = sum v, q = sum v^2 over the position's c values, added in DOUBLE; mean = s / c, var = max(q / c - mean^2, 0),
//             rstd = (float)(1 / sqrt(var + eps)); y = ((v - mean) * rstd) * scales[ch] + b[ch], one float32 rounding per
//             operation (-ffp-contract=off) on the stored float32 mean and rstd.
//   backward: xh = (v - mean) * rstd, t = dy * scales[ch]; per position ds = sum_ch t * xh, db = sum_ch t (float32 terms, added
//             in double, rounded once); dv = (t - (xh * ds + db) / c) * rstd goes back to where v came from; per channel
//             dscales[ch] += sum dy * xh, db[ch] += sum dy over all output positions.
// ADDRESSING. Lanes run along the flattened INPUT positions q = n H W + h W + w of all images (the mirror image of patch
// merging); a tile is 64 of them, one per lane. A source plane is read at q: every load instruction is 64 consecutive floats
// (where the tile crosses an image only the per-lane offset differs). For a fixed channel and block row p1 the lane's P values
// p2 = 0 .. P - 1 are adjacent in dst: ONE 8-byte (P = 2) or 16-byte (P = 4) store, a wave's store instruction covers 64 P
// consecutive floats of an output row. The store address is a multiple of P floats from the base because the output row is
// P W long, so the wide form depends on the base pointer alone; a base that is not aligned takes P 4-byte stores, same bits.
// WORK SPLIT. The P block rows of a position share nothing: no input plane, no statistic, no output row. A unit of work is
// therefore (tile, p1), one workgroup each in the forward (grid.y = p1): a lane carries P pairs of sums, not P^2, and the
// unit's P c values per position are what the register file has to hold, not P^2 c. The waves of the workgroup SPLIT THE
// OUTPUT CHANNELS: wave w takes [w cpw, (w + 1) cpw) and keeps their P cpw values per lane in registers (cpw the smallest
// of 2 .. 32 that needs no more waves than the workgroup has: 32 / P, so a lane may use 64 P registers for data at any
// P), the per-lane sums meet in LDS ([waves][P][2][64] doubles, 32 KB at most) and every thread adds them for its own lane in
// ascending wave order. Three paths, from c and P alone (bcnn_hip_patch_expand_path):
//   column (c <= 8)      : one wave per unit, the lane holds all P c values; no LDS, no barrier.
//   split  (c <= 1024 / P): the above; 512 channels at P = 2, 256 at P = 4.
//   stream (larger c)     : every wave sweeps its channels twice (statistics, then apply; the second read comes from L2).
// BACKWARD. A workgroup is persistent over the units u = g, g + G, ... (u = tile P + p1). Channels go in groups of four: the
// lane folds the P terms dy * xh and the P terms dy of each channel (float32), pe_reduce8 adds the eight values over the 64
// lanes in 10 cross-lane steps, lane 8 j ends with value j and adds it into the workgroup's [2][c] accumulators (doubles in
// LDS to c = 1024, the workgroup's own float row of the partials beyond; a channel has one owner wave and one owner lane).
// The workgroup writes one partial row; pe_finalize_kernel adds the rows in ascending order in double. A backward workgroup
// has 8 waves at most at either P. Up to four channels per wave (c <= 32) x and dy of a unit stay in registers between the
// sums and the data gradient, beyond that the data gradient re-reads them (from L2). dx is written per source plane, 64 consecutive floats per store instruction.
// No atomics; every order follows from the shape alone. No reference counterpart.
#include <algorithm>

#include "common.h"
#include "../../include/bcnn_hip.h"

namespace bcnn_hip {

constexpr int kPeTile = 64;            // input positions of a tile: one per lane of a wave
constexpr int kPeColumnMaxC = 8;       // one wave holds the P c values of a unit: 16 or 32 per lane
constexpr int kPeMaxCpw = 32;          // channels per wave held in registers, at most: 64 P data registers
constexpr int kPeBwdCpw = 4;           // the backward holds x and dy of one group of four channels per wave
constexpr int kPeBwdWaves = 8;         // waves of a backward workgroup, at most, at either P: 256 registers (with 16 waves
                                       // the re-reading P = 2 instance spilled 12 bytes under its 128)
constexpr int kPeAccLdsMaxC = 1024;    // c up to which the per-channel accumulators [2][c] are doubles in LDS (16 KB)
constexpr int kPeMaxGroups = 512;      // persistent workgroups of a backward launch, at most

// waves of a workgroup, at most: 16 (128 registers) at P = 2, 8 (256 registers) at P = 4; the sums' LDS is 32 KB for both
constexpr int pe_max_waves(int p) { return 32 / p; }
static int pe_split_max_c(int p) { return pe_max_waves(p) * kPeMaxCpw; }
static int pe_path(int c, int p) { return c <= kPeColumnMaxC ? 0 : (c <= pe_split_max_c(p) ? 1 : 2); }

// channels per wave of the register-holding forward: the whole column, or the smallest of 2 .. 32 within the workgroup's waves
static int pe_cpw(int c, int p) {
    if (c <= kPeColumnMaxC) return kPeColumnMaxC;
    for (int cpw = 2; cpw < kPeMaxCpw; cpw *= 2)
        if (ceil_div(c, cpw) <= pe_max_waves(p)) return cpw;
    return kPeMaxCpw;
}

struct PeGeom {
    long long Q;   // input positions of all images
    int c;         // output channels
    int W, HW;     // input row length, input plane
    int PW, PHW;   // output row length, output plane
    int cs, bs;    // source plane of (ch, block k = p1 P + p2) = ch cs + k bs
};

// this lane's input position of a unit (tile, p1): plane 0 of it in src, channel 0 of its P adjacent outputs in dst, and the
// first of those output positions
template <int P>
struct PePos {
    long long q;
    bool live;
    size_t src, dst, oq;
    __device__ PePos(long long tile, int p1, const PeGeom& g) {
        q = tile * kPeTile + (threadIdx.x & 63);
        live = q < g.Q;
        const long long n = live ? q / g.HW : 0;
        const int r = live ? (int)(q - n * g.HW) : 0;
        const int h = r / g.W, w = r - h * g.W;
        const size_t orow = (size_t)(P * h + p1) * g.PW + (size_t)(P * w);
        src = (size_t)n * P * P * g.c * g.HW + (size_t)r;
        dst = (size_t)n * g.c * g.PHW + orow;
        oq = (size_t)n * g.PHW + orow;
    }
};

// the P source values of channel ch in block row p1, p2 = 0 .. P - 1: one coalesced load per plane
template <int P>
__device__ __forceinline__ void pe_load_x(const float* x, size_t src, const PeGeom& g, int ch, int p1, float (&v)[P]) {
#pragma unroll
    for (int k = 0; k < P; ++k) v[k] = x[src + (size_t)(ch * g.cs + (p1 * P + k) * g.bs) * g.HW];
}

template <int P>
__device__ __forceinline__ void pe_store_x(float* x, size_t src, const PeGeom& g, int ch, int p1, const float (&v)[P], bool add) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const size_t at = src + (size_t)(ch * g.cs + (p1 * P + k) * g.bs) * g.HW;
        x[at] = add ? x[at] + v[k] : v[k];
    }
}

// the P adjacent floats at `at` of the rearranged side (y, dy): one 8- or 16-byte access, or P 4-byte ones
template <int P>
__device__ __forceinline__ void pe_load_wide(const float* y, size_t at, bool wide, float (&v)[P]) {
    if (!wide) {
#pragma unroll
        for (int k = 0; k < P; ++k) v[k] = y[at + k];
    } else if constexpr (P == 2) {
        const float2 r = *reinterpret_cast<const float2*>(y + at);
        v[0] = r.x; v[1] = r.y;
    } else {
        const float4 r = *reinterpret_cast<const float4*>(y + at);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
}

template <int P>
__device__ __forceinline__ void pe_store_wide(float* y, size_t at, bool wide, const float (&v)[P]) {
    if (!wide) {
#pragma unroll
        for (int k = 0; k < P; ++k) y[at + k] = v[k];
    } else if constexpr (P == 2) {
        *reinterpret_cast<float2*>(y + at) = make_float2(v[0], v[1]);
    } else {
        *reinterpret_cast<float4*>(y + at) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// this lane's totals of the waves' per-lane sums, waves in ascending order; red is [waves][P][2][64] doubles. One wave: no LDS
template <int P>
__device__ __forceinline__ void pe_totals(double* red, int waves, int wid, int lane, double (&a)[P], double (&b)[P]) {
    if (waves == 1) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        red[((wid * P + k) * 2 + 0) * kPeTile + lane] = a[k];
        red[((wid * P + k) * 2 + 1) * kPeTile + lane] = b[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P; ++k) {
        a[k] = 0.0;
        b[k] = 0.0;
        for (int w = 0; w < waves; ++w) {
            a[k] += red[((w * P + k) * 2 + 0) * kPeTile + lane];
            b[k] += red[((w * P + k) * 2 + 1) * kPeTile + lane];
        }
    }
}

__device__ __forceinline__ void pe_stats(double s, double q, int m, float eps, float& mean, float& rstd) {
    const double mu = s / (double)m;
    double var = q / (double)m - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

template <int P>
__device__ __forceinline__ void pe_add_sums(const float (&v)[P], double (&s)[P], double (&sq)[P]) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        s[k] += (double)v[k];
        sq[k] += (double)v[k] * (double)v[k];
    }
}

template <int P>
__device__ __forceinline__ void pe_apply(const float (&v)[P], const float (&mu)[P], const float (&rs)[P], const float* scales,
                                         const float* bias, int ch, float* y, size_t at, int PHW, bool wide) {
    float o[P];
#pragma unroll
    for (int k = 0; k < P; ++k) o[k] = scales ? ((v[k] - mu[k]) * rs[k]) * scales[ch] + bias[ch] : v[k];
    pe_store_wide<P>(y, at + (size_t)ch * PHW, wide, o);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// One workgroup per unit (tile blockIdx.x, block row blockIdx.y); wave wid owns the output channels [wid cpw, (wid + 1) cpw).
// CPW > 0: they stay in registers (cpw == CPW). CPW == 0: two sweeps from memory. scales == nullptr: the rearrangement alone,
// bit for bit. Dynamic LDS: red [waves][P][2][64] doubles (none with one wave).
template <int P, int CPW>
__global__ __launch_bounds__(pe_max_waves(P) * 64) void pe_fwd_kernel(const float* x, const float* scales, const float* bias,
                                                                      float* y, float* mean, float* rstd, PeGeom g, int cpw,
                                                                      float eps, int wide) {
    extern __shared__ double pe_smem[];
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the wave's number, in a scalar register
    const int p1 = blockIdx.y;
    const PePos<P> t(blockIdx.x, p1, g);
    const int c_lo = wid * cpw, c_hi = min(g.c, c_lo + cpw);
    constexpr int KEEP = CPW > 0 ? CPW : 1;
    float v[KEEP][P];
    double s[P], sq[P];
#pragma unroll
    for (int k = 0; k < P; ++k) s[k] = sq[k] = 0.0;
    if (t.live) {
        if (CPW > 0) {
#pragma unroll
            for (int j = 0; j < KEEP; ++j) {
                if (c_lo + j < c_hi) {
                    pe_load_x<P>(x, t.src, g, c_lo + j, p1, v[j]);
                    if (scales) pe_add_sums<P>(v[j], s, sq);  // (uniform) the rearrangement alone needs no sums
                }
            }
        } else if (scales) {
#pragma unroll 4
            for (int ch = c_lo; ch < c_hi; ++ch) {
                pe_load_x<P>(x, t.src, g, ch, p1, v[0]);
                pe_add_sums<P>(v[0], s, sq);
            }
        }
    }
    float mu[P], rs[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        mu[k] = 0.f;
        rs[k] = 1.f;
    }
    if (scales) {
        pe_totals<P>(pe_smem, waves, wid, lane, s, sq);
#pragma unroll
        for (int k = 0; k < P; ++k) pe_stats(s[k], sq[k], g.c, eps, mu[k], rs[k]);
        if (wid == 0 && t.live) {
#pragma unroll
            for (int k = 0; k < P; ++k) {
                if (mean) mean[t.oq + k] = mu[k];
                if (rstd) rstd[t.oq + k] = rs[k];
            }
        }
    }
    if (!t.live) return;
    if (CPW > 0) {
#pragma unroll
        for (int j = 0; j < KEEP; ++j)
            if (c_lo + j < c_hi) pe_apply<P>(v[j], mu, rs, scales, bias, c_lo + j, y, t.dst, g.PHW, wide != 0);
    } else {
#pragma unroll 4
        for (int ch = c_lo; ch < c_hi; ++ch) {
            pe_load_x<P>(x, t.src, g, ch, p1, v[0]);
            pe_apply<P>(v[0], mu, rs, scales, bias, ch, y, t.dst, g.PHW, wide != 0);
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// a[0 .. 7] of the 64 lanes -> lane 8 j holds sum over the lanes of a[j], in a[0]. Three halving exchanges over the lane
// bits 5, 4, 3 (the lane keeps the half its bit selects, sends the other half), three full steps over the bits 2, 1, 0.
__device__ __forceinline__ void pe_reduce8(float (&a)[8], int lane) {
#pragma unroll
    for (int step = 0; step < 3; ++step) {
        const int off = 32 >> step, half = 4 >> step;
        const bool hi = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const float keep = hi ? a[i + half] : a[i], send = hi ? a[i] : a[i + half];
            a[i] = keep + __shfl_xor(send, off, 64);
        }
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1) a[0] += __shfl_xor(a[0], off, 64);
}

// The group of (up to) four channels from c0 of one unit: loaded into xv, dv (zeros for a lane past Q and for a channel past
// c_hi: the cross-lane sums need every lane), their terms into the position sums ds, db, their eight per-channel terms
// reduced over the wave and added into acc [2][c] in LDS or into gacc, the workgroup's own row of the partials (both null: no
// parameter gradient asked for).
template <int P>
__device__ __forceinline__ void pe_bwd_group(const float* x, const float* dy, const float* scales, const PePos<P>& t,
                                             const PeGeom& g, int p1, int c0, int c_hi, const float (&mu)[P],
                                             const float (&rs)[P], bool wide, float (&xv)[4][P], float (&dv)[4][P],
                                             double (&ds)[P], double (&db)[P], double* acc, float* gacc, int lane) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = c0 + j < c_hi;  // (uniform in the wave)
#pragma unroll
        for (int k = 0; k < P; ++k) xv[j][k] = dv[j][k] = 0.f;
        if (ok && t.live) {
            pe_load_x<P>(x, t.src, g, c0 + j, p1, xv[j]);
            pe_load_wide<P>(dy, t.dst + (size_t)(c0 + j) * g.PHW, wide, dv[j]);
        }
        const float sc = ok ? scales[c0 + j] : 0.f;
        float fa = 0.f, fb = 0.f;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float xh = (xv[j][k] - mu[k]) * rs[k];
            const float tt = dv[j][k] * sc;
            ds[k] += (double)(tt * xh);
            db[k] += (double)tt;
            fa += dv[j][k] * xh;
            fb += dv[j][k];
        }
        a[j] = fa;
        a[4 + j] = fb;
    }
    if (!acc && !gacc) return;
    pe_reduce8(a, lane);
    if ((lane & 7) == 0) {
        const int j = lane >> 3;  // 0 .. 3: dy * xh of channel c0 + j, 4 .. 7: dy of channel c0 + j - 4
        const int ch = c0 + (j & 3);
        if (ch < c_hi) {
            const int at = (j >> 2) * g.c + ch;
            if (acc) acc[at] += (double)a[0];
            else gacc[at] += a[0];
        }
    }
}

template <int P>
__device__ __forceinline__ void pe_bwd_dx_group(const float (&xv)[4][P], const float (&dv)[4][P], const float* scales,
                                                const PePos<P>& t, const PeGeom& g, int p1, int c0, int c_hi,
                                                const float (&mu)[P], const float (&rs)[P], const float (&ds)[P],
                                                const float (&db)[P], float* dx, bool add) {
    const float cf = (float)g.c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j < c_hi) {
            const float sc = scales[c0 + j];
            float o[P];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float xh = (xv[j][k] - mu[k]) * rs[k];
                const float tt = dv[j][k] * sc;
                o[k] = (tt - (xh * ds[k] + db[k]) / cf) * rs[k];
            }
            pe_store_x<P>(dx, t.src, g, c0 + j, p1, o, add);
        }
    }
}

// A workgroup is persistent over the units blockIdx.x, + gridDim.x, ...; wave wid owns the output channels
// [wid cpw, (wid + 1) cpw). HOLD: cpw == 4, x and dy of a unit stay in registers between the sums and the data gradient;
// else they are read again. scales == nullptr: the rearrangement's backward, dx (+)= dy moved back.
// Dynamic LDS: red [waves][P][2][64] doubles (none with one wave), then with acc_lds acc [2][c] doubles. partial:
// [gridDim.x][2][c] or null. Without acc_lds the workgroup accumulates in its row of partial itself: a slot has one lane for
// writer and reader over all units.
template <int P, bool HOLD>
__global__ __launch_bounds__(kPeBwdWaves * 64) void pe_bwd_kernel(const float* x, const float* scales, const float* mean,
                                                                  const float* rstd, const float* dy, float* dx,
                                                                  float* partial, PeGeom g, int cpw, int units,
                                                                  int overwrite, int wide, int acc_lds) {
    extern __shared__ double pe_smem[];
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = g.c, c_lo = wid * cpw, c_hi = min(c, c_lo + cpw);
    double* red = pe_smem;
    double* acc = partial && acc_lds ? pe_smem + (waves > 1 ? waves * P * 2 * kPeTile : 0) : nullptr;
    float* gacc = partial && !acc_lds ? partial + (size_t)blockIdx.x * 2 * c : nullptr;
    if (partial) {
        for (int i = threadIdx.x; i < 2 * c; i += blockDim.x) {
            if (acc) acc[i] = 0.0;
            else gacc[i] = 0.f;
        }
        __syncthreads();
    }
    for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int p1 = unit % P;
        const PePos<P> t(unit / P, p1, g);
        if (!scales) {  // the rearrangement: every element of dx has one source in dy
            if (t.live)
                for (int ch = c_lo; ch < c_hi; ++ch) {
                    float d[P];
                    pe_load_wide<P>(dy, t.dst + (size_t)ch * g.PHW, wide != 0, d);
                    pe_store_x<P>(dx, t.src, g, ch, p1, d, !overwrite);
                }
            continue;
        }
        float mu[P], rs[P];
        double ds[P], db[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            mu[k] = t.live ? mean[t.oq + k] : 0.f;
            rs[k] = t.live ? rstd[t.oq + k] : 0.f;
            ds[k] = db[k] = 0.0;
        }
        float xv[4][P], dv[4][P];
        if (HOLD) pe_bwd_group<P>(x, dy, scales, t, g, p1, c_lo, c_hi, mu, rs, wide != 0, xv, dv, ds, db, acc, gacc, lane);
        else
            for (int c0 = c_lo; c0 < c_hi; c0 += 4)
                pe_bwd_group<P>(x, dy, scales, t, g, p1, c0, c_hi, mu, rs, wide != 0, xv, dv, ds, db, acc, gacc, lane);
        if (!dx) continue;  // (uniform) nothing below but the data gradient
        pe_totals<P>(red, waves, wid, lane, ds, db);
        float dsf[P], dbf[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            dsf[k] = (float)ds[k];
            dbf[k] = (float)db[k];
        }
        if (t.live) {
            if (HOLD) pe_bwd_dx_group<P>(xv, dv, scales, t, g, p1, c_lo, c_hi, mu, rs, dsf, dbf, dx, !overwrite);
            else
                for (int c0 = c_lo; c0 < c_hi; c0 += 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < c_hi) {
                            pe_load_x<P>(x, t.src, g, c0 + j, p1, xv[j]);
                            pe_load_wide<P>(dy, t.dst + (size_t)(c0 + j) * g.PHW, wide != 0, dv[j]);
                        }
                    pe_bwd_dx_group<P>(xv, dv, scales, t, g, p1, c0, c_hi, mu, rs, dsf, dbf, dx, !overwrite);
                }
        }
        if (waves > 1) __syncthreads();  // the next unit rewrites red
    }
    if (!acc) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * c; i += blockDim.x) partial[(size_t)blockIdx.x * 2 * c + i] = (float)acc[i];
}

// dscales[ch] += sum_g partial[g][0][ch], db likewise: workgroups in ascending order in double, the start value one float32
// addition
__global__ void pe_finalize_kernel(const float* partial, int groups, int c, float* dscales, float* dbias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * c) return;
    float* out = i < c ? dscales : dbias;
    if (!out) return;
    double a = 0.0;
#pragma unroll 8  // eight workgroups' loads in flight; the additions keep their order
    for (int gi = 0; gi < groups; ++gi) a += (double)partial[(size_t)gi * 2 * c + i];
    const int ch = i < c ? i : i - c;
    out[ch] = out[ch] + (float)a;
}

// 0: refused (an extent below 1, a block other than 2 or 4, c_in no multiple of block^2, an unknown order, 2^31 elements or more)
static int pe_geom(int n, int c_in, int h, int w, int block, int order, PeGeom* g) {
    if (n < 1 || c_in < 1 || h < 1 || w < 1 || (block != 2 && block != 4) || c_in % (block * block)) return 0;
    if (order != BCNN_HIP_PATCH_EXPAND_BLOCKS && order != BCNN_HIP_PATCH_EXPAND_CHANNELS) return 0;
    if ((long long)n * c_in * h * w >= (1LL << 31)) return 0;
    g->Q = (long long)n * h * w;
    g->c = c_in / (block * block);
    g->W = w;
    g->HW = h * w;
    g->PW = block * w;
    g->PHW = block * block * h * w;
    g->cs = order == BCNN_HIP_PATCH_EXPAND_BLOCKS ? 1 : block * block;
    g->bs = order == BCNN_HIP_PATCH_EXPAND_BLOCKS ? g->c : 1;
    return 1;
}

static int pe_geom_or_say(const char* who, int n, int c_in, int h, int w, int block, int order, PeGeom* g) {
    if (pe_geom(n, c_in, h, w, block, order, g)) return 1;
    fprintf(stderr, "[bcnn_hip] %s: refused, nothing done: an extent below 1, a block other than 2 or 4, channels that are no "
                    "multiple of block^2, an unknown order or a tensor of 2^31 elements or more (%d x %d x %d x %d, block %d, "
                    "order %d)\n", who, n, c_in, h, w, block, order);
    return 0;
}

static bool pe_aligned(const void* p, int block) { return (reinterpret_cast<uintptr_t>(p) & (size_t)(4 * block - 1)) == 0; }

static const char* const kPeFwdTag[4] = {"patch_expand_fwd:column", "patch_expand_fwd:split", "patch_expand_fwd:stream",
                                         "patch_expand_fwd:copy"};
static const char* const kPeBwdTag[4] = {"patch_expand_bwd:column", "patch_expand_bwd:split", "patch_expand_bwd:stream",
                                         "patch_expand_bwd:copy"};

template <int P>
static void pe_forward(const bcnn_hip_patch_expand_fwd_args* a, const PeGeom& g) {
    const int c = g.c, path = pe_path(c, P);
    const int cpw = path == 2 ? ceil_div(c, pe_max_waves(P)) : pe_cpw(c, P);
    const int waves = ceil_div(c, cpw);
    const dim3 grid((unsigned)ceil_div(g.Q, kPeTile), P);
    const size_t lds = waves > 1 ? (size_t)waves * P * 2 * kPeTile * sizeof(double) : 0;
    const int wide = pe_aligned(a->y, P);
    const float e = a->eps > 0.f ? a->eps : 1e-5f;
    trace_kernel(kPeFwdTag[a->scales ? path : 3]);
#define PE_FWD(CPW) \
    pe_fwd_kernel<P, CPW><<<grid, waves * 64, lds, current_stream()>>>(a->x, a->scales, a->b, a->y, a->mean, a->rstd, g, cpw, e, wide)
    if (path == 2) PE_FWD(0);
    else if (cpw == 2) PE_FWD(2);
    else if (cpw == 4) PE_FWD(4);
    else if (cpw == 8) PE_FWD(8);
    else if (cpw == 16) PE_FWD(16);
    else PE_FWD(32);
#undef PE_FWD
    KERNEL_CHECK();
}

template <int P>
static void pe_backward(const bcnn_hip_patch_expand_bwd_args* a, const PeGeom& g, bool params) {
    const int c = g.c, path = pe_path(c, P);
    const bool hold = a->scales && c <= kPeBwdCpw * kPeBwdWaves;
    const int cpw = hold ? kPeBwdCpw : ceil_div(c, kPeBwdWaves);
    const int waves = ceil_div(c, cpw);
    const int units = ceil_div(g.Q, kPeTile) * P;
    const int groups = std::min(units, kPeMaxGroups);  // a function of the shape alone
    float* partial = params ? scratch(SCRATCH_REDUCE, (size_t)groups * 2 * c) : nullptr;
    const int acc_lds = c <= kPeAccLdsMaxC;
    const size_t lds = ((waves > 1 ? (size_t)waves * P * 2 * kPeTile : 0) + (params && acc_lds ? (size_t)2 * c : 0)) * sizeof(double);
    const int wide = pe_aligned(a->dy, P);
    trace_kernel(kPeBwdTag[a->scales ? path : 3]);
#define PE_BWD(HOLD)                                                                                                         \
    pe_bwd_kernel<P, HOLD><<<groups, waves * 64, lds, current_stream()>>>(a->x, a->scales, a->mean, a->rstd, a->dy, a->dx, partial, \
                                                                          g, cpw, units, a->overwrite, wide, acc_lds)
    if (hold) PE_BWD(true);
    else PE_BWD(false);
#undef PE_BWD
    KERNEL_CHECK();
    if (params) {
        trace_kernel("patch_expand_finalize");
        pe_finalize_kernel<<<ceil_div(2 * c, 256), 256, 0, current_stream()>>>(partial, groups, c, a->dscales, a->db);
        KERNEL_CHECK();
    }
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_patch_expand_path(int n, int c_in, int h, int w, int block) {
    PeGeom g;
    return pe_geom(n, c_in, h, w, block, BCNN_HIP_PATCH_EXPAND_BLOCKS, &g) ? pe_path(g.c, block) : -1;
}

void bcnn_hip_patch_expand_forward(const bcnn_hip_patch_expand_fwd_args* a) {
    PeGeom g;
    if (!pe_geom_or_say("bcnn_hip_patch_expand_forward", a->n, a->c_in, a->h, a->w, a->block, a->order, &g)) return;
    if (a->block == 2) pe_forward<2>(a, g);
    else pe_forward<4>(a, g);
}

void bcnn_hip_patch_expand_backward(const bcnn_hip_patch_expand_bwd_args* a) {
    PeGeom g;
    if (!pe_geom_or_say("bcnn_hip_patch_expand_backward", a->n, a->c_in, a->h, a->w, a->block, a->order, &g)) return;
    const bool params = a->scales && (a->dscales || a->db);
    if (!a->dx && !params) return;
    if (a->block == 2) pe_backward<2>(a, g, params);
    else pe_backward<4>(a, g, params);
}

}  // extern "C"
