// patch_merge.hip -- the patch-merging node (Swin's stage transition, YOLOv5's Focus): the 2x2 neighbours of src [N,C,H,W]
// move to the channels, dst [N,4C,H/2,W/2], output channel k C + c with k = 2 dx + dy takes src[n, c, 2 oy + dy, 2 ox + dx];
// with a norm every output position is then normalised over its M = 4C values and mapped through scales[M], b[M]. One
// launch does both: the rearranged tensor never exists in memory un-normalised. No reference counterpart.
//   forward : s = sum v, q = sum v^2 over the position's M values, added in DOUBLE (the kernel is bound by memory and the
//             double adds ride along); mean = s / M, var = max(q / M - mean^2, 0), rstd = (float)(1 / sqrt(var + eps));
//             y = ((v - mean) * rstd) * scales[m] + b[m], one float32 rounding per operation (-ffp-contract=off).
//   backward: xh = (v - mean) * rstd, t = dy * scales[m]; per position ds = sum_m t * xh, db = sum_m t (float32 terms, added
//             in double, rounded once); dv = (t - (xh * ds + db) / M) * rstd goes back to where v came from; per channel
//             dscales[m] += sum_q dy * xh, db[m] += sum_q dy.
// ADDRESSING. Lanes run along the flattened output positions q = n OH OW + oy OW + ox of all images; a tile is 64 of them,
// one per lane. For a source channel c the lane needs the pair (2 ox, 2 ox + 1) of the rows 2 oy and 2 oy + 1: two 8-byte
// loads (W is even, so a pair is 8-byte aligned whenever the base is; a base that is not takes four 4-byte loads and gives
// the same bits). Across a wave that is two contiguous 512-byte runs where the 64 positions lie in one output row; where they
// cross a row or an image only the per-lane offset differs. The four values go to the planes c, C + c, 2C + c, 3C + c of dst,
// 256 contiguous bytes per plane and wave. No gathers, no LDS for data.
// WIDTH. M is 384 .. 2048 in the nets this serves, far past what one lane holds. A workgroup owns a tile and SPLITS THE
// SOURCE CHANNELS ACROSS ITS WAVES: wave w takes the channels [w cpw, (w + 1) cpw) and keeps their 4 cpw values per lane in
// registers (cpw is 2, 4, 8 or 16, the smallest that needs no more than 16 waves), so the tile is read once and lives in
// the register file of the workgroup, 64 positions x 1024 floats at most. The waves' per-lane sums meet in LDS (16 KB) and
// every thread adds them for its own lane in ascending wave order. Three paths, from C alone (bcnn_hip_patch_merge_path):
//   column (C <= 8)  : one wave per tile, the lane holds all 4C values; no LDS, no barrier.
//   split  (C <= 256): the above.
//   stream (larger C): 16 waves, each sweeps its channels twice (statistics, then apply; the second read comes from L2).
// The backward follows the same split. It holds v and dy of a tile in registers only with two channels per wave (C <= 32):
// four and eight channels per wave spill under the 128 registers of a 1024-thread workgroup (8 and 90 registers), so
// beyond 32 channels the data gradient re-reads what the sums just read (from L2).
// PER-CHANNEL GRADIENTS IN ONE PASS. The terms dy * xh and dy of a source channel are eight values per lane (4 planes x 2
// sums) that must be added over the 64 lanes. pm_reduce8 does it in 10 cross-lane steps: three halving exchanges (a lane
// keeps half of its values and receives the partner's other half), then three full steps on the one value left; lane 8 j
// ends with the total of value j. Those eight lanes add it into the workgroup's [2][M] accumulators in LDS (double; a
// channel has one owner wave, so no two lanes share a slot). A workgroup is persistent over the tiles g, g + G, ... and writes
// its accumulators once, as one partial row; pm_finalize_kernel adds the rows in ascending order in double. Whatever M
// is, x and dy are read once for the parameter gradients. No atomics; every order follows from the shape alone.
#include <algorithm>

#include "common.h"
#include "../../include/bcnn_hip.h"

namespace bcnn_hip {

constexpr int kPmTile = 64;         // output positions of a tile: one per lane of a wave
constexpr int kPmMaxWaves = 16;     // waves of a workgroup, at most
constexpr int kPmColumnMaxC = 8;    // one wave holds the whole column: 32 values per lane
constexpr int kPmSplitMaxC = 256;   // 16 waves x 16 channels x 4 values: 64 data registers per lane under the 128 of a
                                    // 1024-thread workgroup
constexpr int kPmHoldMaxCBwd = 32;  // the backward holds v and dy: 2 channels per wave, 16 waves
constexpr int kPmAccLdsMaxM = 2048; // 4C up to which the per-channel accumulators [2][4C] are doubles in LDS (32 KB)
constexpr int kPmMaxGroups = 512;   // persistent workgroups of a backward launch, at most

static int pm_path(int c) { return c <= kPmColumnMaxC ? 0 : (c <= kPmSplitMaxC ? 1 : 2); }

// channels per wave of the register-holding kernels: the whole column, or the smallest of 2, 4, 8, 16 within 16 waves
static int pm_cpw(int c) {
    if (c <= kPmColumnMaxC) return kPmColumnMaxC;
    for (int cpw = 2; cpw < 16; cpw *= 2)
        if (ceil_div(c, cpw) <= kPmMaxWaves) return cpw;
    return 16;
}

struct PmGeom {
    long long P;   // output positions of all images
    int C, W;      // source channels, source row length
    int OW, OHW;   // output row length, output positions of an image
    int HW;        // source plane
};

// this lane's output position of a tile: where channel 0 of its 2x2 block starts in src and where plane 0 of it is in dst
struct PmPos {
    long long q;
    bool live;
    size_t src, dst;
    __device__ PmPos(long long tile, const PmGeom& g) {
        q = tile * kPmTile + (threadIdx.x & 63);
        live = q < g.P;
        const long long n = live ? q / g.OHW : 0;
        const int p = live ? (int)(q - n * g.OHW) : 0;
        const int oy = p / g.OW, ox = p - oy * g.OW;
        src = (size_t)n * g.C * g.HW + (size_t)(2 * oy) * g.W + (size_t)(2 * ox);
        dst = (size_t)n * 4 * g.C * g.OHW + (size_t)p;
    }
};

// the 2x2 block at `at`: v[k], k = 2 dx + dy
__device__ __forceinline__ void pm_load(const float* x, size_t at, int W, bool pair, float (&v)[4]) {
    if (pair) {
        const float2 r0 = *reinterpret_cast<const float2*>(x + at), r1 = *reinterpret_cast<const float2*>(x + at + W);
        v[0] = r0.x; v[1] = r1.x; v[2] = r0.y; v[3] = r1.y;
    } else {
        v[0] = x[at]; v[1] = x[at + W]; v[2] = x[at + 1]; v[3] = x[at + W + 1];
    }
}

__device__ __forceinline__ void pm_store(float* x, size_t at, int W, bool pair, const float (&v)[4], bool add) {
    float o[4] = {v[0], v[1], v[2], v[3]};
    if (add) {
        float a[4];
        pm_load(x, at, W, pair, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = a[k] + v[k];
    }
    if (pair) {
        *reinterpret_cast<float2*>(x + at) = make_float2(o[0], o[2]);
        *reinterpret_cast<float2*>(x + at + W) = make_float2(o[1], o[3]);
    } else {
        x[at] = o[0]; x[at + W] = o[1]; x[at + 1] = o[2]; x[at + W + 1] = o[3];
    }
}

// this lane's totals of the waves' per-lane sums, waves in ascending order; red is [waves][2][64] doubles. One wave: no LDS
__device__ __forceinline__ void pm_totals(double* red, int waves, int wid, int lane, double& a, double& b) {
    if (waves == 1) return;
    red[(wid * 2 + 0) * kPmTile + lane] = a;
    red[(wid * 2 + 1) * kPmTile + lane] = b;
    __syncthreads();
    a = 0.0;
    b = 0.0;
    for (int w = 0; w < waves; ++w) {
        a += red[(w * 2 + 0) * kPmTile + lane];
        b += red[(w * 2 + 1) * kPmTile + lane];
    }
}

__device__ __forceinline__ void pm_stats(double s, double q, int M, float eps, float& mean, float& rstd) {
    const double mu = s / (double)M;
    double var = q / (double)M - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// One workgroup per tile; wave wid owns the source channels [wid cpw, (wid + 1) cpw). CPW > 0: they stay in registers
// (cpw == CPW). CPW == 0: two sweeps from memory. scales == nullptr: the rearrangement alone, bit for bit.
// Dynamic LDS: red [waves][2][64] doubles (none with one wave).
template <int CPW>
__global__ __launch_bounds__(kPmMaxWaves * 64) void pm_fwd_kernel(const float* x, const float* scales, const float* bias,
                                                                  float* y, float* mean, float* rstd, PmGeom g, int cpw,
                                                                  float eps, int pair) {
    extern __shared__ double pm_smem[];
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the wave's number, in a scalar register
    const PmPos t(blockIdx.x, g);
    const int C = g.C, c_lo = wid * cpw, c_hi = min(C, c_lo + cpw);
    constexpr int KEEP = CPW > 0 ? CPW : 1;
    float v[KEEP][4];
    double s = 0.0, sq = 0.0;
    if (t.live) {
        if (CPW > 0) {
#pragma unroll
            for (int j = 0; j < KEEP; ++j) {
                if (c_lo + j < c_hi) {
                    pm_load(x, t.src + (size_t)(c_lo + j) * g.HW, g.W, pair != 0, v[j]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        s += (double)v[j][k];
                        sq += (double)v[j][k] * (double)v[j][k];
                    }
                }
            }
        } else if (scales) {
#pragma unroll 4
            for (int c = c_lo; c < c_hi; ++c) {
                pm_load(x, t.src + (size_t)c * g.HW, g.W, pair != 0, v[0]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s += (double)v[0][k];
                    sq += (double)v[0][k] * (double)v[0][k];
                }
            }
        }
    }
    float mu = 0.f, rs = 1.f;
    if (scales) {
        pm_totals(pm_smem, waves, wid, lane, s, sq);
        pm_stats(s, sq, 4 * C, eps, mu, rs);
        if (wid == 0 && t.live) {
            if (mean) mean[t.q] = mu;
            if (rstd) rstd[t.q] = rs;
        }
    }
    if (!t.live) return;
    if (CPW > 0) {
#pragma unroll
        for (int j = 0; j < KEEP; ++j) {
            if (c_lo + j < c_hi) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = k * C + c_lo + j;
                    y[t.dst + (size_t)m * g.OHW] = scales ? ((v[j][k] - mu) * rs) * scales[m] + bias[m] : v[j][k];
                }
            }
        }
    } else {
#pragma unroll 4
        for (int c = c_lo; c < c_hi; ++c) {
            pm_load(x, t.src + (size_t)c * g.HW, g.W, pair != 0, v[0]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = k * C + c;
                y[t.dst + (size_t)m * g.OHW] = scales ? ((v[0][k] - mu) * rs) * scales[m] + bias[m] : v[0][k];
            }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// a[0 .. 7] of the 64 lanes -> lane 8 j holds sum over the lanes of a[j], in a[0]. Three halving exchanges over the lane
// bits 5, 4, 3 (the lane keeps the half its bit selects, sends the other half), three full steps over the bits 2, 1, 0.
__device__ __forceinline__ void pm_reduce8(float (&a)[8], int lane) {
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

// One source channel of one position: its terms into the position sums, its eight per-channel terms reduced over the wave
// and added into acc [2][M] in LDS, or into gacc, the workgroup's own row of the partials (both null: no parameter
// gradient asked for).
__device__ __forceinline__ void pm_bwd_terms(const float (&xv)[4], const float (&dv)[4], const float* scales, int c, int C,
                                             float mu, float rs, double& ds, double& db, double* acc, float* gacc,
                                             int lane) {
    float a[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xh = (xv[k] - mu) * rs;
        const float tt = dv[k] * scales[k * C + c];
        ds += (double)(tt * xh);
        db += (double)tt;
        a[k] = dv[k] * xh;
        a[4 + k] = dv[k];
    }
    if (!acc && !gacc) return;
    pm_reduce8(a, lane);
    if ((lane & 7) == 0) {
        const int j = lane >> 3;  // 0 .. 3: dy * xh of plane j, 4 .. 7: dy of plane j - 4
        const int at = (j >> 2) * 4 * C + (j & 3) * C + c;
        if (acc) acc[at] += (double)a[0];
        else gacc[at] += a[0];
    }
}

__device__ __forceinline__ void pm_bwd_dx(const float (&xv)[4], const float (&dv)[4], const float* scales, int c, int C,
                                          float mu, float rs, float ds, float db, float* dx, size_t at, int W, bool pair,
                                          bool add) {
    const float mf = (float)(4 * C);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xh = (xv[k] - mu) * rs;
        const float tt = dv[k] * scales[k * C + c];
        o[k] = (tt - (xh * ds + db) / mf) * rs;
    }
    pm_store(dx, at, W, pair, o, add);
}

__device__ __forceinline__ void pm_load_dy(const float* dy, size_t dst, int c, int C, int OHW, float (&d)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = dy[dst + (size_t)(k * C + c) * OHW];
}

// A workgroup is persistent over the tiles blockIdx.x, + gridDim.x, ...; wave wid owns the source channels
// [wid cpw, (wid + 1) cpw). CPW > 0: v and dy of a tile stay in registers between the sums and the data gradient;
// CPW == 0: they are read again. scales == nullptr: the rearrangement's backward, dx (+)= dy moved back.
// Dynamic LDS: red [waves][2][64] doubles, then with acc_lds acc [2][4C] doubles. partial: [gridDim.x][2][4C] or null. Without
// acc_lds (4C past what 64 KB hold) the workgroup accumulates in its row of partial itself: a slot has one lane for
// writer and reader over all tiles.
template <int CPW>
__global__ __launch_bounds__(kPmMaxWaves * 64) void pm_bwd_kernel(const float* x, const float* scales, const float* mean,
                                                                  const float* rstd, const float* dy, float* dx,
                                                                  float* partial, PmGeom g, int cpw, int tiles, int overwrite,
                                                                  int pair, int acc_lds) {
    extern __shared__ double pm_smem[];
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = g.C, M = 4 * C, c_lo = wid * cpw, c_hi = min(C, c_lo + cpw);
    double* red = pm_smem;
    double* acc = partial && acc_lds ? pm_smem + (waves > 1 ? waves * 2 * kPmTile : 0) : nullptr;
    float* gacc = partial && !acc_lds ? partial + (size_t)blockIdx.x * 2 * M : nullptr;
    if (partial) {
        for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) {
            if (acc) acc[i] = 0.0;
            else gacc[i] = 0.f;
        }
        __syncthreads();
    }
    constexpr int KEEP = CPW > 0 ? CPW : 1;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const PmPos t(tile, g);
        if (!scales) {  // the rearrangement: every element of dx has one source in dy
            if (t.live)
                for (int c = c_lo; c < c_hi; ++c) {
                    float d[4];
                    pm_load_dy(dy, t.dst, c, C, g.OHW, d);
                    pm_store(dx, t.src + (size_t)c * g.HW, g.W, pair != 0, d, !overwrite);
                }
            continue;
        }
        // a lane past P runs along with zeros: the cross-lane sums need every lane
        const float mu = t.live ? mean[t.q] : 0.f, rs = t.live ? rstd[t.q] : 0.f;
        float xv[KEEP][4], dv[KEEP][4];
        double ds = 0.0, db = 0.0;
        if (CPW > 0) {
#pragma unroll
            for (int j = 0; j < KEEP; ++j) {
                if (c_lo + j < c_hi) {  // (uniform in the wave)
#pragma unroll
                    for (int k = 0; k < 4; ++k) xv[j][k] = dv[j][k] = 0.f;
                    if (t.live) {
                        pm_load(x, t.src + (size_t)(c_lo + j) * g.HW, g.W, pair != 0, xv[j]);
                        pm_load_dy(dy, t.dst, c_lo + j, C, g.OHW, dv[j]);
                    }
                    pm_bwd_terms(xv[j], dv[j], scales, c_lo + j, C, mu, rs, ds, db, acc, gacc, lane);
                }
            }
        } else {
            for (int c = c_lo; c < c_hi; ++c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[0][k] = dv[0][k] = 0.f;
                if (t.live) {
                    pm_load(x, t.src + (size_t)c * g.HW, g.W, pair != 0, xv[0]);
                    pm_load_dy(dy, t.dst, c, C, g.OHW, dv[0]);
                }
                pm_bwd_terms(xv[0], dv[0], scales, c, C, mu, rs, ds, db, acc, gacc, lane);
            }
        }
        if (!dx) continue;  // (uniform) nothing below but the data gradient
        pm_totals(red, waves, wid, lane, ds, db);
        const float dsf = (float)ds, dbf = (float)db;
        if (t.live) {
            if (CPW > 0) {
#pragma unroll
                for (int j = 0; j < KEEP; ++j)
                    if (c_lo + j < c_hi)
                        pm_bwd_dx(xv[j], dv[j], scales, c_lo + j, C, mu, rs, dsf, dbf, dx, t.src + (size_t)(c_lo + j) * g.HW,
                                  g.W, pair != 0, !overwrite);
            } else {
                for (int c = c_lo; c < c_hi; ++c) {
                    pm_load(x, t.src + (size_t)c * g.HW, g.W, pair != 0, xv[0]);
                    pm_load_dy(dy, t.dst, c, C, g.OHW, dv[0]);
                    pm_bwd_dx(xv[0], dv[0], scales, c, C, mu, rs, dsf, dbf, dx, t.src + (size_t)c * g.HW, g.W, pair != 0,
                              !overwrite);
                }
            }
        }
        if (waves > 1) __syncthreads();  // the next tile rewrites red
    }
    if (!acc) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) partial[(size_t)blockIdx.x * 2 * M + i] = (float)acc[i];
}

// dscales[m] += sum_g partial[g][0][m], db likewise: workgroups in ascending order in double, the start value one float32
// addition (accumulate_kernel of activation.hip, for two rows at once)
__global__ void pm_finalize_kernel(const float* partial, int groups, int M, float* dscales, float* dbias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * M) return;
    float* out = i < M ? dscales : dbias;
    if (!out) return;
    double a = 0.0;
#pragma unroll 8  // eight workgroups' loads in flight; the additions keep their order
    for (int gi = 0; gi < groups; ++gi) a += (double)partial[(size_t)gi * 2 * M + i];
    const int m = i < M ? i : i - M;
    out[m] = out[m] + (float)a;
}

// 0: refused (an extent below 1, an odd h or w, 2^31 elements or more)
static int pm_geom(int n, int c, int h, int w, PmGeom* g) {
    if (n < 1 || c < 1 || h < 1 || w < 1 || (h & 1) || (w & 1)) return 0;
    if ((long long)n * c * h * w >= 0x7fffffffLL) return 0;
    g->P = (long long)n * (h / 2) * (w / 2);
    g->C = c;
    g->W = w;
    g->OW = w / 2;
    g->OHW = (h / 2) * (w / 2);
    g->HW = h * w;
    return 1;
}

static void pm_geom_or_exit(const char* who, int n, int c, int h, int w, PmGeom* g) {
    if (pm_geom(n, c, h, w, g)) return;
    fprintf(stderr, "[bcnn_hip] %s: an extent below 1, an odd height or width, or a tensor of 2^31 elements or more "
                    "(%d x %d x %d x %d)\n", who, n, c, h, w);
    exit(1);
}

static bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

static const char* const kPmFwdTag[4] = {"patch_merge_fwd:column", "patch_merge_fwd:split", "patch_merge_fwd:stream",
                                         "patch_merge_fwd:copy"};
static const char* const kPmBwdTag[4] = {"patch_merge_bwd:column", "patch_merge_bwd:split", "patch_merge_bwd:stream",
                                         "patch_merge_bwd:copy"};

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_patch_merge_path(int n, int c, int h, int w) {
    PmGeom g;
    return pm_geom(n, c, h, w, &g) ? pm_path(c) : -1;
}

void bcnn_hip_patch_merge_forward(const float* x, const float* scales, const float* b, float* y, float* mean, float* rstd,
                                  int n, int c, int h, int w, float eps) {
    PmGeom g;
    pm_geom_or_exit("bcnn_hip_patch_merge_forward", n, c, h, w, &g);
    const int path = pm_path(c);
    const int cpw = path == 2 ? ceil_div(c, kPmMaxWaves) : pm_cpw(c);
    const int waves = ceil_div(c, cpw);
    const unsigned tiles = (unsigned)ceil_div(g.P, kPmTile);
    const size_t lds = waves > 1 ? (size_t)waves * 2 * kPmTile * sizeof(double) : 0;
    const int pair = al8(x);
    const float e = eps > 0.f ? eps : 1e-5f;
    trace_kernel(kPmFwdTag[scales ? path : 3]);
#define PM_FWD(CPW) pm_fwd_kernel<CPW><<<tiles, waves * 64, lds, current_stream()>>>(x, scales, b, y, mean, rstd, g, cpw, e, pair)
    if (path == 2) PM_FWD(0);
    else if (cpw == 2) PM_FWD(2);
    else if (cpw == 4) PM_FWD(4);
    else if (cpw == 8) PM_FWD(8);
    else PM_FWD(16);
#undef PM_FWD
    KERNEL_CHECK();
}

void bcnn_hip_patch_merge_backward(const float* x, const float* scales, const float* mean, const float* rstd, const float* dy,
                                   float* dx, float* dscales, float* db, int n, int c, int h, int w, int overwrite_dx) {
    PmGeom g;
    pm_geom_or_exit("bcnn_hip_patch_merge_backward", n, c, h, w, &g);
    const bool params = scales && (dscales || db);
    if (!dx && !params) return;
    const int path = pm_path(c), M = 4 * c;
    const bool hold = scales && c <= kPmHoldMaxCBwd;
    const int cpw = hold ? 2 : ceil_div(c, kPmMaxWaves);
    const int waves = ceil_div(c, cpw);
    const int tiles = ceil_div(g.P, kPmTile);
    const int groups = std::min(tiles, kPmMaxGroups);  // a function of the shape alone
    float* partial = params ? scratch(SCRATCH_REDUCE, (size_t)groups * 2 * M) : nullptr;
    const int acc_lds = M <= kPmAccLdsMaxM;
    const size_t lds = ((waves > 1 ? (size_t)waves * 2 * kPmTile : 0) + (params && acc_lds ? (size_t)2 * M : 0)) * sizeof(double);
    const int pair = dx ? al8(x) && al8(dx) : al8(x);
    trace_kernel(kPmBwdTag[scales ? path : 3]);
#define PM_BWD(CPW) \
    pm_bwd_kernel<CPW><<<groups, waves * 64, lds, current_stream()>>>(x, scales, mean, rstd, dy, dx, partial, g, cpw, tiles, overwrite_dx, pair, acc_lds)
    if (hold) PM_BWD(2);
    else PM_BWD(0);
#undef PM_BWD
    KERNEL_CHECK();
    if (params) {
        trace_kernel("patch_merge_finalize");
        pm_finalize_kernel<<<ceil_div(2 * M, 256), 256, 0, current_stream()>>>(partial, groups, M, dscales, db);
        KERNEL_CHECK();
    }
}

}  // extern "C"
