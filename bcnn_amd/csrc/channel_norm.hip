// channel_norm.hip -- the channel-norm node: every POSITION (n, p) of an NCHW tensor is normalised over its C channels
// (torch's LayerNorm(C) on tokens, LayerNorm2d). No reference counterpart. group_norm.hip's rows are contiguous runs; here the
// row of a position is a column of C floats HW apart, and the per-channel parameter gradients run along the contiguous axis.
//   forward : mean = sum_c x / C, var = max(sum_c x^2 / C - mean^2, 0), rstd = (float)(1 / sqrt(var + eps)), both finished in
//             double; y = ((x - mean) * rstd) * scales[c] + b[c], one float32 rounding per operation (-ffp-contract=off).
//   backward: from mean and rstd. xh = (x - mean) * rstd, t = dy * scales[c]; per position ds = sum_c t * xh, db = sum_c t,
//             dxv = (t - (xh * ds + db) / C) * rstd, dx = dxv or dx + dxv; per channel dscales[c] += sum_{n,p} dy * xh,
//             db[c] += sum_{n,p} dy.
// The positions of all images are flattened, q = n * HW + p in [0, P), P = N * HW, and LANES RUN ALONG q: a wave reads 64
// consecutive floats of a channel plane (or of two images' planes where a tile straddles them), so waves stay full at 7x7 and
// 14x14 maps; the channel loop strides by HW. A tile is 64 positions. Three paths, from C alone (bcnn_hip_channel_norm_path):
//   column   (C <= 16 forward, 8 backward): one lane owns a position and keeps its channel column (backward: x and dy) in
//            registers. No LDS.
//   resident (forward only, C <= 238): a workgroup of 8 waves owns a tile and keeps x of it in LDS; the waves split the
//            channels, their per-lane partial sums meet in LDS and are added in ascending wave order in double.
//            16-byte loads and stores where HW % 4 == 0 and the bases are aligned: the route changes who moves an element, never
//            who adds it, so the bits are those of the 4-byte route.
//   stream   (larger C): 16 waves per tile (8 in the backward), two sweeps over the tile's channels from memory (statistics, then apply; the
//            second is expected from cache).
// Backward, per-channel sums: a workgroup is persistent over the tiles g, g + G, ... (G from the shape alone); every lane adds
// its own column of per-channel terms over those tiles in REGISTERS (a wave owns its channel subset, so an accumulator is
// indexed at compile time); once per workgroup a butterfly adds the 64 lanes and the workgroup writes its [2][C] partials; a
// finalize kernel adds the workgroups in ascending order in double. No atomics, every order follows from the shape alone.
#include <algorithm>

#include "common.h"
#include "../../include/bcnn_hip.h"

namespace bcnn_hip {

constexpr int kCnTile = 64;            // positions of a tile: one per lane of a wave
// up to here a lane keeps the whole column in registers. Set where the measured times cross: past 16
// channels the resident forward is faster, past 8 the stream backward is, or is on a par, at every extent timed
constexpr int kCnColumnMaxC = 16;      // forward
constexpr int kCnColumnMaxCBwd = 8;    // backward
constexpr int kCnResWaves = 8;         // waves of a resident workgroup
constexpr int kCnStreamWaves = 16;     // waves of a stream workgroup, forward
constexpr int kCnStreamWavesBwd = 8;   // backward: half the waves, twice the registers for the per-channel sums of each
constexpr int kCnLdsFloats = 16384;    // 64 KB of LDS
// LDS ahead of the tile: the waves' partial sums [waves][2][64], then mean and rstd of the 64 positions
constexpr int kCnFwdHead = kCnResWaves * 2 * kCnTile + 2 * kCnTile;
constexpr int kCnResMaxCFwd = (kCnLdsFloats - kCnFwdHead) / kCnTile;  // 238
constexpr int kCnMaxGroups = 512;      // persistent workgroups of a backward launch, at most
constexpr int kCnStreamRegC = 32;      // channels of a stream wave whose sums stay in registers in one pass over the tiles

static int cn_path(int c, int backward) {
    if (c <= (backward ? kCnColumnMaxCBwd : kCnColumnMaxC)) return 0;
    if (!backward && c <= kCnResMaxCFwd) return 1;  // (a resident backward was built and was slower than stream at every C)
    return 2;
}

__device__ __forceinline__ void cn_finalize(double s, double q, int C, float eps, float& mean, float& rstd) {
    const double mu = s / (double)C;
    double var = q / (double)C - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ float cn_y(float x, float mu, float rs, float g, float b) {
    const float xh = (x - mu) * rs;
    return xh * g + b;
}

__device__ __forceinline__ float cn_dxv(float x, float d, float g, float mu, float rs, float ds, float db, float cf) {
    const float xh = (x - mu) * rs;
    const float t = d * g;
    return (t - (xh * ds + db) / cf) * rs;
}

// offset of channel 0 of flattened position q
__device__ __forceinline__ size_t cn_base(long long q, int C, int HW) {
    const long long n = q / HW;
    return (size_t)n * (size_t)C * (size_t)HW + (size_t)(q - n * HW);
}

// sum over the 64 lanes, the same bits in every lane
__device__ __forceinline__ float cn_wave_sum(float v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- column --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_fwd_column_kernel(const float* x, const float* scales, const float* bias, float* y,
                                                            float* mean, float* rstd, long long P, int C, int HW, float eps) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    const size_t base = cn_base(q, C, HW);
    float v[kCnColumnMaxC];
    float s = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < kCnColumnMaxC; ++k) {
        v[k] = 0.f;
        if (k < C) {
            v[k] = x[base + (size_t)k * HW];
            s += v[k];
            sq += v[k] * v[k];
        }
    }
    float mu, rs;
    cn_finalize((double)s, (double)sq, C, eps, mu, rs);
    if (mean) mean[q] = mu;
    if (rstd) rstd[q] = rs;
#pragma unroll
    for (int k = 0; k < kCnColumnMaxC; ++k)
        if (k < C) y[base + (size_t)k * HW] = cn_y(v[k], mu, rs, scales[k], bias[k]);
}

// Every WAVE is persistent over the tiles gw, gw + waves, ...; the four waves of a workgroup meet in LDS at the end and the
// workgroup writes partial[blockIdx.x][2][C] (sum dy * xh, sum dy).
__global__ __launch_bounds__(256) void cn_bwd_column_kernel(const float* x, const float* scales, const float* mean,
                                                            const float* rstd, const float* dy, float* dx, float* partial,
                                                            long long P, int C, int HW, int tiles, int overwrite) {
    __shared__ float red[4][2][kCnColumnMaxCBwd];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float cf = (float)C;
    float as[kCnColumnMaxCBwd], ab[kCnColumnMaxCBwd];
#pragma unroll
    for (int k = 0; k < kCnColumnMaxCBwd; ++k) as[k] = ab[k] = 0.f;
    for (long long tile = (long long)blockIdx.x * 4 + wid; tile < tiles; tile += (long long)gridDim.x * 4) {
        const long long q = tile * kCnTile + lane;
        if (q >= P) continue;
        const size_t base = cn_base(q, C, HW);
        const float mu = mean[q], rs = rstd[q];
        float v[kCnColumnMaxCBwd], d[kCnColumnMaxCBwd];
        float ds = 0.f, db = 0.f;
#pragma unroll
        for (int k = 0; k < kCnColumnMaxCBwd; ++k) {
            v[k] = d[k] = 0.f;
            if (k < C) {
                v[k] = x[base + (size_t)k * HW];
                d[k] = dy[base + (size_t)k * HW];
                const float xh = (v[k] - mu) * rs;
                const float t = d[k] * scales[k];
                ds += t * xh;
                db += t;
                as[k] += d[k] * xh;
                ab[k] += d[k];
            }
        }
        if (!dx) continue;
#pragma unroll
        for (int k = 0; k < kCnColumnMaxCBwd; ++k) {
            if (k < C) {
                const float dxv = cn_dxv(v[k], d[k], scales[k], mu, rs, ds, db, cf);
                const size_t at = base + (size_t)k * HW;
                dx[at] = overwrite ? dxv : dx[at] + dxv;
            }
        }
    }
    if (!partial) return;
#pragma unroll
    for (int k = 0; k < kCnColumnMaxCBwd; ++k) {
        if (k < C) {
            const float a = cn_wave_sum(as[k]), b = cn_wave_sum(ab[k]);
            if (lane == 0) {
                red[wid][0][k] = a;
                red[wid][1][k] = b;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        const int h = threadIdx.x / C, k = threadIdx.x - h * C;
        partial[((size_t)blockIdx.x * 2 + h) * C + k] = ((red[0][h][k] + red[1][h][k]) + red[2][h][k]) + red[3][h][k];
    }
}

// ---- resident and stream ---------------------------------------------------------------------------------------------------------
// The geometry of a tile for one thread. Adding: lane = position, wave wid takes the channels [c_lo, c_hi). Moving: either
// the same lane / wave-strided channels (4-byte route) or, with vec, quad = tid & 15 of four positions and the channels
// tid / 16, tid / 16 + T / 16, ... (16-byte route; HW % 4 == 0 keeps a quad inside one image and on a 16-byte boundary).
struct CnTile {
    long long q;      // this lane's position
    bool live;        // q < P
    size_t base;      // offset of its channel 0
    bool qlive;       // the quad's first position < P (P % 4 == 0 with vec: the quad is whole)
    size_t qbase;     // offset of channel 0 of the quad's first position
    __device__ CnTile(long long tile, long long P, int C, int HW, bool vec) {
        const int lane = threadIdx.x & 63;
        q = tile * kCnTile + lane;
        live = q < P;
        base = live ? cn_base(q, C, HW) : 0;
        const long long qq = tile * kCnTile + (threadIdx.x & 15) * 4;
        qlive = vec && qq < P;
        qbase = qlive ? cn_base(qq, C, HW) : 0;
    }
};

// the tile of src -> LDS [C][64]; positions past P become 0
__device__ __forceinline__ void cn_stage(const float* src, float* lds, const CnTile& t, int C, int HW, bool vec) {
    const int T = blockDim.x, tid = threadIdx.x;
    if (vec) {
        const int quad = tid & 15;
#pragma unroll 4
        for (int c = tid >> 4; c < C; c += T >> 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t.qlive) v = *reinterpret_cast<const float4*>(src + t.qbase + (size_t)c * HW);
            *reinterpret_cast<float4*>(lds + c * kCnTile + quad * 4) = v;
        }
    } else {
        const int lane = tid & 63;
#pragma unroll 4
        for (int c = tid >> 6; c < C; c += T >> 6) lds[c * kCnTile + lane] = t.live ? src[t.base + (size_t)c * HW] : 0.f;
    }
}

// per-lane partials of the waves -> totals of the 64 positions in double, waves in ascending order; threads 0 .. 63 only
__device__ __forceinline__ void cn_wave_totals(const float* red, int waves, int lane, double& a, double& b) {
    a = 0.0;
    b = 0.0;
    for (int w = 0; w < waves; ++w) {
        a += (double)red[(w * 2 + 0) * kCnTile + lane];
        b += (double)red[(w * 2 + 1) * kCnTile + lane];
    }
}

// One workgroup per tile. Dynamic LDS: red [waves][2][64], stat [2][64], then with RES the tile of x [C][64].
template <bool RES>
__global__ __launch_bounds__(RES ? kCnResWaves * 64 : kCnStreamWaves * 64) void cn_fwd_tile_kernel(
    const float* x, const float* scales, const float* bias, float* y, float* mean, float* rstd, long long P, int C, int HW,
    int cpw, float eps, int vec) {
    extern __shared__ float4 cn_smem[];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, waves = T >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's number, in a scalar register: so are its channels
    float* red = reinterpret_cast<float*>(cn_smem);
    float* stat = red + waves * 2 * kCnTile;
    float* sx = stat + 2 * kCnTile;
    const CnTile t(blockIdx.x, P, C, HW, vec != 0);
    if (RES) {
        cn_stage(x, sx, t, C, HW, vec != 0);
        __syncthreads();
    }
    const int c_lo = wid * cpw, c_hi = min(C, c_lo + cpw);
    float s = 0.f, sq = 0.f;
    if (t.live) {
#pragma unroll 8
        for (int c = c_lo; c < c_hi; ++c) {
            const float v = RES ? sx[c * kCnTile + lane] : x[t.base + (size_t)c * HW];
            s += v;
            sq += v * v;
        }
    }
    red[(wid * 2 + 0) * kCnTile + lane] = s;
    red[(wid * 2 + 1) * kCnTile + lane] = sq;
    __syncthreads();
    if (tid < kCnTile) {
        double sd, qd;
        cn_wave_totals(red, waves, lane, sd, qd);
        float mu, rs;
        cn_finalize(sd, qd, C, eps, mu, rs);
        stat[lane] = mu;
        stat[kCnTile + lane] = rs;
        if (t.live) {
            if (mean) mean[t.q] = mu;
            if (rstd) rstd[t.q] = rs;
        }
    }
    __syncthreads();
    if (vec) {
        if (!t.qlive) return;
        const int quad = tid & 15;
        const float4 mu = *reinterpret_cast<const float4*>(stat + quad * 4);
        const float4 rs = *reinterpret_cast<const float4*>(stat + kCnTile + quad * 4);
#pragma unroll 4
        for (int c = tid >> 4; c < C; c += T >> 4) {
            const size_t at = t.qbase + (size_t)c * HW;
            const float4 v = RES ? *reinterpret_cast<const float4*>(sx + c * kCnTile + quad * 4)
                                 : *reinterpret_cast<const float4*>(x + at);
            const float g = scales[c], b = bias[c];
            *reinterpret_cast<float4*>(y + at) = make_float4(cn_y(v.x, mu.x, rs.x, g, b), cn_y(v.y, mu.y, rs.y, g, b),
                                                             cn_y(v.z, mu.z, rs.z, g, b), cn_y(v.w, mu.w, rs.w, g, b));
        }
    } else {
        if (!t.live) return;
        const float mu = stat[lane], rs = stat[kCnTile + lane];
#pragma unroll 4
        for (int c = wid; c < C; c += waves) {
            const size_t at = t.base + (size_t)c * HW;
            y[at] = cn_y(RES ? sx[c * kCnTile + lane] : x[at], mu, rs, scales[c], bias[c]);
        }
    }
}

// One position's terms of the channels c0 .. c0 + KMAX - 1 below c_hi, xs / ds at the position (memory or LDS), `stride` floats
// between channels: ds += t * xh, db += t, as[k] += dy * xh, ab[k] += dy. Groups of eight channels: a uniform branch skips a
// group past c_hi, inside a group a channel past c_hi reads the group's last real one and adds zeros -- straight-line code
// with the accumulators indexed at compile time, eight channels' loads in flight.
template <int KMAX>
__device__ __forceinline__ void cn_bwd_terms(const float* xs, const float* dys, size_t stride, const float* scales, int c0,
                                             int c_hi, float mu, float rs, float (&as)[KMAX], float (&ab)[KMAX], float& ds,
                                             float& db) {
#pragma unroll
    for (int k0 = 0; k0 < KMAX; k0 += 8) {
        if (c0 + k0 < c_hi) {
            float v[8], d[8], g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = min(c0 + k0 + j, c_hi - 1);
                v[j] = xs[(size_t)c * stride];
                d[j] = dys[(size_t)c * stride];
                g[j] = scales[c];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dd = c0 + k0 + j < c_hi ? d[j] : 0.f;
                const float xh = (v[j] - mu) * rs;
                const float tt = dd * g[j];
                ds += tt * xh;
                db += tt;
                as[k0 + j] += dd * xh;
                ab[k0 + j] += dd;
            }
        }
    }
}

// A workgroup is persistent over the tiles blockIdx.x, + gridDim.x, ... Wave wid owns the channels [wid cpw, (wid + 1) cpw):
// it adds their t * xh and t into the position sums of every tile, and their dy * xh and dy into KMAX register pairs per lane
// over all its tiles. A wave with more than KMAX channels (C > 8 * 32) takes further passes over the tiles for
// the channels past the first KMAX: pass 0 does everything else, pass j re-reads only its own KMAX channels per wave.
// Dynamic LDS: red [waves][2][64], stat [4][64] (mean, rstd, ds, db).
// partial: [gridDim.x][2][C] or null.
template <int KMAX>
__global__ __launch_bounds__(kCnStreamWavesBwd * 64) void cn_bwd_tile_kernel(
    const float* x, const float* scales, const float* mean, const float* rstd, const float* dy, float* dx, float* partial,
    long long P, int C, int HW, int cpw, int tiles, int overwrite, int vec) {
    extern __shared__ float4 cn_smem[];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, waves = T >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's number, in a scalar register: so are its channels
    float* red = reinterpret_cast<float*>(cn_smem);
    float* stat = red + waves * 2 * kCnTile;
    const int c_lo = wid * cpw, c_hi = min(C, c_lo + cpw);
    const float cf = (float)C;
    for (int pass = 0; pass == 0 || (partial && pass * KMAX < cpw); ++pass) {  // later passes serve the per-channel sums alone
        float as[KMAX], ab[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) as[k] = ab[k] = 0.f;
        for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const CnTile t(tile, P, C, HW, vec != 0);
            const float mu = t.live ? mean[t.q] : 0.f, rs = t.live ? rstd[t.q] : 0.f;
            if (pass > 0) {  // the per-channel sums of this pass's channels alone
                float unused_s = 0.f, unused_b = 0.f;
                if (t.live)
                    cn_bwd_terms<KMAX>(x + t.base, dy + t.base, (size_t)HW, scales, c_lo + pass * KMAX, c_hi, mu, rs, as, ab,
                                       unused_s, unused_b);
                continue;
            }
            float ds = 0.f, db = 0.f;
            if (t.live) {
                cn_bwd_terms<KMAX>(x + t.base, dy + t.base, (size_t)HW, scales, c_lo, c_hi, mu, rs, as, ab, ds, db);
#pragma unroll 4
                for (int c = c_lo + KMAX; c < c_hi; ++c) {  // the channels whose per-channel sums a later pass takes
                    const float xh = (x[t.base + (size_t)c * HW] - mu) * rs;
                    const float tt = dy[t.base + (size_t)c * HW] * scales[c];
                    ds += tt * xh;
                    db += tt;
                }
            }
            if (!dx) continue;  // (uniform) nothing below but the data gradient
            red[(wid * 2 + 0) * kCnTile + lane] = ds;
            red[(wid * 2 + 1) * kCnTile + lane] = db;
            if (wid == 0) {
                stat[lane] = mu;
                stat[kCnTile + lane] = rs;
            }
            __syncthreads();
            if (tid < kCnTile) {
                double a, b;
                cn_wave_totals(red, waves, lane, a, b);
                stat[2 * kCnTile + lane] = (float)a;
                stat[3 * kCnTile + lane] = (float)b;
            }
            __syncthreads();
            if (vec) {
                if (t.qlive) {
                    const int quad = tid & 15;
                    const float4 m4 = *reinterpret_cast<const float4*>(stat + quad * 4);
                    const float4 r4 = *reinterpret_cast<const float4*>(stat + kCnTile + quad * 4);
                    const float4 s4 = *reinterpret_cast<const float4*>(stat + 2 * kCnTile + quad * 4);
                    const float4 b4 = *reinterpret_cast<const float4*>(stat + 3 * kCnTile + quad * 4);
#pragma unroll 2
                    for (int c = tid >> 4; c < C; c += T >> 4) {
                        const size_t at = t.qbase + (size_t)c * HW;
                        const float4 v = *reinterpret_cast<const float4*>(x + at);
                        const float4 d = *reinterpret_cast<const float4*>(dy + at);
                        const float g = scales[c];
                        float4 o = make_float4(cn_dxv(v.x, d.x, g, m4.x, r4.x, s4.x, b4.x, cf),
                                               cn_dxv(v.y, d.y, g, m4.y, r4.y, s4.y, b4.y, cf),
                                               cn_dxv(v.z, d.z, g, m4.z, r4.z, s4.z, b4.z, cf),
                                               cn_dxv(v.w, d.w, g, m4.w, r4.w, s4.w, b4.w, cf));
                        if (!overwrite) {
                            const float4 a = *reinterpret_cast<const float4*>(dx + at);
                            o.x = a.x + o.x; o.y = a.y + o.y; o.z = a.z + o.z; o.w = a.w + o.w;
                        }
                        *reinterpret_cast<float4*>(dx + at) = o;
                    }
                }
            } else if (t.live) {
                const float dsf = stat[2 * kCnTile + lane], dbf = stat[3 * kCnTile + lane];
#pragma unroll 2
                for (int c = wid; c < C; c += waves) {
                    const size_t at = t.base + (size_t)c * HW;
                    const float dxv = cn_dxv(x[at], dy[at], scales[c], mu, rs, dsf, dbf, cf);
                    dx[at] = overwrite ? dxv : dx[at] + dxv;
                }
            }
            __syncthreads();  // the next tile rewrites red and stat
        }
        if (partial) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int c = c_lo + pass * KMAX + k;
                if (c < c_hi) {
                    const float a = cn_wave_sum(as[k]), b = cn_wave_sum(ab[k]);
                    if (lane == 0) {
                        partial[((size_t)blockIdx.x * 2 + 0) * C + c] = a;
                        partial[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
                    }
                }
            }
        }
    }
}

// dscales[c] += sum_g partial[g][0][c], db likewise: workgroups in ascending order in double, the start value one float32
// addition
__global__ void cn_param_kernel(const float* partial, int groups, int C, float* dscales, float* dbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
#pragma unroll 8  // eight workgroups' loads in flight; the additions keep their order
    for (int g = 0; g < groups; ++g) {
        a += (double)partial[((size_t)g * 2 + 0) * C + c];
        b += (double)partial[((size_t)g * 2 + 1) * C + c];
    }
    if (dscales) dscales[c] = dscales[c] + (float)a;
    if (dbias) dbias[c] = dbias[c] + (float)b;
}

static long long cn_total(const char* who, int n, int c, int hw) {
    const long long total = (long long)n * c * hw;
    if (n < 0 || c < 0 || hw < 0 || total >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] %s: a negative extent, or a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    return total;
}

static const char* const kCnFwdTag[3] = {"channel_norm_fwd:column", "channel_norm_fwd:resident", "channel_norm_fwd:stream"};
static const char* const kCnBwdTag[2] = {"channel_norm_bwd:column", "channel_norm_bwd:stream"};  // the backward has no resident path

template <int KMAX>
static void cn_launch_bwd_stream(const bcnn_hip_channel_norm_bwd_args* a, float* partial, long long P, int cpw, int tiles,
                                 int groups, int vec) {
    const size_t lds = (size_t)(kCnStreamWavesBwd * 2 * kCnTile + 4 * kCnTile) * sizeof(float);
    cn_bwd_tile_kernel<KMAX><<<groups, kCnStreamWavesBwd * 64, lds, current_stream()>>>(
        a->x, a->scales, a->mean, a->rstd, a->dy, a->dx, partial, P, a->c, a->hw, cpw, tiles, a->overwrite, vec);
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_channel_norm_path(int n, int c, int hw, int backward) {
    (void)n;
    if (c <= 0 || hw <= 0) return -1;
    return cn_path(c, backward);
}

// every launch is traced under the path's tag: the number of tags is the number of launches
void bcnn_hip_channel_norm_forward(const bcnn_hip_channel_norm_fwd_args* a) {
    const long long total = cn_total("bcnn_hip_channel_norm_forward", a->n, a->c, a->hw);
    if (!total) return;
    const int C = a->c, HW = a->hw;
    const long long P = (long long)a->n * HW;
    const float eps = a->eps > 0.f ? a->eps : 1e-5f;
    const int path = cn_path(C, 0);
    trace_kernel(kCnFwdTag[path]);
    if (path == 0) {
        cn_fwd_column_kernel<<<(unsigned)ceil_div(P, 256), 256, 0, current_stream()>>>(a->x, a->scales, a->b, a->y, a->mean,
                                                                                        a->rstd, P, C, HW, eps);
        KERNEL_CHECK();
        return;
    }
    const int vec = (HW & 3) == 0 && al16(a->x) && al16(a->y);
    const unsigned tiles = (unsigned)ceil_div(P, kCnTile);
    if (path == 1) {
        const size_t lds = (size_t)(kCnFwdHead + C * kCnTile) * sizeof(float);
        cn_fwd_tile_kernel<true><<<tiles, kCnResWaves * 64, lds, current_stream()>>>(
            a->x, a->scales, a->b, a->y, a->mean, a->rstd, P, C, HW, ceil_div(C, kCnResWaves), eps, vec);
    } else {
        const size_t lds = (size_t)(kCnStreamWaves * 2 * kCnTile + 2 * kCnTile) * sizeof(float);
        cn_fwd_tile_kernel<false><<<tiles, kCnStreamWaves * 64, lds, current_stream()>>>(
            a->x, a->scales, a->b, a->y, a->mean, a->rstd, P, C, HW, ceil_div(C, kCnStreamWaves), eps, vec);
    }
    KERNEL_CHECK();
}

void bcnn_hip_channel_norm_backward(const bcnn_hip_channel_norm_bwd_args* a) {
    const long long total = cn_total("bcnn_hip_channel_norm_backward", a->n, a->c, a->hw);
    if (!total || (!a->dx && !a->dscales && !a->db)) return;
    const int C = a->c, HW = a->hw;
    const long long P = (long long)a->n * HW;
    const bool params = a->dscales || a->db;
    const int path = cn_path(C, 1);
    const int tiles = ceil_div(P, kCnTile);
    // the persistent workgroups: a function of the shape alone (a column workgroup is four waves with a tile list each)
    const int groups = path == 0 ? std::min(ceil_div(tiles, 4), kCnMaxGroups) : std::min(tiles, kCnMaxGroups);
    float* partial = params ? scratch(SCRATCH_REDUCE, (size_t)groups * 2 * C) : nullptr;
    const int vec = (HW & 3) == 0 && al16(a->x) && al16(a->dy) && (!a->dx || al16(a->dx));
    trace_kernel(kCnBwdTag[path ? 1 : 0]);
    if (path == 0) {
        cn_bwd_column_kernel<<<groups, 256, 0, current_stream()>>>(a->x, a->scales, a->mean, a->rstd, a->dy, a->dx, partial, P,
                                                                   C, HW, tiles, a->overwrite);
    } else {
        const int cpw = ceil_div(C, kCnStreamWavesBwd);
        if (cpw <= 16) cn_launch_bwd_stream<16>(a, partial, P, cpw, tiles, groups, vec);
        else cn_launch_bwd_stream<kCnStreamRegC>(a, partial, P, cpw, tiles, groups, vec);
    }
    KERNEL_CHECK();
    if (params) {
        trace_kernel("channel_norm_bwd:params");
        cn_param_kernel<<<ceil_div(C, 256), 256, 0, current_stream()>>>(partial, groups, C, a->dscales, a->db);
        KERNEL_CHECK();
    }
}

}  // extern "C"
