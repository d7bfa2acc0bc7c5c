// group_norm.hip -- the group-normalisation node (layer norm over (C,H,W) is groups = 1, instance norm groups = C). No
// reference counterpart. In NCHW the group g of image n is ONE contiguous row of m = (C/G) * HW floats, row r = n * G + g, made
// of C/G planes of HW floats; plane r * (C/G) + p of the tensor has channel g * (C/G) + p. HBM-bound kernels.
//   forward : mean and biased variance of a row from its sums of x and x^2, rstd = (float)(1 / sqrt(var + eps));
//             xh = (x - mean) * rstd, y = xh * gamma[ch] + beta[ch], every operation one float32 rounding (the build has
//             -ffp-contract=off): y is the bits of that numpy float32 expression on the stored float32 mean and rstd.
//   backward: takes mean and rstd, recomputes xh. t = dy * gamma[ch]; ds = sum_m t * xh, db = sum_m t;
//             dxv = (t - (xh * ds + db) / m) * rstd; dx = dxv or dx + dxv. The sweep that forms ds and db sums PLANE by plane
//             and also leaves sum_hw dy * xh and sum_hw dy of every plane in scratch; one small kernel adds them over n, in
//             ascending order in double, into dgamma and dbeta (the start value enters as one float32 addition).
// Three paths, chosen from the shape alone (bcnn_hip_group_norm_path):
//   lanes    (m <= 1024): a group of 2^k lanes (1..64), the smallest that covers the row, owns a row; consecutive groups own
//            consecutive rows, so a wave reads one contiguous run. Scalar accesses throughout (a row is at most 4 KB).
//   resident (m <= 16128 forward, 8064 backward): one workgroup owns a row and keeps it (and dy) in LDS, at most 64 KB:
//            x (and dy) are read from memory once.
//   split    (larger rows): forward cuts a row into slices (chan_splits with the rows as channels), a finalize kernel leaves
//            mean and rstd, a map sweep applies them; backward sums plane by plane (planes as chan_reduce's channels, or a
//            lane group per small plane), a finalize kernel adds a row's planes, a map sweep writes dx.
// Summation order, every path: float32 per lane in ascending index order; lanes by a butterfly whose last step is in double;
// waves, slices and planes in ascending order in double. No atomics: two runs give the same bits.
#include "chan_reduce.h"

namespace bcnn_hip {

constexpr int kGnLanesMaxRow = 1024;         // up to here a lane group owns a row
constexpr int kGnLdsFloats = 16384 - 256;    // 64 KB of LDS less 1 KB for the cross-wave sums: what a resident workgroup holds
constexpr int kGnUnitMaxHW = 1024;           // planes below this are summed by a lane group, larger ones by a workgroup

static int gn_path(int m, int backward) {
    if (m <= kGnLanesMaxRow) return 0;
    if (m <= (backward ? kGnLdsFloats / 2 : kGnLdsFloats)) return 1;
    return 2;
}

// sum over `width` (a power of two, 1..64) consecutive lanes, the same bits in each of them; the last step in double
__device__ __forceinline__ double gn_group_sum(float v, int width) {
    for (int off = width >> 1; off >= 2; off >>= 1) v += __shfl_xor(v, off, 64);
    double d = (double)v;
    if (width >= 2) d += (double)__shfl_xor(v, 1, 64);
    return d;
}

__device__ __forceinline__ void gn_finalize(double s, double q, int m, float eps, float& mean, float& rstd) {
    const double mu = s / (double)m;
    double var = q / (double)m - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ float gn_y(float x, float mu, float rs, float g, float b) {
    const float xh = (x - mu) * rs;
    return xh * g + b;
}

__device__ __forceinline__ float gn_dxv(float x, float d, float g, float mu, float rs, float ds, float db, float mf) {
    const float xh = (x - mu) * rs;
    const float t = d * g;
    return (t - (xh * ds + db) / mf) * rs;
}

// gamma (and beta) of the 4 elements i .. i + 3 of a row; g0 is the row's first channel. One division when the four share
// a plane, else (HW % 4 != 0) per element.
__device__ __forceinline__ void gn_affine4(int i, int HW, int g0, const float* gamma, const float* beta, float (&g)[4],
                                           float (&b)[4]) {
    const int p = i / HW;
    if (i - p * HW + 4 <= HW) {
        g[0] = g[1] = g[2] = g[3] = gamma[g0 + p];
        if (beta) b[0] = b[1] = b[2] = b[3] = beta[g0 + p];
    } else {
        for (int k = 0; k < 4; ++k) {
            const int ch = g0 + (i + k) / HW;
            g[k] = gamma[ch];
            if (beta) b[k] = beta[ch];
        }
    }
}

__device__ __forceinline__ float4 gn_fwd4(float4 v, int i, int HW, int g0, const float* gamma, const float* beta, float mu,
                                          float rs) {
    float g[4], b[4];
    gn_affine4(i, HW, g0, gamma, beta, g, b);
    return make_float4(gn_y(v.x, mu, rs, g[0], b[0]), gn_y(v.y, mu, rs, g[1], b[1]), gn_y(v.z, mu, rs, g[2], b[2]),
                       gn_y(v.w, mu, rs, g[3], b[3]));
}

__device__ __forceinline__ float4 gn_dx4(float4 v, float4 d, int i, int HW, int g0, const float* gamma, float mu, float rs,
                                         float ds, float db, float mf) {
    float g[4], unused[4];
    gn_affine4(i, HW, g0, gamma, nullptr, g, unused);
    return make_float4(gn_dxv(v.x, d.x, g[0], mu, rs, ds, db, mf), gn_dxv(v.y, d.y, g[1], mu, rs, ds, db, mf),
                       gn_dxv(v.z, d.z, g[2], mu, rs, ds, db, mf), gn_dxv(v.w, d.w, g[3], mu, rs, ds, db, mf));
}

// the four sums of a plane: acc[0] += dy * xh, acc[1] += dy, acc[2] += t * xh, acc[3] += t
__device__ __forceinline__ void gn_bwd_term(float x, float d, float g, float mu, float rs, float (&acc)[4]) {
    const float xh = (x - mu) * rs;
    const float t = d * g;
    acc[0] += d * xh;
    acc[1] += d;
    acc[2] += t * xh;
    acc[3] += t;
}

// A unit of `lp` lanes (this lane is number u of it) sums one plane of HW floats at xs / ds (memory or LDS); the totals come
// back in every lane of the unit. Every lane of the wave must call it (shuffles); `valid` guards the reads. A unit wider than
// a wave (the whole workgroup) gets its wave's totals: the caller adds the waves.
__device__ __forceinline__ void gn_plane_unit(const float* xs, const float* ds, int HW, int lp, int u, bool valid, bool vec,
                                              float mu, float rs, float g, double (&tot)[4]) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        if (vec) {
            for (int i = u * 4; i < HW; i += lp * 4) {
                const float4 v = *reinterpret_cast<const float4*>(xs + i);
                const float4 d = *reinterpret_cast<const float4*>(ds + i);
                gn_bwd_term(v.x, d.x, g, mu, rs, acc);
                gn_bwd_term(v.y, d.y, g, mu, rs, acc);
                gn_bwd_term(v.z, d.z, g, mu, rs, acc);
                gn_bwd_term(v.w, d.w, g, mu, rs, acc);
            }
        } else {
            for (int i = u; i < HW; i += lp) gn_bwd_term(xs[i], ds[i], g, mu, rs, acc);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = gn_group_sum(acc[k], lp < kWave ? lp : kWave);
}

// lanes per plane unit: the smallest power of two that covers the plane's elements (float4s with vec), at most `cap`
static int gn_unit_lanes(int HW, bool vec, int cap) {
    const int items = vec ? HW / 4 : HW;
    int lp = 1;
    while (lp < items && lp < cap) lp <<= 1;
    return lp;
}

// ---- lanes ---------------------------------------------------------------------------------------------------------------------
// A group of `lanes` consecutive threads owns row (global thread / lanes); lane j takes elements j, j + lanes, ... (at most 16:
// lanes == 64 whenever the row is longer than 64) and keeps them in registers between the sums and the output.
__global__ __launch_bounds__(256) void gn_fwd_lanes_kernel(const float* x, const float* gamma, const float* beta, float* y,
                                                           float* mean, float* rstd, long long rows, int G, int cg, int HW,
                                                           int m, int lanes, float eps) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t / lanes;
    const int j = (int)(t - row * lanes);
    const bool live = row < rows;  // (whole groups are in or out)
    const size_t base = (size_t)row * m;
    float v[kGnLanesMaxRow / 64];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < kGnLanesMaxRow / 64; ++k) {
        v[k] = 0.f;
        if (k * lanes >= m) break;
        const int i = j + k * lanes;
        if (live && i < m) {
            v[k] = x[base + i];
            s += v[k];
            q += v[k] * v[k];
        }
    }
    const double sd = gn_group_sum(s, lanes), qd = gn_group_sum(q, lanes);
    float mu, rs;
    gn_finalize(sd, qd, m, eps, mu, rs);
    if (!live) return;
    if (j == 0) {
        if (mean) mean[row] = mu;
        if (rstd) rstd[row] = rs;
    }
    const int g0 = (int)(row % G) * cg;
#pragma unroll
    for (int k = 0; k < kGnLanesMaxRow / 64; ++k) {
        if (k * lanes >= m) break;
        const int i = j + k * lanes;
        if (i < m) {
            const int ch = g0 + i / HW;
            y[base + i] = gn_y(v[k], mu, rs, gamma[ch], beta[ch]);
        }
    }
}

// Backward: the group's lanes split into units of lp lanes (lp covers a plane), unit su takes planes su, su + units, ... of the
// row; the units' double sums are added by a butterfly. Then lane j writes dx of elements j, j + lanes, ... (x and dy again,
// from the cache). psum: [2][planes] (sum dy * xh, sum dy) or null.
__global__ __launch_bounds__(256) void gn_bwd_lanes_kernel(const float* x, const float* gamma, const float* mean,
                                                           const float* rstd, const float* dy, float* dx, float* psum,
                                                           long long rows, int G, int cg, int HW, int m, int lanes, int lp,
                                                           int overwrite) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t / lanes;
    const int j = (int)(t - row * lanes);
    const bool live = row < rows;
    const size_t base = (size_t)row * m;
    const long long planes = rows * cg;
    const int units = lanes / lp, su = j / lp, u = j - su * lp;
    const float mu = live ? mean[row] : 0.f, rs = live ? rstd[row] : 0.f;
    const int g0 = live ? (int)(row % G) * cg : 0;
    double rds = 0.0, rdb = 0.0;
    for (int p0 = 0; p0 < cg; p0 += units) {
        const int p = p0 + su;
        const bool valid = live && p < cg;
        double tot[4];
        const size_t at = base + (size_t)p * HW;
        gn_plane_unit(x + at, dy + at, HW, lp, u, valid, false, mu, rs, valid ? gamma[g0 + p] : 0.f, tot);
        rds += tot[2];
        rdb += tot[3];
        if (valid && u == 0 && psum) {
            psum[row * cg + p] = (float)tot[0];
            psum[planes + row * cg + p] = (float)tot[1];
        }
    }
    for (int off = lp; off < lanes; off <<= 1) {
        rds += __shfl_xor(rds, off, 64);
        rdb += __shfl_xor(rdb, off, 64);
    }
    if (!live || !dx) return;
    const float ds = (float)rds, db = (float)rdb, mf = (float)m;
    for (int i = j; i < m; i += lanes) {
        const float dxv = gn_dxv(x[base + i], dy[base + i], gamma[g0 + i / HW], mu, rs, ds, db, mf);
        dx[base + i] = overwrite ? dxv : dx[base + i] + dxv;
    }
}

// ---- resident ------------------------------------------------------------------------------------------------------------------
// per-wave totals (the same in every lane of a wave) -> block totals in every thread, waves in ascending order
template <int NV>
__device__ __forceinline__ void gn_block_combine(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();  // the previous round's readers are done with red
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[wid * NV + k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) {
        double tsum = 0.0;
        for (int w = 0; w < nw; ++w) tsum += red[w * NV + k];
        v[k] = tsum;
    }
}

// One workgroup (256 or 1024 threads) per row; dynamic LDS: the row, then 16 x 4 doubles for the cross-wave sums.
__global__ __launch_bounds__(1024) void gn_fwd_resident_kernel(const float* x, const float* gamma, const float* beta, float* y,
                                                               float* mean, float* rstd, int G, int cg, int HW, int m,
                                                               float eps, int vec) {
    extern __shared__ float4 gn_smem[];
    float* sx = reinterpret_cast<float*>(gn_smem);
    double* red = reinterpret_cast<double*>(sx + ((m + 3) & ~3));
    const int T = blockDim.x, tid = threadIdx.x;
    const long long row = blockIdx.x;
    const size_t base = (size_t)row * m;
    float s = 0.f, q = 0.f;
    if (vec) {
#pragma unroll 4
        for (int i = tid * 4; i < m; i += T * 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + base + i);
            *reinterpret_cast<float4*>(sx + i) = v;
            s += v.x; q += v.x * v.x;
            s += v.y; q += v.y * v.y;
            s += v.z; q += v.z * v.z;
            s += v.w; q += v.w * v.w;
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < m; i += T) {
            const float v = x[base + i];
            sx[i] = v;
            s += v;
            q += v * v;
        }
    }
    double sums[2] = {gn_group_sum(s, 64), gn_group_sum(q, 64)};
    gn_block_combine<2>(sums, red);
    float mu, rs;
    gn_finalize(sums[0], sums[1], m, eps, mu, rs);
    if (tid == 0) {
        if (mean) mean[row] = mu;
        if (rstd) rstd[row] = rs;
    }
    const int g0 = (int)(row % G) * cg;
    if (vec) {
        for (int i = tid * 4; i < m; i += T * 4)
            *reinterpret_cast<float4*>(y + base + i) =
                gn_fwd4(*reinterpret_cast<const float4*>(sx + i), i, HW, g0, gamma, beta, mu, rs);
    } else {
        for (int i = tid; i < m; i += T) {
            const int ch = g0 + i / HW;
            y[base + i] = gn_y(sx[i], mu, rs, gamma[ch], beta[ch]);
        }
    }
}

// dynamic LDS: x of the row, dy of the row, then the cross-wave sums. Planes below kGnUnitMaxHW are summed by units of lp lanes
// (unit su takes planes su, su + units, ...), larger ones by the whole workgroup, one after the other.
__global__ __launch_bounds__(1024) void gn_bwd_resident_kernel(const float* x, const float* gamma, const float* mean,
                                                               const float* rstd, const float* dy, float* dx, float* psum,
                                                               long long rows, int G, int cg, int HW, int m, int lp, int vec,
                                                               int overwrite) {
    extern __shared__ float4 gn_smem[];
    const int m4 = (m + 3) & ~3;
    float* sx = reinterpret_cast<float*>(gn_smem);
    float* sd = sx + m4;
    double* red = reinterpret_cast<double*>(sd + m4);
    const int T = blockDim.x, tid = threadIdx.x;
    const long long row = blockIdx.x;
    const size_t base = (size_t)row * m;
    const long long planes = rows * cg;
    if (vec) {
#pragma unroll 4
        for (int i = tid * 4; i < m; i += T * 4) {
            *reinterpret_cast<float4*>(sx + i) = *reinterpret_cast<const float4*>(x + base + i);
            *reinterpret_cast<float4*>(sd + i) = *reinterpret_cast<const float4*>(dy + base + i);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < m; i += T) {
            sx[i] = x[base + i];
            sd[i] = dy[base + i];
        }
    }
    __syncthreads();
    const float mu = mean[row], rs = rstd[row];
    const int g0 = (int)(row % G) * cg;
    const bool pvec = (HW & 3) == 0;  // a plane starts on a 16-byte boundary of the LDS copy
    double rsum[2] = {0.0, 0.0};
    if (HW < kGnUnitMaxHW) {
        const int units = T / lp, su = tid / lp, u = tid - su * lp;
        for (int p0 = 0; p0 < cg; p0 += units) {
            const int p = p0 + su;
            const bool valid = p < cg;
            double tot[4];
            gn_plane_unit(sx + (size_t)p * HW, sd + (size_t)p * HW, HW, lp, u, valid, pvec, mu, rs,
                          valid ? gamma[g0 + p] : 0.f, tot);
            rsum[0] += tot[2];
            rsum[1] += tot[3];
            if (valid && u == 0 && psum) {
                psum[row * cg + p] = (float)tot[0];
                psum[planes + row * cg + p] = (float)tot[1];
            }
        }
        for (int off = lp; off < 64; off <<= 1) {  // the units of a wave
            rsum[0] += __shfl_xor(rsum[0], off, 64);
            rsum[1] += __shfl_xor(rsum[1], off, 64);
        }
        gn_block_combine<2>(rsum, red);
    } else {
        for (int p = 0; p < cg; ++p) {
            double tot[4];
            gn_plane_unit(sx + (size_t)p * HW, sd + (size_t)p * HW, HW, T, tid, true, pvec, mu, rs, gamma[g0 + p], tot);
            gn_block_combine<4>(tot, red);
            rsum[0] += tot[2];
            rsum[1] += tot[3];
            if (tid == 0 && psum) {
                psum[row * cg + p] = (float)tot[0];
                psum[planes + row * cg + p] = (float)tot[1];
            }
        }
    }
    if (!dx) return;
    const float ds = (float)rsum[0], db = (float)rsum[1], mf = (float)m;
    if (vec) {
        for (int i = tid * 4; i < m; i += T * 4) {
            float4 o = gn_dx4(*reinterpret_cast<const float4*>(sx + i), *reinterpret_cast<const float4*>(sd + i), i, HW, g0,
                              gamma, mu, rs, ds, db, mf);
            if (!overwrite) {
                const float4 a = *reinterpret_cast<const float4*>(dx + base + i);
                o.x = a.x + o.x; o.y = a.y + o.y; o.z = a.z + o.z; o.w = a.w + o.w;
            }
            *reinterpret_cast<float4*>(dx + base + i) = o;
        }
    } else {
        for (int i = tid; i < m; i += T) {
            const float dxv = gn_dxv(sx[i], sd[i], gamma[g0 + i / HW], mu, rs, ds, db, mf);
            dx[base + i] = overwrite ? dxv : dx[base + i] + dxv;
        }
    }
}

// ---- split ---------------------------------------------------------------------------------------------------------------------
struct GnStatF {  // chan_reduce with the rows as channels: sums of x and x^2 of a slice
    static constexpr int kInFlight = 4;
    const float* x;
    bool al;
    __device__ void operator()(long long off, int, float (&acc)[2]) const {
        const float v = x[off];
        acc[0] += v;
        acc[1] += v * v;
    }
    __device__ void vec4(long long off, int c, float (&acc)[2]) const {
        if (!al) {
            for (int k = 0; k < 4; ++k) (*this)(off + k, c, acc);
            return;
        }
        const float4 v = *reinterpret_cast<const float4*>(x + off);
        acc[0] += v.x; acc[1] += v.x * v.x;
        acc[0] += v.y; acc[1] += v.y * v.y;
        acc[0] += v.z; acc[1] += v.z * v.z;
        acc[0] += v.w; acc[1] += v.w * v.w;
    }
};

// One wave per row: lane l adds the slices l, l + 64, ... of the row in ascending order, in double; a butterfly adds the lanes.
// stat[row] = mean, stat[rows + row] = rstd (and the caller's buffers).
__global__ __launch_bounds__(256) void gn_fwd_finalize_kernel(const float* partials, long long rows, int splits, int m,
                                                              float eps, float* stat, float* mean, float* rstd) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = row < rows;
    double s = 0.0, q = 0.0;
    if (live) {
        for (int i = lane; i < splits; i += 64) {
            s += (double)partials[(row * splits + i) * 2];
            q += (double)partials[(row * splits + i) * 2 + 1];
        }
    }
    for (int off = 1; off < 64; off <<= 1) {
        s += __shfl_xor(s, off, 64);
        q += __shfl_xor(q, off, 64);
    }
    if (!live || lane != 0) return;
    float mu, rs;
    gn_finalize(s, q, m, eps, mu, rs);
    stat[row] = mu;
    stat[rows + row] = rs;
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
}

struct GnFwdBody {  // launch_chan_map with the rows as planes: c is the row
    const float* x;
    const float* gamma;
    const float* beta;
    float* y;
    const float* stat;
    unsigned rows;
    int G, cg, HW, m;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float mu = stat[c], rs = stat[rows + c];
        const int g0 = (c % G) * cg, i = (int)(off - (unsigned)c * (unsigned)m);
        if (cnt == 4 && al && (off & 3u) == 0) {
            *reinterpret_cast<float4*>(y + off) = gn_fwd4(*reinterpret_cast<const float4*>(x + off), i, HW, g0, gamma, beta, mu, rs);
        } else {
            for (int k = 0; k < cnt; ++k) {
                const int ch = g0 + (i + k) / HW;
                y[off + k] = gn_y(x[off + k], mu, rs, gamma[ch], beta[ch]);
            }
        }
    }
};

struct GnBwdPlaneF {  // chan_reduce with the PLANES as channels (planes of kGnUnitMaxHW elements and more): the four sums
    static constexpr int kInFlight = 2;
    const float* x;
    const float* gamma;
    const float* mean;
    const float* rstd;
    const float* dy;
    int C, cg;
    bool al;
    __device__ void operator()(long long off, int c, float (&acc)[4]) const {
        const int row = c / cg;
        gn_bwd_term(x[off], dy[off], gamma[c % C], mean[row], rstd[row], acc);
    }
    __device__ void vec4(long long off, int c, float (&acc)[4]) const {
        if (!al) {
            for (int k = 0; k < 4; ++k) (*this)(off + k, c, acc);
            return;
        }
        const int row = c / cg;
        const float g = gamma[c % C], mu = mean[row], rs = rstd[row];
        const float4 v = *reinterpret_cast<const float4*>(x + off);
        const float4 d = *reinterpret_cast<const float4*>(dy + off);
        gn_bwd_term(v.x, d.x, g, mu, rs, acc);
        gn_bwd_term(v.y, d.y, g, mu, rs, acc);
        gn_bwd_term(v.z, d.z, g, mu, rs, acc);
        gn_bwd_term(v.w, d.w, g, mu, rs, acc);
    }
};

// small planes of a long row: a unit of lp lanes per plane, consecutive units own consecutive planes; partials[plane][4]
__global__ __launch_bounds__(256) void gn_bwd_planes_kernel(const float* x, const float* gamma, const float* mean,
                                                            const float* rstd, const float* dy, float* partials,
                                                            long long planes, int C, int cg, int HW, int lp, int vec) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long plane = t / lp;
    const int u = (int)(t - plane * lp);
    const bool valid = plane < planes;
    const long long row = valid ? plane / cg : 0;
    double tot[4];
    const size_t at = (size_t)plane * HW;
    gn_plane_unit(x + at, dy + at, HW, lp, u, valid, vec != 0, valid ? mean[row] : 0.f, valid ? rstd[row] : 0.f,
                  valid ? gamma[plane % C] : 0.f, tot);
    if (valid && u == 0)
        for (int k = 0; k < 4; ++k) partials[plane * 4 + k] = (float)tot[k];
}

// One wave per row: lane l adds the planes l, l + 64, ... of the row (each plane's slices in ascending order), all in double;
// a butterfly adds the lanes. rowsum[row] = ds, rowsum[rows + row] = db; psum as above.
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* partials, long long rows, int cg, int splits,
                                                              float* rowsum, float* psum) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = row < rows;
    const long long planes = rows * cg;
    double ds = 0.0, db = 0.0;
    if (live) {
        for (int p = lane; p < cg; p += 64) {
            const long long plane = row * cg + p;
            double a[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < splits; ++i)
                for (int k = 0; k < 4; ++k) a[k] += (double)partials[(plane * splits + i) * 4 + k];
            if (psum) {
                psum[plane] = (float)a[0];
                psum[planes + plane] = (float)a[1];
            }
            ds += a[2];
            db += a[3];
        }
    }
    for (int off = 1; off < 64; off <<= 1) {
        ds += __shfl_xor(ds, off, 64);
        db += __shfl_xor(db, off, 64);
    }
    if (live && lane == 0) {
        rowsum[row] = (float)ds;
        rowsum[rows + row] = (float)db;
    }
}

struct GnBwdBody {  // launch_chan_map with the rows as planes: dx from the row's ds and db
    const float* x;
    const float* gamma;
    const float* mean;
    const float* rstd;
    const float* dy;
    float* dx;
    const float* rowsum;
    unsigned rows;
    int G, cg, HW, m, overwrite;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float mu = mean[c], rs = rstd[c], ds = rowsum[c], db = rowsum[rows + c], mf = (float)m;
        const int g0 = (c % G) * cg, i = (int)(off - (unsigned)c * (unsigned)m);
        if (cnt == 4 && al && (off & 3u) == 0) {
            float4 o = gn_dx4(*reinterpret_cast<const float4*>(x + off), *reinterpret_cast<const float4*>(dy + off), i, HW, g0,
                              gamma, mu, rs, ds, db, mf);
            if (!overwrite) {
                const float4 a = *reinterpret_cast<const float4*>(dx + off);
                o.x = a.x + o.x; o.y = a.y + o.y; o.z = a.z + o.z; o.w = a.w + o.w;
            }
            *reinterpret_cast<float4*>(dx + off) = o;
        } else {
            for (int k = 0; k < cnt; ++k) {
                const float dxv = gn_dxv(x[off + k], dy[off + k], gamma[g0 + (i + k) / HW], mu, rs, ds, db, mf);
                dx[off + k] = overwrite ? dxv : dx[off + k] + dxv;
            }
        }
    }
};

// dgamma[ch] += sum_n psum[n][ch], dbeta likewise: images in ascending order in double, the start value one float32 addition
__global__ void gn_param_reduce_kernel(const float* psum, int N, int C, long long planes, float* dgamma, float* dbeta) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= C) return;
    double a = 0.0, b = 0.0;
#pragma unroll 8  // eight images' loads in flight; the additions keep their order
    for (int n = 0; n < N; ++n) {
        a += (double)psum[(long long)n * C + ch];
        b += (double)psum[planes + (long long)n * C + ch];
    }
    if (dgamma) dgamma[ch] = dgamma[ch] + (float)a;
    if (dbeta) dbeta[ch] = dbeta[ch] + (float)b;
}

static long long gn_total(const char* who, int n, int c, int hw, int groups) {
    const long long total = (long long)n * c * hw;
    if (n < 0 || c < 0 || hw < 0 || total >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] %s: a negative extent, or a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    if (groups <= 0 || c % groups != 0) {
        fprintf(stderr, "[bcnn_hip] %s: %d groups do not divide %d channels\n", who, groups, c);
        exit(1);
    }
    return total;
}

static const char* const kGnFwdTag[3] = {"group_norm_fwd:lanes", "group_norm_fwd:resident", "group_norm_fwd:split"};
static const char* const kGnBwdTag[3] = {"group_norm_bwd:lanes", "group_norm_bwd:resident", "group_norm_bwd:split"};

static int gn_row_lanes(int m) {
    int lanes = 1;
    while (lanes < m && lanes < kWave) lanes <<= 1;
    return lanes;
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_group_norm_path(int n, int c, int hw, int groups, int backward) {
    (void)n;
    if (groups <= 0 || c <= 0 || c % groups != 0 || hw <= 0) return -1;
    return gn_path((c / groups) * hw, backward);
}

// every launch is traced under the path's tag: the number of tags is the number of launches
void bcnn_hip_group_norm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                 int n, int c, int hw, int groups, float eps) {
    const long long total = gn_total("bcnn_hip_group_norm_forward", n, c, hw, groups);
    if (!total) return;
    const int cg = c / groups, m = cg * hw;
    const long long rows = (long long)n * groups;
    const int path = gn_path(m, 0);
    const char* tag = kGnFwdTag[path];
    if (path == 0) {
        const int lanes = gn_row_lanes(m);
        trace_kernel(tag);
        gn_fwd_lanes_kernel<<<(unsigned)ceil_div(rows * lanes, 256), 256, 0, current_stream()>>>(x, gamma, beta, y, mean, rstd,
                                                                                                  rows, groups, cg, hw, m,
                                                                                                  lanes, eps);
        KERNEL_CHECK();
        return;
    }
    if (path == 1) {
        const int vec = (m & 3) == 0 && al16(x) && al16(y);
        const int threads = m <= 4096 ? 256 : 1024;
        const size_t lds = (size_t)((m + 3) & ~3) * sizeof(float) + 16 * 4 * sizeof(double);
        trace_kernel(tag);
        gn_fwd_resident_kernel<<<(unsigned)rows, threads, lds, current_stream()>>>(x, gamma, beta, y, mean, rstd, groups, cg, hw,
                                                                                   m, eps, vec);
        KERNEL_CHECK();
        return;
    }
    const int splits = chan_splits((int)rows, m);
    float* part = scratch(SCRATCH_REDUCE, (size_t)rows * splits * 2 + (size_t)rows * 2);
    float* stat = part + (size_t)rows * splits * 2;
    trace_kernel(tag);
    launch_chan_reduce<2>(GnStatF{x, al16(x)}, (int)rows, m, m, splits, part);
    trace_kernel(tag);
    gn_fwd_finalize_kernel<<<ceil_div(rows, 4), 256, 0, current_stream()>>>(part, rows, splits, m, eps, stat, mean, rstd);
    KERNEL_CHECK();
    trace_kernel(tag);
    launch_chan_map(GnFwdBody{x, gamma, beta, y, stat, (unsigned)rows, groups, cg, hw, m, al16(x) && al16(y)}, 1, (int)rows, m);
}

void bcnn_hip_group_norm_backward(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy,
                                  float* dx, float* dgamma, float* dbeta, int n, int c, int hw, int groups, int overwrite) {
    const long long total = gn_total("bcnn_hip_group_norm_backward", n, c, hw, groups);
    if (!total || (!dx && !dgamma && !dbeta)) return;
    const int cg = c / groups, m = cg * hw;
    const long long rows = (long long)n * groups, planes = (long long)n * c;
    const bool params = dgamma || dbeta;
    const int path = gn_path(m, 1);
    const char* tag = kGnBwdTag[path];
    float* psum = nullptr;
    if (path == 0) {
        if (params) psum = scratch(SCRATCH_REDUCE, (size_t)planes * 2);
        const int lanes = gn_row_lanes(m);
        trace_kernel(tag);
        gn_bwd_lanes_kernel<<<(unsigned)ceil_div(rows * lanes, 256), 256, 0, current_stream()>>>(
            x, gamma, mean, rstd, dy, dx, psum, rows, groups, cg, hw, m, lanes, gn_unit_lanes(hw, false, lanes), overwrite);
        KERNEL_CHECK();
    } else if (path == 1) {
        if (params) psum = scratch(SCRATCH_REDUCE, (size_t)planes * 2);
        const int vec = (m & 3) == 0 && al16(x) && al16(dy) && al16(dx);
        const int threads = m <= 4096 ? 256 : 1024;
        const size_t lds = (size_t)((m + 3) & ~3) * 2 * sizeof(float) + 16 * 4 * sizeof(double);
        trace_kernel(tag);
        gn_bwd_resident_kernel<<<(unsigned)rows, threads, lds, current_stream()>>>(
            x, gamma, mean, rstd, dy, dx, psum, rows, groups, cg, hw, m, gn_unit_lanes(hw, (hw & 3) == 0, kWave), vec, overwrite);
        KERNEL_CHECK();
    } else {
        const bool big = hw >= kGnUnitMaxHW;
        const int splits = big ? chan_splits((int)planes, hw) : 1;
        float* part = scratch(SCRATCH_REDUCE, (size_t)planes * splits * 4 + (size_t)rows * 2 + (size_t)planes * 2);
        float* rowsum = part + (size_t)planes * splits * 4;
        if (params) psum = rowsum + (size_t)rows * 2;
        trace_kernel(tag);
        if (big) {
            launch_chan_reduce<4>(GnBwdPlaneF{x, gamma, mean, rstd, dy, c, cg, al16(x) && al16(dy)}, (int)planes, hw, hw, splits,
                                  part);
        } else {
            const int vec = (hw & 3) == 0 && al16(x) && al16(dy);
            const int lp = gn_unit_lanes(hw, vec != 0, kWave);
            gn_bwd_planes_kernel<<<(unsigned)ceil_div(planes * lp, 256), 256, 0, current_stream()>>>(x, gamma, mean, rstd, dy, part,
                                                                                                      planes, c, cg, hw, lp, vec);
            KERNEL_CHECK();
        }
        trace_kernel(tag);
        gn_bwd_finalize_kernel<<<(unsigned)ceil_div(rows, 4), 256, 0, current_stream()>>>(part, rows, cg, splits, rowsum, psum);
        KERNEL_CHECK();
        if (dx) {
            trace_kernel(tag);
            launch_chan_map(GnBwdBody{x, gamma, mean, rstd, dy, dx, rowsum, (unsigned)rows, groups, cg, hw, m, overwrite,
                                      al16(x) && al16(dy) && al16(dx)},
                            1, (int)rows, m);
        }
    }
    if (params) {
        trace_kernel("group_norm_bwd:params");
        gn_param_reduce_kernel<<<ceil_div(c, 256), 256, 0, current_stream()>>>(psum, n, c, planes, dgamma, dbeta);
        KERNEL_CHECK();
    }
}

}  // extern "C"
