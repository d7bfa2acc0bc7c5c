// deconv.hip -- the transposed-convolution (deconvolution) node on the fp32 matrix cores: forward, weight gradient and
// data gradient as implicit GEMMs with no col2im / im2col workspace and no atomics.
//
// Reference bcnn_deconv_layer.c:150-246: weights W[ci][co][ky][kx] (c_in = ci, c_out = co = f), input x [n][ci][h][w],
// output y [n][co][ho][wo] with ho = s (h - 1) + k - 2 p. The reference forward is a per-image GEMM Wᵀ x into a
// workspace followed by col2im (scatter-add); here each output pixel GATHERS what lands on it:
//   y[n][co][oy][ox] = b[co] + sum_{ci, ky, kx} W[ci][co][ky][kx] x[n][ci][iy][ix],  s iy + ky = oy + p, s ix + kx = ox + p.
// For one output phase (py, px) = ((oy + p) mod s, (ox + p) mod s) only the taps ky = py + s ty, kx = px + s tx
// contribute, with iy = (oy + p - py) / s - ty: a dense convolution of x with those taps, i.e. one implicit GEMM with
// M = co, N = the pixels of the phase, K = ci x taps. A phase with no taps (s > k) is bias + activation only.
//   dW[ci][co][ky][kx] += (1/n) sum_{n, iy, ix} x[n][ci][iy][ix] dy[n][co][s iy + ky - p][s ix + kx - p]
//     per tap: M = ci, N = co, K = n h w, split along K into a fixed number of chunks whose partial products go to a
//     workspace and are added in chunk order by a second kernel (deterministic, no atomics);
//   dx[n][ci][iy][ix] = sum_{co, ky, kx} W[ci][co][ky][kx] dy[n][co][s iy + ky - p][s ix + kx - p]   (overwrites dx)
//     M = ci, N = n h w, K = taps x co: the strided valid convolution of dy with W read as [ci][co][k][k].
// Out-of-range dy positions read as zero: with pad > 0 this is the crop of the full s (h - 1) + k result.
//
// All three share one kernel body: 256 threads, 2 x 2 waves, a BM x BN tile of 32 x 32 v_mfma_f32_32x32x2_f32
// accumulators per wave, BK = 16, operands gathered from HBM into registers one K step ahead and staged through a
// double-buffered LDS tile. K is ordered tap-major (tap outer, channel inner), so the address of every gathered element
// is a per-thread base fixed for the tap plus channel x plane: one bounds check per tap, not per element.
#include "conv_common.h"

namespace bcnn_hip {

namespace {

constexpr int kDcBK = 16;
enum { DC_FWD = 0, DC_DX = 1, DC_DW = 2 };

struct DcArgs {
    const float* x;     // FWD, DW: the node input
    const float* wt;    // FWD, DX: weights [ci][co][k][k]
    const float* bias;  // FWD
    const float* dy;    // DX, DW: the output gradient (already multiplied by act'(y))
    float* out;         // FWD: y, DX: dx, DW: the split workspace [split][tap][ci][co]
    int n, ci, h, w, co, k, s, p, ho, wo, act;
    int kchunk, splits;  // DW: K (= n h w) pixels per split (a multiple of kDcBK), number of splits
};

// One output phase of the forward pass: the rows q of the phase are oy = s q + py - p for q in [q0, q0 + nq), and its
// taps ky = py + s t for t in [0, nt).
struct DcPhase {
    int q0, nq, nt;
};
__device__ __forceinline__ DcPhase dc_phase(int ph, int out_extent, int k, int s, int p) {
    DcPhase r;
    r.q0 = (p - ph + s - 1) / s;  // p - ph + s - 1 >= 0: ph < s
    const int last = out_extent - 1 + p - ph;  // > -s
    const int q1 = last >= 0 ? last / s : -1;
    r.nq = q1 - r.q0 + 1 > 0 ? q1 - r.q0 + 1 : 0;
    r.nt = ph < k ? (k - 1 - ph) / s + 1 : 0;
    return r;
}

template <int MODE, int BM, int BN>
__global__ __launch_bounds__(256) void deconv_kernel(const DcArgs a) {
    constexpr int BK = kDcBK;
    constexpr int TM = BM / 64, TN = BN / 64;  // 32 x 32 accumulators per wave along M and N
    constexpr int RA = BM * BK / 256, RB = BN * BK / 256;  // staged elements per thread
    __shared__ float As[2][BK][BM];
    __shared__ float Bs[2][BK][BN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int kk2 = a.k * a.k;

    // ---- the GEMM this block computes -------------------------------------------------------------------------------
    int m0, j0, M, NP, nsteps, csteps = 1;
    int py = 0, px = 0, tx_n = 1, tap = 0, split = 0;
    DcPhase phy{0, 0, 0}, phx{0, 0, 0};
    if (MODE == DC_FWD) {
        py = blockIdx.z / a.s;
        px = blockIdx.z % a.s;
        phy = dc_phase(py, a.ho, a.k, a.s, a.p);
        phx = dc_phase(px, a.wo, a.k, a.s, a.p);
        M = a.co;
        NP = a.n * phy.nq * phx.nq;
        csteps = (a.ci + BK - 1) / BK;
        tx_n = phx.nt;
        nsteps = phy.nt * phx.nt * csteps;
        m0 = blockIdx.y * BM;
        j0 = blockIdx.x * BN;
    } else if (MODE == DC_DX) {
        M = a.ci;
        NP = a.n * a.h * a.w;
        csteps = (a.co + BK - 1) / BK;
        nsteps = kk2 * csteps;
        m0 = blockIdx.y * BM;
        j0 = blockIdx.x * BN;
    } else {
        M = a.ci;
        NP = a.co;
        tap = blockIdx.z / a.splits;
        split = blockIdx.z % a.splits;
        const int ktot = a.n * a.h * a.w, kbeg = split * a.kchunk;
        const int kend = min(ktot, kbeg + a.kchunk);
        nsteps = (kend - kbeg + BK - 1) / BK;
        m0 = blockIdx.y * BM;
        j0 = blockIdx.x * BN;
    }
    if (j0 >= NP || m0 >= M) return;  // uniform: a phase smaller than the grid's largest

    // ---- per-thread staging coordinates -------------------------------------------------------------------------------
    // FWD / DX: A thread -> (row tid % BM, k row tid / BM + (256 / BM) r), B thread -> (column tid % BN, k row tid / BN + ..)
    // DW:       both operands k-contiguous: thread -> (k row tid % BK, row / column tid / BK + 16 r)
    const int a_row = MODE == DC_DW ? tid / BK : tid % BM, a_k = MODE == DC_DW ? tid % BK : tid / BM;
    const int b_col = MODE == DC_DW ? tid / BK : tid % BN, b_k = MODE == DC_DW ? tid % BK : tid / BN;
    constexpr int A_RSTEP = MODE == DC_DW ? 256 / BK : 0, A_KSTEP = MODE == DC_DW ? 0 : 256 / BM;
    constexpr int B_CSTEP = MODE == DC_DW ? 256 / BK : 0, B_KSTEP = MODE == DC_DW ? 0 : 256 / BN;

    // FWD / DX: this thread's B column is one output (FWD) / input (DX) pixel for the whole K loop
    int pn = 0, pq_y = 0, pq_x = 0;
    bool pvalid = false;
    if (MODE != DC_DW) {
        const int P = j0 + b_col;
        pvalid = P < NP;
        const int ny = MODE == DC_FWD ? phy.nq : a.h, nx = MODE == DC_FWD ? phx.nq : a.w;
        const int Pc = pvalid ? P : 0;
        pn = Pc / (ny * nx);
        const int r = Pc - pn * ny * nx;
        pq_y = r / nx;
        pq_x = r - pq_y * nx;
    }
    const size_t hw = (size_t)a.h * a.w, ohw = (size_t)a.ho * a.wo;

    float ra[RA], rb[RB];
    auto load = [&](int st) {
        if (MODE == DC_FWD) {
            const int t = st / csteps, c0 = (st - t * csteps) * BK;
            const int ty = t / tx_n, tx = t - ty * tx_n;
            const int ky = py + a.s * ty, kx = px + a.s * tx;
            const int iy = phy.q0 + pq_y - ty, ix = phx.q0 + pq_x - tx;
            const bool tv = pvalid && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
            const float* xb = a.x + ((size_t)pn * a.ci * a.h + (tv ? iy : 0)) * a.w + (tv ? ix : 0);
            const int co = m0 + a_row;
            const float* wb = a.wt + (size_t)co * kk2 + ky * a.k + kx;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int ci = c0 + a_k + A_KSTEP * r;
                ra[r] = (co < a.co && ci < a.ci) ? wb[(size_t)ci * a.co * kk2] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int ci = c0 + b_k + B_KSTEP * r;
                rb[r] = (tv && ci < a.ci) ? xb[(size_t)ci * hw] : 0.f;
            }
        } else if (MODE == DC_DX) {
            const int t = st / csteps, c0 = (st - t * csteps) * BK;
            const int ky = t / a.k, kx = t - ky * a.k;
            const int oy = a.s * pq_y + ky - a.p, ox = a.s * pq_x + kx - a.p;
            const bool tv = pvalid && oy >= 0 && oy < a.ho && ox >= 0 && ox < a.wo;
            const float* db = a.dy + ((size_t)pn * a.co * a.ho + (tv ? oy : 0)) * a.wo + (tv ? ox : 0);
            const int ci = m0 + a_row;
            const float* wb = a.wt + (size_t)ci * a.co * kk2 + t;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int co = c0 + a_k + A_KSTEP * r;
                ra[r] = (ci < a.ci && co < a.co) ? wb[(size_t)co * kk2] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int co = c0 + b_k + B_KSTEP * r;
                rb[r] = (tv && co < a.co) ? db[(size_t)co * ohw] : 0.f;
            }
        } else {
            const int ktot = a.n * a.h * a.w;
            const int kend = min(ktot, (split + 1) * a.kchunk);
            const int kk = split * a.kchunk + st * BK + a_k;
            const bool kv = kk < kend;
            const int kc = kv ? kk : 0;
            const int n = kc / (int)hw, pix = kc - n * (int)hw;
            const int iy = pix / a.w, ix = pix - iy * a.w;
            const int ky = tap / a.k, kx = tap - ky * a.k;
            const int oy = a.s * iy + ky - a.p, ox = a.s * ix + kx - a.p;
            const bool dv = kv && oy >= 0 && oy < a.ho && ox >= 0 && ox < a.wo;
            const float* xb = a.x + (size_t)n * a.ci * hw + pix;
            const float* db = a.dy + ((size_t)n * a.co * a.ho + (dv ? oy : 0)) * a.wo + (dv ? ox : 0);
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int ci = m0 + a_row + A_RSTEP * r;
                ra[r] = (kv && ci < a.ci) ? xb[(size_t)ci * hw] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int co = j0 + b_col + B_CSTEP * r;
                rb[r] = (dv && co < a.co) ? db[(size_t)co * ohw] : 0.f;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < RA; ++r) As[buf][a_k + A_KSTEP * r][a_row + A_RSTEP * r] = ra[r];
#pragma unroll
        for (int r = 0; r < RB; ++r) Bs[buf][b_k + B_KSTEP * r][b_col + B_CSTEP * r] = rb[r];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int l31 = lane & 31, lhi = lane >> 5;
    if (nsteps > 0) {
        load(0);
        store(0);
        __syncthreads();
    }
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if (st + 1 < nsteps) load(st + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[cur][2 * ks + lhi][wm * (BM / 2) + 32 * i + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[cur][2 * ks + lhi][wn * (BN / 2) + 32 * j + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
        }
        if (st + 1 < nsteps) store(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue -----------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = j0 + wn * (BN / 2) + 32 * j + l31;
        if (col >= NP) continue;
        size_t obase = 0;
        if (MODE == DC_FWD) {
            const int ny = phy.nq, nx = phx.nq;
            const int n = col / (ny * nx), r = col - n * ny * nx;
            const int qy = r / nx, qx = r - qy * nx;
            const int oy = a.s * (phy.q0 + qy) + py - a.p, ox = a.s * (phx.q0 + qx) + px - a.p;
            obase = ((size_t)n * a.co * a.ho + oy) * a.wo + ox;
        } else if (MODE == DC_DX) {
            const int n = col / (int)hw, pix = col - n * (int)hw;
            obase = (size_t)n * a.ci * hw + pix;
        } else {
            obase = ((size_t)(split * kk2 + tap) * a.ci) * a.co + col;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = m0 + wm * (BM / 2) + 32 * i + mfma_row(q, lane);
                if (row >= M) continue;
                float v = acc[i][j][q];
                if (MODE == DC_FWD) {
                    // bias as bcnn_add_bias adds it (bcnn_add_scalar skips 0.0f and 1.0f exactly, bcnn_mat.c:381-383)
                    const float b = a.bias[row];
                    if (b != 0.0f && b != 1.0f) v += b;
                    a.out[obase + (size_t)row * ohw] = act_fwd(v, a.act, 0.f);
                } else if (MODE == DC_DX) {
                    a.out[obase + (size_t)row * hw] = v;
                } else {
                    a.out[obase + (size_t)row * a.co] = v;
                }
            }
    }
}

template <int MODE>
void launch(const DcArgs& a, int M, int NP, int gz) {
    const dim3 blk(256);
    const bool bm = M > 64, bn = NP > 64;
    const dim3 grid(ceil_div(NP, bn ? 128 : 64), ceil_div(M, bm ? 128 : 64), gz);
    if (bm && bn) deconv_kernel<MODE, 128, 128><<<grid, blk, 0, current_stream()>>>(a);
    else if (bm) deconv_kernel<MODE, 128, 64><<<grid, blk, 0, current_stream()>>>(a);
    else if (bn) deconv_kernel<MODE, 64, 128><<<grid, blk, 0, current_stream()>>>(a);
    else deconv_kernel<MODE, 64, 64><<<grid, blk, 0, current_stream()>>>(a);
    KERNEL_CHECK();
}

// K-split of the weight gradient: enough blocks for two per CU, chunks of at least 4 K steps, at most `max_splits`
// (0: unlimited). A function of the shape only, so two runs split alike.
SplitK dw_split(int n, int c, int h, int w, int f, int k, size_t max_splits) {
    const long long blocks = (long long)k * k * ceil_div(c, c > 64 ? 128 : 64) * ceil_div(f, f > 64 ? 128 : 64);
    return split_k(n * h * w, blocks, 2, kDcBK, 4, max_splits);
}

void check_shape(const char* what, int n, int c, int h, int w, int f, int k, int stride, int pad) {
    const long long ho = (long long)stride * (h - 1) + k - 2LL * pad, wo = (long long)stride * (w - 1) + k - 2LL * pad;
    const bool ok = n > 0 && c > 0 && h > 0 && w > 0 && f > 0 && k > 0 && stride > 0 && pad >= 0 && ho > 0 && wo > 0 &&
                    (long long)n * c * h * w < (1LL << 31) && (long long)n * f * ho * wo < (1LL << 31);
    if (!ok) {
        fprintf(stderr, "[bcnn_hip] %s: unsupported shape n %d c %d h %d w %d f %d k %d stride %d pad %d\n", what, n, c,
                h, w, f, k, stride, pad);
        exit(1);
    }
}

DcArgs make_args(int n, int c, int h, int w, int f, int k, int stride, int pad) {
    DcArgs a{};
    a.n = n; a.ci = c; a.h = h; a.w = w; a.co = f; a.k = k; a.s = stride; a.p = pad;
    a.ho = stride * (h - 1) + k - 2 * pad;
    a.wo = stride * (w - 1) + k - 2 * pad;
    return a;
}

}  // namespace

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

size_t bcnn_hip_deconv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad) {
    (void)stride; (void)pad;
    return (size_t)dw_split(n, c, h, w, f, k, 0).splits * k * k * c * f;
}

void bcnn_hip_deconv_forward(const float* x_d, const float* w_d, const float* bias_d, float* y_d, int n, int c, int h,
                             int w, int f, int k, int stride, int pad, int act) {
    check_shape("bcnn_hip_deconv_forward", n, c, h, w, f, k, stride, pad);
    if (act == BCNN_HIP_ACT_PRELU) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_deconv_forward: PReLU is not supported\n");
        exit(1);
    }
    DcArgs a = make_args(n, c, h, w, f, k, stride, pad);
    a.x = x_d; a.wt = w_d; a.bias = bias_d; a.out = y_d; a.act = act;
    // the grid covers the largest phase: ceil(extent / s) rows and columns
    const int NP = n * ceil_div(a.ho, stride) * ceil_div(a.wo, stride);
    trace_kernel("deconv_fwd_kernel");
    launch<DC_FWD>(a, f, NP, stride * stride);
}

void bcnn_hip_deconv_backward(const float* x_d, const float* w_d, const float* y_d, float* dy_d, float* dx_d,
                              float* dw_d, float* dbias_d, int n, int c, int h, int w, int f, int k, int stride, int pad,
                              int act, float* workspace_d, size_t workspace_elems) {
    check_shape("bcnn_hip_deconv_backward", n, c, h, w, f, k, stride, pad);
    DcArgs a = make_args(n, c, h, w, f, k, stride, pad);
    const size_t ysz = (size_t)n * f * a.ho * a.wo;
    // dy <- dy * act'(y) in place, then db += sum dy (reference :208-215)
    bcnn_hip_activation_backward(y_d, dy_d, ysz, act, nullptr, nullptr, a.ho * a.wo, f);
    if (dbias_d) bcnn_hip_grad_bias(dbias_d, dy_d, n, f, a.ho * a.wo);
    a.x = x_d; a.wt = w_d; a.dy = dy_d;
    if (dw_d) {
        const size_t per_split = (size_t)k * k * c * f;
        const size_t max_splits = workspace_elems / per_split;
        if (max_splits < 1 || workspace_d == nullptr) {
            fprintf(stderr, "[bcnn_hip] bcnn_hip_deconv_backward: workspace of %zu floats, needs at least %zu\n",
                    workspace_elems, per_split);
            exit(1);
        }
        const SplitK sk = dw_split(n, c, h, w, f, k, max_splits);
        a.kchunk = sk.chunk; a.splits = sk.splits;
        a.out = workspace_d;
        trace_kernel("deconv_dw_kernel");
        launch<DC_DW>(a, c, f, k * k * a.splits);
        conv_dw_taps_reduce(workspace_d, dw_d, a.splits, k * k, c * f, 1.0f / (float)n);
    }
    if (dx_d) {
        a.out = dx_d;
        trace_kernel("deconv_dx_kernel");
        launch<DC_DX>(a, c, n * h * w, 1);
    }
}

}  // extern "C"
