// conv_dilated.hip -- the dilated (atrous) convolution node on the fp32 matrix cores: forward, weight gradient and data
// gradient as implicit GEMMs with no im2col / col2im workspace, no zero-expanded weights and no atomics. A node of its
// own, like the transposed convolution (deconv.hip), whose kernel body this one follows; no reference counterpart.
//
// Weights W[f][c][ky][kx] with c in [0, C/g), g groups; x [n][C][h][w]; y [n][F][oh][ow] with
// oh = (h + 2 p - d (k - 1) - 1) / s + 1. Per group (blockIdx.z):
//   y[n][f][oy][ox] = act(b[f] + sum_{c, ky, kx} W[f][c][ky][kx] x[n][c][s oy - p + d ky][s ox - p + d kx])
//     M = F/g, N = n oh ow, K = taps x C/g;
//   dW[f][c][ky][kx] += sum_{n, oy, ox} dy[n][f][oy][ox] x[n][c][s oy - p + d ky][s ox - p + d kx]
//     per tap: M = F/g, N = C/g, K = n oh ow, split along K into chunks whose partial products go to a workspace
//     [split][tap][F][C/g] and are added in chunk order by a second kernel (deterministic, no atomics);
//   dx[n][c][iy][ix] = sum_{f, ky, kx} W[f][c][ky][kx] dy[n][f][(iy + p - d ky) / s][(ix + p - d kx) / s]   (overwrites dx)
//     M = C/g, N = n h w, K = taps x F/g; a tap contributes where both divisions are exact and in range (every tap is
//     tested: at stride 1, the case that matters, every tap divides).
// Out-of-range reads are zero.
//
// One kernel body: 256 threads, 2 x 2 waves, a BM x BN tile of 32 x 32 v_mfma_f32_32x32x2_f32 accumulators per wave,
// BK = 16, operands gathered from HBM into registers one K step ahead and staged through a double-buffered LDS tile. K
// is ordered tap-major (tap outer, channel inner): the dilated offset d ky, d kx only moves a per-thread base address
// that is fixed for the tap, and the bounds test is one per tap, not one per element.
#include "conv_common.h"

namespace bcnn_hip {

namespace {

constexpr int kDlBK = 16;
enum { DL_FWD = 0, DL_DX = 1, DL_DW = 2 };

struct DlArgs {
    const float* x;     // FWD, DW: the node input
    const float* wt;    // FWD, DX: weights [f][c/g][k][k]
    const float* bias;  // FWD
    const float* dy;    // DX, DW: the output gradient (already multiplied by act'(y))
    float* out;         // FWD: y, DX: dx, DW: the split workspace [split][tap][f][c/g]
    int n, c, h, w, f, k, s, p, d, g, cg, mg, oh, ow, act;
    int kchunk, splits;  // DW: K (= n oh ow) pixels per split (a multiple of kDlBK), number of splits
};

template <int MODE, int BM, int BN>
__global__ __launch_bounds__(256) void dilated_kernel(const DlArgs a) {
    constexpr int BK = kDlBK;
    constexpr int TM = BM / 64, TN = BN / 64;  // 32 x 32 accumulators per wave along M and N
    constexpr int RA = BM * BK / 256, RB = BN * BK / 256;  // staged elements per thread
    // rows padded by one float: a k-contiguous staging thread group (16 lanes, one row or column, k = 0 .. 15) then
    // writes 16 different banks instead of one; the MFMA operand reads (32 consecutive floats of a row) stay conflict-free
    __shared__ float As[2][BK][BM + 1];
    __shared__ float Bs[2][BK][BN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int kk2 = a.k * a.k;
    const int hw = a.h * a.w, ohw = a.oh * a.ow;

    // ---- the GEMM this block computes -------------------------------------------------------------------------------
    int M, NP, nsteps, csteps = 1, grp, tap = 0, split = 0;
    if (MODE == DL_FWD) {
        grp = blockIdx.z;
        M = a.mg;
        NP = a.n * ohw;
        csteps = (a.cg + BK - 1) / BK;
        nsteps = kk2 * csteps;
    } else if (MODE == DL_DX) {
        grp = blockIdx.z;
        M = a.cg;
        NP = a.n * hw;
        csteps = (a.mg + BK - 1) / BK;
        nsteps = kk2 * csteps;
    } else {
        split = blockIdx.z % a.splits;
        const int gt = blockIdx.z / a.splits;
        tap = gt % kk2;
        grp = gt / kk2;
        M = a.mg;
        NP = a.cg;
        const int ktot = a.n * ohw, kbeg = split * a.kchunk;
        const int kend = min(ktot, kbeg + a.kchunk);
        nsteps = (kend - kbeg + BK - 1) / BK;
    }
    const int m0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
    const int f0 = grp * a.mg, c0g = grp * a.cg;  // first filter / input channel of the group

    // ---- per-thread staging coordinates -------------------------------------------------------------------------------
    // Consecutive lanes take what is closest in memory. Row / column fast: thread -> (row tid % BM, k row tid / BM +
    // (256 / BM) r); k fast: thread -> (k row tid % BK, row / column tid / BK + 16 r).
    //   FWD: A = W[f][c][tap], rows f are C/g k k floats apart and channels k k floats: k fast; B = pixels: column fast
    //   DX:  A = W[f][c][tap] with rows c (k k floats apart) and k = f: row fast; B = pixels: column fast
    //   DW:  both operands are pixels along k: k fast
    constexpr bool A_KFAST = MODE != DL_DX, B_KFAST = MODE == DL_DW;
    const int a_row = A_KFAST ? tid / BK : tid % BM, a_k = A_KFAST ? tid % BK : tid / BM;
    const int b_col = B_KFAST ? tid / BK : tid % BN, b_k = B_KFAST ? tid % BK : tid / BN;
    constexpr int A_RSTEP = A_KFAST ? 256 / BK : 0, A_KSTEP = A_KFAST ? 0 : 256 / BM;
    constexpr int B_CSTEP = B_KFAST ? 256 / BK : 0, B_KSTEP = B_KFAST ? 0 : 256 / BN;

    // FWD / DX: this thread's B column is one output (FWD) / input (DX) pixel for the whole K loop
    int pn = 0, pq_y = 0, pq_x = 0;
    bool pvalid = false;
    if (MODE != DL_DW) {
        const int P = j0 + b_col;
        pvalid = P < NP;
        const int ny = MODE == DL_FWD ? a.oh : a.h, nx = MODE == DL_FWD ? a.ow : a.w;
        const int Pc = pvalid ? P : 0;
        pn = Pc / (ny * nx);
        const int r = Pc - pn * ny * nx;
        pq_y = r / nx;
        pq_x = r - pq_y * nx;
    }

    float ra[RA], rb[RB];
    auto load = [&](int st) {
        if (MODE == DL_FWD) {
            const int t = st / csteps, c0 = (st - t * csteps) * BK;
            const int ky = t / a.k, kx = t - ky * a.k;
            const int iy = a.s * pq_y - a.p + a.d * ky, ix = a.s * pq_x - a.p + a.d * kx;
            const bool tv = pvalid && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
            const float* xb = a.x + ((size_t)(pn * a.c + c0g) * a.h + (tv ? iy : 0)) * a.w + (tv ? ix : 0);
            const int ci = c0 + a_k;
            const float* wb = a.wt + ((size_t)(f0 + m0 + a_row) * a.cg + ci) * kk2 + t;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int fr = m0 + a_row + A_RSTEP * r;
                ra[r] = (fr < a.mg && ci < a.cg) ? wb[(size_t)(A_RSTEP * r) * a.cg * kk2] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int ci = c0 + b_k + B_KSTEP * r;
                rb[r] = (tv && ci < a.cg) ? xb[(size_t)ci * hw] : 0.f;
            }
        } else if (MODE == DL_DX) {
            const int t = st / csteps, c0 = (st - t * csteps) * BK;
            const int ky = t / a.k, kx = t - ky * a.k;
            const int ny = pq_y + a.p - a.d * ky, nx = pq_x + a.p - a.d * kx;  // s oy, s ox
            const int oy = ny / a.s, ox = nx / a.s;
            const bool tv = pvalid && ny >= 0 && nx >= 0 && oy * a.s == ny && ox * a.s == nx && oy < a.oh && ox < a.ow;
            const float* db = a.dy + ((size_t)(pn * a.f + f0) * a.oh + (tv ? oy : 0)) * a.ow + (tv ? ox : 0);
            const int cr = m0 + a_row;
            const float* wb = a.wt + ((size_t)f0 * a.cg + cr) * kk2 + t;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int fi = c0 + a_k + A_KSTEP * r;
                ra[r] = (cr < a.cg && fi < a.mg) ? wb[(size_t)fi * a.cg * kk2] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int fi = c0 + b_k + B_KSTEP * r;
                rb[r] = (tv && fi < a.mg) ? db[(size_t)fi * ohw] : 0.f;
            }
        } else {
            const int ktot = a.n * ohw;
            const int kend = min(ktot, (split + 1) * a.kchunk);
            const int kk = split * a.kchunk + st * BK + a_k;
            const bool kv = kk < kend;
            const int kc = kv ? kk : 0;
            const int n = kc / ohw, pix = kc - n * ohw;
            const int oy = pix / a.ow, ox = pix - oy * a.ow;
            const int ky = tap / a.k, kx = tap - ky * a.k;
            const int iy = a.s * oy - a.p + a.d * ky, ix = a.s * ox - a.p + a.d * kx;
            const bool xv = kv && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
            const float* db = a.dy + (size_t)(n * a.f + f0) * ohw + pix;
            const float* xb = a.x + ((size_t)(n * a.c + c0g) * a.h + (xv ? iy : 0)) * a.w + (xv ? ix : 0);
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int fr = m0 + a_row + A_RSTEP * r;
                ra[r] = (kv && fr < a.mg) ? db[(size_t)fr * ohw] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int ci = j0 + b_col + B_CSTEP * r;
                rb[r] = (xv && ci < a.cg) ? xb[(size_t)ci * hw] : 0.f;
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
        size_t obase, rstride;
        if (MODE == DL_FWD) {
            const int n = col / ohw, pix = col - n * ohw;
            obase = (size_t)(n * a.f + f0) * ohw + pix;
            rstride = (size_t)ohw;
        } else if (MODE == DL_DX) {
            const int n = col / hw, pix = col - n * hw;
            obase = (size_t)(n * a.c + c0g) * hw + pix;
            rstride = (size_t)hw;
        } else {
            obase = ((size_t)(split * kk2 + tap) * a.f + f0) * a.cg + col;
            rstride = (size_t)a.cg;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = m0 + wm * (BM / 2) + 32 * i + mfma_row(q, lane);
                if (row >= M) continue;
                float v = acc[i][j][q];
                if (MODE == DL_FWD) v = act_fwd(v + a.bias[f0 + row], a.act, 0.f);
                a.out[obase + (size_t)row * rstride] = v;
            }
    }
}

template <int MODE>
void launch(const DlArgs& a, int M, int NP, int gz) {
    const dim3 blk(256);
    const bool bm = M > 64, bn = NP > 64;
    const dim3 grid(ceil_div(NP, bn ? 128 : 64), ceil_div(M, bm ? 128 : 64), gz);
    if (bm && bn) dilated_kernel<MODE, 128, 128><<<grid, blk, 0, current_stream()>>>(a);
    else if (bm) dilated_kernel<MODE, 128, 64><<<grid, blk, 0, current_stream()>>>(a);
    else if (bn) dilated_kernel<MODE, 64, 128><<<grid, blk, 0, current_stream()>>>(a);
    else dilated_kernel<MODE, 64, 64><<<grid, blk, 0, current_stream()>>>(a);
    KERNEL_CHECK();
}

// K-split of the weight gradient: enough blocks for two per CU, chunks of at least 4 K steps, at most `max_splits`
// (0: unlimited). A function of the shape and the workspace size only, so two runs split alike.
SplitK dw_split(const DlArgs& a, size_t max_splits) {
    const long long blocks = (long long)a.k * a.k * a.g * ceil_div(a.mg, a.mg > 64 ? 128 : 64) *
                             ceil_div(a.cg, a.cg > 64 ? 128 : 64);
    return split_k(a.n * a.oh * a.ow, blocks, 2, kDlBK, 4, max_splits);
}

DlArgs make_args(const char* what, int n, int c, int h, int w, int f, int k, int stride, int pad, int dilation,
                 int groups) {
    const bool pos = n > 0 && c > 0 && h > 0 && w > 0 && f > 0 && k > 0 && stride > 0 && pad >= 0 && dilation > 0 &&
                     groups > 0;
    const long long eh = (long long)h + 2LL * pad - (long long)dilation * (k - 1) - 1;
    const long long ew = (long long)w + 2LL * pad - (long long)dilation * (k - 1) - 1;
    const long long oh = pos && eh >= 0 ? eh / stride + 1 : 0, ow = pos && ew >= 0 ? ew / stride + 1 : 0;
    const bool ok = pos && oh > 0 && ow > 0 && c % groups == 0 && f % groups == 0 &&
                    (long long)n * c * h * w < (1LL << 31) && (long long)n * f * oh * ow < (1LL << 31) &&
                    (long long)f * (c / groups) * k * k < (1LL << 31) &&
                    (long long)groups * k * k < 32768 &&  // blockIdx.z of the weight gradient: groups x taps x splits
                    (long long)dilation * (k - 1) + 2LL * pad + h + w < (1LL << 30);
    if (!ok) {
        fprintf(stderr,
                "[bcnn_hip] %s: unsupported shape n %d c %d h %d w %d f %d k %d stride %d pad %d dilation %d groups %d\n",
                what, n, c, h, w, f, k, stride, pad, dilation, groups);
        exit(1);
    }
    DlArgs a{};
    a.n = n; a.c = c; a.h = h; a.w = w; a.f = f; a.k = k; a.s = stride; a.p = pad; a.d = dilation; a.g = groups;
    a.cg = c / groups; a.mg = f / groups;
    a.oh = (int)oh; a.ow = (int)ow;
    return a;
}

void refuse_prelu(const char* what, int act) {
    if (act != BCNN_HIP_ACT_PRELU) return;
    fprintf(stderr, "[bcnn_hip] %s: PReLU is not supported\n", what);
    exit(1);
}

}  // namespace

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

size_t bcnn_hip_dilated_conv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad, int dilation,
                                            int groups) {
    const DlArgs a = make_args("bcnn_hip_dilated_conv_workspace_size", n, c, h, w, f, k, stride, pad, dilation, groups);
    return (size_t)dw_split(a, 0).splits * k * k * a.cg * f;
}

void bcnn_hip_dilated_conv_forward(const float* x_d, const float* w_d, const float* bias_d, float* y_d, int n, int c,
                                   int h, int w, int f, int k, int stride, int pad, int dilation, int groups, int act) {
    DlArgs a = make_args("bcnn_hip_dilated_conv_forward", n, c, h, w, f, k, stride, pad, dilation, groups);
    refuse_prelu("bcnn_hip_dilated_conv_forward", act);
    a.x = x_d; a.wt = w_d; a.bias = bias_d; a.out = y_d; a.act = act;
    trace_kernel("dilated_fwd_kernel");
    launch<DL_FWD>(a, a.mg, n * a.oh * a.ow, groups);
}

void bcnn_hip_dilated_conv_backward(const float* x_d, const float* w_d, const float* y_d, float* dy_d, float* dx_d,
                                    float* dw_d, float* dbias_d, int n, int c, int h, int w, int f, int k, int stride,
                                    int pad, int dilation, int groups, int act, float* workspace_d,
                                    size_t workspace_elems) {
    DlArgs a = make_args("bcnn_hip_dilated_conv_backward", n, c, h, w, f, k, stride, pad, dilation, groups);
    refuse_prelu("bcnn_hip_dilated_conv_backward", act);
    const size_t ysz = (size_t)n * f * a.oh * a.ow;
    // dy <- dy * act'(y) in place, then db += sum dy
    bcnn_hip_activation_backward(y_d, dy_d, ysz, act, nullptr, nullptr, a.oh * a.ow, f);
    if (dbias_d) bcnn_hip_grad_bias(dbias_d, dy_d, n, f, a.oh * a.ow);
    a.x = x_d; a.wt = w_d; a.dy = dy_d; a.act = act;
    if (dw_d) {
        const size_t per_split = (size_t)k * k * a.cg * f;
        const size_t max_splits = workspace_elems / per_split;
        if (max_splits < 1 || workspace_d == nullptr) {
            fprintf(stderr, "[bcnn_hip] bcnn_hip_dilated_conv_backward: workspace of %zu floats, needs at least %zu\n",
                    workspace_elems, per_split);
            exit(1);
        }
        const SplitK sk = dw_split(a, max_splits);
        a.kchunk = sk.chunk; a.splits = sk.splits;
        a.out = workspace_d;
        trace_kernel("dilated_dw_kernel");
        launch<DL_DW>(a, a.mg, a.cg, groups * k * k * a.splits);
        conv_dw_taps_reduce(workspace_d, dw_d, a.splits, k * k, f * a.cg, 1.0f);
    }
    if (dx_d) {
        a.out = dx_d;
        trace_kernel("dilated_dx_kernel");
        launch<DL_DX>(a, a.cg, n * h * w, groups);
    }
}

}  // extern "C"
