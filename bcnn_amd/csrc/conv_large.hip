// conv_large.hip -- convolutions with kernels larger than 7x7 (the 11x11 / s4 stem of the AlexNet family, the 9x9 layers of
// converted Caffe models): forward, data gradient and weight gradient as implicit GEMMs on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32), for any stride, padding, group count and channel counts. DESIGN.md section 14.
//
// The register-staged kernel of conv_igemm.hip keeps a column's tap validity in one 64-bit mask and a class's taps in a
// by-value nibble table; neither stretches past 49 taps. Here nothing is tabulated per tap:
//   forward : r = (c, kr, kc) is decoded with two multiply-high divisions; a gathered element is valid when
//             ih = oh*s - p + kr and iw = ow*s - p + kc lie inside the plane (two unsigned compares)
//   dX      : the taps of stride-parity class (ra, rb) are the product lattice kr = ra + i*s, kc = rb + j*s of extents
//             nkr x nkc, so a class is six integers derived from its index (large_class) and r = (f, i, j) decodes the
//             same way; dy is read at (qa - i, qb - j) with qa = (ih + p) / s. A class without taps (k < s) has an empty
//             reduction and stores zeros: dX overwrites (quirk 3)
//   dW      : rows f, columns r = (c, kr, kc), reduction over q = (n, oh, ow) split across workgroups and waves; the
//             partials go to the caller's workspace and are added to dw in a fixed order (deterministic, beta = 1)
// Every global load is unconditional from a clamped, always legal offset and validity is applied when the value goes to
// LDS, so the staging code is straight-line. Offsets are 32-bit against wave-uniform bases:
// the host chunks a launch over images so that they fit, and refuses a reduction the divisions are not exact for.
#include "conv_paths.h"

namespace bcnn_hip {

// n / d with magic = magic_of(d) (conv_common.h); exact while n * d < 2^32. The same function as conv_igemm.hip's.
__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }

bool conv_large_wanted(const ConvShape& s, int) { return s.ksz > 7 && !s.pointwise; }

// dX: stride-parity class (ra, rb) = the input pixels with (ih + pad) % s == ra, (iw + pad) % s == rb
struct LargeClass {
    int ih0, iw0;  // first input row / column of the class
    int Hc, Wc;    // rows / columns of the class per image
    int nkr, nkc;  // extents of its tap lattice kr = ra + i*s, kc = rb + j*s
};
__host__ __device__ __forceinline__ LargeClass large_class(const ConvShape& s, int ra, int rb) {
    const int st = s.stride;
    LargeClass c;
    c.ih0 = ((ra - s.pad) % st + st) % st;
    c.iw0 = ((rb - s.pad) % st + st) % st;
    c.Hc = c.ih0 < s.H ? (s.H - c.ih0 + st - 1) / st : 0;
    c.Wc = c.iw0 < s.W ? (s.W - c.iw0 + st - 1) / st : 0;
    c.nkr = ra < s.ksz ? (s.ksz - ra + st - 1) / st : 0;
    c.nkc = rb < s.ksz ? (s.ksz - rb + st - 1) / st : 0;
    return c;
}

// ================================================================================================
// forward and dX: D[m][col] = sum_r A[m][r] * B[r][col], B gathered from an NCHW tensor with zero fill
// ================================================================================================
struct LargeArgs {
    const float* a_base;  // weights
    const float* b_base;  // gathered tensor (x for forward, dy for dX), first image of this launch
    float* out;           // y or dx, first image of this launch
    const float* bias;    // forward epilogue (may be NULL)
    const float* slopes;  // PReLU (may be NULL)
    ConvShape s;          // N: the images of this launch
    int mode;             // 0 forward, 1 dX
    int act, add_bias;
    int M;                // rows per group: Mg (forward) or Cg (dX)
    int a_row_stride;     // A(m, r) = a_base[g * a_group_stride + m * a_row_stride + aoff(r)]
    long long a_group_stride;
    int mtiles;
    unsigned kk2_magic, ksz_magic;  // forward: magic_of(ksz * ksz), magic_of(ksz)
};

constexpr int kLargeNoCol = -(1 << 30);  // row coordinate of a column past the end: no tap offset brings it into a plane

template <int WM, int WN, int TM, int TN, int BK>
__global__ __launch_bounds__(256) void conv_large_gemm_kernel(const LargeArgs a) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int LDA = BM + 1;
    constexpr int B_ROWS = 256 / BN, B_IT = BK / B_ROWS, A_IT = BM * BK / 256;
    static_assert(WM * WN == 4 && BN <= 256 && 256 % BN == 0 && (BM * BK) % 256 == 0, "tile");
    __shared__ float As[2][BK][LDA];
    __shared__ float Bs[2][BK][BN];
    __shared__ int4 ktab[2][BK];  // {A offset, B offset, (du & 0xffff) | dv << 16, valid}

    const ConvShape& s = a.s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int g = blockIdx.y;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = lb % a.mtiles, pt = lb / a.mtiles;
    const int m0 = mt * BM;
    const bool fwd = (a.mode == 0);

    // ---- the block's column grid and reduction: the output plane (forward) or one stride-parity class (dX) ----
    int c_ih0 = 0, c_iw0 = 0, c_Hc = s.OH, c_Wc = s.OW, kr0 = 0, kc0 = 0;
    int ntaps = s.ksz * s.ksz, nkc = s.ksz, KR = s.K;
    unsigned ntaps_magic = a.kk2_magic, nkc_magic = a.ksz_magic;
    if (!fwd) {
        kr0 = (int)blockIdx.z / s.stride; kc0 = (int)blockIdx.z - kr0 * s.stride;
        const LargeClass ci = large_class(s, kr0, kc0);
        c_ih0 = ci.ih0; c_iw0 = ci.iw0; c_Hc = ci.Hc; c_Wc = ci.Wc;
        ntaps = ci.nkr * ci.nkc; nkc = ci.nkc;
        KR = s.Mg * ntaps;
        ntaps_magic = ntaps > 1 ? (unsigned)((0x100000000ULL + (unsigned)ntaps - 1) / (unsigned)ntaps) : 0u;
        nkc_magic = nkc > 1 ? (unsigned)((0x100000000ULL + (unsigned)nkc - 1) / (unsigned)nkc) : 0u;
    }
    const int col_per_img = c_Hc * c_Wc;
    const long long total_cols = (long long)s.N * col_per_img;
    const long long p0 = (long long)pt * BN;
    if (p0 >= total_cols) return;  // class smaller than the grid (uniform per block)
    const int nk = (KR + BK - 1) / BK;
    const int U = fwd ? s.H : s.OH, V = fwd ? s.W : s.OW;  // the gathered plane

    // ---- one column: offset of its window origin in the gathered tensor, the origin's coordinates, output offset ----
    auto decode = [&](long long col, int& bbase, int& u0, int& v0, unsigned& obase) -> bool {
        if (col >= total_cols) { bbase = 0; u0 = kLargeNoCol; v0 = 0; obase = 0; return false; }
        const unsigned n = (unsigned)(col / col_per_img);
        const unsigned pix = (unsigned)(col - (long long)n * col_per_img);
        const unsigned u = pix / (unsigned)c_Wc, v = pix - u * (unsigned)c_Wc;
        if (fwd) {
            u0 = (int)u * s.stride - s.pad; v0 = (int)v * s.stride - s.pad;
            bbase = (int)((n * (unsigned)s.C + (unsigned)(g * s.Cg)) * (unsigned)s.HW) + u0 * s.W + v0;
            obase = (n * (unsigned)s.F + (unsigned)(g * s.Mg)) * (unsigned)s.OHOW + pix;
        } else {
            const int ih = c_ih0 + (int)u * s.stride, iw = c_iw0 + (int)v * s.stride;
            u0 = (ih + s.pad) / s.stride; v0 = (iw + s.pad) / s.stride;  // tap (i, j) reads dy at (u0 - i, v0 - j)
            bbase = (int)((n * (unsigned)s.F + (unsigned)(g * s.Mg)) * (unsigned)s.OHOW) + u0 * s.OW + v0;
            obase = (n * (unsigned)s.C + (unsigned)(g * s.Cg)) * (unsigned)s.HW + (unsigned)(ih * s.W + iw);
        }
        return true;
    };

    // ---- this thread's staging column ----
    const int bj = tid % BN, bk0 = tid / BN;
    int b_base = 0, b_u0 = 0, b_v0 = 0;
    unsigned o_unused = 0;
    decode(p0 + bj, b_base, b_u0, b_v0, o_unused);

    // ---- this thread's A rows ----
    const int ak = tid % BK, am0 = tid / BK;
    const float* abase = a.a_base + (long long)g * a.a_group_stride;
    unsigned a_rowoff[A_IT];
    unsigned a_rowok = 0;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int m = m0 + am0 + i * (256 / BK);
        const bool ok = m < a.M;
        a_rowoff[i] = ok ? (unsigned)m * (unsigned)a.a_row_stride : 0u;
        a_rowok |= (ok ? 1u : 0u) << i;
    }

    // table entry of reduction index r (one thread per entry): r -> (major, tap) -> (major, i, j)
    auto fill_ktab = [&](int kt, int slot) {
        if (tid < BK) {
            const int r = kt * BK + tid;
            int4 e = make_int4(0, 0, 0, 0);
            if (r < KR) {
                const unsigned major = fast_div((unsigned)r, ntaps_magic);
                const unsigned tap = (unsigned)r - major * (unsigned)ntaps;
                const unsigned i = fast_div(tap, nkc_magic), j = tap - i * (unsigned)nkc;
                e.w = 1;
                if (fwd) {  // major = c, (i, j) = (kr, kc)
                    e.x = r;  // W[f][c*k*k + tap], row stride K
                    e.y = (int)(major * (unsigned)s.HW + i * (unsigned)s.W + j);
                    e.z = (int)(i | (j << 16));
                } else {    // major = f, tap (kr0 + i*s, kc0 + j*s)
                    const int kr = kr0 + (int)i * s.stride, kc = kc0 + (int)j * s.stride;
                    e.x = (int)(major * (unsigned)s.K) + kr * s.ksz + kc;  // W[f][c][kr][kc], row (c) stride k*k
                    e.y = (int)(major * (unsigned)s.OHOW) - ((int)i * s.OW + (int)j);
                    e.z = (int)(((0u - i) & 0xffffu) | ((0u - j) << 16));
                }
            }
            ktab[slot][tid] = e;
        }
    };

    // Staging registers. Every global load is UNCONDITIONAL from a clamped (always legal) offset; validity is applied
    // when the value is written to LDS, so load_tile is straight-line code.
    float ra[A_IT], rb[B_IT];
    unsigned a_ok = 0, b_ok = 0;
    auto load_tile = [&](int slot) {
        {
            const int4 e = ktab[slot][ak];
            a_ok = e.w ? a_rowok : 0u;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) ra[i] = abase[e.w ? a_rowoff[i] + (unsigned)e.x : 0u];
        }
        int4 e[B_IT];
#pragma unroll
        for (int i = 0; i < B_IT; ++i) e[i] = ktab[slot][bk0 + i * B_ROWS];
        b_ok = 0;
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int du = (e[i].z << 16) >> 16, dv = e[i].z >> 16;
            const bool ok = e[i].w != 0 && (unsigned)(b_u0 + du) < (unsigned)U && (unsigned)(b_v0 + dv) < (unsigned)V;
            rb[i] = a.b_base[ok ? (unsigned)(b_base + e[i].y) : 0u];
            b_ok |= (ok ? 1u : 0u) << i;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) As[buf][ak][am0 + i * (256 / BK)] = ((a_ok >> i) & 1u) ? ra[i] : 0.f;
#pragma unroll
        for (int i = 0; i < B_IT; ++i) Bs[buf][bk0 + i * B_ROWS][bj] = ((b_ok >> i) & 1u) ? rb[i] : 0.f;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lhi = lane >> 5;
    if (nk > 0) {
        fill_ktab(0, 0);
        __syncthreads();
        load_tile(0);
        store_tile(0);
        if (nk > 1) fill_ktab(1, 1);
        __syncthreads();
    }
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load_tile(cur ^ 1);  // global loads in flight under the MFMAs
        // always BK/2 steps: entries past the end of the reduction are zero in LDS (table `valid` = 0)
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = As[cur][2 * ks + lhi][(wm * TM + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = Bs[cur][2 * ks + lhi][(wn * TN + j) * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
        }
        if (kt + 1 < nk) store_tile(cur ^ 1);
        if (kt + 2 < nk) fill_ktab(kt + 2, cur);
        __syncthreads();
    }

    // ---- epilogue: bias (quirk 2: exactly 0 and 1 are skipped), activation; dX stores plainly (overwrite) ----
    const unsigned o_row_stride = fwd ? (unsigned)s.OHOW : (unsigned)s.HW;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        int bb, u0, v0;
        unsigned ob;
        if (!decode(p0 + (wn * TN + j) * 32 + l31, bb, u0, v0, ob)) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + i) * 32 + mfma_row(r, lane);
                if (m >= a.M) continue;
                float v = acc[i][j][r];
                if (fwd) v = conv_store_value(v, g * s.Mg + m, a.bias, a.add_bias, a.act, a.slopes);
                a.out[(size_t)ob + (size_t)m * o_row_stride] = v;
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------

template <int WM, int WN, int TM, int TN>
static void launch_large(LargeArgs& a, long long max_cols, int nclass) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    a.mtiles = ceil_div(a.M, BM);
    const long long blocks = (long long)a.mtiles * ceil_div(max_cols, BN);
    if (blocks >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] conv (kernel size %d): %lld column tiles exceed one grid\n", a.s.ksz, blocks);
        exit(1);
    }
    dim3 grid((unsigned)blocks, (unsigned)a.s.groups, (unsigned)nclass);
    conv_large_gemm_kernel<WM, WN, TM, TN, 16><<<grid, 256, 0, current_stream()>>>(a);
    KERNEL_CHECK();
}

// the row tile that pads M least (the larger one on a tie); 64 rows when 128 would leave CUs without a workgroup
static void dispatch_large(LargeArgs& a, long long max_cols, int nclass) {
    auto padded = [&](int bm) { return ceil_div(a.M, bm) * bm; };
    int bm = 32;
    if (a.M > 32) {
        bm = 64;
        if (padded(96) <= padded(bm)) bm = 96;
        if (padded(128) <= padded(bm)) bm = 128;
        const long long tiles = (long long)ceil_div(a.M, 128) * ceil_div(max_cols, 128) * a.s.groups * nclass;
        if (bm == 128 && tiles < 2 * kCUs) bm = 64;
    }
    if (bm == 32) launch_large<1, 4, 1, 1>(a, max_cols, nclass);       // 32 x 128
    else if (bm == 64) launch_large<2, 2, 1, 2>(a, max_cols, nclass);  // 64 x 128
    else if (bm == 96) launch_large<1, 4, 3, 1>(a, max_cols, nclass);  // 96 x 128
    else launch_large<2, 2, 2, 2>(a, max_cols, nclass);                // 128 x 128
}

// Index range. Offsets into x, y, dy, dx are 32-bit and signed against the first image of a launch, so a launch takes at
// most chunk images with chunk * max(C*H*W, F*OH*OW) < 2^30 (this also bounds its columns, and leaves room for a window
// origin in the padding and for a column index rounded up to the tile). The multiply-high divisions
// decode r < KR + 16 by d <= k*k and are exact while r * d < 2^32: (rows * k*k + 16) * k*k < 2^32 with rows = C/g
// (forward, dW) or F/g (dX). A layer outside either bound is refused aloud.
static int large_chunk_images(const ConvShape& s) {
    const long long in = (long long)s.C * s.HW, out = (long long)s.F * s.OHOW;
    const long long per = in > out ? in : out;
    if (per >= (1LL << 30)) {
        fprintf(stderr, "[bcnn_hip] conv (kernel size %d): one image of %lld floats exceeds the 32-bit offsets\n", s.ksz, per);
        exit(1);
    }
    const long long chunk = per > 0 ? ((1LL << 30) - 1) / per : s.N;
    return (int)(chunk < s.N ? chunk : s.N);
}
static void large_check_reduction(const ConvShape& s, int rows) {
    const unsigned long long kk2 = (unsigned long long)s.ksz * s.ksz;
    if (((unsigned long long)rows * kk2 + 16) * kk2 >= (1ULL << 32)) {
        fprintf(stderr, "[bcnn_hip] conv (kernel size %d): a reduction over %d channels exceeds the exact range of the "
                        "index decode\n", s.ksz, rows);
        exit(1);
    }
}

// (emits no statistics: the caller runs the stand-alone sweep)
void conv_forward_large(const ConvFwdCall& c) {
    const ConvShape& s = c.s;
    large_check_reduction(s, s.Cg);
    const int chunk = large_chunk_images(s);
    KTimer kt(K_CONV_FWD, conv_gemm_flops(s), conv_gemm_bytes(s));
    trace_kernel("conv_large_gemm_kernel:fwd");
    for (int n0 = 0; n0 < s.N; n0 += chunk) {
        const int nb = s.N - n0 < chunk ? s.N - n0 : chunk;
        LargeArgs a;
        a.s = make_conv_shape(nb, s.C, s.H, s.W, s.F, s.ksz, s.stride, s.pad, s.groups);
        a.a_base = c.w; a.b_base = c.x + (size_t)n0 * s.C * s.HW; a.out = c.y + (size_t)n0 * s.F * s.OHOW;
        a.bias = c.bias; a.slopes = c.slopes;
        a.mode = 0;
        a.act = c.raw ? BCNN_HIP_ACT_NONE : c.act;
        a.add_bias = c.raw ? 0 : 1;
        a.M = s.Mg; a.a_row_stride = s.K; a.a_group_stride = (long long)s.Mg * s.K;
        a.kk2_magic = magic_of(s.ksz * s.ksz); a.ksz_magic = magic_of(s.ksz);
        dispatch_large(a, a.s.total_q, 1);
    }
}

void conv_backward_data_large(const ConvDxCall& c) {
    const ConvShape& s = c.s;
    large_check_reduction(s, s.Mg);
    const int chunk = large_chunk_images(s);
    KTimer kt(K_CONV_DX, conv_gemm_flops(s), conv_gemm_bytes(s));
    trace_kernel("conv_large_gemm_kernel:dx");
    const int st = s.stride;
    for (int n0 = 0; n0 < s.N; n0 += chunk) {
        const int nb = s.N - n0 < chunk ? s.N - n0 : chunk;
        LargeArgs a;
        a.s = make_conv_shape(nb, s.C, s.H, s.W, s.F, s.ksz, s.stride, s.pad, s.groups);
        a.a_base = c.w; a.b_base = c.dy + (size_t)n0 * s.F * s.OHOW; a.out = c.dx + (size_t)n0 * s.C * s.HW;
        a.bias = nullptr; a.slopes = nullptr;
        a.mode = 1; a.act = BCNN_HIP_ACT_NONE; a.add_bias = 0;
        a.M = s.Cg; a.a_row_stride = s.ksz * s.ksz; a.a_group_stride = (long long)s.Mg * s.K;
        a.kk2_magic = 0; a.ksz_magic = 0;
        // every class in one launch (blockIdx.z); the grid is sized by the largest one, the others' surplus blocks return
        long long max_cols = 0;
        for (int ra = 0; ra < st; ++ra)
            for (int rb = 0; rb < st; ++rb) {
                const LargeClass ci = large_class(a.s, ra, rb);
                const long long cols = (long long)nb * ci.Hc * ci.Wc;
                if (cols > max_cols) max_cols = cols;
            }
        if (max_cols > 0) dispatch_large(a, max_cols, st * st);
    }
}

// ================================================================================================
// dW: rows f (BM = TM * 32), columns r = (c, kr, kc) (64 per workgroup), reduction over q split across workgroups and,
// inside one, across its four waves (16 of the 64 staged q each). Column K of the last column tile is all ones when the
// padded tile has room for it: its sums are the bias gradient.
// ================================================================================================
struct LargeDwArgs {
    const float* x;   // first image of this launch
    const float* dy;
    float* partials;  // [qsplits * 4][groups][mtiles * BM][ntiles * 64]
    ConvShape s;      // N: the images of this launch
    int mtiles, ntiles;
    int q_per_split;  // multiple of 64
    int bias_col;
    unsigned kk2_magic, ksz_magic;
};

constexpr int LDW_BQ = 64, LDW_BN = 64;
enum { LDW_VALID = 0x10000, LDW_ONES = 0x20000 };

template <int TM>
__global__ __launch_bounds__(256) void conv_large_dw_kernel(const LargeDwArgs a) {
    constexpr int TN = LDW_BN / 32, BM = TM * 32;
    constexpr int LDA = BM + 1, LDB = LDW_BN + 1;  // odd strides: transposing stores and fragment reads conflict-free
    constexpr int A_IT = BM * LDW_BQ / 256, B_IT = LDW_BN * LDW_BQ / 256;
    __shared__ float As[LDW_BQ][LDA];  // As[q][f]
    __shared__ float Bs[LDW_BQ][LDB];  // Bs[q][r]
    __shared__ int2 ktab[LDW_BN];      // {offset of (c, kr, kc) in an image group, kr | kc << 8 | flags}

    const ConvShape& s = a.s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = blockIdx.z, qs = blockIdx.y;
    const int mt = (int)blockIdx.x % a.mtiles, nt = (int)blockIdx.x / a.mtiles;
    const int f0 = mt * BM, k0 = nt * LDW_BN;
    const int qbeg = qs * a.q_per_split;
    const int total_q = (int)s.total_q;
    const int qend = qbeg + a.q_per_split < total_q ? qbeg + a.q_per_split : total_q;

    if (tid < LDW_BN) {
        const int k = k0 + tid;
        int2 e = make_int2(0, 0);
        if (k < s.K) {
            const unsigned c = fast_div((unsigned)k, a.kk2_magic), tap = (unsigned)k - c * (unsigned)(s.ksz * s.ksz);
            const unsigned kr = fast_div(tap, a.ksz_magic), kc = tap - kr * (unsigned)s.ksz;
            e.x = (int)(c * (unsigned)s.HW + kr * (unsigned)s.W + kc);
            e.y = (int)(kr | (kc << 8)) | LDW_VALID;
        } else if (k == s.K && a.bias_col) {
            e.y = LDW_ONES;
        }
        ktab[tid] = e;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int qi = tid & 63, r0 = tid >> 6;  // this thread stages q = qi of the step, rows r0 + 4*i of both tiles
    const int l31 = lane & 31, lhi = lane >> 5;
    __syncthreads();

    // unconditional loads from clamped offsets; what is invalid becomes 0 (or 1: the bias column) on the way to LDS
    float ra[A_IT], rb[B_IT];
    auto load_step = [&](int qstep) {
        const int q = qstep + qi;
        const bool qv = q < qend;
        const unsigned qq = qv ? (unsigned)q : 0u;
        const unsigned n = qq / (unsigned)s.OHOW, pix = qq - n * (unsigned)s.OHOW;
        const unsigned oh = pix / (unsigned)s.OW, ow = pix - oh * (unsigned)s.OW;
        const int ihq = (int)oh * s.stride - s.pad, iw0 = (int)ow * s.stride - s.pad;
        const int ih0 = qv ? ihq : kLargeNoCol;  // a q past the end: no tap is inside the plane
        const unsigned goff = (n * (unsigned)s.F + (unsigned)(g * s.Mg)) * (unsigned)s.OHOW + pix;
        const int xoff = (int)((n * (unsigned)s.C + (unsigned)(g * s.Cg)) * (unsigned)s.HW) + ihq * s.W + iw0;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int f = f0 + r0 + 4 * i;
            const bool ok = qv && f < s.Mg;
            const float v = a.dy[ok ? goff + (unsigned)f * (unsigned)s.OHOW : 0u];
            ra[i] = ok ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int2 e = ktab[r0 + 4 * i];
            const int kr = e.y & 0xff, kc = (e.y >> 8) & 0xff;
            const bool ok = (e.y & LDW_VALID) && (unsigned)(ih0 + kr) < (unsigned)s.H && (unsigned)(iw0 + kc) < (unsigned)s.W;
            const float v = a.x[ok ? (unsigned)(xoff + e.x) : 0u];
            rb[i] = ok ? v : ((qv && (e.y & LDW_ONES)) ? 1.0f : 0.f);
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) As[qi][r0 + 4 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < B_IT; ++i) Bs[qi][r0 + 4 * i] = rb[i];
    };

    if (qbeg < qend) load_step(qbeg);
    for (int qstep = qbeg; qstep < qend; qstep += LDW_BQ) {
        __syncthreads();  // previous step's fragments consumed
        store_step();
        __syncthreads();
        if (qstep + LDW_BQ < qend) load_step(qstep + LDW_BQ);  // next step's loads fly under the MFMAs
        const int qrow = wid * 16;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = As[qrow + 2 * ks + lhi][i * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = Bs[qrow + 2 * ks + lhi][j * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
        }
    }

    // each wave publishes its own partial tile (its quarter of the block's q range)
    const int MP = a.mtiles * BM, NP = a.ntiles * LDW_BN;
    const int part = qs * 4 + wid;
    float* out = a.partials + (((size_t)part * s.groups + g) * MP) * NP;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = f0 + i * 32 + mfma_row(r, lane);
                const int k = k0 + j * 32 + l31;
                out[(size_t)f * NP + k] = acc[i][j][r];
            }
}

struct LargeDwPlan {
    int TM, mtiles, ntiles, qsplits, q_per_split, bias_col;
    size_t partial_floats;
};

// s: the shape of ONE launch (a chunk of images)
static LargeDwPlan plan_large_dw(const ConvShape& s, bool want_bias_col) {
    LargeDwPlan p;
    auto padded = [&](int bm) { return ceil_div(s.Mg, bm) * bm; };
    p.TM = 1;
    if (s.Mg > 32) {
        p.TM = 2;
        if (padded(96) < padded(64)) p.TM = 3;
    }
    const int BM = p.TM * 32;
    p.mtiles = ceil_div(s.Mg, BM);
    p.ntiles = ceil_div(s.K, LDW_BN);
    p.bias_col = (want_bias_col && (s.K % LDW_BN) != 0) ? 1 : 0;  // needs a free slot in the padded column tile
    // ~4 workgroups per CU, >= 4 steps per workgroup
    const SplitK sk = split_k(s.total_q, (long long)p.mtiles * p.ntiles * s.groups, 4, LDW_BQ, 4);
    p.q_per_split = sk.chunk;
    p.qsplits = sk.splits;
    p.partial_floats = (size_t)p.qsplits * 4 * s.groups * (size_t)(p.mtiles * BM) * (size_t)(p.ntiles * LDW_BN);
    return p;
}

static bool large_dw_runs(const ConvShape& s) { return conv_large_wanted(s) && s.total_q > 0 && s.Mg > 0 && s.Cg > 0; }

// the first chunk of images is the largest launch
static ConvShape large_first_chunk(const ConvShape& s) {
    return make_conv_shape(large_chunk_images(s), s.C, s.H, s.W, s.F, s.ksz, s.stride, s.pad, s.groups);
}

size_t conv_dw_large_workspace_floats(const ConvShape& s) {
    if (!large_dw_runs(s)) return 0;
    return plan_large_dw(large_first_chunk(s), true).partial_floats;
}

bool conv_backward_weights_large(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                 float* workspace, size_t workspace_floats, bool* bias_done) {
    if (!conv_large_wanted(s)) return false;
    if (!large_dw_runs(s)) return true;
    large_check_reduction(s, s.Cg);
    const int chunk = large_chunk_images(s);
    conv_require_workspace(workspace, workspace_floats, plan_large_dw(large_first_chunk(s), dbias != nullptr).partial_floats);
    KTimer kt(K_CONV_DW, conv_gemm_flops(s), conv_gemm_bytes(s));
    trace_kernel("conv_large_dw_kernel");
    int bias_col = 0;
    for (int n0 = 0; n0 < s.N; n0 += chunk) {  // beta = 1: every chunk adds its sums onto dw, in this order
        const int nb = s.N - n0 < chunk ? s.N - n0 : chunk;
        LargeDwArgs a;
        a.s = make_conv_shape(nb, s.C, s.H, s.W, s.F, s.ksz, s.stride, s.pad, s.groups);
        const LargeDwPlan p = plan_large_dw(a.s, dbias != nullptr);
        a.x = x + (size_t)n0 * s.C * s.HW; a.dy = dy + (size_t)n0 * s.F * s.OHOW; a.partials = workspace;
        a.mtiles = p.mtiles; a.ntiles = p.ntiles; a.q_per_split = p.q_per_split; a.bias_col = p.bias_col;
        a.kk2_magic = magic_of(s.ksz * s.ksz); a.ksz_magic = magic_of(s.ksz);
        bias_col = p.bias_col;
        dim3 grid((unsigned)(p.mtiles * p.ntiles), (unsigned)p.qsplits, (unsigned)s.groups);
        if (p.TM == 1) conv_large_dw_kernel<1><<<grid, 256, 0, current_stream()>>>(a);
        else if (p.TM == 2) conv_large_dw_kernel<2><<<grid, 256, 0, current_stream()>>>(a);
        else conv_large_dw_kernel<3><<<grid, 256, 0, current_stream()>>>(a);
        KERNEL_CHECK();
        conv_dw_tiles_finalize(workspace, p.qsplits * 4, s.groups, s.Mg, s.K, p.mtiles * p.TM * 32, p.ntiles * LDW_BN, p.bias_col,
                               dw, dbias, 16);
    }
    *bias_done = bias_col != 0;
    return true;
}

}  // namespace bcnn_hip
