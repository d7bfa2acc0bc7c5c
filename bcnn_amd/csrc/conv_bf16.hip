// conv_bf16.hip -- the opt-in reduced-precision forward of the convolution node (PREDICT / VALID mode only; DESIGN.md
// section 15): an implicit GEMM on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16) with an fp32 accumulator, for every
// non-depthwise shape the node accepts: any kernel size, stride, padding, group count and channel counts.
//
// Rows are the output channels of a group, columns the output pixels with the batch folded in, the reduction runs over
// r = (c, kr, kc). Activations and weights stay fp32 in memory: a tile is gathered into registers as fp32 (unconditional
// loads from clamped, always legal offsets, as in conv_large.hip), rounded to bf16 round-to-nearest-even in pairs
// (v_cvt_pk_bf16_f32; NaN and Inf survive) and written to LDS with the reduction index contiguous, so that a lane's MFMA
// fragment (row / column l & 31, k = 8 (l >> 5) .. + 7) is one 16-byte read. What is outside the plane, the reduction or
// the tile is zero in LDS. No copy of the weights outlives the call: there is nothing that could go stale.
//   LDS image : [row or column][32 k as bf16 + 8 of padding] = 80-byte rows: the 16 lanes that ds_read_b128 serves in one
//               cycle fall on 16 distinct 4-bank slots (20 r mod 64 is injective on every group); double-buffered
//   r decode  : one table entry per k (offset into the image, kr, kc, valid), filled by the first 32 threads with two
//               multiply-high divisions; a gathered element is valid when ih = oh*s - p + kr and iw = ow*s - p + kc lie
//               inside the plane (two unsigned compares). k == 1 reads the raw [Cg][OH*OW] view (quirk 1)
//   epilogue  : pixels are on the accumulator's column index (lane & 31): a store covers 32 consecutive pixels of one
//               channel row; bias and activation are conv_store_value, the epilogue of the fp32 GEMM kernels
#include "conv_paths.h"

namespace bcnn_hip {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// n / d with magic = magic_of(d) (conv_common.h); exact while n * d < 2^32. The same function as conv_large.hip's.
__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }

// two fp32 -> two bf16 in one dword, round-to-nearest-even (lo: the lower k)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

struct Bf16Args {
    const float* w;
    const float* x;       // first image of this launch
    float* y;             // first image of this launch
    const float* bias;    // may be NULL
    const float* slopes;  // PReLU (may be NULL)
    ConvShape s;          // N: the images of this launch
    int act, add_bias;
    int mtiles;
    unsigned x_floats;    // floats of x in this launch: bound of the raw view of a 1x1 kernel
    unsigned kk2_magic, ksz_magic;
};

constexpr int kBf16BK = 32;                  // reduction indices per LDS tile (two MFMA steps of 16)
constexpr int kBf16LD = kBf16BK + 8;         // bf16 per LDS row: 64 bytes of data + 16 of padding
constexpr int kBf16NoCol = -(1 << 30);       // row coordinate of a column past the end: no tap brings it into a plane

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void conv_bf16_gemm_kernel(const Bf16Args a) {
    constexpr int BK = kBf16BK, LD = kBf16LD;
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int A_IT = BM / 32;  // rows per thread, 4 consecutive k each
    constexpr int B_IT = 16;       // consecutive k per thread, one column
    static_assert(WM * WN == 4 && BN == 128, "tile");
    __shared__ __attribute__((aligned(16))) unsigned short As[2][BM][LD];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[2][BN][LD];
    __shared__ int4 ktab[2][BK];  // {offset in the image group, kr, kc, valid}

    const ConvShape& s = a.s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int g = blockIdx.y;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = lb % a.mtiles, pt = lb / a.mtiles;
    const int m0 = mt * BM;
    const long long total_cols = s.total_q;
    const long long p0 = (long long)pt * BN;
    const int K = s.K, nk = (K + BK - 1) / BK;
    const int kk2 = s.ksz * s.ksz;
    // the gathered plane; a 1x1 kernel reads the raw view: every (column, k) inside the tensor is valid
    const int U = s.pointwise ? 1 : s.H, V = s.pointwise ? 1 : s.W;

    // ---- one column: offset of its window origin in x, the origin's coordinates, output offset ----
    auto decode = [&](long long col, int& bbase, int& u0, int& v0, unsigned& obase) -> bool {
        if (col >= total_cols) { bbase = 0; u0 = kBf16NoCol; v0 = 0; obase = 0; return false; }
        const unsigned n = (unsigned)(col / s.OHOW);
        const unsigned pix = (unsigned)(col - (long long)n * s.OHOW);
        obase = (n * (unsigned)s.F + (unsigned)(g * s.Mg)) * (unsigned)s.OHOW + pix;
        const unsigned img = (n * (unsigned)s.C + (unsigned)(g * s.Cg)) * (unsigned)s.HW;
        if (s.pointwise) {
            u0 = 0; v0 = 0;
            bbase = (int)(img + pix);
        } else {
            const unsigned u = pix / (unsigned)s.OW, v = pix - u * (unsigned)s.OW;
            u0 = (int)u * s.stride - s.pad; v0 = (int)v * s.stride - s.pad;
            bbase = (int)img + u0 * s.W + v0;
        }
        return true;
    };

    // ---- this thread's staging column (B) and rows (A) ----
    const int bj = tid % BN, bk0 = (tid / BN) * B_IT;
    int b_base = 0, b_u0 = 0, b_v0 = 0;
    unsigned o_unused = 0;
    decode(p0 + bj, b_base, b_u0, b_v0, o_unused);

    const int akq = (tid & 7) * 4, am0 = tid >> 3;
    const float* wg = a.w + (long long)g * s.Mg * K;
    unsigned a_rowoff[A_IT];
    unsigned a_rowok = 0;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int m = m0 + am0 + i * 32;
        const bool ok = m < s.Mg;
        a_rowoff[i] = ok ? (unsigned)m * (unsigned)K : 0u;
        a_rowok |= (ok ? 1u : 0u) << i;
    }

    // table entry of reduction index r (one thread per entry): r -> (c, tap) -> (c, kr, kc)
    auto fill_ktab = [&](int kt, int slot) {
        if (tid < BK) {
            const int r = kt * BK + tid;
            int4 e = make_int4(0, 0, 0, 0);
            if (r < K) {
                e.w = 1;
                if (s.pointwise) {
                    e.x = r * s.OHOW;  // r-th row of the raw [Cg][OH*OW] view
                } else {
                    const unsigned c = fast_div((unsigned)r, a.kk2_magic);
                    const unsigned tap = (unsigned)r - c * (unsigned)kk2;
                    const unsigned kr = fast_div(tap, a.ksz_magic), kc = tap - kr * (unsigned)s.ksz;
                    e.x = (int)(c * (unsigned)s.HW + kr * (unsigned)s.W + kc);
                    e.y = (int)kr; e.z = (int)kc;
                }
            }
            ktab[slot][tid] = e;
        }
    };

    // Staging registers. Every global load is UNCONDITIONAL from a clamped (always legal) offset; validity is applied
    // when the value is rounded and written to LDS, so load_tile is straight-line code.
    float ra[A_IT][4], rb[B_IT];
    unsigned a_ok = 0, b_ok = 0;  // A: bit i*4 + j; B: bit i
    auto load_tile = [&](int kt, int slot) {
        a_ok = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = kt * BK + akq + j;
            const bool kok = r < K;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                const bool ok = kok && ((a_rowok >> i) & 1u);
                ra[i][j] = wg[ok ? a_rowoff[i] + (unsigned)r : 0u];
                a_ok |= (ok ? 1u : 0u) << (i * 4 + j);
            }
        }
        b_ok = 0;
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int4 e = ktab[slot][bk0 + i];
            const unsigned off = (unsigned)(b_base + e.x);
            const bool ok = e.w != 0 && (unsigned)(b_u0 + e.y) < (unsigned)U && (unsigned)(b_v0 + e.z) < (unsigned)V &&
                            off < a.x_floats;
            rb[i] = a.x[ok ? off : 0u];
            b_ok |= (ok ? 1u : 0u) << i;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ((a_ok >> (i * 4 + j)) & 1u) ? ra[i][j] : 0.f;
            uint2 p;
            p.x = pack_bf16(v[0], v[1]); p.y = pack_bf16(v[2], v[3]);
            *reinterpret_cast<uint2*>(&As[buf][am0 + i * 32][akq]) = p;
        }
#pragma unroll
        for (int h = 0; h < B_IT / 8; ++h) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ((b_ok >> (h * 8 + j)) & 1u) ? rb[h * 8 + j] : 0.f;
            uint4 p;
            p.x = pack_bf16(v[0], v[1]); p.y = pack_bf16(v[2], v[3]);
            p.z = pack_bf16(v[4], v[5]); p.w = pack_bf16(v[6], v[7]);
            *reinterpret_cast<uint4*>(&Bs[buf][bj][bk0 + h * 8]) = p;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lhi = lane >> 5;
    if (p0 < total_cols && nk > 0) {  // (uniform per block)
        fill_ktab(0, 0);
        __syncthreads();
        load_tile(0, 0);
        store_tile(0);
        if (nk > 1) fill_ktab(1, 1);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) load_tile(kt + 1, cur ^ 1);  // global loads in flight under the MFMAs
            // always both steps: entries past the end of the reduction are zero in LDS
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                bf16x8 af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = *reinterpret_cast<const bf16x8*>(&As[cur][(wm * TM + i) * 32 + l31][ks * 16 + lhi * 8]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bf[j] = *reinterpret_cast<const bf16x8*>(&Bs[cur][(wn * TN + j) * 32 + l31][ks * 16 + lhi * 8]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
            if (kt + 1 < nk) store_tile(cur ^ 1);
            if (kt + 2 < nk) fill_ktab(kt + 2, cur);
            __syncthreads();
        }
    }
    if (p0 >= total_cols) return;

    // ---- epilogue: 32 consecutive pixels of one channel row per store ----
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
                if (m >= s.Mg) continue;
                a.y[(size_t)ob + (size_t)m * (unsigned)s.OHOW] =
                    conv_store_value(acc[i][j][r], g * s.Mg + m, a.bias, a.add_bias, a.act, a.slopes);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------

template <int WM, int WN, int TM, int TN>
static void launch_bf16(Bf16Args& a) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    a.mtiles = ceil_div(a.s.Mg, BM);
    const long long blocks = (long long)a.mtiles * ceil_div(a.s.total_q, BN);
    if (blocks >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] conv (bf16): %lld column tiles exceed one grid\n", blocks);
        exit(1);
    }
    dim3 grid((unsigned)blocks, (unsigned)a.s.groups, 1);
    conv_bf16_gemm_kernel<WM, WN, TM, TN><<<grid, 256, 0, current_stream()>>>(a);
    KERNEL_CHECK();
}

// the row tile that pads Mg least (the larger one on a tie); 64 rows when 128 would leave CUs without a workgroup
static void dispatch_bf16(Bf16Args& a) {
    const int M = a.s.Mg;
    auto padded = [&](int bm) { return ceil_div(M, bm) * bm; };
    int bm = 32;
    if (M > 32) {
        bm = 64;
        if (padded(96) <= padded(bm)) bm = 96;
        if (padded(128) <= padded(bm)) bm = 128;
        const long long tiles = (long long)ceil_div(M, 128) * ceil_div(a.s.total_q, 128) * a.s.groups;
        if (bm == 128 && tiles < 2 * kCUs) bm = 64;
    }
    if (bm == 32) launch_bf16<1, 4, 1, 1>(a);       // 32 x 128
    else if (bm == 64) launch_bf16<2, 2, 1, 2>(a);  // 64 x 128
    else if (bm == 96) launch_bf16<1, 4, 3, 1>(a);  // 96 x 128
    else launch_bf16<2, 2, 2, 2>(a);                // 128 x 128
}

// Index range, as in conv_large.hip: offsets into x and y are 32-bit against the first image of a launch, so a launch
// takes at most chunk images with chunk * max(C*H*W, F*OH*OW) < 2^30; the multiply-high divisions decode r < K + 32 by
// d <= k*k and are exact while r * d < 2^32. A layer outside either bound is refused aloud.
static int bf16_chunk_images(const ConvShape& s) {
    const long long in = (long long)s.C * s.HW, out = (long long)s.F * s.OHOW;
    const long long per = in > out ? in : out;
    if (per >= (1LL << 30)) {
        fprintf(stderr, "[bcnn_hip] conv (bf16): one image of %lld floats exceeds the 32-bit offsets\n", per);
        exit(1);
    }
    const long long chunk = per > 0 ? ((1LL << 30) - 1) / per : s.N;
    return (int)(chunk < s.N ? chunk : s.N);
}

bool conv_forward_bf16(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                       int act, int raw, ConvStats* stats) {
    if (stats) stats->splits = 0;  // PREDICT / VALID only: nobody consumes batch statistics
    if (s.total_q <= 0 || s.Mg == 0) return true;
    const unsigned long long kk2 = (unsigned long long)s.ksz * s.ksz;
    if (((unsigned long long)s.K + kBf16BK) * kk2 >= (1ULL << 32) ||
        ((unsigned long long)s.K + kBf16BK) * (unsigned long long)s.OHOW >= (1ULL << 31)) {
        fprintf(stderr, "[bcnn_hip] conv (bf16): a reduction over %d channels of kernel size %d exceeds the exact range of the "
                        "index decode\n", s.Cg, s.ksz);
        exit(1);
    }
    const int chunk = bf16_chunk_images(s);
    KTimer kt(K_CONV_FWD, conv_gemm_flops(s), conv_gemm_bytes(s));
    trace_kernel("conv_bf16_gemm_kernel");
    for (int n0 = 0; n0 < s.N; n0 += chunk) {
        const int nb = s.N - n0 < chunk ? s.N - n0 : chunk;
        Bf16Args a;
        a.s = make_conv_shape(nb, s.C, s.H, s.W, s.F, s.ksz, s.stride, s.pad, s.groups);
        a.w = w; a.x = x + (size_t)n0 * s.C * s.HW; a.y = y + (size_t)n0 * s.F * s.OHOW;
        a.bias = bias; a.slopes = slopes;
        a.act = raw ? BCNN_HIP_ACT_NONE : act;
        a.add_bias = (raw || bias == nullptr) ? 0 : 1;
        a.x_floats = (unsigned)((long long)nb * s.C * s.HW);
        a.kk2_magic = magic_of(s.ksz * s.ksz); a.ksz_magic = magic_of(s.ksz);
        dispatch_bf16(a);
    }
    return true;
}

}  // namespace bcnn_hip
