// conv_common.h -- shapes and MFMA helpers shared by the convolution kernels.
#pragma once
#include "common.h"

namespace bcnn_hip {

// One convolution problem, whole batch. Derived fields filled by make_conv_shape().
struct ConvShape {
    int N, C, H, W, F, ksz, stride, pad, groups;
    int OH, OW, OHOW, HW, Cg, Mg, K;  // Cg = C/groups, Mg = F/groups, K = Cg*ksz*ksz
    long long total_q;                // N*OH*OW output pixel columns (batch folded into GEMM-N)
    long long total_p;                // N*H*W input pixel columns (for dX)
    int pointwise;                    // ksz == 1: source read as a raw [Cg][OH*OW] matrix (quirk 1)
};

inline ConvShape make_conv_shape(int n, int c, int h, int w, int f, int k, int stride, int pad,
                                 int groups) {
    ConvShape s;
    s.N = n; s.C = c; s.H = h; s.W = w; s.F = f; s.ksz = k; s.stride = stride; s.pad = pad;
    s.groups = groups;
    s.OH = (h + 2 * pad - k) / stride + 1;  // reference bcnn_conv_layer.c:126-134
    s.OW = (w + 2 * pad - k) / stride + 1;
    s.OHOW = s.OH * s.OW; s.HW = h * w;
    s.Cg = c / groups; s.Mg = f / groups; s.K = s.Cg * k * k;
    s.total_q = (long long)n * s.OHOW;
    s.total_p = (long long)n * s.HW;
    s.pointwise = (k == 1);
    return s;
}

// what the profile (KTimer, common.h) charges a layer that runs as the plain GEMM: its multiply-adds, and every tensor once
inline double conv_gemm_flops(const ConvShape& s) { return 2.0 * (double)s.total_q * s.Mg * s.K * s.groups; }
inline double conv_gemm_bytes(const ConvShape& s) {
    return 4.0 * ((double)s.N * s.C * s.HW + (double)s.F * s.K + (double)s.N * s.F * s.OHOW);
}
// a weight-gradient kernel's split partials go to the caller's workspace (bcnn_hip_conv_workspace_size floats)
inline void conv_require_workspace(const float* workspace, size_t given, size_t need) {
    if (workspace != nullptr && given >= need) return;
    fprintf(stderr, "[bcnn_hip] conv backward: workspace too small (%zu floats given, %zu needed)\n", given, need);
    exit(1);
}
// How a split-K weight gradient cuts its reduction of `total` into `splits` chunks of `chunk` (a multiple of the kernel's K
// `step`): enough workgroups for `per_cu` per CU over `tiles` output tiles, at least `min_steps` steps per chunk, at most
// `max_splits` chunks (0: unlimited). A function of its arguments only, so two runs split alike.
struct SplitK {
    int chunk, splits;
};
inline SplitK split_k(long long total, long long tiles, int per_cu, int step, int min_steps, size_t max_splits = 0) {
    long long want = ((long long)per_cu * kCUs + tiles - 1) / tiles;
    const long long by_len = (total + (long long)min_steps * step - 1) / ((long long)min_steps * step);
    if (want > by_len) want = by_len;
    if (max_splits > 0 && want > (long long)max_splits) want = (long long)max_splits;
    if (want < 1) want = 1;
    const long long chunk = ((total + want - 1) / want + step - 1) / step * step;
    return {(int)chunk, (int)((total + chunk - 1) / chunk)};
}
// conv_bwd.hip. dw[g][f][k] += the sum over p of partials[p][g][f][k] (partial tiles of MP x NP), column K (bias_col) to
// dbias[g * Mg + f]; `outs` outputs x 256 / outs interleaved sub-sums per workgroup (4 or 16), added in a fixed order
void conv_dw_tiles_finalize(const float* partials, int nparts, int groups, int Mg, int K, int MP, int NP, int bias_col,
                            float* dw, float* dbias, int outs);
// conv_bwd.hip. dw[(row, col)][tap] += alpha * the sum over the splits of ws[split][tap][rows_cols], in a fixed order
void conv_dw_taps_reduce(const float* ws, float* dw, int splits, int kk2, int rows_cols, float alpha);
// ceil(2^32 / d), the multiplier of the kernels' multiply-high divisions by d (0 for d <= 1); every caller's d is >= 0
inline unsigned magic_of(int d) { return d > 1 ? (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d) : 0u; }

// Batch-norm statistics produced by a convolution kernel's epilogue (conv_igemm_dma.hip):
// partials[(channel * splits + i) * 2 + {sum, sum of squares}], the layout bn_stats_finalize consumes.
struct ConvStats {
    float* partials;
    int splits;
    size_t capacity;  // floats behind `partials`; every forward path checks its own slot count against it
};

// Backward sums of the stand-alone batch-norm node IN FRONT of a 1x1 convolution, emitted by that convolution's data-gradient
// kernel from the tile it is about to store (bcnn_batchnorm_layer.c:263-281 needs S1 = sum dz, S2 = sum dz * (y - mean)
// over (n, h, w) per channel; dz is this kernel's output, y the batch-norm node's input):
// partials[(channel * splits + column tile) * 2 + {S1, S2}], the layout bn_bwd_finalize consumes.
struct DxBnSums {
    const float* y;      // the batch-norm node's input (same shape as the convolution's input)
    const float* mean;   // its saved batch mean [C]
    float* partials;
    size_t capacity;     // floats behind `partials`
    int splits;          // out: partials per channel written, 0 = this path does not emit them
};

// A following eltwise node folded into a convolution node's batch-norm apply pass (bcnn_eltwise_layer.c:82-113)
struct BnResidual {
    const float* res;  // the eltwise node's second operand
    size_t count;      // elements of it that are added (the reference adds min_c * H * W of them: image 0)
    int act;           // the eltwise node's activation
};

// ---- weight packs made ahead of their use, for many layers in one launch (conv.hip: bcnn_hip_conv_prepack) -------
// The convolution kernels read the filter bank re-arranged: G g G^T in [16][Jpad][Mpad] (fused Winograd), A^T in
// [group][tap][Jpad][Mpad] (LDS-DMA GEMM). Stand-alone calls pack right before the kernel (one ~5 us launch per call);
// a caller that knows all layers of a pass hands them over at its start and the packs of a kind become ONE launch.
enum { PREPACK_WINO = 0, PREPACK_IGEMM = 1, PREPACK_KINDS = 2 };
struct WinoPackJob {
    const float* w;
    float* u;
    int F, C, dx_mode, Jpad, Mpad;
    int blocks;  // of 256 threads
    int npos;    // 16: G g G^T of F(2x2,3x3) (conv_winograd_fused.hip); 36: of F(4x4,3x3) (conv_winograd43.hip)
    int layout;  // npos 36 only: wino43_pack_one's layout (1: the stage order of conv_winograd43b.hip)
};
constexpr int kPackMaxTaps = 49;
struct IgemmPackJob {
    const float* w;
    float* at;
    int Mg, Cg, kk2, ksz;
    int M, J, Jpad, Mpad;
    int mode, groups;
    int gx, gy, gz;  // block grid of this job: 64 m x 4 j per block, gz = groups * taps
    unsigned char tapoff[kPackMaxTaps];  // kr*ksz + kc of packed tap index
    // forward form only, optional (BnFold below): row j (input channel c = g * Cg + j) of the pack is multiplied by
    // fold_scales[c] / sqrtf(fold_var[c] + 1e-6f)
    const float* fold_var;
    const float* fold_scales;
};

// The stand-alone batch-norm node IN FRONT of a 1x1 convolution, folded into that convolution (TRAIN mode, no activation in
// between: z = a y + b per channel with a = scale / sqrt(var + 1e-6), b = bias - mean a, bcnn_batchnorm_layer.c:226-241):
// W z = (W diag(a)) y + W b, so the GEMM reads the batch-norm's INPUT y with column-scaled weights and the per-filter
// constant W b only moves the mean of the convolution's own batch-norm behind it (conv.hip: bcnn_hip_conv_set_input_bnfold).
struct BnFold {
    const float* mean;   // saved batch mean [C]; nullptr: no fold
    const float* var;
    const float* scales;
    const float* bias;
};
#ifdef __HIPCC__
__device__ __forceinline__ float bnfold_a(const float* __restrict__ var, const float* __restrict__ scales, int c) {
    return scales[c] / sqrtf(var[c] + 0.000001f);  // one formula for the pack, the constant and the weight gradient
}
#endif
// true while the calling thread's weight gradients go to the side stream without a join per call (conv.hip)
bool conv_side_stream_deferred();
// the pack of (w, kind, mode) made by the current prepack batch and not yet used, or nullptr (conv.hip)
float* prepack_take(const float* w, int kind, int mode, size_t floats);
// what a family's kernel needs packed for a layer its *_wanted rule holds for (conv_paths.h). One signature for the table's
// hook; only wino_fused_pack_plan can still say false (experiment build: the split-bf16 kernels read no fp32 pack)
bool wino_fused_pack_plan(const ConvShape& s, int dx_mode, WinoPackJob* job, size_t* floats);  // conv_winograd_fused.hip
bool wino43_pack_plan(const ConvShape& s, int dx_mode, WinoPackJob* job, size_t* floats);      // conv_winograd43.hip
bool dma_pack_plan(const ConvShape& s, int dx_mode, IgemmPackJob* job, size_t* floats);        // conv_igemm_dma.hip
void wino_fused_pack_launch(const WinoPackJob* jobs_dev, int n, int max_blocks);
void dma_pack_launch(const IgemmPackJob* jobs_dev, int n, int max_blocks);

#ifdef __HIPCC__
typedef float f32x16 __attribute__((ext_vector_type(16)));

// v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32], exact fp32 fma chain (guide section 3).
// lane l holds A[i = l&31][k = l>>5], B[k = l>>5][j = l&31];
// D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5) for accumulator register r in [0,16).
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mfma_row(int r, int lane) {
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
// What a forward GEMM kernel stores for accumulator v of output channel fc: the bias (bcnn_add_scalar of the AVX build
// skips exactly 0 and 1: quirk 2), then a cheap activation. One copy for the fp32 kernels (conv_igemm.hip,
// conv_large.hip) and the bf16 one (conv_bf16.hip): equal accumulators give equal bits.
__device__ __forceinline__ float conv_store_value(float v, int fc, const float* bias, int add_bias, int act,
                                                  const float* slopes) {
    if (add_bias) {
        const float b = bias[fc];
        if (b != 0.0f && b != 1.0f) v += b;
    }
    if (act != BCNN_HIP_ACT_NONE) v = act_fwd_cheap(v, act, act == BCNN_HIP_ACT_PRELU ? slopes[fc] : 0.f);
    return v;
}
#endif

}  // namespace bcnn_hip
