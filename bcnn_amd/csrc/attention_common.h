// attention_common.h -- what the attention node's fp32 kernels (attention.hip) and its bf16 inference forward
// (attention_bf16.hip) share: the limits and refusals, the scale, the exponential, the instance ladder and the store of an
// accumulator whose lanes hold one query each; and the fp32 -> bf16 packing of both bf16 forwards (attention_window_bf16.hip too).
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

constexpr int kAttnMaxDim = 128;   // d and c: Q (or K, V) as a B operand is dim / 2 registers, an accumulator dim / 2
constexpr int kAttnBlock = 128;    // queries (or keys) of a workgroup: 4 waves of one 32-column MFMA tile each
constexpr float kLog2e = 1.4426950408889634f;

// exp(x) for x <= 0 (and -inf): the maximum is subtracted BEFORE the scaling to base 2, so the argument's rounding error is
// relative to the distance from the maximum, not to the score
__device__ __forceinline__ float attn_exp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// ---- the bf16 inference forwards (attention_bf16.hip, attention_window_bf16.hip) ---------------------------------------------
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// two fp32 -> two bf16 in one dword, round-to-nearest-even (lo: the lower reduction index)
__device__ __forceinline__ unsigned attn_pack_bf16(float lo, float hi) {
    f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ bf16x8 attn_pack8(float a, float b, float c, float d, float e, float f, float g, float h) {
    u32x4 p = {attn_pack_bf16(a, b), attn_pack_bf16(c, d), attn_pack_bf16(e, f), attn_pack_bf16(g, h)};
    return __builtin_bit_cast(bf16x8, p);
}

// acc[tile][r] (row tile * 32 + mfma_row(r, lane), column x) times f, assigned or added to dst [rows][L]
template <int TILES>
__device__ __forceinline__ void attn_store_acc(float* dst, const f32x16 (&acc)[TILES], int rows, int L, int x, int lane,
                                               float f, int overwrite) {
    if (x >= L) return;
#pragma unroll
    for (int tile = 0; tile < TILES; ++tile) {
        if (tile * 32 >= rows) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile * 32 + mfma_row(r, lane);
            if (row >= rows) continue;
            float* at = dst + (size_t)row * L + x;
            const float val = acc[tile][r] * f;
            *at = overwrite ? val : *at + val;
        }
    }
}

static bool attn_check(const char* who, int n, int heads, int d, int c, int lq, int lk) {
    if (n < 0 || heads < 0 || lq < 0 || lk < 0 || d < 1 || c < 1 || d > kAttnMaxDim || c > kAttnMaxDim) {
        fprintf(stderr, "[bcnn_hip] %s: a negative extent, or a head of %d / %d channels outside 1 .. %d\n", who, d, c,
                kAttnMaxDim);
        exit(1);
    }
    const long long nh = (long long)n * heads, dim = d > c ? d : c, len = lq > lk ? lq : lk;
    if (nh * dim * len >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] %s: a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    return nh > 0 && lq > 0 && lk > 0;
}

static float attn_scale(float scale, int d) { return scale != 0.f ? scale : 1.0f / sqrtf((float)d); }

// f.template operator()<DMAX, CT>() for the smallest of 32 / 64 / 128 channels that hold d, and of 1 / 2 / 4 tiles that hold c
template <class F>
static void attn_dispatch(int d, int c, F f) {
    const int ct = c <= 32 ? 1 : c <= 64 ? 2 : 4;
#define ATTN_ROW(DM)                                  \
    do {                                              \
        if (ct == 1) f.template operator()<DM, 1>();  \
        else if (ct == 2) f.template operator()<DM, 2>(); \
        else f.template operator()<DM, 4>();          \
    } while (0)
    if (d <= 32) ATTN_ROW(32);
    else if (d <= 64) ATTN_ROW(64);
    else ATTN_ROW(128);
#undef ATTN_ROW
}

}  // namespace bcnn_hip
