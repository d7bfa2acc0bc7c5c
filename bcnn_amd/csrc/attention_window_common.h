// attention_window_common.h -- what the window-attention node's fp32 kernels (attention_window.hip) and its bf16 inference
// forward (attention_window_bf16.hip) share: the limits and refusals, the geometry of a launch, a position's place in the
// unrolled map and its shift region, the dense bias tile and its launch, and the instance ladder.
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

constexpr int kWaMaxLen = 64;     // positions of a window: two MFMA tiles of 32
constexpr int kWaMaxDim = 64;     // d and c
constexpr int kWaWaves = 1024;    // the waves a launch aims at (256 CUs x 4 SIMDs): G = ceil(kWaWaves / heads), at most the units

struct WaGeom {
    int n, heads, d, c, h, w, ws, shift, len, nwx, nwy, units;
    float scale;
};

// Lane p's position p of window (wy, wx): its offset inside a channel plane of the source map (0 for p >= len) and its shift
// region, 3 * (row region) + (column region), region 0 below extent - ws, 1 below extent - shift, else 2.
__device__ __forceinline__ void wa_position(const WaGeom& g, int wy, int wx, int p, int& off, int& code) {
    const int yi = p / g.ws, xi = p - yi * g.ws;
    const int y = wy * g.ws + yi, x = wx * g.ws + xi;
    int sy = y + g.shift, sx = x + g.shift;
    if (sy >= g.h) sy -= g.h;
    if (sx >= g.w) sx -= g.w;
    off = p < g.len ? sy * g.w + sx : 0;
    code = 3 * (y < g.h - g.ws ? 0 : y < g.h - g.shift ? 1 : 2) + (x < g.w - g.ws ? 0 : x < g.w - g.shift ? 1 : 2);
}

// ---- the dense bias tile ---------------------------------------------------------------------------------------------------
// dense[h][j][i] = table[h][rel(i, j)] for i, j < L, 0 elsewhere: the transposed result layout, lanes along the queries
// (static: every file that includes this header launches its own copy)
static __global__ __launch_bounds__(256) void wa_bias_kernel(const float* table, float* dense, int heads, int ws) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= heads * kWaMaxLen * kWaMaxLen) return;
    const int h = idx >> 12, j = (idx >> 6) & 63, i = idx & 63, len = ws * ws, span = 2 * ws - 1;
    float val = 0.f;
    if (i < len && j < len) {
        const int yi = i / ws, xi = i - yi * ws, yj = j / ws, xj = j - yj * ws;
        val = table[(size_t)h * span * span + (yi - yj + ws - 1) * span + (xi - xj + ws - 1)];
    }
    dense[idx] = val;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int wa_check(int n, int heads, int d, int c, int h, int w, int ws, int shift) {
    if (n < 1 || heads < 1 || heads > 65535 || h < 1 || w < 1) return BCNN_HIP_WINDOW_ATTN_BAD_EXTENT;  // (heads is gridDim.y)
    if (ws < 1 || ws * ws > kWaMaxLen) return BCNN_HIP_WINDOW_ATTN_BAD_WINDOW;
    if (h % ws != 0 || w % ws != 0) return BCNN_HIP_WINDOW_ATTN_RAGGED_MAP;
    if (shift < 0 || shift >= ws) return BCNN_HIP_WINDOW_ATTN_BAD_SHIFT;
    if (d < 1 || c < 1 || d > kWaMaxDim || c > kWaMaxDim) return BCNN_HIP_WINDOW_ATTN_BAD_HEAD_DIM;
    if ((long long)n * heads * (d > c ? d : c) * h * w >= 0x7fffffffLL) return BCNN_HIP_WINDOW_ATTN_TOO_LARGE;
    return 0;
}

static WaGeom wa_geom(const char* who, int n, int heads, int d, int c, int h, int w, int ws, int shift, float scale) {
    const int code = wa_check(n, heads, d, c, h, w, ws, shift);
    if (code != 0) {
        fprintf(stderr, "[bcnn_hip] %s: refused with code %d (n %d heads %d d %d c %d map %d x %d window %d shift %d)\n", who, code,
                n, heads, d, c, h, w, ws, shift);
        exit(1);
    }
    WaGeom g;
    g.n = n; g.heads = heads; g.d = d; g.c = c; g.h = h; g.w = w; g.ws = ws; g.shift = shift; g.len = ws * ws;
    g.nwx = w / ws; g.nwy = h / ws; g.units = n * g.nwx * g.nwy;
    g.scale = scale != 0.f ? scale : 1.0f / sqrtf((float)d);
    return g;
}

// the persistent workgroups of one head: a function of the shape alone
static int wa_groups(const WaGeom& g) { return std::min(g.units, ceil_div(kWaWaves, g.heads)); }

// the dense bias tiles [heads][64][64] at the head of the SCRATCH_REDUCE block, `extra` floats behind them
static float* wa_dense_bias(const float* table, const WaGeom& g, size_t extra) {
    const size_t dense = table ? (size_t)g.heads * kWaMaxLen * kWaMaxLen : 0;
    float* block = scratch(SCRATCH_REDUCE, dense + extra);
    if (table) {
        trace_kernel("window_attention_bias");
        wa_bias_kernel<<<(unsigned)ceil_div((long long)dense, 256), 256, 0, current_stream()>>>(table, block, g.heads, g.ws);
        KERNEL_CHECK();
    }
    return block;
}

// f.template operator()<DMAX, CT>() for the smaller of the 32 / 64 channel instances that hold d and c
template <class F>
static void wa_dispatch(int d, int c, F f) {
    if (d <= 32 && c <= 32) f.template operator()<32, 1>();
    else if (d <= 32) f.template operator()<32, 2>();
    else if (c <= 32) f.template operator()<64, 1>();
    else f.template operator()<64, 2>();
}

}  // namespace bcnn_hip
