// interp.hip -- bilinear interpolation to a given output extent (the interp node), forward and backward. As measured
//  neither direction is bound by its bytes yet: the forward by the request stream of its gathered
// loads, the backward by its per-contribution inner loop.
//
// Semantics: torch.nn.functional.interpolate(mode="bilinear", size=(out_h, out_w)) for both values of align_corners,
// include/bcnn_hip.h. The per-axis rule (step, the two taps of an output index and their weights) is interp_rule.h and
// nothing else: every call first tabulates it on the device (interp_tables_kernel, one launch, library scratch
// SCRATCH_INTERP) and the two workers only look the tables up, so forward, backward and the host-side
// bcnn_hip_interp_axis_taps cannot disagree. This file is compiled with -ffp-contract=off like the rest of the library:
//   y = h0 * (w0 * x[y0][x0] + w1 * x[y0][x1]) + h1 * (w0 * x[y1][x0] + w1 * x[y1][x1])
// is seven roundings in exactly this association.
//
// The tables of one call, in one scratch block:
//   cols [round_up(out_w, 4)] and rows [out_h]  Tap {i0, i1, l0, l1}; the columns past out_w repeat the last one, so the
//                                                forward's four-column items read no garbage and need no branch
//   col_range [w] and row_range [h]             backward only: the output indices [lo, hi) one of whose taps names this input
//                                                index. Both tap sequences are non-decreasing in the output index, and
//                                                i1 == i0 + 1 except at the far edge, so these are the outputs with
//                                                i0 in {i - 1, i}: one contiguous run, found by two binary searches over
//                                                the rule itself. Empty when downsampling skips the element.
// Every kernel is a grid-stride loop over a capped 1-D grid; plane counts are bounded only by the 32-bit element index
// (fewer than 2^31 elements per tensor). Index divisions are multiply-high by host constants (FastDiv, common.h).
#include <cstdint>

#include "common.h"
#include "interp_rule.h"

namespace bcnn_hip {

struct alignas(16) InterpTap {
    int i0, i1;
    float l0, l1;
};

struct InterpGeom {
    int H, W, OH, OW, OWp, align_corners;  // OWp: out_w rounded up to 4
};

__device__ __forceinline__ InterpTap make_tap(int in, float step, int align_corners, int o) {
    InterpTap t;
    bcnn_interp_tap(in, step, align_corners, o, &t.i0, &t.i1, &t.l1);
    t.l0 = 1.0f - t.l1;
    return t;
}

// first output index in [0, out] whose i0 is >= bound (out: none)
__device__ __forceinline__ int first_i0_at_least(int in, int out, float step, int align_corners, int bound) {
    int lo = 0, hi = out;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (make_tap(in, step, align_corners, mid).i0 >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- prologue: the tables of one call. One thread per table entry ---------------------------------------------------------
__global__ __launch_bounds__(256) void interp_tables_kernel(InterpTap* __restrict__ cols, InterpTap* __restrict__ rows,
                                                            int2* __restrict__ col_range, int2* __restrict__ row_range,
                                                            const InterpGeom g, float step_w, float step_h, int with_ranges) {
    const unsigned n_taps = (unsigned)g.OWp + g.OH, total = n_taps + (with_ranges ? (unsigned)g.W + g.H : 0u);
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        if (t < (unsigned)g.OWp) {
            cols[t] = make_tap(g.W, step_w, g.align_corners, min((int)t, g.OW - 1));
        } else if (t < n_taps) {
            rows[t - g.OWp] = make_tap(g.H, step_h, g.align_corners, (int)(t - g.OWp));
        } else {
            const bool is_col = t - n_taps < (unsigned)g.W;
            const int i = (int)(is_col ? t - n_taps : t - n_taps - g.W);
            const int in = is_col ? g.W : g.H, out = is_col ? g.OW : g.OH;
            const float step = is_col ? step_w : step_h;
            const int2 r = make_int2(first_i0_at_least(in, out, step, g.align_corners, i - 1),
                                     first_i0_at_least(in, out, step, g.align_corners, i + 1));
            if (is_col) col_range[i] = r; else row_range[i] = r;
        }
    }
}

// ---- forward: one thread per FOUR consecutive outputs of a row --------------------------------------------------------------
// One 16-byte store per item where VEC (out_w % 4 == 0, y aligned), guarded scalar stores otherwise. Per item the kernel
// issues five 16-byte table loads (the row tap, four column taps) and sixteen 4-byte source loads on two source rows.
// When upsampling they hit the cache, but each is a vector-memory instruction behind a table entry: measured, this
// request stream and not the output write bounds the kernel (4 - 5 times a memset of y).
template <bool VEC>
__global__ __launch_bounds__(256) void interp_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const InterpTap* __restrict__ cols, const InterpTap* __restrict__ rows,
                                                         const InterpGeom g, const FastDiv dq, const FastDiv doh,
                                                         unsigned total_items) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total_items; t += gstride) {
        const unsigned rowid = fdiv(t, dq), q = t - rowid * dq.d;
        const unsigned plane = fdiv(rowid, doh), oy = rowid - plane * doh.d;
        const InterpTap rt = rows[oy];
        const float* __restrict__ r0 = x + (size_t)plane * g.H * g.W + (size_t)rt.i0 * g.W;
        const float* __restrict__ r1 = x + (size_t)plane * g.H * g.W + (size_t)rt.i1 * g.W;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const InterpTap ct = cols[q * 4 + e];
            v[e] = rt.l0 * (ct.l0 * r0[ct.i0] + ct.l1 * r0[ct.i1]) + rt.l1 * (ct.l0 * r1[ct.i0] + ct.l1 * r1[ct.i1]);
        }
        const size_t out = (size_t)rowid * g.OW + q * 4;
        if (VEC) {
            *reinterpret_cast<float4*>(y + out) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((int)q * 4 + e < g.OW) y[out + e] = v[e];
        }
    }
}

// ---- backward: gather form, no atomics ------------------------------------------------------------------------------------
// One thread per SOURCE element (h, w) visits the output rows of row_range[h] and the output columns of col_range[w] in
// ascending order and adds hw * (ww * dy) for every (row tap, column tap) pair that names it: tap 0 before tap 1 on both
// axes (at the far edge both taps of one output name the same element, two separate additions). The order is fixed by the
// shape alone: two runs give the same bits. OVERWRITE: start from 0 and always store; an element with no contributor
// becomes 0 and otherwise is not written. Upsampling by f an element has 4 f^2 contributions, each a table load, a dy
// load through the cache, two compares and up to two multiply-multiply-adds: measured, this loop bounds the kernel
// (158 - 300 GB/s of dy + dx), not the bytes.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void interp_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                         const InterpTap* __restrict__ cols, const InterpTap* __restrict__ rows,
                                                         const int2* __restrict__ col_range, const int2* __restrict__ row_range,
                                                         const InterpGeom g, const FastDiv dw, const FastDiv dh, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gstride) {
        const unsigned t = fdiv(s, dw), w = s - t * dw.d;
        const unsigned plane = fdiv(t, dh), h = t - plane * dh.d;
        const int2 rr = row_range[h], cr = col_range[w];
        const bool any = rr.x < rr.y && cr.x < cr.y;
        if (!OVERWRITE && !any) continue;
        float acc = OVERWRITE ? 0.f : dx[s];
        const float* __restrict__ gp = dy + (size_t)plane * g.OH * g.OW;
        for (int oy = rr.x; oy < rr.y; ++oy) {
            const InterpTap rt = rows[oy];
            const float* __restrict__ grow = gp + (size_t)oy * g.OW;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                if ((a ? rt.i1 : rt.i0) != (int)h) continue;
                const float hw = a ? rt.l1 : rt.l0;
                for (int ox = cr.x; ox < cr.y; ++ox) {
                    const InterpTap ct = cols[ox];
                    const float gv = grow[ox];
                    if (ct.i0 == (int)w) acc += hw * (ct.l0 * gv);
                    if (ct.i1 == (int)w) acc += hw * (ct.l1 * gv);
                }
            }
        }
        dx[s] = acc;
    }
}

// geometry and the limit of the 32-bit element index; exits like every other entry point handed a shape it cannot run
static InterpGeom interp_geom(const char* who, const bcnn_hip_interp_desc* d, int n, int c, int h, int w, long long& in_total,
                              long long& out_total) {
    InterpGeom g{};
    const bool ok = d && d->out_h >= 1 && d->out_w >= 1 && d->out_w <= 0x7ffffff0 && n >= 0 && c >= 0 && h >= 1 && w >= 1;
    in_total = ok ? (long long)n * c * h * w : 0;
    out_total = ok ? (long long)n * c * d->out_h * d->out_w : 0;
    if (!ok || in_total >= 0x7fffffffLL || out_total >= 0x7fffffffLL - 3) {
        fprintf(stderr, "[bcnn_hip] %s: invalid interpolation extents, or a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    g.H = h; g.W = w; g.OH = d->out_h; g.OW = d->out_w;
    g.OWp = (d->out_w + 3) & ~3;
    g.align_corners = d->align_corners ? 1 : 0;
    return g;
}

struct InterpTables {
    InterpTap *cols, *rows;
    int2 *col_range, *row_range;
};

// carves the call's scratch block and launches the prologue on the current stream
static InterpTables interp_tables(const InterpGeom& g, bool with_ranges) {
    const size_t taps = (size_t)g.OWp + g.OH, ranges = with_ranges ? (size_t)g.W + g.H : 0;
    float* block = scratch(SCRATCH_INTERP, taps * 4 + ranges * 2);
    InterpTables t;
    t.cols = reinterpret_cast<InterpTap*>(block);
    t.rows = t.cols + g.OWp;
    t.col_range = reinterpret_cast<int2*>(t.rows + g.OH);
    t.row_range = t.col_range + g.W;
    trace_kernel("interp_tables_kernel");
    interp_tables_kernel<<<stream_grid(taps + ranges, 256), 256, 0, current_stream()>>>(
        t.cols, t.rows, t.col_range, t.row_range, g, bcnn_interp_step(g.W, g.OW, g.align_corners),
        bcnn_interp_step(g.H, g.OH, g.align_corners), with_ranges ? 1 : 0);
    KERNEL_CHECK();
    return t;
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

void bcnn_hip_interp_axis_taps(int in, int out, int align_corners, int* i0, int* i1, float* l1) {
    if (in < 1 || out < 1) return;
    const float step = bcnn_interp_step(in, out, align_corners ? 1 : 0);
    for (int o = 0; o < out; ++o) bcnn_interp_tap(in, step, align_corners ? 1 : 0, o, i0 + o, i1 + o, l1 + o);
}

void bcnn_hip_interp_forward(const bcnn_hip_interp_desc* desc, const float* x, float* y, int n, int c, int h, int w) {
    long long in_total, total;
    const InterpGeom g = interp_geom("bcnn_hip_interp_forward", desc, n, c, h, w, in_total, total);
    if (!total) return;
    const InterpTables t = interp_tables(g, false);
    const unsigned qpr = (unsigned)g.OWp / 4;  // items per output row
    const long long items = (long long)n * c * g.OH * qpr;
    const FastDiv dq = make_fdiv(qpr, (unsigned long long)items);
    const FastDiv doh = make_fdiv((unsigned)g.OH, (unsigned long long)n * c * g.OH);
    const bool vec = (g.OW & 3) == 0 && al16(y);
    const int grid = stream_grid((size_t)items, 256);
    trace_kernel(vec ? "interp_fwd_kernel:v4" : "interp_fwd_kernel");
    if (vec) interp_fwd_kernel<true><<<grid, 256, 0, current_stream()>>>(x, y, t.cols, t.rows, g, dq, doh, (unsigned)items);
    else interp_fwd_kernel<false><<<grid, 256, 0, current_stream()>>>(x, y, t.cols, t.rows, g, dq, doh, (unsigned)items);
    KERNEL_CHECK();
}

void bcnn_hip_interp_backward(const bcnn_hip_interp_desc* desc, const float* dy, float* dx, int n, int c, int h, int w,
                              int overwrite) {
    long long total, out_total;
    const InterpGeom g = interp_geom("bcnn_hip_interp_backward", desc, n, c, h, w, total, out_total);
    if (!total) return;
    const InterpTables t = interp_tables(g, true);
    const FastDiv dw = make_fdiv((unsigned)w, (unsigned long long)total);
    const FastDiv dh = make_fdiv((unsigned)h, (unsigned long long)n * c * h);
    const int grid = stream_grid((size_t)total, 256);
    trace_kernel(overwrite ? "interp_bwd_kernel:overwrite" : "interp_bwd_kernel");
    if (overwrite) interp_bwd_kernel<true><<<grid, 256, 0, current_stream()>>>(dy, dx, t.cols, t.rows, t.col_range, t.row_range, g, dw, dh, (unsigned)total);
    else interp_bwd_kernel<false><<<grid, 256, 0, current_stream()>>>(dy, dx, t.cols, t.rows, t.col_range, t.row_range, g, dw, dh, (unsigned)total);
    KERNEL_CHECK();
}

}  // extern "C"
