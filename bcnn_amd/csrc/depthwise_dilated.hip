// depthwise_dilated.hip -- the dilated (atrous) depthwise convolution: one filter per channel whose k x k taps sit
// `dilation` pixels apart. fp32 NCHW; weights [c][k][k] (the depthwise node's layout; as [c][1][k][k] the same floats are
// the dilated node's at groups == c); oh = (h + 2 pad - dilation (k - 1) - 1) / stride + 1. No reference counterpart:
// torch.nn.functional.conv2d(groups = c, dilation = d) is the oracle.
//
// THE ROUNDING RULE. The forward accumulates the taps in the depthwise reference's order (ky outer, kx inner) from +0,
// every product and every add rounded on its own (no contraction), then adds the bias, then the activation. An
// out-of-range tap adds w * 0, which leaves the sum's bits alone. The data gradient follows
// bcnn_depthwise_conv_layer.c:432-547 as depthwise.hip does: per input pixel the taps run ky = k-1 .. 0, kx = k-1 .. 0
// (ascending output row, then column), starting from dx (accumulate) or +0 (overwrite); a tap that reaches no output is
// skipped. Consequence: at dilation 1, y and dx carry the bits of bcnn_hip_depthwise_forward / _backward. One exception,
// on purpose: the bias is always added (the depthwise kernels skip a bias of exactly 1.0, the reference's bcnn_add_bias
// quirk, which torch does not share).
//
// dw and dbias have no atomics and the same bits on every run: each workgroup writes the k k tap sums and the bias sum of
// its (plane, band) into the caller's workspace [n c][bands][k k + 1]; a finalize kernel adds them per channel in index
// order (image, then band) in double and does dw +=, dbias +=. The split is a function of the shape only.
//
// Paths (bcnn_hip_dilated_depthwise_path), k == 3 and stride 1 unless generic:
//   1 plane    the staged plane (x forward, g = dy act'(y) backward) is at most kDdLdsFloats floats: one workgroup per
//              (n, c) plane copies it into LDS as it lies in memory (pitch = width: consecutive lanes read consecutive
//              banks for every tap) and reads a tap d rows / d columns away; the border is a select, not a zero halo.
//              Backward is ONE kernel: it stages g (applying act'(y) and writing dy back, summing dbias on the way), then
//              per input pixel reads the nine g taps once for both dx and, times x, the nine dw sums.
//   2 bands    larger planes: bands of rows with a 2 d halo, as many rows as kDdLdsFloats holds. Backward applies act'(y)
//              and sums dbias in a pass of its own first: a band's halo rows belong to its neighbours.
//   0 generic  k != 3, stride > 1, or a row so wide that 2 d + 1 of them do not fit: direct kernels from memory.
#include "chan_reduce.h"

namespace bcnn_hip {

namespace {

constexpr int kDdLdsFloats = 12288;  // 48 KiB of staged rows per workgroup: three workgroups per CU at the limit
constexpr int kDdRed = 40;           // backward: 4 waves x (9 taps + bias) cross-wave sums in front of the staged rows

struct DdArgs {
    const float* x;
    const float* wt;
    const float* bias;
    const float* y;
    float* out;   // forward: y
    float* dy;
    float* dx;    // may be NULL
    float* part;  // [planes][bands][k k + 1]
    int n, c, h, w, k, s, p, d, oh, ow, act;
    int bands, band_rows;  // band_rows: output rows (forward) / input rows (backward) per workgroup
    int overwrite;
};

// ---- paths 1 and 2, forward: k == 3, stride 1 -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ddw_fwd_lds_kernel(const DdArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / a.bands, band = blockIdx.x - plane * a.bands;
    const int ch = plane % a.c;
    const int r0 = band * a.band_rows, r1 = min(a.oh, r0 + a.band_rows);
    const int xlo = max(0, r0 - a.p), xhi = min(a.h, r1 - a.p + 2 * a.d);  // the input rows this band's taps reach
    const int rows = xhi - xlo;  // <= 0: the band lies in the padding
    const float* __restrict__ xp = a.x + (size_t)plane * a.h * a.w + (size_t)xlo * a.w;
    const int cnt = rows * a.w;
    for (int i = tid; i < cnt; i += 256) lds[i] = xp[i];
    __syncthreads();
    float wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = a.wt[ch * 9 + t];
    const float b = a.bias[ch];
    const int nout = (r1 - r0) * a.ow;
    float* __restrict__ yp = a.out + (size_t)plane * a.oh * a.ow + (size_t)r0 * a.ow;
    // (row, column) of the running output are carried along: one division per thread, none per output
    int oy = tid / a.ow, ox = tid - oy * a.ow;
    const int sy = 256 / a.ow, sx = 256 - sy * a.ow;
    for (int o = tid; o < nout; o += 256) {
        const int ry0 = r0 + oy - a.p - xlo, cx0 = ox - a.p;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ry = ry0 + ky * a.d;
            const bool vy = (unsigned)ry < (unsigned)rows;  // rows <= 0 (a band in the padding) is tested below
            const int rbase = ry * a.w;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int cx = cx0 + kx * a.d;
                const bool v = vy && rows > 0 && (unsigned)cx < (unsigned)a.w;
                const float t = lds[v ? rbase + cx : 0];
                acc = __fadd_rn(acc, __fmul_rn(wk[ky * 3 + kx], v ? t : 0.f));
            }
        }
        acc += b;
        yp[o] = act_fwd_cheap(acc, a.act, 0.f);
        ox += sx;
        oy += sy;
        if (ox >= a.ow) { ox -= a.ow; ++oy; }
    }
}

// ---- paths 1 and 2, backward: k == 3, stride 1 ------------------------------------------------------------------------------
// FUSED (path 1): the workgroup owns the whole g plane: it applies act'(y), writes dy back and sums dbias while staging.
// Otherwise (path 2) dy already holds g and slot 9 of band 0 the plane's bias sum (ddw_prepass_kernel).
template <bool FUSED>
__global__ __launch_bounds__(256) void ddw_bwd_lds_kernel(const DdArgs a) {
    extern __shared__ float lds[];
    float* red = lds;
    float* gs = lds + kDdRed;
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / a.bands, band = blockIdx.x - plane * a.bands;
    const int ch = plane % a.c;
    const int i0 = band * a.band_rows, i1 = min(a.h, i0 + a.band_rows);
    const int glo = FUSED ? 0 : max(0, i0 + a.p - 2 * a.d), ghi = FUSED ? a.oh : min(a.oh, i1 + a.p);
    const int rows = ghi - glo;
    const size_t gbase = (size_t)plane * a.oh * a.ow + (size_t)glo * a.ow;
    const int cnt = rows * a.ow;
    float sums[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) sums[t] = 0.f;
    for (int i = tid; i < cnt; i += 256) {
        float g = a.dy[gbase + i];
        if (FUSED) {
            if (a.act != BCNN_HIP_ACT_NONE) {
                g *= act_bwd_cheap(a.y[gbase + i], a.act, 0.f);
                a.dy[gbase + i] = g;
            }
            sums[9] += g;
        }
        gs[i] = g;
    }
    __syncthreads();
    float wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = a.wt[ch * 9 + t];
    const size_t xbase = (size_t)plane * a.h * a.w + (size_t)i0 * a.w;
    const float* __restrict__ xp = a.x + xbase;
    float* dxp = a.dx ? a.dx + xbase : nullptr;
    const int nin = (i1 - i0) * a.w;
    int iy = tid / a.w, ix = tid - iy * a.w;
    const int sy = 256 / a.w, sx = 256 - sy * a.w;
    for (int o = tid; o < nin; o += 256) {
        const float xv = xp[o];
        float acc = (dxp && !a.overwrite) ? dxp[o] : 0.f;
        const int ry0 = i0 + iy + a.p - glo, cx0 = ix + a.p;
#pragma unroll
        for (int ky = 2; ky >= 0; --ky) {
            const int ry = ry0 - ky * a.d;
            const bool vy = rows > 0 && (unsigned)ry < (unsigned)rows;
            const int rbase = ry * a.ow;
#pragma unroll
            for (int kx = 2; kx >= 0; --kx) {
                const int cx = cx0 - kx * a.d;
                const bool v = vy && (unsigned)cx < (unsigned)a.ow;
                const float t = gs[v ? rbase + cx : 0];
                const float gv = v ? t : 0.f;
                const float nx = __fadd_rn(acc, __fmul_rn(wk[ky * 3 + kx], gv));
                acc = v ? nx : acc;  // a tap that reaches no output is skipped, not added as zero: -0 stays -0
                sums[ky * 3 + kx] += xv * gv;
            }
        }
        if (dxp) dxp[o] = acc;
        ix += sx;
        iy += sy;
        if (ix >= a.w) { ix -= a.w; ++iy; }
    }
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        const float v = wave_sum(sums[t]);
        if (lane == 0) red[wid * 10 + t] = v;
    }
    __syncthreads();
    if (tid < 10 && (FUSED || tid < 9 || band > 0))
        a.part[((size_t)plane * a.bands + band) * 10 + tid] = (red[tid] + red[10 + tid]) + (red[20 + tid] + red[30 + tid]);
}

// ---- path 0 (and path 2's first pass) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ddw_fwd_generic_kernel(const DdArgs a, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gstride) {
        const unsigned ox = o % (unsigned)a.ow, t = o / (unsigned)a.ow;
        const unsigned oy = t % (unsigned)a.oh, plane = t / (unsigned)a.oh;
        const int ch = (int)(plane % (unsigned)a.c);
        const float* src = a.x + (size_t)plane * a.h * a.w;
        const float* wk = a.wt + (size_t)ch * a.k * a.k;
        const long long iy0 = (long long)oy * a.s - a.p, ix0 = (long long)ox * a.s - a.p;
        float acc = 0.f;
        for (int ky = 0; ky < a.k; ++ky) {
            const long long iy = iy0 + (long long)ky * a.d;
            if (iy < 0 || iy >= a.h) continue;
            for (int kx = 0; kx < a.k; ++kx) {
                const long long ix = ix0 + (long long)kx * a.d;
                if (ix < 0 || ix >= a.w) continue;
                acc = __fadd_rn(acc, __fmul_rn(wk[ky * a.k + kx], src[iy * a.w + ix]));
            }
        }
        acc += a.bias[ch];
        a.out[o] = act_fwd_cheap(acc, a.act, 0.f);
    }
}

// dy *= act'(y) in place and the plane's sum of it into part[plane * pitch + slot]; one workgroup per plane
__global__ __launch_bounds__(256) void ddw_prepass_kernel(const DdArgs a, int pitch, int slot) {
    __shared__ float red[4];
    const size_t base = (size_t)blockIdx.x * a.oh * a.ow;
    const int cnt = a.oh * a.ow;
    float s = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        float g = a.dy[base + i];
        if (a.act != BCNN_HIP_ACT_NONE) {
            g *= act_bwd_factor(a.y[base + i], a.act, 0.f);
            a.dy[base + i] = g;
        }
        s += g;
    }
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.x * pitch + slot] = t;
}

// the k k tap sums of one plane, tap by tap; one workgroup per plane
__global__ __launch_bounds__(256) void ddw_dw_generic_kernel(const DdArgs a) {
    __shared__ float red[4];
    const size_t plane = blockIdx.x;
    const float* __restrict__ xp = a.x + plane * a.h * a.w;
    const float* gp = a.dy + plane * a.oh * a.ow;
    const int cnt = a.oh * a.ow, kk = a.k * a.k;
    for (int tap = 0; tap < kk; ++tap) {
        const int ky = tap / a.k, kx = tap - ky * a.k;
        float s = 0.f;
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const int oy = i / a.ow, ox = i - oy * a.ow;
            const long long iy = (long long)oy * a.s - a.p + (long long)ky * a.d;
            const long long ix = (long long)ox * a.s - a.p + (long long)kx * a.d;
            if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) s += xp[iy * a.w + ix] * gp[i];
        }
        const float t = block_sum(s, red);
        if (threadIdx.x == 0) a.part[plane * (kk + 1) + tap] = t;
    }
}

__global__ __launch_bounds__(256) void ddw_dx_generic_kernel(const DdArgs a, unsigned total) {
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const unsigned ix = i % (unsigned)a.w, t = i / (unsigned)a.w;
        const unsigned iy = t % (unsigned)a.h, plane = t / (unsigned)a.h;
        const int ch = (int)(plane % (unsigned)a.c);
        const float* gp = a.dy + (size_t)plane * a.oh * a.ow;
        const float* wk = a.wt + (size_t)ch * a.k * a.k;
        float acc = a.overwrite ? 0.f : a.dx[i];
        for (int ky = a.k - 1; ky >= 0; --ky) {
            const long long th = (long long)iy + a.p - (long long)ky * a.d;
            if (th < 0 || th % a.s) continue;
            const long long oy = th / a.s;
            if (oy >= a.oh) continue;
            for (int kx = a.k - 1; kx >= 0; --kx) {
                const long long tw = (long long)ix + a.p - (long long)kx * a.d;
                if (tw < 0 || tw % a.s) continue;
                const long long ox = tw / a.s;
                if (ox >= a.ow) continue;
                acc = __fadd_rn(acc, __fmul_rn(wk[ky * a.k + kx], gp[oy * a.ow + ox]));
            }
        }
        a.dx[i] = acc;
    }
}

// dw[c][t] += and dbias[c] += the partials of channel c in index order: image, then band
__global__ void ddw_finalize_kernel(const float* __restrict__ part, int n, int c, int bands, int nt, float* dw,
                                    float* dbias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * (nt + 1)) return;
    const int ch = i / (nt + 1), t = i - ch * (nt + 1);
    double s = 0.0;
    for (int img = 0; img < n; ++img)
        for (int b = 0; b < bands; ++b) s += (double)part[(((size_t)img * c + ch) * bands + b) * (nt + 1) + t];
    if (t < nt) {
        if (dw) dw[(size_t)ch * nt + t] += (float)s;
    } else if (dbias) {
        dbias[ch] += (float)s;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
bool dd_shape(DdArgs* a, int n, int c, int h, int w, int k, int stride, int pad, int dilation) {
    const bool pos = n > 0 && c > 0 && h > 0 && w > 0 && k > 0 && stride > 0 && pad >= 0 && dilation > 0;
    const long long eh = (long long)h + 2LL * pad - (long long)dilation * (k - 1) - 1;
    const long long ew = (long long)w + 2LL * pad - (long long)dilation * (k - 1) - 1;
    const long long oh = pos && eh >= 0 ? eh / stride + 1 : 0, ow = pos && ew >= 0 ? ew / stride + 1 : 0;
    const bool ok = pos && oh > 0 && ow > 0 && (long long)n * c * h * w < (1LL << 31) &&
                    (long long)n * c * oh * ow < (1LL << 31) && (long long)c * k * k < (1LL << 31) &&
                    (long long)n * c * (k * k + 1) < (1LL << 31) &&
                    (long long)dilation * (k - 1) + 2LL * pad + h + w < (1LL << 30);
    if (!ok) return false;
    *a = DdArgs{};
    a->n = n; a->c = c; a->h = h; a->w = w; a->k = k; a->s = stride; a->p = pad; a->d = dilation;
    a->oh = (int)oh; a->ow = (int)ow;
    return true;
}

DdArgs dd_args(const char* what, int n, int c, int h, int w, int k, int stride, int pad, int dilation) {
    DdArgs a;
    if (!dd_shape(&a, n, c, h, w, k, stride, pad, dilation)) {
        fprintf(stderr, "[bcnn_hip] %s: unsupported shape n %d c %d h %d w %d k %d stride %d pad %d dilation %d\n", what, n,
                c, h, w, k, stride, pad, dilation);
        exit(1);
    }
    return a;
}

// The path and its bands: a function of the shape only. Forward stages x (bands of output rows), backward stages g (bands
// of input rows); both need the band's rows and 2 d rows of halo.
int dd_plan(const DdArgs& a, int backward, int* bands, int* band_rows) {
    const int rows_total = backward ? a.h : a.oh;  // what the bands divide
    const int st_rows = backward ? a.oh : a.h, st_w = backward ? a.ow : a.w;  // the staged plane
    *bands = 1;
    *band_rows = rows_total;
    if (a.k != 3 || a.s != 1) return 0;
    if ((long long)st_rows * st_w <= kDdLdsFloats) return 1;
    const long long fit = kDdLdsFloats / st_w - 2LL * a.d;  // rows of a band next to its halo
    if (fit < 1) return 0;
    *band_rows = (int)std::min<long long>(fit, rows_total);
    *bands = ceil_div(rows_total, *band_rows);
    if ((long long)a.n * a.c * *bands * 10 >= (1LL << 31)) { *bands = 1; *band_rows = rows_total; return 0; }
    return 2;
}

void refuse_act(const char* what, int act) {
    if (act != BCNN_HIP_ACT_PRELU && !act_needs_input(act)) return;
    fprintf(stderr, "[bcnn_hip] %s: activation %d is not supported (PReLU and the self-gated ones)\n", what, act);
    exit(1);
}

}  // namespace

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_dilated_depthwise_path(int n, int c, int h, int w, int k, int stride, int pad, int dilation, int backward) {
    DdArgs a;
    if (!dd_shape(&a, n, c, h, w, k, stride, pad, dilation)) return -1;
    int bands, band_rows;
    return dd_plan(a, backward != 0, &bands, &band_rows);
}

size_t bcnn_hip_dilated_depthwise_workspace_size(int n, int c, int h, int w, int k, int stride, int pad, int dilation) {
    const DdArgs a = dd_args("bcnn_hip_dilated_depthwise_workspace_size", n, c, h, w, k, stride, pad, dilation);
    int bands, band_rows;
    dd_plan(a, 1, &bands, &band_rows);
    return (size_t)n * c * bands * (k * k + 1);
}

void bcnn_hip_dilated_depthwise_forward(const float* x_d, const float* w_d, const float* bias_d, float* y_d, int n, int c,
                                        int h, int w, int k, int stride, int pad, int dilation, int act) {
    DdArgs a = dd_args("bcnn_hip_dilated_depthwise_forward", n, c, h, w, k, stride, pad, dilation);
    refuse_act("bcnn_hip_dilated_depthwise_forward", act);
    a.x = x_d; a.wt = w_d; a.bias = bias_d; a.out = y_d;
    a.act = act_is_cheap(act) ? act : BCNN_HIP_ACT_NONE;  // the others run as a pass of their own over y
    const size_t total = (size_t)n * c * a.oh * a.ow;
    const int path = dd_plan(a, 0, &a.bands, &a.band_rows);
    if (path == 0) {
        trace_kernel("ddw_fwd_generic_kernel");
        ddw_fwd_generic_kernel<<<stream_grid(total, 256), 256, 0, current_stream()>>>(a, (unsigned)total);
    } else {
        const int st_rows = path == 1 ? h : std::min(h, a.band_rows + 2 * dilation);
        const size_t lds = sizeof(float) * std::max<size_t>((size_t)st_rows * w, 1);
        trace_kernel(path == 1 ? "ddw_fwd_lds_kernel:plane" : "ddw_fwd_lds_kernel:bands");
        ddw_fwd_lds_kernel<<<(unsigned)(n * c * a.bands), 256, lds, current_stream()>>>(a);
    }
    KERNEL_CHECK();
    if (a.act != act) bcnn_hip_activation_forward(y_d, total, act, nullptr, a.oh * a.ow, c);
}

void bcnn_hip_dilated_depthwise_backward(const float* x_d, const float* w_d, const float* y_d, float* dy_d, float* dx_d,
                                         float* dw_d, float* dbias_d, int n, int c, int h, int w, int k, int stride, int pad,
                                         int dilation, int act, int overwrite, float* workspace_d, size_t workspace_elems) {
    DdArgs a = dd_args("bcnn_hip_dilated_depthwise_backward", n, c, h, w, k, stride, pad, dilation);
    refuse_act("bcnn_hip_dilated_depthwise_backward", act);
    const int path = dd_plan(a, 1, &a.bands, &a.band_rows);
    const size_t need = (size_t)n * c * a.bands * (k * k + 1);
    if (workspace_d == nullptr || workspace_elems < need) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_dilated_depthwise_backward: workspace of %zu floats, needs %zu\n",
                workspace_d ? workspace_elems : (size_t)0, need);
        exit(1);
    }
    a.x = x_d; a.wt = w_d; a.y = y_d; a.dy = dy_d; a.dx = dx_d; a.part = workspace_d; a.act = act;
    a.overwrite = overwrite != 0;
    const size_t total_o = (size_t)n * c * a.oh * a.ow, total_i = (size_t)n * c * h * w;
    if (path == 1) {
        if (!act_bwd_is_cheap(act)) {  // softplus, relu6, hard-sigmoid: the derivative in a pass of its own
            bcnn_hip_activation_backward(y_d, dy_d, total_o, act, nullptr, nullptr, a.oh * a.ow, c);
            a.act = BCNN_HIP_ACT_NONE;
        }
        const size_t lds = sizeof(float) * (kDdRed + (size_t)a.oh * a.ow);
        trace_kernel("ddw_bwd_lds_kernel:plane");
        ddw_bwd_lds_kernel<true><<<(unsigned)(n * c), 256, lds, current_stream()>>>(a);
        KERNEL_CHECK();
    } else {
        const int nt = k * k;
        trace_kernel("ddw_prepass_kernel");
        ddw_prepass_kernel<<<(unsigned)(n * c), 256, 0, current_stream()>>>(a, a.bands * (nt + 1), nt);
        KERNEL_CHECK();
        if (path == 2) {
            const int st_rows = std::min(a.oh, a.band_rows + 2 * dilation);
            const size_t lds = sizeof(float) * (kDdRed + (size_t)st_rows * a.ow);
            trace_kernel("ddw_bwd_lds_kernel:bands");
            ddw_bwd_lds_kernel<false><<<(unsigned)(n * c * a.bands), 256, lds, current_stream()>>>(a);
            KERNEL_CHECK();
        } else {
            trace_kernel("ddw_dw_generic_kernel");
            ddw_dw_generic_kernel<<<(unsigned)(n * c), 256, 0, current_stream()>>>(a);
            KERNEL_CHECK();
            if (dx_d) {
                trace_kernel("ddw_dx_generic_kernel");
                ddw_dx_generic_kernel<<<stream_grid(total_i, 256), 256, 0, current_stream()>>>(a, (unsigned)total_i);
                KERNEL_CHECK();
            }
        }
    }
    if (dw_d || dbias_d) {
        ddw_finalize_kernel<<<ceil_div((long long)c * (k * k + 1), 256), 256, 0, current_stream()>>>(
            workspace_d, n, c, a.bands, k * k, dw_d, dbias_d);
        KERNEL_CHECK();
    }
}

}  // extern "C"
