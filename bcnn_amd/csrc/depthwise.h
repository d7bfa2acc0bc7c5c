// depthwise.h -- shapes, call descriptions and kernel families of the depthwise convolution. depthwise.hip holds the C-ABI, the
// two ordered family tables and the kernels for any shape; depthwise_march.hip and depthwise_lds.hip hold one fused 3x3
// family each and know nothing of each other.
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

struct DwShape {
    int N, C, H, W, OH, OW, ksz, stride, pad;
};
// a kernel larger than the padded plane has no output: (3 - 5) / 1 + 1 = -1 each way must not multiply to one pixel per plane
inline int dw_extent(int e) { return e < 0 ? 0 : e; }
inline DwShape dw_shape(int n, int c, int h, int w, int k, int stride, int pad) {
    const int st = stride < 1 ? 1 : stride;  // a size query may carry anything; no family takes such a shape
    return DwShape{n, c, h, w, dw_extent((h + 2 * pad - k) / st + 1), dw_extent((w + 2 * pad - k) / st + 1), k, stride, pad};
}

// Batch-norm coefficients of the stand-alone batch-norm node that consumes a depthwise layer's output, for the backward
// kernel that applies bcnn_batchnorm_layer.c:292-296 to the incoming gradient on the fly (device pointers, [C] each).
struct DwBnBwd {
    const float* dz;      // gradient with respect to the batch-norm OUTPUT
    const float* mean;    // saved batch mean
    const float* var;     // saved batch variance
    const float* scale;
    const float* dmean;   // written by bn_bwd_finalize_kernel
    const float* dvar;
};

// The convolution node (batch-norm + cheap activation) whose output is this layer's input, when the executor let it stop
// after its batch statistics: `x` handed to the kernels below is then that node's PRE-NORMALISATION output and every loaded
// element goes through act(bn(.)) first (bn_one of bn_math.h: the values the producer's apply sweep would have written).
struct DwBnIn {
    const float* mean;   // saved batch mean [C]; NULL: x is the input itself
    const float* var;
    const float* scale;
    const float* bias;
    int act;
};
// what a kernel that normalises its input on load can apply
inline bool dw_in_ok(const DwBnIn* in) {
    return !in || (in->mean && act_is_cheap(in->act) && in->act != BCNN_HIP_ACT_PRELU);
}

// y = act(dwconv(x) + bias); with `stats` also the per-channel sum / sum of squares partials of y (stats->splits: the slots
// per channel written, 0: not emitted); with `in`, x is normalised on load
struct DwFwdCall {
    const float *x, *w, *bias;
    float* y;
    DwShape s;
    int act;
    ConvStats* stats;
    const DwBnIn* in;
};
// g = dy * act'(y) (written back over dy when `write_back`), or with `bn` g = BNbackward(bn->dz) * act'(y) and dy is not
// touched; dbias += sum g; dw += sum x * g; dx = (overwrite ? 0 : dx) + w * g
// in_sums (with `in`, overwrite): the kernel also emits the backward sums of the producer's batch-norm over the dx it
// writes -- partials[(channel * splits + i) * 2 + {S1, S2}], the layout bn_bwd_finalize consumes; out: splits (0: not emitted)
struct DwBwdCall {
    const float *x, *w, *y;
    float *dy, *dx, *dw, *dbias;
    DwShape s;
    int act, overwrite, write_back;
    const DwBnBwd* bn;
    const DwBnIn* in;
    ConvStats* in_sums;
    float* partials;  // fused families: C * (most slots of any of them) * kDwPartFloats floats of scratch, from the ladder
};
constexpr int kDwPartFloats = 12;  // a fused backward kernel's partial per slot and channel: nine taps, bias sum, two unused

// what the kernel timer is told: forward and fused backward, one sweep; the unfused backward, the sweeps of its sequence
struct DwWork {
    double flops, bytes;
};
inline DwWork dw_fwd_work(const DwShape& s) {
    const double in = (double)s.N * s.C * s.H * s.W, out = (double)s.N * s.C * s.OH * s.OW;
    return DwWork{2.0 * out * s.ksz * s.ksz, 4.0 * (in + out)};
}
inline DwWork dw_bwd_work(const DwBwdCall& c) {
    const DwShape& s = c.s;
    const double in = (double)s.N * s.C * s.H * s.W, out = (double)s.N * s.C * s.OH * s.OW;
    double bytes;
    if (c.bn || c.in)  // dz (or dy read and written), y, x read; dx written (read too when it accumulates)
        bytes = (c.bn ? 2.0 : 3.0) * out + (c.overwrite ? 2.0 : 3.0) * in;
    else  // activation backward (y, dy r/w), bias gradient (dy), dW (x, dy), dX (dy, dx r/w)
        bytes = ((c.act != BCNN_HIP_ACT_NONE) ? 3.0 : 0.0) * out + out +
                (c.dx ? (in + out) + (out + (c.overwrite ? 1.0 : 2.0) * in) : 0.0);
    return DwWork{4.0 * out * s.ksz * s.ksz, 4.0 * bytes};
}

// the caller's buffer when it holds `splits` slots of two floats per channel (st->splits then says so), else NULL
inline float* dw_stats_slots(ConvStats* st, int C, int splits) {
    if (!st || !st->partials || st->capacity < (size_t)C * splits * 2) return nullptr;
    st->splits = splits;
    return st->partials;
}
// the sums of the producer's batch-norm backward are of the COMPLETE gradient: only when the kernel is dx's sole writer, and
// for producer activations whose derivative is 0 or 1
inline bool dw_in_sums_wanted(const DwBwdCall& c) {
    return c.in && c.in_sums && c.overwrite && (c.in->act == BCNN_HIP_ACT_NONE || c.in->act == BCNN_HIP_ACT_RELU);
}

// A fused family (depthwise_march.hip, depthwise_lds.hip) is asked only for 3x3 / pad 1 / stride 1 or 2 layers whose
// activations its kernels can apply (dw_fused_fwd_ok / dw_fused_bwd_ok of depthwise.hip). `takes` decides everything else that
// can refuse the layer -- plane geometry, alignment, LDS -- and touches nothing; `run` then launches. `slots`: partials per
// channel of its statistics / sums / weight-gradient partials, 0 when the shape is not the family's.
// The marching family also asks its tensors to be aligned to a lane's access (16 / 8 / 4 bytes), which no shape tells: slots
// for a shape do not promise that it takes a call. The LDS family asks nothing of the pointers and has one `slots` per
// direction: non-zero exactly for the shapes that direction's `takes` accepts (the tiling AND a workgroup's LDS).
size_t depthwise_march_splits(const DwShape& s);
bool depthwise_march_fwd_takes(const DwFwdCall& c);
void depthwise_march_forward(const DwFwdCall& c);
bool depthwise_march_bwd_takes(const DwBwdCall& c);
void depthwise_march_backward(const DwBwdCall& c);

size_t depthwise_lds_fwd_slots(const DwShape& s);
size_t depthwise_lds_bwd_slots(const DwShape& s);
bool depthwise_lds_fwd_takes(const DwFwdCall& c);
void depthwise_lds_forward(const DwFwdCall& c);
bool depthwise_lds_bwd_takes(const DwBwdCall& c);
void depthwise_lds_backward(const DwBwdCall& c);
// dw, dbias += the `splits` partials of a fused backward kernel (depthwise_lds.hip; both families write its layout)
void dwl_finalize_launch(const float* partials, int splits, int C, float* dw, float* dbias, hipStream_t st);

}  // namespace bcnn_hip
