// batchnorm.h -- the batch-norm entry points of batchnorm.hip that the convolution and pooling nodes call (conv.hip, pool.hip),
// and the call descriptions they take: filled by name at the call site, zero-initialised, what is absent stays zero.
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

struct BnExtent { int n, c, hw; };                 // tensors are [n][c][hw], per-channel vectors [c]
struct BnParams { const float *scales, *bias; };   // bias: the one the forward pass adds
struct BnSaved { const float *mean, *var; };       // the batch statistics the forward pass saved, as the backward pass reads them
struct BnRunning { float *run_mean, *run_var; };
struct BnGrads { float *dscales, *dbias, *dmean, *dvar; };

// workspace: copy of x kept for the backward pass (may be x itself); x_norm: the normalised values, which only
// bcnn_hip_batchnorm_forward[_stats] can still ask for; saved_*: written in TRAIN mode; pre: statistics partials the convolution
// epilogue left (pre->splits > 0); res: a following eltwise node folded into the apply sweep; stats_only: no apply sweep;
// mean_shift [c]: added to the batch mean that goes into the running mean (BnFold)
struct BnFwdCall {
    const float* x;
    float *y, *workspace, *x_norm, *saved_mean, *saved_var;
    BnExtent e;
    int mode, act;
    BnParams p;
    BnRunning run;
    const ConvStats* pre;
    const BnResidual* res;
    bool stats_only;
    const float* mean_shift;
};
void batchnorm_forward_impl(const BnFwdCall& f);

// dy: the gradient of the output, overwritten with that of the input and copied to dx (optional) -- or dout in its place where
// it must not be rewritten: the result then goes to dx alone. y: the forward output; workspace: the pre-normalisation input.
// p.bias (optional): with it the forward output is recomputed from `workspace` instead of read from y.
// sums (optional): whoever wrote dy left partials[(channel * splits + i) * 2 + {S1, S2}]: no read-only sweep.
// dout with res, dres, res_count: the backward of dout * act'(y) of a following eltwise node folded into the forward pass (y its
// output, act its activation), its second operand, that one's gradient (accumulated, may be NULL) and how much of it was added.
// consts: the table the sums sweep leaves for the apply sweep, consts_fM its divisor of dmean (0: n * hw)
struct BnBwdCall {
    float *dy, *dx, *dres;
    const float *dout, *y, *workspace, *sums, *res;
    int act, splits;
    size_t res_count;
    BnExtent e;
    BnParams p;
    BnSaved s;
    BnGrads g;
    float4* consts;
    float consts_fM;
};
void batchnorm_backward_impl(const BnBwdCall& b);
// the first sweep alone: S1, S2 per channel -> dbias, dscales, dmean, dvar
void batchnorm_backward_sums(const BnBwdCall& b);

}  // namespace bcnn_hip
