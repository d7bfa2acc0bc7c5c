// batchnorm.h -- the batch-norm entry points of batchnorm.hip that the convolution and pooling nodes call (conv.hip, pool.hip).
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

// pre: statistics partials the convolution epilogue left (pre->splits > 0); res: a following eltwise node folded into the
// apply sweep; mean_shift [c]: added to the batch mean that goes into the running mean (BnFold)
void batchnorm_forward_impl(const float* x, float* y, float* run_mean, float* run_var, const float* scales,
                            const float* bias, float* saved_mean, float* saved_var, float* x_norm, float* workspace,
                            int n, int c, int hw, int mode, int act, const ConvStats* pre, const BnResidual* res,
                            bool stats_only, const float* mean_shift = nullptr);
// fwd_bias (optional): the forward bias; with it the forward output is recomputed from `workspace` instead of read from y
void batchnorm_backward_impl(float* dy, float* dx, const float* y, int act, const float* scales, float* dscales,
                             float* dbias, const float* saved_mean, const float* saved_var, float* dmean,
                             float* dvar, const float* workspace, int n, int c, int hw, const float* fwd_bias);
// the same when whoever wrote dy left the sums as partials[(channel * splits + i) * 2 + {S1, S2}]: no read-only sweep
void batchnorm_backward_presummed(float* dy, const float* y, int act, const float* scales, float* dscales, float* dbias,
                                  const float* saved_mean, const float* saved_var, float* dmean, float* dvar,
                                  const float* workspace, int n, int c, int hw, const float* fwd_bias, const float* sums,
                                  int splits);
// batch-norm backward of dout * act'(out) of a following eltwise node (out recomputed, dout not rewritten), result to dx
void batchnorm_backward_residual(const float* dout, const float* out, int act_res, const float* res, float* dres,
                                 size_t res_count, float* dx, const float* scales, float* dscales, float* dbias,
                                 const float* fwd_bias, const float* saved_mean, const float* saved_var, float* dmean,
                                 float* dvar, const float* workspace, int n, int c, int hw);
// the first sweep alone: S1, S2 per channel -> dbias, dscales, dmean, dvar. consts_fM: divisor of dmean in `consts` (0: n * hw)
void batchnorm_backward_sums(const float* dy, const float* y, int act, const float* scales, float* dscales, float* dbias,
                             const float* saved_mean, const float* saved_var, float* dmean, float* dvar,
                             const float* workspace, int n, int c, int hw, const float* fwd_bias,
                             const float* res = nullptr, unsigned res_count = 0, float4* consts = nullptr,
                             float consts_fM = 0.f);

}  // namespace bcnn_hip
