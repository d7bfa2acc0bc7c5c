// conv_paths.h -- the kernel families behind the convolution node: what one conv*.hip file defines and another one calls.
// conv.hip holds one ordered table per direction (kConvFwdFamilies, kConvDxFamilies, kDwFamilies); the tables are the order.
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

// y = act(conv(x, w) + bias); raw = 1: the bare convolution (a batch-norm follows). stats (optional, raw only): in -> a
// partials buffer, out -> splits = partials written per channel (the ladder has set it to 0: none)
struct ConvFwdCall {
    const float *x, *w, *bias, *slopes;
    float* y;
    ConvShape s;
    int act, raw;
    ConvStats* stats;
};
// dx = conv^T(dy, w). bs (optional): the backward sums of a batch-norm node in front, emitted by the kernels that can
// (bs->splits > 0; the ladder has set it to 0)
struct ConvDxCall {
    const float *w, *dy;
    float* dx;
    ConvShape s;
    DxBnSums* bs;
};
// A forward / data-gradient family is a row of conv.hip's tables made of:
//   *_wanted(s, raw)  the pure shape rule, all that is known without pointers (what bcnn_hip_conv_prepack can know). The
//                     layer has output (forward) / input (data gradient) pixels; the data gradient's rules ignore `raw`
//   *_usable(call)    only where pointers or buffers can still refuse a wanted layer; touches nothing
//   the run function  cannot refuse: opens its own KTimer, writes its trace name, launches
//   *_pack_plan       only where the kernel reads re-arranged weights (conv_common.h), asked behind *_wanted

// conv_window.hip: window-in-LDS kernels for 3x3 / s1 layers with K <= 27, and the 7x7 / s2 stem
bool conv_window_fwd_wanted(const ConvShape& s, int raw);
void conv_forward_window(const ConvFwdCall& c);
bool conv_stem_fwd_wanted(const ConvShape& s, int raw);
void conv_forward_stem(const ConvFwdCall& c);
// conv_direct.hip: LDS-free kernels for 3x3 layers of up to three channels per group and 5x5 layers of one
bool conv_direct_fwd_wanted(const ConvShape& s, int raw);
void conv_forward_direct(const ConvFwdCall& c);
// conv_winograd43.hip: F(4x4, 3x3) for planes of whole 4 x 4 tiles; the forward in the raw form only
bool conv_winograd43_fwd_wanted(const ConvShape& s, int raw);
bool conv_winograd43_fwd_usable(const ConvFwdCall& c);
void conv_forward_winograd43(const ConvFwdCall& c);
bool conv_winograd43_dx_wanted(const ConvShape& s, int);
bool conv_winograd43_dx_usable(const ConvDxCall& c);
void conv_backward_data_winograd43(const ConvDxCall& c);
// conv_winograd_fused.hip: F(2x2, 3x3) in one kernel for the wide-and-shallow layers
bool conv_winograd_fused_fwd_wanted(const ConvShape& s, int raw);
void conv_forward_winograd_fused(const ConvFwdCall& c);
bool conv_winograd_fused_dx_wanted(const ConvShape& s, int);
void conv_backward_data_winograd_fused(const ConvDxCall& c);
// conv_winograd.hip: F(2x2, 3x3) as three kernels for the deep 3x3 / s1 layers (transforms w in a kernel of its own)
bool conv_winograd_fwd_wanted(const ConvShape& s, int raw);
void conv_forward_winograd(const ConvFwdCall& c);
bool conv_winograd_dx_wanted(const ConvShape& s, int);
void conv_backward_data_winograd(const ConvDxCall& c);
// conv_large.hip: every non-pointwise layer with a kernel larger than 7x7 (the three directions; reads w as it is)
bool conv_large_wanted(const ConvShape& s, int raw = 0);
void conv_forward_large(const ConvFwdCall& c);
void conv_backward_data_large(const ConvDxCall& c);
// conv_bf16.hip: the opt-in inference forward on the bf16 matrix cores, fp32 accumulator (takes every shape)
bool conv_forward_bf16(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                       int act, int raw, ConvStats* stats);
// conv_igemm_dma.hip: the LDS-DMA GEMM. conv_forward_dma is the GEMM alone, untimed, false when the shape is not covered
// (conv_winograd.hip runs its 16 grouped GEMMs on it, conv.hip a folded layer); fold: the batch-norm in front of the layer
// whose per-channel factors go into the packed weights
bool conv_dma_fwd_wanted(const ConvShape& s, int raw = 0);
bool conv_forward_dma(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                      int act, int raw, ConvStats* stats, const BnFold* fold = nullptr);
void conv_forward_dma_timed(const ConvFwdCall& c);
bool conv_dma_dx_wanted(const ConvShape& s, int);
void conv_backward_data_dma(const ConvDxCall& c);
// conv_igemm_dma.hip: few input channels (the RGB stem) as a padded-plane GEMM; the zero-padded copy of x, which
// conv_dw_dma.hip reads too
bool conv_small_c_fwd_wanted(const ConvShape& s, int raw = 0);  // the weight gradient's few-channel family asks it too
void conv_forward_small_c(const ConvFwdCall& c);
float* conv_small_c_padded_input(const float* x, const ConvShape& s, size_t extra_floats, float** extra, int for_dw);
// conv_igemm.hip: the register-staged kernel (takes every shape) and the few-channel col2im form of the data gradient
void conv_forward_igemm(const ConvFwdCall& c);
void conv_backward_data_igemm(const ConvDxCall& c);
bool conv_small_c_dx_wanted(const ConvShape& s, int);
void conv_backward_data_small_c(const ConvDxCall& c);
// conv_direct.hip: pulls a small input into the Infinity Cache ahead of a kernel that streams a large output
void conv_prefetch_input(const float* x, const ConvShape& s, float* sink);

// ---- weight gradient: dw += dy (x) x, one signature for every family (the rows of kDwFamilies, conv.hip). `workspace` takes
// the split partials and is checked against the family's own *_workspace_floats(s) (0: not its shape); *bias_done is set when
// the family accumulated dbias as well: the first three and the last two can, and do for dbias != nullptr. Each times itself ------
size_t conv_dw_window_workspace_floats(const ConvShape& s);  // conv_window.hip: 3x3 / s1 layers with K <= 27
bool conv_backward_weights_window(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                  float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_stem_workspace_floats(const ConvShape& s);  // conv_window.hip: the 7x7 / s2 stem
bool conv_backward_weights_stem(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_direct_workspace_floats(const ConvShape& s);  // conv_direct.hip: K < 32, LDS-free
bool conv_backward_weights_direct(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                  float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_winograd43_workspace_floats(const ConvShape& s);  // conv_winograd43_dw.hip: F(4x4, 3x3), transposed form
bool conv_backward_weights_winograd43(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                      float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_winograd_fused_workspace_floats(const ConvShape& s);  // conv_winograd_fused.hip
bool conv_backward_weights_winograd_fused(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                          float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_winograd_workspace_floats(const ConvShape& s);  // conv_winograd.hip: 16 grouped GEMMs on the dma kernel
bool conv_backward_weights_winograd(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                    float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_dma_workspace_floats(const ConvShape& s);  // conv_dw_dma.hip: per-tap GEMM, LDS-DMA staging (general fast path)
bool conv_backward_weights_dma_timed(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                     float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_small_c_workspace_floats(const ConvShape& s);  // conv_dw_dma.hip: few input channels, one GEMM
bool conv_backward_weights_small_c(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                   float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_large_workspace_floats(const ConvShape& s);  // conv_large.hip: kernels larger than 7x7
bool conv_backward_weights_large(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                                 float* workspace, size_t workspace_floats, bool* bias_done);
size_t conv_dw_workspace_floats(const ConvShape& s);  // conv_bwd.hip: register-staged, takes every shape
bool conv_backward_weights(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s,
                           float* workspace, size_t workspace_floats, bool* bias_done);
// conv_dw_dma.hip: the LDS-DMA GEMM alone, untimed (conv_winograd.hip runs its 16 grouped GEMMs on it under its own timer).
// fold: the layer ran on W diag(a) (BnFold): the weight gradient's columns take the same factors
bool conv_backward_weights_dma(const float* x, const float* dy, float* dw, const ConvShape& s, float* workspace,
                               size_t workspace_floats, const BnFold* fold = nullptr);

// conv_winograd43b.hip: the second form of the F(4x4, 3x3) kernel (whole-tile planes), run by conv_winograd43.hip
void wino43b_run(const float* src, const float* w, float* dst, const ConvShape& s, int dx_mode, ConvStats* stats);
int wino43b_stats_slots(const ConvShape& s);
void wino43b_pack_dims(int J, int M, int* Jpad, int* Mpad);

}  // namespace bcnn_hip
