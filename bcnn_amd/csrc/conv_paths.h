// conv_paths.h -- the kernel families behind the convolution node: what one conv*.hip file defines and another one calls
// (conv.hip tries them in order; the prepack helpers are in conv_common.h). A bool return is "took the layer": false means
// the shape, or an alignment the kernel needs, is not covered, nothing was launched and the caller tries the next family.
#pragma once
#include "conv_common.h"

namespace bcnn_hip {

// ---- forward: y = act(conv(x, w) + bias); raw = 1: the bare convolution (a batch-norm follows). stats (optional, raw only):
// in -> a partials buffer, out -> splits = partials written per channel (0: none) -----------------------------------------
// conv_window.hip: window-in-LDS kernels for 3x3 / s1 layers with K <= 27, and the 7x7 / s2 stem
bool conv_forward_window(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                         int act, int raw);
bool conv_forward_stem(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                       int act, int raw, ConvStats* stats);
// conv_direct.hip: LDS-free kernels for small reduction lengths (K <= 32)
bool conv_forward_direct(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                         int act, int raw);
// conv_winograd43.hip: F(4x4, 3x3) for planes of whole 4 x 4 tiles, raw output only
bool conv_forward_winograd43(const float* x, const float* w, float* y, const ConvShape& s, int raw, ConvStats* stats);
// conv_winograd_fused.hip: F(2x2, 3x3) in one kernel for the wide-and-shallow layers
bool conv_forward_winograd_fused(const float* x, const float* w, const float* bias, const float* slopes, float* y,
                                 const ConvShape& s, int act, int raw, ConvStats* stats);
// conv_winograd.hip: F(2x2, 3x3) as three kernels for the deep 3x3 / s1 layers
bool conv_forward_winograd(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                           int act, int raw, ConvStats* stats);
// conv_large.hip: every non-pointwise layer with a kernel larger than 7x7 (the three directions; reads w as it is)
bool conv_large_takes(const ConvShape& s);
bool conv_forward_large(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                        int act, int raw, ConvStats* stats);
// conv_bf16.hip: the opt-in inference forward on the bf16 matrix cores, fp32 accumulator (takes every shape)
bool conv_forward_bf16(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                       int act, int raw, ConvStats* stats);
// conv_igemm.hip: the LDS-DMA GEMM, the few-channel padded-plane GEMM, else the register-staged kernel (takes every shape)
void conv_forward_dispatch(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                           int act, int raw, ConvStats* stats);
// conv_igemm_dma.hip. fold: the batch-norm in front of the layer whose per-channel factors go into the packed weights
bool conv_forward_dma_supported(const ConvShape& s);
bool conv_forward_dma(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                      int act, int raw, ConvStats* stats, const BnFold* fold = nullptr);
bool conv_forward_small_c(const float* x, const float* w, const float* bias, const float* slopes, float* y, const ConvShape& s,
                          int act, int raw, ConvStats* stats);
// conv_igemm_dma.hip: few input channels (the RGB stem); their zero-padded copy of x, which conv_dw_dma.hip reads too
bool conv_small_c_applicable(const ConvShape& s);
float* conv_small_c_padded_input(const float* x, const ConvShape& s, size_t extra_floats, float** extra, int for_dw);
// conv_direct.hip: pulls a small input into the Infinity Cache ahead of a kernel that streams a large output
void conv_prefetch_input(const float* x, const ConvShape& s, float* sink);

// ---- data gradient ---------------------------------------------------------------------------------------------------
bool conv_backward_data_winograd43(const float* w, const float* dy, float* dx, const ConvShape& s);       // conv_winograd43.hip
bool conv_backward_data_winograd_fused(const float* w, const float* dy, float* dx, const ConvShape& s);  // conv_winograd_fused.hip
bool conv_backward_data_winograd(const float* w, const float* dy, float* dx, const ConvShape& s);        // conv_winograd.hip
bool conv_backward_data_large(const float* w, const float* dy, float* dx, const ConvShape& s);           // conv_large.hip
// conv_igemm.hip: the few-channel col2im form, the LDS-DMA GEMM, else the register-staged kernel (takes every shape).
// bs (optional): the backward sums of a batch-norm node in front, emitted by the kernels that can (bs->splits > 0)
void conv_backward_data(const float* w, const float* dy, float* dx, const ConvShape& s, DxBnSums* bs = nullptr);
bool conv_dx_small_c_takes(const ConvShape& s);  // conv_igemm.hip: the few-channel form takes the layer (reads w as it is)
bool conv_backward_data_dma(const float* w, const float* dy, float* dx, const ConvShape& s, DxBnSums* bs);  // conv_igemm_dma.hip

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
// conv_direct.hip: dw, dbias += the partials of its kernel and of conv_window.hip's (same layout)
void conv_dw_direct_finalize(const float* partials, int nparts, int groups, int Mg, int K, int MP, int bias_col, float* dw,
                             float* dbias);

// conv_winograd43b.hip: the second form of the F(4x4, 3x3) kernel (whole-tile planes), run by conv_winograd43.hip
void wino43b_run(const float* src, const float* w, float* dst, const ConvShape& s, int dx_mode, ConvStats* stats);
int wino43b_stats_slots(const ConvShape& s);
void wino43b_pack_dims(int J, int M, int* Jpad, int* Mpad);

}  // namespace bcnn_hip
