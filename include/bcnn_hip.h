/*
 * bcnn_hip.h -- C-ABI of the MI355X (gfx950) back-end for bcnn's conv/GEMM hot path.
 *
 * This is the drop-in boundary: a C99 host (bcnn_net / bcnn_node, the reference's own layer code)
 * links against libbcnn_hip.so and calls these entry points where the reference's CUDA build calls
 * its `bcnn_cuda_*` helper family and per-layer `*_gpu` workers. Only plain pointers, ints, floats
 * and size_t cross the boundary; every pointer named `*_d` / documented "device" is HBM memory
 * obtained from bcnn_hip_malloc_*. Unlike the reference helpers, operator entry points take
 * WHOLE-BATCH shapes (one launch per direction, not one cublasSgemm per image).
 *
 * Error convention (reference: src/bcnn_utils.h:174-195): a failing HIP call prints
 * file:line + the HIP error string to stderr and exit()s; entry points therefore return void.
 *
 * Each declaration cites the reference interface it replaces (file:line in jnbraun/bcnn).
 * All tensors: dense NCHW fp32, idx(n,c,h,w) = ((n*C + c)*H + h)*W + w.
 */
#ifndef BCNN_HIP_H
#define BCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum bcnn_activation values (inc/bcnn/bcnn.h:164-175) -- passed as int `act`. */
enum {
    BCNN_HIP_ACT_NONE = 0, BCNN_HIP_ACT_TANH, BCNN_HIP_ACT_RELU, BCNN_HIP_ACT_RAMP,
    BCNN_HIP_ACT_SOFTPLUS, BCNN_HIP_ACT_LRELU, BCNN_HIP_ACT_ABS, BCNN_HIP_ACT_CLAMP,
    BCNN_HIP_ACT_PRELU, BCNN_HIP_ACT_LOGISTIC,
    /* appended, no reference counterpart. RELU6 / HARD_SIGMOID: derivative from the output, accepted by every `act`
     * argument (always as a separate pass, like SOFTPLUS). HARD_SWISH / SWISH / MISH: derivative from the INPUT; forward
     * through bcnn_hip_activation_forward[_keep], backward through bcnn_hip_activation_backward_from_input only; every
     * other `act` argument handed one of them exits. */
    BCNN_HIP_ACT_RELU6, BCNN_HIP_ACT_HARD_SIGMOID, BCNN_HIP_ACT_HARD_SWISH, BCNN_HIP_ACT_SWISH, BCNN_HIP_ACT_MISH
};
/* enum bcnn_mode values (inc/bcnn/bcnn.h:105-112) -- passed as int `mode`. */
enum { BCNN_HIP_MODE_PREDICT = 0, BCNN_HIP_MODE_TRAIN = 1, BCNN_HIP_MODE_VALID = 2 };

/* ---------------------------------------------------------------------------------------------
 * Runtime: device, memory, stream, events.  Replaces src/bcnn_utils.h:197-213 / bcnn_utils.c:101-201
 * (bcnn_cuda_set_device, bcnn_cuda_malloc_f32/i32, bcnn_cuda_memcpy_*, bcnn_cuda_free,
 *  bcnn_cuda_fill_f32) -- no library-global handle singletons, one explicit stream per thread.
 * ------------------------------------------------------------------------------------------- */
int bcnn_hip_device_count(void);
void bcnn_hip_set_device(int id);                 /* bcnn_cuda_set_device, bcnn_utils.c:201 */
int bcnn_hip_get_device(void);
const char *bcnn_hip_device_name(void);           /* gcnArchName of the current device, e.g. "gfx950:..." */
float *bcnn_hip_malloc_f32(size_t n);             /* bcnn_cuda_malloc_f32, bcnn_utils.c:133-140; zero-filled here */
int *bcnn_hip_malloc_i32(size_t n);               /* bcnn_cuda_malloc_i32, bcnn_utils.c:124-131; zero-filled here */
void bcnn_hip_free(void *p_d);                    /* bcnn_cuda_free, bcnn_utils.c:182-185 */
void bcnn_hip_memcpy_h2d(void *dst_d, const void *src_h, size_t bytes); /* bcnn_cuda_memcpy_host2dev */
void bcnn_hip_memcpy_d2h(void *dst_h, const void *src_d, size_t bytes); /* bcnn_cuda_memcpy_dev2host */
void bcnn_hip_memcpy_d2d(void *dst_d, const void *src_d, size_t bytes);
/* bcnn_cuda_fill_f32, bcnn_mat.cu:52-60. A zero of either sign is a memset: value == -0.0f stores +0.0f (all-zero bits);
 * every other value is stored with its own bits. x_d needs float alignment only. */
void bcnn_hip_fill_f32(float *x_d, size_t n, float value);
void bcnn_hip_sync(void);                         /* waits for the calling thread's stream */
/* The stream all entry points launch on (per host thread). NULL = the device's null stream, which
 * is also PyTorch-ROCm's default stream. bcnn_hip_stream_create returns an opaque hipStream_t. */
void *bcnn_hip_stream_create(void);
void bcnn_hip_stream_destroy(void *stream);
void bcnn_hip_set_stream(void *stream);
void *bcnn_hip_get_stream(void);
/* HIP events recorded on the CURRENT stream (used by bench.py for per-kernel durations). */
void *bcnn_hip_event_create(void);
void bcnn_hip_event_destroy(void *ev);
void bcnn_hip_event_record(void *ev);
void bcnn_hip_event_sync(void *ev);
float bcnn_hip_event_elapsed_ms(void *start, void *stop);

/* Per-kernel-class timing (measurement aid, off by default): while enabled every launch of a classified
 * kernel is bracketed by HIP events on the launch stream together with its ALGORITHMIC flops / bytes;
 * read() sums them per class since the last reset(). Classes: bcnn_hip_profile_class_name(i). */
void bcnn_hip_profile_enable(int on);
void bcnn_hip_profile_reset(void);
int bcnn_hip_profile_num_classes(void);
const char *bcnn_hip_profile_class_name(int cls);
void bcnn_hip_profile_read(int cls, double *ms, long long *launches, double *flops, double *bytes);
/* the part of the class's `flops` that is not tile padding (Winograd classes on odd-sized planes; otherwise == flops) */
double bcnn_hip_profile_read_useful_flops(int cls);

/* Dispatch trace (test aid, off by default): while enabled every dispatcher decision of the calling thread appends the name
 * of the kernel family it launched ("wino43_kernel", "wino43_tail_fixup", "wino_fused_kernel", "maxpool_bwd_pair_bn", ...),
 * one per line, so a parity test can assert WHICH kernels produced the tensors it compares instead of assuming the
 * size-dependent dispatch rules. enable(1) clears the log; read() copies at most cap - 1 bytes + a terminating 0 and
 * returns the full length of the log. */
/* Weight gradients on a side stream (per host thread). mode 0: off (default); 1: bcnn_hip_conv_backward* queue the
 * weight-gradient kernels of a layer that also has a data gradient on a private stream and order the caller's stream behind
 * them before returning; 2: ... and do NOT order it: the caller does, with bcnn_hip_conv_side_join(), before anything reads
 * the weight gradients (bcnn_backward: at its end, and before every gradient-ready callback). Returns the previous mode. */
int bcnn_hip_conv_side_stream_mode(int mode);
void bcnn_hip_conv_side_join(void);

void bcnn_hip_trace_enable(int on);
size_t bcnn_hip_trace_read(char *buf, size_t cap);

/* ---------------------------------------------------------------------------------------------
 * BLAS-1 / per-channel helpers.  Replaces bcnn_cuda_axpy/scal/copy (bcnn_mat.cu:44-100),
 * bcnn_cuda_add_bias / bcnn_cuda_grad_bias (bcnn_mat.cu:348-391), bcnn_scales_gpu /
 * bcnn_grad_scales_gpu (bcnn_mat.cu:393-438); CPU semantics bcnn_mat.c:52-115, 319-412, 761-811.
 * Tensor pointers need float alignment only: every helper takes its 16-byte accesses when the pointers it is handed are
 * 16-byte aligned and 4-byte accesses otherwise; the two gradient helpers add the same terms in the same order either
 * way, so a misaligned call gives the bits of the aligned one.
 * ------------------------------------------------------------------------------------------- */
/* y = fl(fl(x*a) + y): the product and the sum are rounded separately (never one fused multiply-add) */
void bcnn_hip_axpy(size_t n, float a, const float *x_d, float *y_d);
/* x *= a; a == 0 stores +0.0f whatever x holds (NaN included), a == 1 touches nothing */
void bcnn_hip_scal(size_t n, float a, float *x_d);
void bcnn_hip_copy_f32(size_t n, const float *x_d, float *y_d);          /* bit copy; x_d == y_d is a no-op */
/* y[b][c][:] += bias[c]; channels whose bias is exactly 0.0f or 1.0f are left untouched, as in
 * the reference AVX build (bcnn_add_scalar, bcnn_mat.c:366-412). */
void bcnn_hip_add_bias(float *y_d, const float *bias_d, int n, int c, int hw);
void bcnn_hip_grad_bias(float *dbias_d, const float *g_d, int n, int c, int hw);  /* dbias[c] += sum */
void bcnn_hip_scales(float *y_d, const float *scales_d, int n, int c, int hw);
void bcnn_hip_grad_scales(const float *x_norm_d, const float *g_d, int n, int c, int hw,
                          float *dscales_d);                                     /* dscales[c] += sum g*x_norm */

/* ---------------------------------------------------------------------------------------------
 * GEMM / im2col / col2im.  Replaces bcnn_cuda_gemm (bcnn_mat.cu:31-42), bcnn_cuda_im2col (:477-524),
 * bcnn_cuda_col2im (:526-576); semantics of bcnn_gemm (bcnn_mat.c:2627-2650), bcnn_im2col (:817-854),
 * bcnn_col2im (:935-970, zero-fills then scatter-adds => OVERWRITES im).
 * Row-major C[m x n] = alpha * op(A) * op(B) + beta * C on the fp32 MFMA path.
 * im2col writes every element of col (zeros for padding); col2im writes every element of im (zeros where no window
 * reaches) and adds a pixel's terms in ascending (kr, kc) order, the order the reference's scatter reaches it in.
 * A shape no window fits in (height + 2 pad < ksize or width + 2 pad < ksize): im2col has no output and touches
 * nothing; col2im reads nothing and zero-fills im, as the reference's does.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_gemm(int trans_a, int trans_b, int m, int n, int k, float alpha, const float *a_d,
                   int lda, const float *b_d, int ldb, float beta, float *c_d, int ldc);
void bcnn_hip_im2col(const float *im_d, int channels, int height, int width, int ksize, int pad,
                     int stride, float *col_d);
void bcnn_hip_col2im(const float *col_d, int channels, int height, int width, int ksize, int pad,
                     int stride, float *im_d);

/* ---------------------------------------------------------------------------------------------
 * Activation map.  Replaces bcnn_forward/backward_activation_gpu (bcnn_activation_layer.cu:32-113);
 * semantics of bcnn_forward_activation_cpu / bcnn_backward_activation_cpu
 * (bcnn_activation_layer.c:90-146, 165-226), incl. softplus/abs/prelu which the CUDA build lacks.
 * In place. `slopes_d` (PReLU, one per channel) may be NULL otherwise. Backward uses the
 * POST-activation values `x_d`; `dslopes_d` accumulates (PReLU only, may be NULL to skip).
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_activation_forward(float *x_d, size_t size, int act, const float *slopes_d,
                                 int spatial, int channels);
void bcnn_hip_activation_backward(const float *x_d, float *dx_d, size_t size, int act,
                                  const float *slopes_d, float *dslopes_d, int spatial, int channels);
/* The self-gated activations (HARD_SWISH, SWISH, MISH; activation.hip), whose derivative needs the input.
 *   forward_keep: one sweep; reads x_d once, stores the input into x_saved_d (may be NULL: nothing is stored) and f(x) in
 *     place. 12 bytes per element with a saved copy, 8 without. Any other activation id is accepted too (its value is
 *     that of bcnn_hip_activation_forward without slopes); PRELU exits.
 *   backward_from_input: one sweep; dx_d *= f'(x_saved_d), 12 bytes per element. Only the three ids above (others exit).
 *   hard_swish: f = (x min(max(x + 3, 0), 6)) / 6, f' = x < -3 ? 0 : x <= 3 ? x / 3 + 0.5 : 1 (torch's choices at the kinks).
 *   swish: f = x s, f' = s (1 + x (1 - s)), s = 1 / (1 + exp(-x)) with exp evaluated in double like LOGISTIC.
 *   mish: f = x tanh(softplus(x)), f' = t + x s (1 - t t), t = tanh(softplus(x)); evaluated in double, rounded once.
 * 16-byte accesses where the bases allow (both bases 16-byte aligned), a scalar route otherwise and for the tail. */
void bcnn_hip_activation_forward_keep(float *x_d, float *x_saved_d, size_t size, int act);
void bcnn_hip_activation_backward_from_input(const float *x_saved_d, float *dx_d, size_t size, int act);

/* ---------------------------------------------------------------------------------------------
 * Batch normalisation.  Replaces bcnn_forward/backward_batchnorm_gpu (bcnn_batchnorm_layer.cu:187-377);
 * semantics of the CPU path (bcnn_batchnorm_layer.c:196-242, 301-332): biased one-pass variance,
 * eps 1e-6 forward / 1e-5 backward, running = 0.9*running + 0.1*batch.
 *   forward : x_d -> y_d (may alias). TRAIN: writes saved_mean/saved_var, updates run_mean/run_var,
 *             keeps the pre-normalisation input in workspace_d (needed by backward; may alias x_d when
 *             x_d != y_d) and, if x_norm_d != NULL, the normalised values. VALID: normalises with the
 *             running statistics. PREDICT: y = x*scale + bias.
 *   backward: dy_d is transformed IN PLACE into the gradient w.r.t. the BN input (as the reference
 *             does) and copied to dx_d if dx_d != NULL && dx_d != dy_d; dbias_d/dscales_d accumulate;
 *             dmean_d/dvar_d (saved_mean.grad / saved_variance.grad) are overwritten.
 *             x_norm_d may be NULL (recomputed from workspace_d, mean, var).
 * `act`/`y_d` in backward: optional fused activation-backward (conv+BN+act nodes): pass the
 * post-activation output and its activation, or act = NONE.
 * Tensor pointers (x_d, y_d, dy_d, dx_d, workspace_d, x_norm_d) must be 16-byte aligned: the statistics and gradient-sum
 * sweeps take their float4 path on hw % 4 == 0 alone (only the elementwise sweeps check the pointers and fall back).
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_batchnorm_forward(const float *x_d, float *y_d, float *run_mean_d, float *run_var_d,
                                const float *scales_d, const float *bias_d, float *saved_mean_d,
                                float *saved_var_d, float *x_norm_d, float *workspace_d, int n, int c,
                                int hw, int mode, int act);
void bcnn_hip_batchnorm_backward(float *dy_d, float *dx_d, const float *y_d, int act,
                                 const float *scales_d, float *dscales_d, float *dbias_d,
                                 const float *saved_mean_d, const float *saved_var_d, float *dmean_d,
                                 float *dvar_d, const float *x_norm_d, const float *workspace_d, int n,
                                 int c, int hw);

/* ---------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on fp32 MFMA; no materialised im2col buffer).
 * Replaces bcnn_forward_conv_layer_gpu / bcnn_backward_conv_layer_gpu (bcnn_conv_layer.c:589-792)
 * with the semantics of the CPU workers (bcnn_conv_layer.c:367-485, 487-587):
 *   - weights [f][c/groups][k][k], bias [f]; out size (h + 2*pad - k)/stride + 1;
 *   - 1x1 kernels read the source as a raw [c/groups][oh*ow] matrix regardless of stride/pad (:445-446);
 *   - forward: y = act(conv + bias) (bias skipped for channels with bias == 0.0f or 1.0f exactly), or
 *     with batch_norm != 0: y = act(BN(conv)) using the bn_* arguments (see batchnorm_forward);
 *   - backward: dy_d <- dy_d * act'(y_d) in place; then BN backward or dbias += sum; dw += (beta = 1);
 *     dx_d (if non-NULL) is OVERWRITTEN (col2im zero-fill semantics); 1x1 writes only the
 *     [c/groups][oh*ow] prefix of each image-group of dx_d.
 * workspace_d: scratch of at least bcnn_hip_conv_workspace_size(...) floats (split-K partials of dw;
 * the reference's per-net conv workspace, bcnn_net.c:337-352, plays the same role).
 * PReLU slopes: slopes_d (one per output channel), else NULL.
 * backward bias_d: the bias the forward pass used (the reference worker has it as node->src[2]); may be
 * NULL. With it the fused batch-norm backward recomputes the forward output from bn_workspace_d bit for
 * bit instead of reading y_d (one full-tensor read less in each of its two passes).
 * x_norm_d is accepted for signature parity with the reference layer and never touched: the normalised
 * values are recomputed from bn_workspace_d, saved_mean_d and saved_var_d.
 * ------------------------------------------------------------------------------------------- */
size_t bcnn_hip_conv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad,
                                    int groups);
void bcnn_hip_conv_forward(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n,
                           int c, int h, int w, int f, int k, int stride, int pad, int groups, int act,
                           const float *slopes_d,
                           /* fused batch-norm (batch_norm == 0: all NULL) */
                           int batch_norm, float *run_mean_d, float *run_var_d, const float *scales_d,
                           float *saved_mean_d, float *saved_var_d, float *x_norm_d,
                           float *bn_workspace_d, int mode);
void bcnn_hip_conv_backward(const float *x_d, const float *w_d, const float *bias_d, const float *y_d,
                            float *dy_d, float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w, int f,
                            int k, int stride, int pad, int groups, int act, const float *slopes_d,
                            float *dslopes_d, int batch_norm, const float *scales_d, float *dscales_d,
                            const float *saved_mean_d, const float *saved_var_d, float *dmean_d,
                            float *dvar_d, const float *x_norm_d, const float *bn_workspace_d,
                            float *workspace_d, size_t workspace_elems);
/* bcnn_hip_conv_forward for inference with the convolution on the bf16 matrix cores: x_d and w_d stay fp32 in memory and
 * are rounded to bf16 (round-to-nearest-even) on their way into the kernel, the accumulator is fp32, and bias, fused
 * batch-norm and activation are the fp32 path's own code. Per output the result differs from bcnn_hip_conv_forward by at
 * most about 2^-8 * sum |x| |w|: NOT the 1e-4 parity of the default path, hence opt-in. mode must be
 * BCNN_HIP_MODE_PREDICT or _VALID (the training-only buffers may be NULL): returns 1 when it ran; 0 for _TRAIN, in
 * which case nothing is launched and nothing is written (the backward pass needs the fp32 forward). No packed copy of
 * the weights is kept between calls. */
int bcnn_hip_conv_forward_bf16(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n, int c, int h,
                               int w, int f, int k, int stride, int pad, int groups, int act, const float *slopes_d,
                               int batch_norm, float *run_mean_d, float *run_var_d, const float *scales_d,
                               float *saved_mean_d, float *saved_var_d, float *x_norm_d, float *bn_workspace_d,
                               int mode);

/* ---------------------------------------------------------------------------------------------
 * A convolution node with batch-norm (no activation) whose output is the first operand of the eltwise node that
 * follows it (the residual block: bcnn_conv_layer.c:367-485 then bcnn_eltwise_layer.c:82-113; backward
 * bcnn_eltwise_layer.c:115-152 then bcnn_conv_layer.c:487-587). For an executor that runs whole passes:
 *   bcnn_hip_conv_residual_fusable   non-zero when the pair below may replace the two workers (TRAIN mode, batch-norm
 *                                    with its pre-normalisation workspace, cheap eltwise activation, aligned tensors)
 *   bcnn_hip_conv_forward_residual   bcnn_hip_conv_forward whose batch-norm apply pass also adds res_d[0 .. res_count)
 *                                    (the reference adds its second operand to the first min_c * h * w elements only)
 *                                    and applies the eltwise activation; the result goes to res_out_d, the
 *                                    convolution node's own output tensor is NOT written (bcnn_hip_batchnorm_apply on
 *                                    bn_workspace_d produces it when somebody asks)
 *   bcnn_hip_conv_backward_residual  the eltwise backward (g = dres_out_d * act'(res_out_d), dres_d[0 .. res_count) += g)
 *                                    and bcnn_hip_conv_backward in one: dres_out_d is read, not rewritten; dy_d receives
 *                                    the batch-norm backward of g as in bcnn_hip_conv_backward. Of res_out_d only the
 *                                    first res_count elements are read: the value act' needs is recomputed from
 *                                    bn_workspace_d, bias_d and res_d with the forward's own operations
 *   bcnn_hip_batchnorm_apply         y = act((x - mean) / sqrtf(var + 1e-6) * scale + bias) with GIVEN statistics: the
 *                                    apply sweep of a TRAIN-mode forward alone, no side effects
 * ------------------------------------------------------------------------------------------- */
int bcnn_hip_conv_residual_fusable(int batch_norm, int act, int res_act, int mode, const float *bn_workspace_d,
                                   const float *res_d, const float *res_out_d);
void bcnn_hip_conv_forward_residual(const float *x_d, const float *w_d, const float *bias_d, int n, int c, int h, int w,
                                    int f, int k, int stride, int pad, int groups, float *run_mean_d, float *run_var_d,
                                    const float *scales_d, float *saved_mean_d, float *saved_var_d,
                                    float *bn_workspace_d, const float *res_d, size_t res_count, int res_act,
                                    float *res_out_d);
void bcnn_hip_conv_backward_residual(const float *x_d, const float *w_d, const float *bias_d, float *dy_d, float *dx_d,
                                     float *dw_d, float *dbias_d, int n, int c, int h, int w, int f, int k, int stride,
                                     int pad, int groups, const float *scales_d, float *dscales_d,
                                     const float *saved_mean_d, const float *saved_var_d, float *dmean_d, float *dvar_d,
                                     const float *bn_workspace_d, float *workspace_d, size_t workspace_elems,
                                     const float *res_out_d, const float *dres_out_d, int res_act, const float *res_d,
                                     float *dres_d, size_t res_count);
void bcnn_hip_batchnorm_apply(const float *x_d, float *y_d, const float *scales_d, const float *bias_d,
                              const float *saved_mean_d, const float *saved_var_d, int n, int c, int hw, int act);

/* Weight packs of a whole pass in one launch, for an executor that knows its layers (bcnn_forward / bcnn_backward).
 * The convolution kernels read the filter bank re-arranged (transformed G g G^T for the Winograd kernels, A^T per tap
 * for the LDS-DMA GEMM); bcnn_hip_conv_forward / _backward make that copy right before their kernel, one small launch
 * per call. bcnn_hip_conv_prepack makes the copies of `count` layers at once -- forward form (data_gradient = 0) or
 * data-gradient form (1) -- into buffers the library keeps; the NEXT forward (resp. backward) call for each of these
 * layers (same weight pointer and shape, this thread, this stream) uses its copy instead of packing again. A copy is
 * used at most once, and a later bcnn_hip_conv_prepack call discards every unused copy, so the caller only has to leave
 * the weights unwritten between the prepack call and the calls that consume it. Layers whose kernel needs no copy are
 * skipped. bcnn_hip_conv_prepack_reset frees the buffers (synchronises the device). */
typedef struct {
    const float *w_d;
    int n, c, h, w, f, k, stride, pad, groups;
} bcnn_hip_conv_desc;
void bcnn_hip_conv_prepack(const bcnn_hip_conv_desc *layers, int count, int data_gradient);
void bcnn_hip_conv_prepack_reset(void);
/* every copy made so far and not consumed is stale from here on (end of a pass: the weights may be rewritten next) */
void bcnn_hip_conv_prepack_discard(void);

/* ---------------------------------------------------------------------------------------------
 * Pooling.  Replaces bcnn_forward/backward_maxpool_layer_gpu (bcnn_maxpool_layer.cu:28-166) and
 * bcnn_forward/backward_avgpool_layer_gpu (bcnn_avgpool_layer.cu:29-90); CPU semantics
 * bcnn_maxpool_layer.c:145-191, 258-273 and bcnn_avgpool_layer.c:82-125.
 *   maxpool: window at (i*stride, j*stride) (bottom/right padding only), rows outer / cols inner,
 *   first strict maximum wins, NaN never wins, indexes = flat int32 offset into the whole source
 *   tensor -- BIT-EXACT with the CPU path. backward: dx[indexes[o]] += dy[o], applied in ascending
 *   output order per source element (deterministic, same order as the CPU loop). overwrite != 0:
 *   the caller guarantees dx is semantically all-zero (it skipped the zero fill of bcnn_net.c:361-375
 *   because this node is the tensor's only gradient writer): dx is assigned 0 + the same sums.
 *   avgpool: global mean per (n,c); backward dx += dy/(h*w).
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_maxpool_forward(const float *x_d, float *y_d, int *indexes_d, int n, int c, int h, int w,
                              int out_h, int out_w, int size, int stride);
void bcnn_hip_maxpool_backward(const float *dy_d, const int *indexes_d, float *dx_d, int n, int c,
                               int h, int w, int out_h, int out_w, int size, int stride, int overwrite);
/* A 1x1 convolution node whose input is the output of a stand-alone batch-norm node (MobileNet: [batchnorm] -> [conv 1x1]).
 * bcnn_hip_conv_backward_bnsums is bcnn_hip_conv_backward whose data-gradient kernel also emits, from the tile it stores,
 * the per-channel partial sums the batch-norm node's backward starts with (S1 = sum dz, S2 = sum dz * (prev_y - prev_mean),
 * bcnn_batchnorm_layer.c:263-281; prev_y_d = that node's INPUT, prev_mean_d its saved mean) into sums_d
 * (bcnn_hip_conv_bnsums_size floats). Returns the number of partials per channel, 0 when this shape's kernel does not
 * emit them (then run bcnn_hip_batchnorm_backward_sums). bcnn_hip_batchnorm_backward_finalize turns the partials into
 * dbias / dscales (accumulated) and dmean / dvar (written), like the finalize step of bcnn_hip_batchnorm_backward_sums. */
size_t bcnn_hip_conv_bnsums_size(int n, int c, int h, int w);
int bcnn_hip_conv_backward_bnsums(const float *x_d, const float *w_d, const float *bias_d, const float *y_d, float *dy_d,
                                  float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w, int f, int k,
                                  int stride, int pad, int groups, int act, const float *slopes_d, float *dslopes_d,
                                  int batch_norm, const float *scales_d, float *dscales_d, const float *saved_mean_d,
                                  const float *saved_var_d, float *dmean_d, float *dvar_d, const float *x_norm_d,
                                  const float *bn_workspace_d, float *workspace_d, size_t workspace_elems,
                                  const float *prev_y_d, const float *prev_mean_d, float *sums_d, size_t sums_floats);
/* The other direction of the same idea, for a convolution node with batch-norm whose output feeds a depthwise node that
 * reads its pre-normalisation tensor (bcnn_hip_depthwise_backward_bnin / _bn_bnin below): that depthwise kernel writes the
 * gradient of the convolution node's OUTPUT and holds the pre-normalisation values it belongs to, so
 * bcnn_hip_depthwise_backward_bnin_sums (bn_mean_d == NULL: no batch-norm node behind the depthwise node, dy_d is updated
 * in place; else dy_d is that node's output gradient, read only) also leaves S1 = sum g, S2 = sum g * (raw - mean) with
 * g = dx * act'(act(bn(raw))) per channel in in_sums_d (bcnn_hip_depthwise_insums_size floats) and returns the number of
 * partials per channel (0: not emitted -- overwrite == 0, or the buffer is too small). bcnn_hip_conv_backward_presummed is
 * bcnn_hip_conv_backward_bnsums (prev_* may be NULL) that takes those partials (own_sums_d, own_splits > 0) instead of
 * sweeping (dy, pre-normalisation tensor) for them; with own_splits == 0 it is bcnn_hip_conv_backward_bnsums.
 * bcnn_hip_depthwise_insums_size is the most any kernel that may take the shape writes: a non-zero size does NOT say that the
 * layer is fusable (a kernel that wants aligned tensors counts towards it); ask bcnn_hip_depthwise_bnin_fusable for that. */
size_t bcnn_hip_depthwise_insums_size(int n, int c, int h, int w, int k, int stride, int pad);
int bcnn_hip_depthwise_backward_bnin_sums(const float *x_raw_d, const float *w_d, const float *y_d, float *dy_d, float *dx_d,
                                          float *dw_d, float *dbias_d, int n, int c, int h, int w, int k, int stride, int pad,
                                          int act, int overwrite, const float *bn_mean_d, const float *bn_var_d,
                                          const float *bn_scales_d, const float *bn_dmean_d, const float *bn_dvar_d,
                                          const float *in_mean_d, const float *in_var_d, const float *in_scale_d,
                                          const float *in_bias_d, int in_act, float *in_sums_d, size_t in_sums_floats);
int bcnn_hip_conv_backward_presummed(const float *x_d, const float *w_d, const float *bias_d, const float *y_d, float *dy_d,
                                     float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w, int f, int k,
                                     int stride, int pad, int groups, int act, const float *slopes_d, float *dslopes_d,
                                     int batch_norm, const float *scales_d, float *dscales_d, const float *saved_mean_d,
                                     const float *saved_var_d, float *dmean_d, float *dvar_d, const float *x_norm_d,
                                     const float *bn_workspace_d, float *workspace_d, size_t workspace_elems,
                                     const float *own_sums_d, int own_splits, const float *prev_y_d,
                                     const float *prev_mean_d, float *prev_sums_d, size_t prev_sums_floats);
void bcnn_hip_batchnorm_backward_finalize(const float *sums_d, int splits, const float *scales_d, float *dscales_d,
                                          float *dbias_d, const float *saved_var_d, float *dmean_d, float *dvar_d, int c);

/* The pooling node behind a convolution node with batch-norm (the ResNet stem), for an executor that runs whole passes:
 * bcnn_hip_maxpool_forward over act(batch-norm(x_d)) computed on the fly from the convolution node's pre-normalisation
 * output and saved statistics -- the values, scan order and indexes of bcnn_hip_batchnorm_apply followed by
 * bcnn_hip_maxpool_forward, without writing and re-reading the normalised tensor. Ask bcnn_hip_maxpool_bn_fusable
 * (stride 2, size 2 or 3, w % 4 == 0, cheap activation). bcnn_hip_conv_forward_stats_only is the convolution node's part:
 * bcnn_hip_conv_forward (batch-norm, TRAIN mode) up to and including the batch statistics, without the apply sweep. */
void bcnn_hip_conv_forward_stats_only(const float *x_d, const float *w_d, const float *bias_d, int n, int c, int h, int w,
                                      int f, int k, int stride, int pad, int groups, float *run_mean_d, float *run_var_d,
                                      const float *scales_d, float *saved_mean_d, float *saved_var_d,
                                      float *bn_workspace_d);
int bcnn_hip_maxpool_bn_fusable(int n, int c, int h, int w, int out_h, int out_w, int size, int stride, int act,
                                const float *x_d);
void bcnn_hip_maxpool_forward_bn(const float *x_d, float *y_d, int *indexes_d, int n, int c, int h, int w, int out_h,
                                 int out_w, int size, int stride, const float *scales_d, const float *bias_d,
                                 const float *saved_mean_d, const float *saved_var_d, int act);
/* ... and its backward. bcnn_hip_maxpool_forward_bn_keep is bcnn_hip_maxpool_forward_bn that also keeps, per pooled
 * element, the pre-normalisation value that won its window (raw_at_max_d, the pooled shape). With it
 * bcnn_hip_maxpool_bn_backward does the pooling node's backward AND the convolution node's batch-norm backward in a sweep
 * over the pooled tensors plus ONE sweep over the un-pooled ones: the sums S1, S2 of bcnn_batchnorm_layer.c:263-281 are
 * taken over (dpool_d, raw_at_max_d) -- the un-pooled gradient is zero except at the winning places, where it is the sum
 * of the pooled gradients that selected them -- into dscales_d / dbias_d (accumulated) and dmean_d / dvar_d (written),
 * and one kernel then gathers each un-pooled gradient value like bcnn_hip_maxpool_backward (overwrite form) and applies
 * :292-296 to it in registers, writing dx_d = the gradient of the convolution's PRE-NORMALISATION output (what
 * bcnn_hip_conv_backward leaves in dy_d after its batch-norm step). bcnn_hip_conv_backward_bn_done is the rest of that
 * node's backward: weight gradient and, if dx_d != NULL, data gradient from such a dy_d (no bias gradient: the bias of a
 * batch-norm convolution is the batch-norm's). Ask bcnn_hip_maxpool_bn_backward_fusable (3x3 / stride 2, out_w == w / 2,
 * cheap activation, aligned pointers; raw_d = the convolution's pre-normalisation output). */
void bcnn_hip_maxpool_forward_bn_keep(const float *x_d, float *y_d, int *indexes_d, int n, int c, int h, int w, int out_h,
                                      int out_w, int size, int stride, const float *scales_d, const float *bias_d,
                                      const float *saved_mean_d, const float *saved_var_d, int act, float *raw_at_max_d);
int bcnn_hip_maxpool_bn_backward_fusable(int n, int c, int h, int w, int out_h, int out_w, int size, int stride, int act,
                                         const float *raw_d, const float *dpool_d, const int *indexes_d, const float *dx_d);
void bcnn_hip_maxpool_bn_backward(const float *dpool_d, const int *indexes_d, const float *raw_at_max_d, const float *raw_d,
                                  float *dx_d, int n, int c, int h, int w, int out_h, int out_w, int size, int stride,
                                  const float *scales_d, float *dscales_d, const float *bias_d, float *dbias_d,
                                  const float *saved_mean_d, const float *saved_var_d, float *dmean_d, float *dvar_d, int act);
void bcnn_hip_conv_backward_bn_done(const float *x_d, const float *w_d, float *dy_d, float *dx_d, float *dw_d, int n, int c,
                                    int h, int w, int f, int k, int stride, int pad, int groups, float *workspace_d,
                                    size_t workspace_elems);
void bcnn_hip_avgpool_forward(const float *x_d, float *y_d, int n, int c, int h, int w);
void bcnn_hip_avgpool_backward(const float *dy_d, float *dx_d, int n, int c, int h, int w);

/* ---------------------------------------------------------------------------------------------
 * Windowed pooling with symmetric padding (the pool2d node; pool2d.hip). No reference counterpart: the semantics are
 * those of torch.nn.functional.max_pool2d / avg_pool2d, which are Caffe's. The two nodes above are untouched by it.
 *   A square window of `size`, `stride` apart, with `pad` (0 <= pad <= size / 2) on all four sides. Output extent per
 *   axis: out = floor_or_ceil((in + 2 pad - size) / stride) + 1 and, in ceil mode, out - 1 if (out - 1) stride >= in + pad
 *   (the last window starts inside the input or its leading padding). bcnn_hip_pool2d_out_extent returns it, or 0 for a
 *   parameter set that is refused: kind unknown, size < 1, stride < 1, pad < 0, pad > size / 2, in < 1, in + 2 pad < size.
 *   Window (i, j) covers rows i stride - pad .. + size - 1 and the same columns, clipped to the input.
 *   max: rows outer / columns inner, replace only on `>` (first maximum wins, a NaN never wins, padding never wins);
 *     indexes_d = int32 flat offset into the whole source tensor, the format of bcnn_hip_maxpool_forward; it may be NULL
 *     (PREDICT: nothing is stored). average: sum of the real elements / divisor (a true division), divisor =
 *     (min(hstart + size, h + pad) - hstart) (min(wstart + size, w + pad) - wstart) with count_include_pad, else the
 *     number of real elements; indexes_d is ignored.
 *   backward: gather form, one thread per source element (or four), the covering windows in ascending output order, no
 *     atomics: dx += dy[o] where indexes_d[o] selects the element (max), dx += dy[o] / divisor(o) (average).
 *     overwrite != 0: the caller guarantees dx is semantically all-zero (this node is the gradient's only writer and the
 *     zero fill was skipped): dx = 0 + the same sums, and an element no window covers (stride > size) becomes 0; with
 *     overwrite == 0 such an element keeps its value.
 *   Tensors of 2^31 elements or more do not fit the index format; the two workers exit on them as on refused parameters.
 * ------------------------------------------------------------------------------------------- */
enum { BCNN_HIP_POOL2D_MAX = 0, BCNN_HIP_POOL2D_AVG = 1 };
typedef struct bcnn_hip_pool2d_desc {
    int kind;              /* BCNN_HIP_POOL2D_MAX / _AVG */
    int size, stride, pad;
    int ceil_mode;         /* 0: floor */
    int count_include_pad; /* average only */
} bcnn_hip_pool2d_desc;
int bcnn_hip_pool2d_out_extent(const bcnn_hip_pool2d_desc *desc, int in);
void bcnn_hip_pool2d_forward(const bcnn_hip_pool2d_desc *desc, const float *x_d, float *y_d, int *indexes_d, int n, int c,
                             int h, int w);
void bcnn_hip_pool2d_backward(const bcnn_hip_pool2d_desc *desc, const float *dy_d, const int *indexes_d, float *dx_d, int n,
                              int c, int h, int w, int overwrite);

/* ---------------------------------------------------------------------------------------------
 * Bilinear interpolation to a given extent (the interp node; interp.hip). No reference counterpart: the semantics are
 * those of torch.nn.functional.interpolate(mode="bilinear", size=(out_h, out_w)) for both values of align_corners.
 *   Per axis, input extent I, output extent O, output index o, all in float32 and every operation rounded on its own
 *   (csrc/interp_rule.h is the one definition; host and device share it):
 *     align_corners != 0: s = O > 1 ? (float)(I - 1) / (float)(O - 1) : 0;  src = s * (float)o
 *     align_corners == 0: s = (float)I / (float)O;  src = max(s * ((float)o + 0.5f) - 0.5f, 0)
 *     i0 = min((int)src, I - 1);  i1 = i0 + (i0 < I - 1);  l1 = clamp(src - (float)i0, 0, 1);  l0 = 1 - l1
 *   forward : y = h0 * (w0 * x[y0][x0] + w1 * x[y0][x1]) + h1 * (w0 * x[y1][x0] + w1 * x[y1][x1]) in this association
 *     (h*: the row weights l0 / l1, w*: the column weights). Every element of y is written.
 *   backward: gather form, one thread per source element, no atomics, the same bits on every run: dx += the sum of
 *     h * (w * dy) over every (output row, output column, row tap, column tap) that names the element, output rows and
 *     columns ascending, tap 0 before tap 1. overwrite != 0: the caller guarantees dx is semantically all-zero (this node
 *     is the gradient's only writer and the zero fill was skipped): dx = 0 + the same sums, and an element no output
 *     names (downsampling) becomes 0; with overwrite == 0 such an element keeps its bits.
 *   bcnn_hip_interp_axis_taps: host only, needs no device: i0[o], i1[o], l1[o] for o in [0, out) by the same rule.
 *   Tensors of 2^31 elements or more, and extents below 1, exit like the other entry points handed a shape they cannot run.
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_interp_desc {
    int out_h, out_w;
    int align_corners; /* 0: half-pixel centres (torch's default) */
} bcnn_hip_interp_desc;
void bcnn_hip_interp_forward(const bcnn_hip_interp_desc *desc, const float *x_d, float *y_d, int n, int c, int h, int w);
void bcnn_hip_interp_backward(const bcnn_hip_interp_desc *desc, const float *dy_d, float *dx_d, int n, int c, int h, int w,
                              int overwrite);
void bcnn_hip_interp_axis_taps(int in, int out, int align_corners, int *i0, int *i1, float *l1);

/* ---------------------------------------------------------------------------------------------
 * Softmax over the channels + cross-entropy against a class-index label map (the softmax-loss node; softmax_loss.hip).
 * No reference counterpart: torch's F.cross_entropy(x, t, ignore_index=...) with three normalisers.
 *   x, p, dx are [n][c][hw]; label is [n][1][hw], class indices stored as floats. One label value t is (the one definition
 *   is csrc/softmax_loss_rule.h, shared by host and device):
 *     ignored       ignore_label >= 0 and t == (float)ignore_label
 *     valid         t is an integer value in [0, c)
 *     out of range  anything else (negative, >= c, fractional, not finite): contributes like an ignored pixel, is counted
 *                   on its own, never indexes memory
 *   forward : p = softmax over c of x (float arithmetic, one reciprocal per pixel). With label_d and record_d:
 *     l = log(sum_c exp(x_c - max)) - (x_t - max) per valid pixel, V = the number of valid pixels,
 *     D = 1 (norm 0, NONE), max(V, 1) (norm 1, VALID) or max(V, 1) / n (norm 2, VALID_PER_IMAGE),
 *     record = {(sum l) / D, scale / D, V, ignored, out of range, valid pixels whose first argmax of x is t}.
 *     The sums are per-workgroup partials (l in double) added in a fixed order by a finalize kernel: no host
 *     synchronisation, no floating-point atomics, the same bits on every run. label_d or record_d NULL: p only.
 *   backward: dx += record.grad_factor * (p - [c == t]) on valid pixels; the elements of every other pixel keep their bits.
 *     overwrite != 0: the caller guarantees dx is semantically all-zero: dx = the same values, +0.0 on the other pixels.
 *     Reads the record on the device: nothing is read back on the host between forward and backward.
 *   confusion: counts_d[t * c + a] (c * c unsigned, zeroed by the call) = valid pixels with label t whose first argmax
 *     of p is a. Not on the training path; integer atomics.
 *   16-byte accesses when hw % 4 == 0 and the tensors of the call are 16-byte aligned, 4-byte accesses otherwise. The
 *   forward's dispatch is a function of (c, hw, alignment) alone; bcnn_hip_softmax_loss_c_reg() is the largest c whose
 *   logits the pixel kernels hold in registers. Tensors of 2^31 elements or more, an ignore label of 2^24 or more and an
 *   unknown normaliser exit like the other entry points handed arguments they cannot run.
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_softmax_loss_desc {
    int ignore_label; /* negative: no label is ignored on purpose */
    int norm;         /* 0 none, 1 valid, 2 valid per image (bcnn_loss_norm of include/bcnn/bcnn.h) */
    float scale;
} bcnn_hip_softmax_loss_desc;
typedef struct bcnn_hip_softmax_loss_record {
    float loss;        /* (sum l) / D */
    float grad_factor; /* scale / D */
    int valid, ignored, out_of_range, correct;
} bcnn_hip_softmax_loss_record;
void bcnn_hip_softmax_loss_forward(const bcnn_hip_softmax_loss_desc *desc, const float *x_d, const float *label_d, float *p_d,
                                   bcnn_hip_softmax_loss_record *record_d, int n, int c, int hw);
void bcnn_hip_softmax_loss_backward(const bcnn_hip_softmax_loss_desc *desc, const float *p_d, const float *label_d,
                                    const bcnn_hip_softmax_loss_record *record_d, float *dx_d, int n, int c, int hw,
                                    int overwrite);
void bcnn_hip_softmax_loss_confusion(const bcnn_hip_softmax_loss_desc *desc, const float *p_d, const float *label_d,
                                     unsigned *counts_d, int n, int c, int hw);
int bcnn_hip_softmax_loss_c_reg(void);

/* ---------------------------------------------------------------------------------------------
 * Label maps at each image's own size (label_map.hip). No reference counterpart: the output end of semantic
 * segmentation, as bcnn_hip_yolo_detect_batch is the detector's. From x_d, [n][c][h][w] on the device (logits or
 * probabilities: the call resamples what it is given), image b of the call gets one class index per pixel of ITS extent:
 *   a rectangle (roi_x, roi_y, roi_w, roi_h) of plane b is resampled bilinearly to out_w x out_h -- the interp node's rule
 *   (csrc/interp_rule.h) applied to the rectangle as if it were a tensor of that extent, the same float32 association,
 *   so every value is, bit for bit, what bcnn_hip_interp_forward writes for the cropped rectangle -- and the label is the
 *   FIRST maximum over the classes (start at class 0, replace on strict >; a NaN never wins and a NaN at class 0 is never
 *   replaced). The resampled c x out_h x out_w floats are never stored. The one definition is csrc/label_map_rule.h.
 *   label_map_fit (host only, no device needed): the rectangle of an iw x ih image in the W x H plane for a fit of
 *     BCNN_HIP_IMAGE_FIT_*: the whole plane (STRETCH) or the letterbox geometry of bcnn_hip_fill_images, (x_off, y_off,
 *     new_w, new_h). 1 with *out untouched: out NULL, an extent below 1, an unknown fit, a letterbox extent of 0.
 *   label_maps_plan (host only): the layout of the result block the call stages -- image b's labels are out_h rows of
 *     row_strides[b] = round_up(out_w, 4) bytes at offsets[b], every image on a 16-byte boundary, *total_bytes in all
 *     (each output may be NULL). The truths of an evaluating call are staged in a second block of the same layout. 1 with
 *     nothing written: what label_maps_batch refuses about imgs, num_images (< 1), c, h, w, or a total -- doubled when
 *     with_truths != 0 -- past 2^31 bytes.
 *   label_maps_batch: labels[b] (host) receives out_h rows of out_w bytes, label_strides[b] bytes apart (label_strides
 *     NULL: out_w); bytes between out_w and the stride are not written. labels may be NULL when truths are given.
 *     truths[b] (host, same extents, truth_strides likewise) turns the call into an evaluation: a truth byte t is ignored
 *     (ignore_label >= 0 and t == ignore_label), valid (t < c) or out of range (csrc/softmax_loss_rule.h on (float)t);
 *     a valid pixel with label a adds 1 to counts[t * c + a]. counts (c * c), *ignored and *out_of_range (either may be
 *     NULL) are ADDED into, so that a validation set accumulates over its batches. Integer atomics only: two runs give
 *     the same counts.
 *     One host-to-device copy (descriptors, truths), one kernel for the whole batch whatever the image sizes, one
 *     device-to-host copy (label bytes, counts), one synchronise of the calling thread's stream: the outputs are complete
 *     when the call returns.
 *     Returns 1, with every output untouched and nothing queued, for: x_d or imgs NULL; n < 1; num_images < 1 or > n;
 *     c < 1 or > 256; h or w < 1; an output extent < 1; a rectangle that is empty or leaves the plane; labels and truths
 *     both NULL; a NULL labels[b] / truths[b]; a stride below out_w; truths without counts; ignore_label >= 256 (no byte
 *     equals it; negative: nothing is ignored); a plane of more than 2^30 elements; a total past 2^31 bytes.
 *   label_maps_kernel_ms (measurement only): enable != 0 makes the later calls of this thread bracket their kernel with
 *     two device events -- the call is synchronous, so events recorded around it span its copies too; returns the kernel
 *     time of the latest bracketed call in milliseconds (-1: none yet).
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_label_map_image {
    int out_w, out_h, roi_x, roi_y, roi_w, roi_h;
} bcnn_hip_label_map_image;
int bcnn_hip_label_map_fit(int fit, int W, int H, int iw, int ih, bcnn_hip_label_map_image *out);
int bcnn_hip_label_maps_plan(const bcnn_hip_label_map_image *imgs, int num_images, int c, int h, int w, int with_truths,
                             unsigned *row_strides, unsigned long long *offsets, unsigned long long *total_bytes);
int bcnn_hip_label_maps_batch(const float *x_d, int n, int c, int h, int w, int align_corners,
                              const bcnn_hip_label_map_image *imgs, int num_images, uint8_t *const *labels,
                              const int *label_strides, const uint8_t *const *truths, const int *truth_strides,
                              int ignore_label, long long *counts, long long *ignored, long long *out_of_range);
float bcnn_hip_label_maps_kernel_ms(int enable);

/* ---------------------------------------------------------------------------------------------
 * Channel scaling (the scale-channels node; scale_channels.hip). No reference counterpart.
 *   x is [n][c][hw]; gate is [n][c] (same_shape == 0: one factor per plane) or [n][c][hw] (same_shape != 0).
 *   forward : y = x * gate, one multiply per element (8 bytes per element moved, 12 with a same-shape gate).
 *   backward: ONE sweep over (x, dy[, gate]): dx += dy * gate, and dgate[n][c] += sum over the plane of dy * x
 *     (dgate += dy * x elementwise for the same-shape gate). dx_d or dgate_d may be NULL: that half is skipped and what
 *     only it needs is not read. The plane sums use no atomics: each plane is cut into a fixed number of slices by the
 *     shape alone, a slice is summed by one wave or one workgroup in a fixed order, and the slice sums are added in
 *     ascending order (in double) -- two runs give the same bits.
 *   Tensors of 2^31 elements or more exit, like the other entry points handed a shape they cannot run.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_scale_channels_forward(const float *x_d, const float *gate_d, float *y_d, int n, int c, int hw,
                                     int same_shape);
void bcnn_hip_scale_channels_backward(const float *x_d, const float *gate_d, const float *dy_d, float *dx_d,
                                      float *dgate_d, int n, int c, int hw, int same_shape);

/* ---------------------------------------------------------------------------------------------
 * Group normalisation (the group-norm node; group_norm.hip). No reference counterpart. Layer norm over (C,H,W) is
 * groups == 1, instance norm groups == c.
 *   x is [n][c][hw]; gamma, beta are [c]; mean, rstd are [n * groups]. Group g of image n is the contiguous row of
 *   m = (c / groups) * hw floats at row n * groups + g; element i of it has channel ch = g * (c / groups) + i / hw.
 *   forward : mean and the biased variance of every row (float32 sums of x and x^2 in a fixed order, combined and
 *     finalised in double), rstd = (float)(1 / sqrt(var + eps)); xh = (x - mean) * rstd; y = xh * gamma[ch] + beta[ch] with
 *     the float32 mean and rstd, one float32 rounding per operation: y is the bits of that expression. mean_d / rstd_d
 *     may be NULL (nothing is stored).
 *   backward: takes mean and rstd and recomputes xh. t = dy * gamma[ch]; ds = sum_m t * xh; db = sum_m t;
 *     dxv = (t - (xh * ds + db) / m) * rstd; dx = dxv (overwrite != 0) or dx + dxv. dgamma[ch] += sum_n sum_hw dy * xh,
 *     dbeta[ch] += sum_n sum_hw dy: plane sums added over n in ascending order in double, the start value enters as one
 *     float32 addition. Each of dx_d, dgamma_d, dbeta_d may be NULL: that output is skipped.
 *   No atomics; the order of every sum follows from the shape alone: two runs give the same bits.
 *   bcnn_hip_group_norm_path: the kernel family the shape runs on, 0 lanes (rows of up to 1024 floats: a group of lanes
 *     per row), 1 resident (one workgroup keeps the row in LDS: up to 16128 floats forward, 8064 backward), 2 split
 *     (slices, a finalize kernel, a map sweep); -1 for a shape the workers refuse. With the dispatch trace on, every
 *     launch is named group_norm_fwd:<path> / group_norm_bwd:<path>, the parameter-gradient kernel group_norm_bwd:params:
 *     forward 1 launch (split 3), backward at most 2 (split 4).
 *   groups <= 0, groups that do not divide c and tensors of 2^31 elements or more exit.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_group_norm_forward(const float *x_d, const float *gamma_d, const float *beta_d, float *y_d, float *mean_d,
                                 float *rstd_d, int n, int c, int hw, int groups, float eps);
void bcnn_hip_group_norm_backward(const float *x_d, const float *gamma_d, const float *mean_d, const float *rstd_d,
                                  const float *dy_d, float *dx_d, float *dgamma_d, float *dbeta_d, int n, int c, int hw,
                                  int groups, int overwrite);
int bcnn_hip_group_norm_path(int n, int c, int hw, int groups, int backward);

/* ---------------------------------------------------------------------------------------------
 * Depthwise convolution.  Replaces the kernels of bcnn_depthwise_conv_layer.cu:33-200; CPU semantics
 * bcnn_depthwise_conv_layer.c:165-293, 295-547: weights [c][k][k]; y = act(dwconv + bias);
 * backward: dy *= act'(y) in place, dbias += ..., and ONLY IF dx_d != NULL: dw += ..., dx += ...
 * (accumulating, no zero-fill). No unsynchronised `+=` races (the CUDA kernel at :113 has one).
 * overwrite != 0 (same contract as bcnn_hip_maxpool_backward): the caller guarantees dx is semantically all-zero
 * (it skipped the executor's zero fill because this node is the tensor's only gradient writer): dx is assigned
 * 0 + the same sums, without being read.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_depthwise_forward(const float *x_d, const float *w_d, const float *bias_d, float *y_d,
                                int n, int c, int h, int w, int k, int stride, int pad, int act);
void bcnn_hip_depthwise_backward(const float *x_d, const float *w_d, const float *y_d, float *dy_d,
                                 float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w,
                                 int k, int stride, int pad, int act, int overwrite);

/* ---------------------------------------------------------------------------------------------
 * A depthwise layer whose output feeds a stand-alone batch-norm node (the MobileNet block, reference
 * examples/... mobilenet configs: [depthwise-conv] -> [batchnorm] -> [conv 1x1]). The reference runs the two nodes'
 * workers back to back (bcnn_depthwise_conv_layer.c:165-293 then bcnn_batchnorm_layer.c:196-242; backward
 * bcnn_batchnorm_layer.c:301-332 then bcnn_depthwise_conv_layer.c:295-547); these entry points let an executor that
 * runs whole passes share work between the two workers. Results are those of the separate calls (forward, dx: the
 * same operations in the same order; statistics and gradient sums: fixed-order two-level sums).
 *   bcnn_hip_depthwise_stats_size      floats the statistics scratch of this layer shape needs; 0 = this shape's
 *                                      forward kernel emits no statistics. The most any kernel that may take the shape
 *                                      writes: a non-zero size promises neither statistics (the return value of
 *                                      bcnn_hip_depthwise_forward_stats does) nor that the layer is fusable
 *   bcnn_hip_depthwise_forward_stats   bcnn_hip_depthwise_forward that also leaves per-channel partial sums
 *                                      (sum, sum of squares of y) in stats_d; returns the number of partials per
 *                                      channel, 0 when none were written
 *   bcnn_hip_batchnorm_forward_stats   bcnn_hip_batchnorm_forward (TRAIN mode) that takes those partials instead of
 *                                      reading x_d for its statistics (splits == 0: plain bcnn_hip_batchnorm_forward)
 *   bcnn_hip_depthwise_bn_fusable      non-zero when bcnn_hip_depthwise_backward_bn handles this layer, whatever the
 *                                      alignment of the tensors it is then given. (A layer only the kernels that want
 *                                      16- / 8- / 4-byte aligned tensors could take -- planes of a few columns and
 *                                      hundreds of rows -- is not fusable; nor is one whose LDS tile does not fit: 2 rows
 *                                      of 476 to 511 columns at stride 1.) bcnn_hip_depthwise_backward_bn ends the
 *                                      process on a layer this refuses.
 *   bcnn_hip_batchnorm_backward_sums   first half of bcnn_hip_batchnorm_backward: dbias / dscales accumulate, dmean /
 *                                      dvar are written; dy_d is NOT rewritten (x_d: the batch-norm input)
 *   bcnn_hip_batchnorm_backward_apply  second half of bcnn_hip_batchnorm_backward alone (dmean / dvar from the first):
 *                                      dy_d rewritten in place and copied to dx_d -- what the executor runs when a
 *                                      caller asks for a gradient tensor the fused pass did not have to write
 *   bcnn_hip_depthwise_backward_bn     bcnn_hip_depthwise_backward on g = BNbackward(dz_d) (second half of
 *                                      bcnn_hip_batchnorm_backward, bcnn_batchnorm_layer.c:292-296, applied on the fly);
 *                                      neither dz_d nor the depthwise output gradient is written
 * ------------------------------------------------------------------------------------------- */
size_t bcnn_hip_depthwise_stats_size(int n, int c, int h, int w, int k, int stride, int pad);
int bcnn_hip_depthwise_forward_stats(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n, int c,
                                     int h, int w, int k, int stride, int pad, int act, float *stats_d,
                                     size_t stats_floats);
void bcnn_hip_batchnorm_forward_stats(const float *x_d, float *y_d, float *run_mean_d, float *run_var_d,
                                      const float *scales_d, const float *bias_d, float *saved_mean_d,
                                      float *saved_var_d, float *x_norm_d, float *workspace_d, int n, int c, int hw,
                                      int mode, int act, const float *stats_d, int splits);
/* A stand-alone batch-norm node (no activation) whose only consumer is a 1x1 / stride 1 / one-group convolution with its own
 * fused batch-norm, TRAIN mode (MobileNet: [depthwise] -> [batchnorm] -> [conv 1x1 + BN]): z = a y + b per channel, so
 * W z = (W diag(a)) y + W b and the batch-norm's apply sweep (bcnn_batchnorm_layer.c:226-241) folds into the GEMM.
 *   bcnn_hip_batchnorm_forward_stats_only  the batch-norm node's part: saved and running statistics, nothing written
 *   bcnn_hip_conv_bnfold_fusable           1: the convolution's kernels take the folded form for this shape
 *   bcnn_hip_conv_set_input_bnfold         announces, to the NEXT bcnn_hip_conv_forward* / bcnn_hip_conv_backward* call of
 *                                          this thread (which consumes it), that its x_d is the batch-norm's INPUT y and
 *                                          the batch-norm is (mean, var, scales, bias): forward packs W diag(a) and shifts
 *                                          only the running mean of the convolution's own batch-norm by W b (the stored
 *                                          pre-normalisation values are W diag(a) y: every later use subtracts the batch
 *                                          mean); backward returns (dy y^T) diag(a) as the weight gradient. */
void bcnn_hip_batchnorm_forward_stats_only(const float *x_d, float *run_mean_d, float *run_var_d, const float *scales_d,
                                           const float *bias_d, float *saved_mean_d, float *saved_var_d, int n, int c,
                                           int hw, const float *stats_d, int splits);
int bcnn_hip_conv_bnfold_fusable(int n, int c, int h, int w, int f);
void bcnn_hip_conv_set_input_bnfold(const float *mean_d, const float *var_d, const float *scales_d, const float *bias_d);
int bcnn_hip_depthwise_bn_fusable(int n, int c, int h, int w, int k, int stride, int pad, int act);
void bcnn_hip_batchnorm_backward_sums(const float *dy_d, const float *scales_d, float *dscales_d, float *dbias_d,
                                      const float *saved_mean_d, const float *saved_var_d, float *dmean_d,
                                      float *dvar_d, const float *x_d, int n, int c, int hw);
void bcnn_hip_batchnorm_backward_apply(float *dy_d, float *dx_d, const float *scales_d, const float *saved_mean_d,
                                       const float *saved_var_d, const float *dmean_d, const float *dvar_d,
                                       const float *x_d, int n, int c, int hw);
void bcnn_hip_depthwise_backward_bn(const float *x_d, const float *w_d, const float *y_d, const float *dz_d,
                                    float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w, int k,
                                    int stride, int pad, int act, int overwrite, const float *bn_mean_d,
                                    const float *bn_var_d, const float *bn_scales_d, const float *bn_dmean_d,
                                    const float *bn_dvar_d);

/* A depthwise layer whose INPUT is the output of a convolution node with batch-norm (+ cheap activation) that has no other
 * consumer (MobileNet: every 1x1 convolution feeds the next block's depthwise layer). For an executor that runs whole
 * passes: the convolution node stops after its batch statistics (bcnn_hip_conv_forward_stats_only) and these three read
 * its PRE-NORMALISATION output x_raw_d, applying act(batch-norm(.)) with the in_* vectors (saved mean / variance, scales,
 * bias of that node) to every element on its way in -- the values the producer's apply sweep would have written
 * (bcnn_batchnorm_layer.c:226-241), so results are those of bcnn_hip_depthwise_forward_stats / _backward / _backward_bn.
 * Ask bcnn_hip_depthwise_bnin_fusable first. */
int bcnn_hip_depthwise_bnin_fusable(int n, int c, int h, int w, int k, int stride, int pad, int act, int in_act);
int bcnn_hip_depthwise_forward_bnin(const float *x_raw_d, const float *w_d, const float *bias_d, float *y_d, int n, int c,
                                    int h, int w, int k, int stride, int pad, int act, float *stats_d, size_t stats_floats,
                                    const float *in_mean_d, const float *in_var_d, const float *in_scale_d,
                                    const float *in_bias_d, int in_act);
void bcnn_hip_depthwise_backward_bnin(const float *x_raw_d, const float *w_d, const float *y_d, float *dy_d, float *dx_d,
                                      float *dw_d, float *dbias_d, int n, int c, int h, int w, int k, int stride, int pad,
                                      int act, int overwrite, const float *in_mean_d, const float *in_var_d,
                                      const float *in_scale_d, const float *in_bias_d, int in_act);
void bcnn_hip_depthwise_backward_bn_bnin(const float *x_raw_d, const float *w_d, const float *y_d, const float *dz_d,
                                         float *dx_d, float *dw_d, float *dbias_d, int n, int c, int h, int w, int k,
                                         int stride, int pad, int act, int overwrite, const float *bn_mean_d,
                                         const float *bn_var_d, const float *bn_scales_d, const float *bn_dmean_d,
                                         const float *bn_dvar_d, const float *in_mean_d, const float *in_var_d,
                                         const float *in_scale_d, const float *in_bias_d, int in_act);

/* ---------------------------------------------------------------------------------------------
 * SGD step on a parameter arena.  Replaces bcnn_sgd_update_gpu (bcnn_learner.c:86-104); semantics
 * of bcnn_sgd_update_cpu (:67-83) fused into one pass per buffer:
 *   b -= (lr/batch)*db; db *= momentum; dw += (decay*batch)*w; w -= (lr/batch)*dw; dw *= momentum.
 * Either pair may be NULL.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_sgd_update(float *w_d, float *b_d, float *dw_d, float *db_d, size_t w_size,
                         size_t b_size, int batch_size, float learning_rate, float momentum,
                         float decay);

/* Adam step.  Replaces bcnn_adam_update_gpu (bcnn_learner.c:133-163) with the semantics of
 * bcnn_adam_update_cpu (:106-131): biases take the momentum-SGD step; weights
 *   dw += (decay*batch)*w; m = (1-b1)*dw + b1*m; v = (1-b2)*dw^2 + b2*v;
 *   w -= (lr/batch)*mu * m/(sqrt(v)+1e-7); dw = 0,  mu = sqrt(1-b2^(iter+1))/(1-b1^(iter+1)).
 * `iter` is what the reference passes: learner->seen (samples, not steps). adam_m_d / adam_v_d are
 * w_size floats each, zero before the first step, owned by the caller.
 * Every product, sum, the division and the square root are single correctly rounded float operations; the reference
 * takes powf(v, 0.5f) for the root, so w may differ from it in the last bits while m, v and dw are its bits. */
void bcnn_hip_adam_update(float *w_d, float *b_d, float *dw_d, float *db_d, float *adam_m_d,
                          float *adam_v_d, size_t w_size, size_t b_size, int batch_size, int iter,
                          float beta1, float beta2, float learning_rate, float momentum, float decay);

/* The same step for MANY buffers in one launch (a net's update loop, bcnn_net.c:316-326, issues one
 * bcnn_sgd_update per node: ~40 tiny launches for ResNet-18). `chunks_d` is a device array of
 * bcnn_hip_sgd_chunk, each at most BCNN_HIP_SGD_CHUNK elements of one buffer; `use_decay` selects the
 * weights rule (decay term) or the biases rule. The caller builds the table once per net. */
#define BCNN_HIP_SGD_CHUNK 2048
typedef struct bcnn_hip_sgd_chunk {
    float *w_d;
    float *g_d;
    unsigned int count;
    unsigned int use_decay;
} bcnn_hip_sgd_chunk;
void bcnn_hip_sgd_update_chunks(const bcnn_hip_sgd_chunk *chunks_d, int num_chunks, int batch_size,
                                float learning_rate, float momentum, float decay);

/* Zero fill of MANY buffers in one launch: the executor resets every destination gradient before the node runs
 * (bcnn_net.c:361-375), ~40 small hipMemset-sized launches per ResNet-18 step; nothing reads a gradient during the
 * forward pass, so the fills that are not provably dead are issued together at its start. `chunks_d`: device array,
 * each entry at most BCNN_HIP_FILL_CHUNK floats of one buffer. */
#define BCNN_HIP_FILL_CHUNK 16384
typedef struct bcnn_hip_fill_chunk {
    float *p_d;
    unsigned int count;
    unsigned int reserved;
} bcnn_hip_fill_chunk;
void bcnn_hip_zero_chunks(const bcnn_hip_fill_chunk *chunks_d, int num_chunks);

/* ---------------------------------------------------------------------------------------------
 * "Next" rows: the nodes either side of the hot path that a ResNet-style
 * graph needs, kept on the device so that a training step has no host round trip.
 *   axpy_strided : bcnn_axpy_strided (bcnn_mat.c:159-177), the residual add of the eltwise node for
 *                  operands of different spatial size / depth (bcnn_eltwise_layer.c:119-150);
 *                  y[n][k][j*sy][i*sy] += a * x[n][k][j*sx][i*sx] over min_dim = {c,h,w}.
 *   add_rowvec   : y[r][:] += v[:] for r < rows (bias add of the full-connected node,
 *                  bcnn_fc_layer.c:170-172; plain axpy, no 0/1 quirk).
 *   softmax      : bcnn_forward_softmax_layer_cpu (bcnn_softmax_layer.c:88-155), log-sum-exp form,
 *                  over c for every (n, spatial position).
 *   eltwise_*    : the same-shape path of the eltwise node in one pass each way
 *                  (bcnn_eltwise_layer.c:112-121 copy + axpy + activation; :136-147 activation backward +
 *                  two axpys): y = act(a + b) where b only covers the first b_count elements (the
 *                  reference's stride-1 path adds the second operand to IMAGE 0 only -- quirk 5);
 *                  backward: g = dy * act'(y) stored over dy, da += g, db[i] += g[i] for i < b_count.
 *                  da_d / db_d may be NULL. overwrite_a != 0: da is assigned 0 + g instead of da += g
 *                  (same contract as bcnn_hip_maxpool_backward's overwrite).
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_eltwise_forward(const float *a_d, const float *b_d, float *y_d, size_t n, size_t b_count, int act);
void bcnn_hip_eltwise_backward(const float *y_d, float *dy_d, float *da_d, float *db_d, size_t n, size_t b_count,
                               int act, int overwrite_a);
/* The cost node's scalar metric computed on the device (bcnn_compute_error, bcnn_cost_layer.c:142-244, which
 * reads whole tensors back to the host): metric = bcnn_loss_metric value (0 error rate, 1 logloss, 2 SSE, 3 MSE,
 * 4 CRPS, 5 dice); pred_d / label_d / grad_d are [batch][per]; the result is written to out_d[0]. */
void bcnn_hip_cost_metric(int metric, const float *pred_d, const float *label_d, const float *grad_d, int batch,
                          int per, float *out_d);
void bcnn_hip_axpy_strided(int num_batches, float a, const float *x_d, float *y_d, int stride_y,
                           int stride_x, int x_c, int x_h, int x_w, int y_c, int y_h, int y_w, int min_c,
                           int min_h, int min_w);
void bcnn_hip_add_rowvec(float *y_d, const float *v_d, int rows, int cols);
void bcnn_hip_softmax_forward(const float *x_d, float *y_d, int n, int c, int hw);

/* ---------------------------------------------------------------------------------------------
 * Detector graph nodes (yolov3-tiny: [route], [upsample], [yolo]).  Replace the reference's
 * bcnn_forward/backward_concat_layer_gpu (bcnn_concat_layer.c:113-146: num_src x n copies / axpys),
 * bcnn_forward/backward_upsample_layer_gpu (bcnn_upsample_layer.cu) and the activation part of
 * bcnn_forward_yolo_layer (bcnn_yolo.c:417-440, done on the host there).
 *   concat_forward  : for every image j < n and source i, dst[j*dst_size3d + off_i ..] = src_i[j*size_i ..],
 *                     off_i = sum of the sizes before i. One launch for the node.
 *   concat_backward : src_grad_i[j*size_i ..] += dst_grad[j*dst_size3d + off_i ..] (one float add per element,
 *                     bit-exact with the reference's axpy); NULL entries of src_grad_d are skipped.
 *                     src_d / src_grad_d / src_size3d are HOST arrays of num_src entries.
 *   upsample_forward  : nearest neighbour by the integer `size`: y[n][c][h*size][w*size] from x[n][c][h][w].
 *   upsample_backward : dx[e] += the size x size block of dy over e, added row by row, left to right, onto the
 *                       current dx (the reference CPU order: bit-exact, no atomics).
 *   yolo_activate   : y = x with the logistic of bcnn_activation_layer.c applied to entries 0, 1 and
 *                     coords .. coords+classes of each of the `num` boxes; x is [n][num*(coords+classes+1)][hw].
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_concat_forward(int num_src, const float *const *src_d, const int *src_size3d, float *dst_d,
                             int dst_size3d, int n);
void bcnn_hip_concat_backward(int num_src, float *const *src_grad_d, const int *src_size3d, const float *dst_grad_d,
                              int dst_size3d, int n);
void bcnn_hip_upsample_forward(const float *x_d, float *y_d, int n, int c, int h, int w, int size);
void bcnn_hip_upsample_backward(float *dx_d, const float *dy_d, int n, int c, int h, int w, int size);
void bcnn_hip_yolo_activate(const float *x_d, float *y_d, int n, int num, int coords, int classes, int hw);

/* ---------------------------------------------------------------------------------------------
 * Detections of a whole batch on the device: threshold, box decode, ordered compaction and NMS of every YOLO head of
 * a net (bcnn_yolo.c:99-145 get_yolo_box / correct_region_boxes, :470-639; bcnn_yolo_get_detections does the same on
 * the host for one image per call after reading every head back). Two launches for the batch:
 *   candidates : a lane per (image, head, cell, anchor). Reads the ACTIVATED objectness from the head's output tensor
 *                (yolo_activate wrote it); where objectness > thresh it decodes the box with the host's expressions
 *                (fp32, expf, the double sub-terms of correct_region_boxes), forms prob_j = objectness * p_j (0 when
 *                <= thresh) and writes one record. The records of an image are compacted IN CANDIDATE ORDER -- heads
 *                in table order, then cell row * w + col, then anchor -- by ballots and prefix sums, never through an
 *                atomic counter, so the layout is the same from run to run. count[b] is always the true number of
 *                candidates of image b; records past record_cap are dropped.
 *   nms        : one workgroup per image with count <= min(record_cap, nms_cap). Sorts the records' (objectness
 *                descending, record slot ascending) keys in LDS, then walks them in that order: a live box i clears
 *                every later box j with box_iou(i, j) > nms_thresh (the host's expression). Writes order[b][r] = slot
 *                of the r-th box (bit 31 set: cleared), and zeroes objectness and prob of the cleared records.
 *                Images with more candidates are left to the caller (order[b] is not written).
 * heads      : HOST table of num_heads <= BCNN_HIP_YOLO_MAX_HEADS entries; out_d is [n][num * (coords + classes + 1)]
 *              [h * w], anchor_w / anchor_h the extents of the head's MASKED anchors (num <= BCNN_HIP_YOLO_MAX_ANCHORS).
 * image_geom : HOST, n x 4 ints (w, h, new_w, new_h): the image's own size and its letter-boxed size inside netw x neth,
 *              as correct_region_boxes computes it.
 * in_w, in_h : extent of the net's input tensor (the divisor of the anchor extents).
 * result_host: HOST buffer of bcnn_hip_yolo_detect_result_words(n, record_cap, max classes of the heads) 4-byte words:
 *                int   count[n]
 *                int   order[n][record_cap]
 *                float record[n][record_cap][BCNN_HIP_YOLO_RECORD_HEAD + max classes]
 *                      = x, y, w, h, objectness, candidate index (an int), prob[classes of its head], zero padding
 *              filled by ONE device-to-host copy queued behind the two launches on the current stream; the caller
 *              synchronises (bcnn_hip_sync) before reading it. The device side lives in the library's scratch table.
 * nms_cap <= 0 or above bcnn_hip_yolo_nms_capacity() (what the LDS layout holds, a compile-time constant) means that
 * capacity. Returns 0, or 1 when an argument is out of range (nothing is queued then).
 * ------------------------------------------------------------------------------------------- */
#define BCNN_HIP_YOLO_MAX_HEADS 8
#define BCNN_HIP_YOLO_MAX_ANCHORS 16
#define BCNN_HIP_YOLO_RECORD_HEAD 6
typedef struct bcnn_hip_yolo_head {
    const float *out_d;
    int h, w, num, coords, classes;
    float anchor_w[BCNN_HIP_YOLO_MAX_ANCHORS], anchor_h[BCNN_HIP_YOLO_MAX_ANCHORS];
} bcnn_hip_yolo_head;
int bcnn_hip_yolo_nms_capacity(void);
size_t bcnn_hip_yolo_detect_result_words(int n, int record_cap, int max_classes);
int bcnn_hip_yolo_detect_batch(const bcnn_hip_yolo_head *heads, int num_heads, int n, const int *image_geom, int in_w,
                               int in_h, int netw, int neth, float thresh, int relative, float nms_thresh,
                               int record_cap, int nms_cap, void *result_host);

/* ---------------------------------------------------------------------------------------------
 * TRAIN-mode forward of the YOLOv3 head (bcnn_yolo.c:226-415; a host loop in the reference, behind a read-back of the
 * head, in its CUDA build too). Four launches on the current stream, no atomics, every sum a fixed-order tree:
 *   forward : a lane per predicted box (image, anchor, cell). y = the activation of yolo_activate; EVERY element of
 *             grad is written: objectness gets y, or 0 when the best box_iou against the image's truths is > 0.5,
 *             everything else 0 (the reference's memset). The truths of an image are label_d[b * label_stride + 5 t ..]
 *             = x, y, w, h, class, t < BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS; the list ends at the first x == 0.
 *   truths  : one wave per image, the truths in order: best anchor of all `total` against the truth at the origin
 *             (strict >, first wins); when `mask` holds it, the four box deltas (scale 2 - w h), the objectness delta
 *             y - 1 and the class deltas of delta_yolo_class, which depend on what an earlier truth left in the same
 *             slot. A truth whose cell (int)(x w), (int)(y h) or class lies outside the head is skipped as a whole
 *             (the reference writes out of bounds there); it still takes part in `forward`.
 *   cost    : sum of grad^2 over the head, then one block folds it and the statistics partials into *record_d: the
 *             SUMS the reference divides before printing (avg_iou .. recall75 by count, avg_anyobj by n num h w).
 * Writes y_d, grad_d, *record_d and workspace_d only. coords must be 4, num <= BCNN_HIP_YOLO_MAX_ANCHORS, total <=
 * BCNN_HIP_YOLO_TRAIN_MAX_TOTAL, label_stride >= 5 * BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS: otherwise 1 is returned and nothing
 * is queued (workspace_size: 0). biases: the extents (w, h) of all `total` anchors in input pixels.
 * ------------------------------------------------------------------------------------------- */
#define BCNN_HIP_YOLO_TRAIN_MAX_TRUTHS 50
#define BCNN_HIP_YOLO_TRAIN_MAX_TOTAL 32
typedef struct bcnn_hip_yolo_train_head {
    int n, h, w, num, coords, classes, total;
    int in_w, in_h;   /* extent of the net's input tensor */
    int label_stride; /* floats per image of label_d */
    int mask[BCNN_HIP_YOLO_MAX_ANCHORS];
    float biases[2 * BCNN_HIP_YOLO_TRAIN_MAX_TOTAL];
} bcnn_hip_yolo_train_head;
typedef struct bcnn_hip_yolo_train_record {
    float cost, avg_iou, avg_cat, avg_obj, avg_anyobj, recall, recall75;
    int count;
} bcnn_hip_yolo_train_record;
size_t bcnn_hip_yolo_train_workspace_size(const bcnn_hip_yolo_train_head *head); /* floats */
int bcnn_hip_yolo_train_forward(const bcnn_hip_yolo_train_head *head, const float *x_d, const float *label_d, float *y_d,
                                float *grad_d, bcnn_hip_yolo_train_record *record_d, float *workspace_d);

/* ---------------------------------------------------------------------------------------------
 * The input tensor of a batch from raw uint8 images (image_fill.hip): entries 0 .. num_images - 1 of the NCHW float
 * tensor dst_d [n][c][h][w]; entries num_images .. n - 1 are not written. images / widths / heights / strides are HOST
 * arrays of num_images entries: interleaved HWC uint8 pixels, extent in pixels, row pitch in bytes (strides NULL:
 * widths[b] * c). Image b is resized with bip_resize_bilinear's fixed-point rule (half-pixel centres, fractions in 1/16,
 * rounding + 128 >> 8; the taps come from the host's own function, bcnn_amd/host/bip_resize_tap.h) to
 *   BCNN_HIP_IMAGE_FIT_STRETCH   : w x h;
 *   BCNN_HIP_IMAGE_FIT_LETTERBOX : new_w x new_h with (float)w / iw < (float)h / ih ? (w, (ih * w) / iw)
 *                                  : ((iw * h) / ih, h), pasted at ((w - new_w) / 2, (h - new_h) / 2) onto a canvas of
 *                                  bytes 128,
 * and converted like bcnn_convert_img_to_float (bcnn_data.c:70-100): plane k = ((float)byte[ks] - mean[ks]) * norm_coeff
 * with ks = 2 - k when swap_to_bgr and c == 3, else k; mean = (mean_r, mean_g, mean_b) when c == 3, else mean_r. The
 * result equals the host composition of the two functions bit for bit.
 * The call packs per-image descriptors, tap tables and the pixels (row padding dropped) into one pinned host block,
 * sends it with ONE copy on the current stream into the library's scratch table and queues ONE kernel for the batch:
 * a lane computes 8 consecutive pixels of a row for all c planes (canvas pixels included, there is no fill pass) and
 * stores them 16 bytes wide between a scalar head and tail. The images have been copied when the call returns. A later
 * call waits for the earlier call's copy (not its kernel) before it reuses the pinned block.
 * Returns 0, or 1 with nothing staged or queued: NULL dst_d / images / widths / heights / images[b]; n, h or w < 1;
 * c outside 1..4; num_images outside 1..n; an extent < 1; a stride < widths[b] * c; unknown fit; a letterbox extent of
 * 0; more than 2 GiB to stage.
 * ------------------------------------------------------------------------------------------- */
#define BCNN_HIP_IMAGE_FIT_STRETCH 0
#define BCNN_HIP_IMAGE_FIT_LETTERBOX 1
int bcnn_hip_fill_images(float *dst_d, int n, int c, int h, int w, int num_images, const uint8_t *const *images,
                         const int *widths, const int *heights, const int *strides, int fit, float norm_coeff,
                         int swap_to_bgr, float mean_r, float mean_g, float mean_b);

/* ---------------------------------------------------------------------------------------------
 * The input tensor of a batch from JPEG streams (jpeg_pixels.hip): the decoder's pixel stage on the device. The caller
 * does the serial half of the decoder -- headers and entropy decoding into DEQUANTISED int16 coefficient blocks
 * (libbip.so: bip_jpeg_frame_info, bip_jpeg_read_coefficients; this library does not depend on it) -- and this library
 * does the rest: inverse DCT, chroma upsampling, Y Cb Cr -> R G B, then the resize / letterbox / conversion of
 * bcnn_hip_fill_images with the same fit, norm_coeff, swap_to_bgr and means. Entries 0 .. num_images - 1 of dst_d
 * [n][c][h][w] are written, the others are not. The arithmetic is the host decoder's own
 * (bcnn_amd/host/bip_jpeg_pixels.h, integer throughout), so the tensor equals bcnn_hip_fill_images on the host-decoded
 * pixels bit for bit.
 *   bcnn_hip_jpeg_stage_begin  checks every frame and the sizes, lays the batch out in the pinned staging block of the
 *       calling thread (the one bcnn_hip_fill_images uses; it waits for an earlier call's copy), writes the descriptors
 *       and tap tables and returns in coeff[b] where image b's coefficients go: frames[b].comp[0]'s blocks_w * blocks_h
 *       blocks of 64 int16, row-major, then the next component's. Returns 0, or 1 with nothing staged: NULL frames /
 *       coeff; n, h or w < 1; c not 1 or 3; num_images outside 1..n; unknown fit; a frame whose ncomp is not c or whose
 *       numbers do not fit together; a letterbox extent of 0; more than 2 GiB for the device block. *failed_image
 *       (may be NULL) is then the index of the image the refusal is about, or -1.
 *   bcnn_hip_jpeg_stage_run    after the caller has filled every coeff[b]: ONE copy of descriptors, taps and coefficients
 *       (2 bytes per sample of every component plane) on the current stream and THREE kernels: jpeg_idct_kernel (8 lanes
 *       per block, all blocks of all components of all images; blocks bx < idct_w, by < idct_h of a component are
 *       transformed, the set the host transforms), jpeg_colour_kernel (a lane per 8 pixels of a row) and
 *       fill_images_kernel. Planes and pixels stay in the library's scratch table. Returns 0, or 1 when no batch is
 *       pending or dst_d is NULL.
 *   bcnn_hip_jpeg_stage_cancel drops the pending batch (a stream failed to decode): nothing has been queued.
 * Between _begin and _run / _cancel the calling thread makes no other call that stages images. _run checks it: after such
 * a call, or on another device than _begin's, it returns 1 as when no batch is pending (the batch is dropped).
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_jpeg_component {
    int h, v;               /* sampling factors */
    int width, height;      /* samples with image content */
    int pitch, rows;        /* plane: 8 * blocks_w, 8 * blocks_h */
    int blocks_w, blocks_h; /* coefficient blocks: whole MCUs */
    int idct_w, idct_h;     /* blocks that are transformed */
} bcnn_hip_jpeg_component;
typedef struct bcnn_hip_jpeg_frame {
    int width, height, ncomp, hmax, vmax;
    bcnn_hip_jpeg_component comp[3];
} bcnn_hip_jpeg_frame;
int bcnn_hip_jpeg_stage_begin(int n, int c, int h, int w, int num_images, const bcnn_hip_jpeg_frame *frames, int fit,
                              int16_t **coeff, int *failed_image);
int bcnn_hip_jpeg_stage_run(float *dst_d, float norm_coeff, int swap_to_bgr, float mean_r, float mean_g, float mean_b);
void bcnn_hip_jpeg_stage_cancel(void);

/* ---------------------------------------------------------------------------------------------
 * The input tensor of a training batch from the loader's raw uint8 samples (augment.hip): online augmentation, centre
 * crop and conversion on the device. Entries 0 .. num_samples - 1 of the NCHW float tensor dst_d [n][c][h][w] are
 * written; the others are not. pixels (HOST) holds num_samples dense interleaved HWC samples of src_w x src_h x c bytes,
 * records (HOST) one record per sample with what the host drew for it (bcnn_data.c draws from rand() in the reference's
 * order and does every float -> integer step with its own arithmetic; the kernels only do integer and fp32 work whose
 * result does not depend on the order of evaluation). With S0 the sample, per pixel (x, y) and channel:
 *   FLIP     S1(x, y) = S0(src_w - 1 - x, y)
 *   SHIFT    S2(x, y) = S1(x + x_ul, y + y_ul) inside the sample, else 128          (bip_crop_image onto a grey canvas)
 *   SCALE    S3(x, y) = bip_resize_blend of the four S2 samples at (tapx[x], tapy[y]) where both taps have an index
 *            >= 0, else S2(x, y). taps (HOST; may be NULL when no record has SCALE) holds per sample src_w (index,
 *            fraction) int32 pairs for the columns followed by src_h pairs for the rows: the tap of the resized image's
 *            column x + x_ul by bip_resize_tap (bcnn_amd/host/bip_resize_tap.h), or index -1 where the resized image
 *            pasted back at the shift's origin does not cover the column
 *   ROTATE   S4(x, y): 16.16 inverse map about (src_w / 2, src_h / 2) with ca = cos * 65536, sa = sin * 65536 and 32-bit
 *            wrap-around; 0 unless 0 <= mx < src_w - 1 and 0 <= my < src_h - 1; the blend is four products of three
 *            fp32 factors summed left to right, truncated                                             (bip_rotate_image)
 *   CONTRAST S5 = clamp(((S4 - mean) * gain + 2048 >> 12) + mean), mean = per-channel sum of S4 / (src_w * src_h) in
 *            unsigned 32-bit arithmetic, gain in 20.12                                            (bip_contrast_stretch)
 *   always   S6 = clamp(S5 + brightness); plane k of entry b = ((float)S6(x + (src_w - w) / 2, y + (src_h - h) / 2)[ks]
 *            - 127.5f) * (1 / 127.5f), ks = 2 - k when swap_to_bgr and c == 3, else k   (bcnn_convert_img_to_float)
 * A stage whose flag is clear is the identity; a zeroed record is centre crop and conversion only. The result equals the
 * host loader's (bcnn_apply_data_augmentation, bip_crop_image, bcnn_convert_img_to_float) bit for bit.
 * One pinned staging block (records, zeroed channel sums, taps, pixels) goes up in ONE copy on the current stream; TWO
 * kernels follow, whatever the batch size: the first writes S4 to a uint8 scratch of the library's table (a lane per
 * pixel) and adds the per-channel sums of the samples with CONTRAST with one integer atomicAdd per wave (integer sums
 * do not depend on the order: the result is the same from run to run); the second applies S5, S6, crop and conversion, a
 * lane per 8 pixels of a row for all c planes, 16-byte stores between a scalar head and tail. The samples have been copied
 * when the call returns; a later call waits for the earlier call's copy before it reuses the pinned block.
 * Returns 0, or 1 with nothing staged or queued: a NULL dst_d / pixels / records; n, h or w < 1; c outside 1..4;
 * num_samples outside 1..n; src_w < w or src_h < h; a record with SCALE and taps == NULL, or a tap index outside
 * [-1, max(extent - 2, 0)]; more than 2 GiB to stage.
 * ------------------------------------------------------------------------------------------- */
#define BCNN_HIP_AUG_FLIP 1
#define BCNN_HIP_AUG_SHIFT 2
#define BCNN_HIP_AUG_SCALE 4
#define BCNN_HIP_AUG_ROTATE 8
#define BCNN_HIP_AUG_CONTRAST 16
typedef struct bcnn_hip_augment_record {
    int32_t flags;      /* BCNN_HIP_AUG_* */
    int32_t x_ul, y_ul; /* SHIFT */
    int32_t ca, sa;     /* ROTATE */
    int32_t gain;       /* CONTRAST */
    int32_t brightness; /* added last; 0 = none */
    int32_t reserved;   /* 0 */
} bcnn_hip_augment_record; /* the bits BCNN_HIP_AUG_DISTORT / _SPOTS of `flags` are ignored: see bcnn_hip_augment_effects_begin */
int bcnn_hip_augment_batch(float *dst_d, int n, int c, int h, int w, int num_samples, int src_w, int src_h,
                           const uint8_t *pixels, const bcnn_hip_augment_record *records, const int32_t *taps,
                           int swap_to_bgr);

/* ---------------------------------------------------------------------------------------------
 * The class-index label maps that belong to such a batch (augment_label.hip): plane b of the float tensor label_d
 * [n][1][h][w] gets, per pixel, (float) of ONE byte of the b-th mask or of `fill` -- the pull-back of the mask through the
 * geometry stages of its image (FLIP, SHIFT, SCALE, ROTATE of bcnn_hip_augment_batch; nearest picks where the image
 * blends; `fill` where the image gets its canvas). The rule is bcnn_amd/host/bip_label_warp.h, which libbip's
 * bip_warp_label_map is written on as well: the result equals that function's byte for byte. maps (HOST) holds
 * num_samples dense w x h byte maps; records and taps (HOST) are laid out as for bcnn_hip_augment_batch with src_w = w and
 * src_h = h (taps may be NULL when no record has SCALE); CONTRAST, brightness and the effects are ignored. Planes
 * num_samples .. n - 1 are not written.
 * One pinned staging block of its own (records, taps, maps; grow-only, one per host thread and device -- the image
 * batch's copy in flight is not waited for) goes up in ONE copy on the current stream; ONE kernel follows: a lane per four
 * consecutive pixels of a row and one 16-byte store when w % 4 == 0 and label_d is 16-byte aligned (dispatch trace
 * `augment_label:v4`), else a lane per pixel (`augment_label`). The maps have been copied when the call returns.
 * Returns 0, or 1 with nothing staged or queued: a NULL label_d / maps / records; n, h or w < 1; num_samples outside
 * 1..n; fill outside 0..255; a record with SCALE and taps == NULL, or a tap index outside [-1, max(extent - 2, 0)]; more
 * than 2 GiB to stage.
 * ------------------------------------------------------------------------------------------- */
int bcnn_hip_augment_label_batch(float *label_d, int n, int h, int w, int num_samples, const uint8_t *maps,
                                 const bcnn_hip_augment_record *records, const int32_t *taps, int fill);

/* ---------------------------------------------------------------------------------------------
 * The same batch when some of its samples are still JPEG coefficient blocks (augment.hip + the two kernels of
 * jpeg_pixels.hip): the list loaders' opt-in device decoding. The stored sample is the net input itself (w x h x c, c 1
 * or 3); a sample is either a dense w x h x c block of bytes the caller decoded and cropped, or a JPEG frame whose
 * entropy decoding the caller did and whose pixels exist only on the device. There the sample is the w x h WINDOW at
 * (x_ul, y_ul) of the decoded wi x hi image: raw byte (x, y, k) = image[((y + y_ul) wi + x + x_ul) c + k] where
 * 0 <= x + x_ul < wi and 0 <= y + y_ul < hi, else 0 -- bip_crop_image onto a zeroed buffer. The window is S0 of
 * bcnn_hip_augment_batch: flip, shift, scale, rotation, contrast, brightness and conversion follow unchanged, and the
 * result is bit for bit what that call gives on the host-decoded, host-cropped samples.
 *   bcnn_hip_augment_jpeg_begin  frames[b] describes sample b (bcnn_hip_jpeg_frame as for bcnn_hip_jpeg_stage_begin;
 *       ncomp 0: not a JPEG candidate). Lays the batch out in the pinned staging block of the calling thread (the one
 *       bcnn_hip_augment_batch uses; it waits for an earlier call's copy) and returns in coeff[b] where the coefficients
 *       of sample b go, or NULL for a sample the caller has to decode itself (ncomp 0, ncomp != c, numbers that do not
 *       fit together). Returns 0, or 1 with nothing pending: NULL frames / coeff; n, h or w < 1; c not 1 or 3;
 *       num_samples outside 1..n; no candidate at all; more than 2 GiB for the device block.
 *   bcnn_hip_augment_jpeg_run    decoded[b] != 0: the coefficients of sample b are in place and origins[2 b], [2 b + 1]
 *       is its window's origin; decoded[b] == 0: sample b is pixels + b w h c (the other slots of `pixels` are not read).
 *       records / taps / swap_to_bgr as for bcnn_hip_augment_batch with src_w = w, src_h = h. ONE copy of the block
 *       (records, zeroed sums, taps, windows, plane and image tables, the coefficients of every candidate, the raw
 *       samples) on the current stream, then at most FOUR kernels: jpeg_idct_kernel and jpeg_colour_kernel over the
 *       decoded samples (none decoded: skipped), the windowed geometry kernel, the convert kernel. Returns 0, or 1 with
 *       nothing queued and the batch dropped: nothing pending; a NULL argument; decoded[b] set for a sample that got no
 *       coeff[b]; a record with SCALE and taps == NULL or a tap index out of range.
 *   bcnn_hip_augment_jpeg_cancel drops the pending batch: nothing has been queued.
 * Between _begin and _run / _cancel the calling thread makes no other call that stages a training batch. _run checks it:
 * after such a call, or on another device than _begin's, it returns 1 as when nothing is pending (the batch is dropped).
 * ------------------------------------------------------------------------------------------- */
int bcnn_hip_augment_jpeg_begin(int n, int c, int h, int w, int num_samples, const bcnn_hip_jpeg_frame *frames,
                                int16_t **coeff);
int bcnn_hip_augment_jpeg_run(float *dst_d, const uint8_t *decoded, const uint8_t *pixels,
                              const bcnn_hip_augment_record *records, const int32_t *taps, const int32_t *origins,
                              int swap_to_bgr);
void bcnn_hip_augment_jpeg_cancel(void);

/* ---------------------------------------------------------------------------------------------
 * The same batch when every sample is still a decoded image of its own size that has to be letterboxed first
 * (augment.hip): the detection-list loader's opt-in device path. For sample b, S0 of bcnn_hip_augment_batch is a
 * w x h x c canvas (src_w = w, src_h = h: no centre crop) that holds 128 everywhere except at
 * [x_off, x_off + new_w) x [y_off, y_off + new_h), where it holds bip_resize_bilinear(images[b]) to new_w x new_h:
 * bip_resize_tap with bip_resize_scale(w, new_w) / bip_resize_scale(h, new_h) per axis and bip_resize_blend. A source
 * axis of extent 1 replicates. records / taps / swap_to_bgr describe the augmentation of the CANVAS, as for
 * bcnn_hip_augment_batch; every later stage and the conversion are that call's. The result equals, bit for bit, the host
 * composition bip_resize_bilinear, memset to 128, bip_crop_image at (-x_off, -y_off), the pixel step of
 * bcnn_apply_data_augmentation and bcnn_convert_img_to_float with 127.5 / (1 / 127.5).
 * One pinned staging block goes up in ONE copy on the current stream: [records][zeroed channel sums][augmentation
 * taps][one descriptor per image][letterbox tap tables, tabulated here with bip_resize_tap][the packed source pixels of
 * every image]; behind it, on the device only: [canvases][rotated samples]. THREE kernels follow, whatever the batch size
 * and the image sizes: augment_letterbox_kernel writes all canvases (a lane per run of 16 consecutive canvas bytes of one
 * row, 16-byte stores where the address allows, integer work only, source images addressed by offsets into the block),
 * then the geometry and the convert kernel of bcnn_hip_augment_batch, unchanged. The images have been copied when the
 * call returns.
 * Returns 0, or 1 with nothing staged or queued: a NULL dst_d / images / records / pixels pointer; n, h or w < 1; c
 * outside 1..4; num_samples outside 1..n; an image extent < 1; new_w outside 1..w or new_h outside 1..h; x_off outside
 * 0..w - new_w or y_off outside 0..h - new_h; a record with SCALE and taps == NULL, or a tap index outside
 * [-1, max(extent - 2, 0)]; more than 2 GiB for the staging block plus the device part.
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_letterbox_image {
    const uint8_t *pixels;   /* HOST: h rows of w * c bytes, dense */
    int32_t w, h;            /* source extent, >= 1 */
    int32_t new_w, new_h;    /* extent of the resized image, 1 .. W / 1 .. H */
    int32_t x_off, y_off;    /* where it is pasted, 0 .. W - new_w / 0 .. H - new_h */
} bcnn_hip_letterbox_image;
int bcnn_hip_augment_letterbox_batch(float *dst_d, int n, int c, int h, int w, int num_samples,
                                     const bcnn_hip_letterbox_image *images, const bcnn_hip_augment_record *records,
                                     const int32_t *taps, int swap_to_bgr);

/* ---------------------------------------------------------------------------------------------
 * The augmenter's last two stages on the device (augment.hip): Perlin distortion and random spotlights, between S6 and the
 * centre crop of bcnn_hip_augment_batch. bcnn_hip_augment_effects_begin stages them for the calling thread's NEXT batch
 * call -- bcnn_hip_augment_batch, bcnn_hip_augment_jpeg_run or bcnn_hip_augment_letterbox_batch, whichever comes first --
 * which consumes them on every return: it puts them into its one staging block (still ONE copy per batch) and launches
 * augment_convert_effects_kernel in place of the convert kernel. A batch call with nothing staged does what it always
 * did, launch for launch. The two flag bits below live in effects[b].flags; the same bits of a record are ignored.
 * With T = S6 (contrast and brightness are pointwise, so T is evaluated at the taps), per pixel (x, y) of sample b:
 *   DISTORT  n = bip_perlin_noise(cell_x[x], cell_y[y], weight_x[x], weight_y[y], seed); (px, py) = ((norm_x[x] + n *
 *            distortion) * src_w, (norm_y[y] + n * distortion) * src_h); S7 = bip_distort_blend of T at (ix, iy) ..
 *            (ix + 1, iy + 1) where bip_distort_map accepts the position, else 0. perlin (HOST) holds per sample
 *            2 (src_w + src_h) floats -- norm of the columns, norm of the rows, weight of the columns, weight of the rows
 *            -- and cells (HOST) per sample src_w + src_h int32, columns then rows, all as bip_perlin_axis
 *            (include/bip/bip.h) tabulates them; read for the samples with DISTORT only, and both may be NULL when no
 *            sample has it
 *   SPOTS    for spots[first_spot .. first_spot + num_spots) in order: inside the spot's box {x0, y0, bw, bh},
 *            S8 = bip_spot_add(spot_tables[table + (y - y0) bw + (x - x0)], S8), outside it the byte stays. The tables
 *            are bip_spot_table's; the caller chooses the box so that no byte outside it would change.
 * The arithmetic is bcnn_amd/host/bip_effects.h on both sides: no cos, exp or division on the device, so the bytes are
 * the host functions' (bip_perlin_distortion_seeded, bip_add_spotlights) bit for bit.
 * Returns 0, or 1 with nothing staged: a NULL effects; num_samples, src_w or src_h < 1; flags other than the two below;
 * DISTORT with a NULL perlin / cells or a distortion that is not finite; SPOTS with a range outside
 * [0, num_spots] or spots / spot_tables NULL; a box that is empty, leaves the sample or whose bw x bh floats end
 * behind num_table_floats; more than 2 GiB to stage. The batch call returns 1 (nothing queued, the staged data dropped)
 * when num_samples, src_w (w for the two other routes) or src_h do not equal its own, or when its block with the effects
 * would pass 2 GiB. bcnn_hip_augment_effects_cancel drops what is staged.
 * ------------------------------------------------------------------------------------------- */
#define BCNN_HIP_AUG_DISTORT 32
#define BCNN_HIP_AUG_SPOTS 64
typedef struct bcnn_hip_augment_effect {
    int32_t flags;                 /* BCNN_HIP_AUG_DISTORT | BCNN_HIP_AUG_SPOTS */
    int32_t seed;                  /* DISTORT */
    float distortion;
    int32_t first_spot, num_spots; /* SPOTS */
} bcnn_hip_augment_effect;
typedef struct bcnn_hip_augment_spot {
    int32_t x0, y0, bw, bh; /* the box of its table, inside the sample */
    uint32_t table;         /* first float of its table in spot_tables */
} bcnn_hip_augment_spot;
int bcnn_hip_augment_effects_begin(int num_samples, int src_w, int src_h, const bcnn_hip_augment_effect *effects,
                                   const float *perlin, const int32_t *cells, const bcnn_hip_augment_spot *spots,
                                   int num_spots, const float *spot_tables, size_t num_table_floats);
void bcnn_hip_augment_effects_cancel(void);

/* ---------------------------------------------------------------------------------------------
 * Transposed convolution (deconvolution), implicit GEMMs on fp32 MFMA with no col2im / im2col buffer.
 * Replaces bcnn_forward_deconv_layer_gpu / bcnn_backward_deconv_layer_gpu (bcnn_deconv_layer.c:249-320) with the
 * semantics of the CPU workers (:150-193, :195-246):
 *   - x [n][c][h][w], weights [c][f][k][k] (c_in major, as the reference's Wᵀ GEMM reads them), bias [f],
 *     y [n][f][s (h - 1) + k - 2 pad][s (w - 1) + k - 2 pad];
 *   - forward: y = act(transposed conv + bias), OVERWRITTEN; the bias is skipped for channels whose bias is exactly
 *     0.0f or 1.0f, as bcnn_hip_add_bias does; PReLU is not supported (the reference passes NULL slopes);
 *   - backward: dy_d <- dy_d * act'(y_d) in place; dbias += sum dy; dw += (1/n) sum x dy (beta = 1; the factor
 *     1/n of the reference's GEMM alpha, :209, is kept); dx_d (if non-NULL) is OVERWRITTEN (beta = 0); dw_d may be
 *     NULL (no weight gradient).
 * pad > 0: the reference's GPU and CPU paths read the col2im / im2col workspace with the wrong extent; here pad crops
 * the full s (h - 1) + k result by pad on each side (torch.nn.functional.conv_transpose2d(padding=pad)).
 * workspace_d: at least bcnn_hip_deconv_workspace_size(...) floats (the K-split partials of dw; a smaller one of at
 * least c f k k floats splits less). The weight gradient is bit-identical from run to run (fixed split, no atomics).
 * ------------------------------------------------------------------------------------------- */
size_t bcnn_hip_deconv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad);
void bcnn_hip_deconv_forward(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n, int c, int h,
                             int w, int f, int k, int stride, int pad, int act);
void bcnn_hip_deconv_backward(const float *x_d, const float *w_d, const float *y_d, float *dy_d, float *dx_d,
                              float *dw_d, float *dbias_d, int n, int c, int h, int w, int f, int k, int stride, int pad,
                              int act, float *workspace_d, size_t workspace_elems);

/* ---------------------------------------------------------------------------------------------
 * Dilated (atrous) convolution, implicit GEMMs on fp32 MFMA with no im2col / col2im buffer and no zero-expanded weights
 * (conv_dilated.hip). No reference counterpart; torch.nn.functional.conv2d(stride, padding, dilation, groups) is the oracle.
 *   - x [n][c][h][w], weights [f][c / groups][k][k], bias [f], y [n][f][oh][ow] with
 *     oh = (h + 2 pad - dilation (k - 1) - 1) / stride + 1; groups divides c and f; dilation >= 1 (1: a plain convolution);
 *   - forward: y = act(conv + bias), OVERWRITTEN; out-of-range taps read zero; PReLU is not supported;
 *   - backward: dy_d <- dy_d * act'(y_d) in place; dbias += sum dy; dw += sum x dy (beta = 1, no scaling, as the
 *     convolution node); dx_d (if non-NULL) is OVERWRITTEN; dw_d may be NULL (no weight gradient).
 * workspace_d: at least bcnn_hip_dilated_conv_workspace_size(...) floats (the K-split partials of dw; a smaller one of
 * at least f (c / groups) k k floats splits less; smaller than that, or NULL with dw_d set, ends the process). The split is
 * a function of the shape and workspace_elems only and the partials are added in split order: the weight gradient is
 * bit-identical from run to run. An unsupported shape (a non-positive extent, a tensor of 2^31 elements or more) ends the
 * process with a message.
 * ------------------------------------------------------------------------------------------- */
size_t bcnn_hip_dilated_conv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad, int dilation,
                                            int groups);
void bcnn_hip_dilated_conv_forward(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n, int c,
                                   int h, int w, int f, int k, int stride, int pad, int dilation, int groups, int act);
void bcnn_hip_dilated_conv_backward(const float *x_d, const float *w_d, const float *y_d, float *dy_d, float *dx_d,
                                    float *dw_d, float *dbias_d, int n, int c, int h, int w, int f, int k, int stride,
                                    int pad, int dilation, int groups, int act, float *workspace_d,
                                    size_t workspace_elems);

/* ---------------------------------------------------------------------------------------------
 * Dilated (atrous) depthwise convolution: one k x k filter per channel, taps `dilation` pixels apart
 * (depthwise_dilated.hip). No reference counterpart; torch.nn.functional.conv2d(groups = c,
 * dilation) is the oracle. The entry points mirror bcnn_hip_depthwise_forward / _backward with `dilation` added.
 *   - x [n][c][h][w], weights [c][k][k] (the depthwise node's layout; the same floats are the dilated node's
 *     [c][1][k][k] at groups == c), bias [c], y [n][c][oh][ow], oh = (h + 2 pad - dilation (k - 1) - 1) / stride + 1;
 *     any k >= 1, stride >= 1, pad >= 0, dilation >= 1;
 *   - forward: y = act(sum of taps + bias), OVERWRITTEN; out-of-range taps read zero. The taps are added ky outer, kx
 *     inner, every product and add rounded on its own: at dilation 1 y has the bits of bcnn_hip_depthwise_forward
 *     (except that a bias of exactly 1.0 is added here too);
 *   - backward, in this order: dy_d <- dy_d * act'(y_d) in place; dbias_d += and dw_d += (unscaled; either may be NULL);
 *     dx_d NULL: no data gradient, else dx_d += or, with overwrite != 0, assigned (every element, those no tap reaches
 *     too). At dilation 1 dx has the bits of bcnn_hip_depthwise_backward. The weight gradient does not depend on dx_d;
 *   - activations: those of the dilated convolution (no PReLU, none that need the layer's input).
 * workspace_d: at least bcnn_hip_dilated_depthwise_workspace_size floats, the per-(plane, band) partial sums of dw and
 * dbias that a finalize kernel adds in index order: no atomics, the same bits on every run; a smaller one ends the
 * process. bcnn_hip_dilated_depthwise_path: the kernel family of the shape, 0 generic (k != 3, stride > 1, rows too wide
 * for a band), 1 plane (the staged plane, x forward and dy backward, is at most 12288 floats: one workgroup per plane in
 * LDS), 2 bands (row bands with a 2 dilation halo); -1 for a shape the workers refuse. The two queries need no device. An
 * unsupported shape (a non-positive extent, a tensor of 2^31 elements or more) ends the process with a message.
 * ------------------------------------------------------------------------------------------- */
size_t bcnn_hip_dilated_depthwise_workspace_size(int n, int c, int h, int w, int k, int stride, int pad, int dilation);
void bcnn_hip_dilated_depthwise_forward(const float *x_d, const float *w_d, const float *bias_d, float *y_d, int n, int c,
                                        int h, int w, int k, int stride, int pad, int dilation, int act);
void bcnn_hip_dilated_depthwise_backward(const float *x_d, const float *w_d, const float *y_d, float *dy_d, float *dx_d,
                                         float *dw_d, float *dbias_d, int n, int c, int h, int w, int k, int stride,
                                         int pad, int dilation, int act, int overwrite, float *workspace_d,
                                         size_t workspace_elems);
int bcnn_hip_dilated_depthwise_path(int n, int c, int h, int w, int k, int stride, int pad, int dilation, int backward);

/* ---------------------------------------------------------------------------------------------
 * Local response normalisation across channels (Caffe / torch.nn.functional.local_response_norm). The reference's
 * device workers are empty (bcnn_lrn_layer.c:207-225); its CPU workers (:106-201) are wrong for every local_size
 * (INTEGRATION.md). NCHW, channel stride h*w; with n_w = local_size:
 *   s_c = k + (alpha / n_w) * sum_{c' in W(c)} x_{c'}^2,   W(c) = [c - (n_w - 1)/2, c + n_w/2] clipped to [0, c),
 *   forward : y_c = x_c * s_c^-beta, OVERWRITTEN;
 *   backward: dx_j (=, overwrite != 0 / +=, overwrite == 0) dy_j s_j^-beta
 *                      - (2 alpha beta / n_w) x_j sum_{c in [j - n_w/2, j + (n_w - 1)/2]} dy_c y_c / s_c,
 *             s and y recomputed from x (no saved scale tensor).
 * Each s_c is the window sum in ascending channel order, whatever the launch shape (bit-identical results).
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_lrn_forward(const float *x_d, float *y_d, int n, int c, int h, int w, int local_size, float alpha,
                          float beta, float k);
void bcnn_hip_lrn_backward(const float *x_d, const float *dy_d, float *dx_d, int n, int c, int h, int w,
                           int local_size, float alpha, float beta, float k, int overwrite);

/* ---------------------------------------------------------------------------------------------
 * Dropout, in place (reference bcnn_dropout_layer.c:32-126 with a reproducible mask instead of the reference's
 * time-seeded cuRAND one). The mask of element i (0 <= i < size) is defined as:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (q lo32, q hi32, step lo32, step hi32), key = (key lo32, key hi32)),
 *   q = i / 4; multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85 (Salmon et al., SC11);
 *   u_i = (w_{i % 4} >> 8) * 2^-24;  dropped <=> u_i < rate.
 * forward: x_i <- dropped ? 0 : x_i * scale, scale = 1.0f / (1.0f - rate) (as the reference's param->scale);
 * backward: the same map on the gradient, with the (key, step) of the forward. rate 0 leaves the tensor unchanged.
 * The net gives node i of rank r the key bcnn_dropout_key(seed, i, r) (host/bcnn_layers_lrn_dropout.c) and counts
 * its TRAIN forwards in `step`.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_dropout_forward(float *x_d, size_t size, float rate, uint64_t key, uint64_t step);
void bcnn_hip_dropout_backward(float *dx_d, size_t size, float rate, uint64_t key, uint64_t step);

/* ---------------------------------------------------------------------------------------------
 * Lifted-structure loss of the cost node (Song et al., "Deep Metric Learning via Lifted Structured Feature
 * Embedding"). The reference computes it on the host, in its CUDA build too (bcnn_lifted_structure_loss.c:16-298):
 * every positive pair walks every negative of both anchors, O(P B K). Here, with x [B][K] the embedding,
 * cls[i] the index of the first entry > 0 in row i of the [B][K] label (-1 if none) and m = margin:
 *   D_ij  = |x_i - x_j|                                   (Gram form on fp32 MFMA for K >= 32, differences below)
 *   neg(i,k) = cls[i] != cls[k]        pos(i,j) = cls[i] == cls[j] and i != j
 *   E_ik  = exp(m - D_ik) if neg(i,k) else 0              S_i = sum_k E_ik
 *   L_ij  = max(0, log(S_i + S_j) + D_ij) for pos(i,j)    (0 when S_i + S_j == 0)
 *   P     = number of unordered positive pairs            loss = sum_{i<j, pos} L_ij^2 / P
 *   Wp_ij = 2 L_ij / (D_ij + 1e-10) for pos(i,j), else 0
 *   T_i   = sum_{j: pos(i,j)} 2 L_ij / (S_i + S_j)        (term 0 when S_i + S_j == 0)
 *   Wn_ik = -T_i E_ik / D_ik for neg(i,k), else 0         A = Wp + Wn + Wn^T
 *   g     = diag(rowsum(A)) x - A x                       ([B][K]; what the reference's forward leaves in the gradient)
 * forward : g_d = g (accumulate == 0) or g_d += g (accumulate != 0, the reference's add onto the zero fill);
 *           record_d = {loss, P}; no positive pair: loss 0, P 0, g = 0 (the reference divides 0 by 0).
 * backward: g_d *= scale / P with P read from record_d on the device (P == 0: g_d *= 0).
 * workspace_d: at least bcnn_hip_lifted_struct_workspace_size(batch, k) floats, about batch^2; it needs no
 * initialisation and its contents afterwards are unspecified. No atomics and a summation order that depends on
 * (batch, k) only: two calls on the same input give the same bits. Two samples of different classes with identical
 * embeddings divide by D = 0, as in the reference.
 * ------------------------------------------------------------------------------------------- */
typedef struct bcnn_hip_lifted_struct_record {
    float loss;
    int num_constraints;
} bcnn_hip_lifted_struct_record;
size_t bcnn_hip_lifted_struct_workspace_size(int batch, int k);
void bcnn_hip_lifted_struct_forward(const float *x_d, const float *label_d, float *g_d, int batch, int k, float margin,
                                    int accumulate, bcnn_hip_lifted_struct_record *record_d, float *workspace_d);
void bcnn_hip_lifted_struct_backward(float *g_d, int batch, int k, float scale,
                                     const bcnn_hip_lifted_struct_record *record_d);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel exchange (RCCL over xGMI).  No reference counterpart (the reference is single-device); process
 * model = the reference's one device per process (bcnn_cuda_set_device once in main, src/cli/bcnn_cl.c:281-285,
 * src/bcnn_utils.c:201): N processes, each after bcnn_hip_set_device(local rank), form one communicator.
 *   comm_init     : rank 0 creates the RCCL unique id and publishes it at `id_path` (a file all ranks can see;
 *                   atomic rename), the others wait for it (<= 120 s), then ncclCommInitRank on the current device;
 *                   rank 0 unlinks the file once that collective call has returned. A record left behind by a job
 *                   that died in between is told from this job's by BCNN_HIP_JOB_NONCE (environment, any string,
 *                   the same on every rank of a job and different per job: records with another nonce are ignored)
 *                   and by its age (older than BCNN_HIP_ID_MAX_AGE_S, default 600 s, when the wait starts = stale).
 *                   world == 1 may pass NULL. RCCL is dlopen'ed here, not linked. One communicator per process,
 *                   reference-counted: comm_retain adds a holder, comm_destroy drops one and tears the
 *                   communicator down with the last (two nets of one process may train over it).
 *   rendezvous_publish / _fetch : the file rendezvous by itself (what comm_init uses for the ncclUniqueId): publish
 *                   stores up to 256 bytes + world size + nonce + time at `path` (0 = ok, -1 = I/O error); fetch
 *                   polls for a record of this job (0 = fetched, 1 = timed out, 2 = published for another world size).
 *   allreduce_sum : in-place sum of n floats across the ranks, queued on the communicator's own stream AFTER the
 *                   work queued so far on the calling thread's stream (event ordering, no host block). Every rank
 *                   must issue the same sequence of calls.
 *   broadcast     : rank `root`'s n floats replace every other rank's, same ordering rules (a data-parallel job
 *                   starts from rank 0's parameters whatever each rank's own initialisation drew).
 *   comm_join     : the calling thread's stream waits for every collective queued so far (no host block).
 * Any RCCL / HIP failure prints and exit()s like every other device error.
 * ------------------------------------------------------------------------------------------- */
void bcnn_hip_comm_init(int rank, int world, const char *id_path);
void bcnn_hip_comm_retain(void);
void bcnn_hip_comm_destroy(void);
int bcnn_hip_rendezvous_publish(const char *path, const void *blob, size_t n, int world);
int bcnn_hip_rendezvous_fetch(const char *path, void *blob, size_t n, int world, int timeout_ms);
int bcnn_hip_comm_world(void);   /* 0 while no communicator exists */
int bcnn_hip_comm_rank(void);
void bcnn_hip_allreduce_sum(float *buf_d, size_t n);
void bcnn_hip_broadcast(float *buf_d, size_t n, int root);
void bcnn_hip_comm_join(void);

#ifdef __cplusplus
}
#endif
#endif /* BCNN_HIP_H */
