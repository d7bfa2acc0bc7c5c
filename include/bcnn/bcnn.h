/*
 * bcnn/bcnn.h -- public C API of the MI355X build of bcnn's conv/GEMM hot path.
 *
 * Source-compatible with the reference's inc/bcnn/bcnn.h (jnbraun/bcnn): same enumerators (values
 * matter for INI files and saved models), same `struct bcnn_tensor` members, same 52 entry points with
 * identical signatures, so `bcnn-cl` and the examples compile against it unchanged.
 * Differences: the device mirror members are guarded by BCNN_USE_HIP (reference: BCNN_USE_CUDA,
 * bcnn.h:251-254) and a few data-parallel helpers are appended at the end (new, no reference
 * counterpart). Entry points outside the hot path return
 * BCNN_INVALID_PARAMETER with a log line; they are listed in INTEGRATION.md.
 */
#ifndef BCNN_H
#define BCNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) && defined(BCNN_BUILD_SHARED)
#define BCNN_API __attribute__((visibility("default")))
#else
#define BCNN_API
#endif

#define BCNN_VERSION_MAJOR 0
#define BCNN_VERSION_MINOR 2
#define BCNN_VERSION_PATCH 0

typedef struct bcnn_net bcnn_net;
typedef struct bcnn_tensor bcnn_tensor;
typedef struct bcnn_output_detection bcnn_output_detection;

/* ---- enumerations (values identical to the reference, bcnn.h:90-242) ---- */
typedef enum {
    BCNN_SUCCESS, BCNN_INVALID_PARAMETER, BCNN_INVALID_DATA, BCNN_INVALID_MODEL, BCNN_FAILED_ALLOC,
    BCNN_INTERNAL_ERROR, BCNN_CUDA_FAILED_ALLOC, BCNN_UNKNOWN_ERROR
} bcnn_status;

typedef enum { BCNN_MODE_PREDICT, BCNN_MODE_TRAIN, BCNN_MODE_VALID } bcnn_mode;

typedef enum {
    BCNN_LOAD_MNIST, BCNN_LOAD_CIFAR10, BCNN_LOAD_CLASSIFICATION_LIST, BCNN_LOAD_REGRESSION_LIST,
    BCNN_LOAD_DETECTION_LIST, BCNN_NUM_LOADERS
} bcnn_loader_type;
/* The segmentation-list loader ("image-path mask-path" lines; bcnn_set_data_loader below), the value behind the
 * enumerator list: a constant of the enum's type next to the enum, like the layer types since BCNN_LAYER_POOL2D, so that
 * the enumerators and BCNN_NUM_LOADERS keep the reference's values. */
#define BCNN_LOAD_SEGMENTATION_LIST ((bcnn_loader_type)(BCNN_NUM_LOADERS + 1))

typedef enum {
    BCNN_LR_DECAY_CONSTANT, BCNN_LR_DECAY_STEP, BCNN_LR_DECAY_INV, BCNN_LR_DECAY_EXP, BCNN_LR_DECAY_POLY,
    BCNN_LR_DECAY_SIGMOID
} bcnn_lr_decay;

typedef enum {
    BCNN_LAYER_CONV2D, BCNN_LAYER_TRANSPOSE_CONV2D, BCNN_LAYER_DEPTHWISE_CONV2D, BCNN_LAYER_ACTIVATION,
    BCNN_LAYER_FULL_CONNECTED, BCNN_LAYER_MAXPOOL, BCNN_LAYER_AVGPOOL, BCNN_LAYER_SOFTMAX, BCNN_LAYER_DROPOUT,
    BCNN_LAYER_BATCHNORM, BCNN_LAYER_LRN, BCNN_LAYER_CONCAT, BCNN_LAYER_ELTWISE, BCNN_LAYER_UPSAMPLE,
    BCNN_LAYER_YOLOV3, BCNN_LAYER_RESHAPE, BCNN_LAYER_COST,
    BCNN_LAYER_POOL2D /* windowed pooling with padding (bcnn_add_pool2d_layer); appended: the values above are the reference's */
} bcnn_layer_type;
/* The layer type of bcnn_add_scale_channels_layer (a feature map times a per-channel or same-shape gate), the value behind
 * BCNN_LAYER_POOL2D. A constant of the enum's type next to the enum, not an enumerator: the enumerator list stays the one
 * tests/test_pool2d_abi.py pins, which ends with BCNN_LAYER_POOL2D. */
#define BCNN_LAYER_SCALE_CHANNELS ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 1))
/* The layer type of bcnn_add_groupnorm_layer, likewise a constant behind the enumerator list. */
#define BCNN_LAYER_GROUPNORM ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 2))
/* The layer type of bcnn_add_dilated_conv_layer with dilation > 1, likewise a constant behind the enumerator list. */
#define BCNN_LAYER_DILATED_CONV2D ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 3))
/* The layer type of bcnn_add_interp_layer, likewise a constant behind the enumerator list. */
#define BCNN_LAYER_INTERP ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 4))
/* The layer type of bcnn_add_softmax_loss_layer, likewise a constant behind the enumerator list. */
#define BCNN_LAYER_SOFTMAX_LOSS ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 5))
/* The layer type of bcnn_add_dilated_depthwise_conv_layer with dilation > 1, likewise a constant behind the enumerator list. */
#define BCNN_LAYER_DILATED_DEPTHWISE_CONV2D ((bcnn_layer_type)(BCNN_LAYER_POOL2D + 6))

typedef enum {
    BCNN_ACT_NONE, BCNN_ACT_TANH, BCNN_ACT_RELU, BCNN_ACT_RAMP, BCNN_ACT_SOFTPLUS,
    BCNN_ACT_LRELU, /* negative slope 0.1 in the code (the reference's comment says 0.01) */
    BCNN_ACT_ABS, BCNN_ACT_CLAMP, BCNN_ACT_PRELU, BCNN_ACT_LOGISTIC,
    /* appended, without a reference counterpart (the values above are the reference's).
     * RELU6 = min(max(x, 0), 6) and HARD_SIGMOID = min(max(x + 3, 0), 6) / 6 (torch's hardsigmoid) are accepted wherever
     * an activation is taken. HARD_SWISH = x min(max(x + 3, 0), 6) / 6, SWISH = x sigmoid(x) and MISH = x tanh(softplus(x))
     * have a derivative that is no function of the output: they exist in the stand-alone activation node
     * (bcnn_add_activation_layer) only, and every builder that takes a fused activation refuses them with
     * BCNN_INVALID_PARAMETER. */
    BCNN_ACT_RELU6, BCNN_ACT_HARD_SIGMOID, BCNN_ACT_HARD_SWISH, BCNN_ACT_SWISH, BCNN_ACT_MISH
} bcnn_activation;

typedef enum { BCNN_LOSS_EUCLIDEAN, BCNN_LOSS_LIFTED_STRUCT } bcnn_loss;

typedef enum {
    BCNN_METRIC_ERROR_RATE, BCNN_METRIC_LOGLOSS, BCNN_METRIC_SSE, BCNN_METRIC_MSE, BCNN_METRIC_CRPS,
    BCNN_METRIC_DICE
} bcnn_loss_metric;

/* The denominator D of the softmax-loss node (bcnn_add_softmax_loss_layer): loss = (sum l) / D, dx = scale / D * (p - y).
 * V is the number of valid pixels of the batch of n images. */
typedef enum {
    BCNN_LOSS_NORM_NONE,           /* D = 1: with no ignored pixel, the gradient of the softmax -> Euclidean cost chain */
    BCNN_LOSS_NORM_VALID,          /* D = max(V, 1): torch's reduction="mean", Caffe's VALID */
    BCNN_LOSS_NORM_VALID_PER_IMAGE /* D = max(V, 1) / n: the learner divides by n again, so the step is the mean over V */
} bcnn_loss_norm;

typedef enum { BCNN_PADDING_SAME, BCNN_PADDING_VALID, BCNN_PADDING_CAFFE } bcnn_padding;

typedef enum { BCNN_OPTIM_SGD, BCNN_OPTIM_ADAM } bcnn_optimizer;

typedef enum { BCNN_LOG_INFO = 0, BCNN_LOG_WARNING = 1, BCNN_LOG_ERROR = 2, BCNN_LOG_SILENT = 3 } bcnn_log_level;

typedef enum bcnn_filler_type { BCNN_FILLER_FIXED, BCNN_FILLER_XAVIER, BCNN_FILLER_MSRA } bcnn_filler_type;

#define BCNN_DETECTION_MAX_BOXES 50

typedef void (*bcnn_log_callback)(const char *fmt, ...);

/* Dense NCHW fp32 tensor. Host buffers are 32-byte aligned and zero-initialised; with BCNN_USE_HIP
 * every tensor also owns device mirrors that the kernels work on (sync points: INTEGRATION.md). */
struct bcnn_tensor {
    int n;            /* batch */
    int c;            /* channels */
    int h;            /* height */
    int w;            /* width */
    int has_grad;     /* carries a gradient buffer in TRAIN/VALID nets */
    char *name;
    float *data;
    float *grad_data;
#ifdef BCNN_USE_HIP
    float *data_gpu;
    float *grad_data_gpu;
#endif
};

struct bcnn_output_detection {
    int num_classes;
    float x, y, w, h;
    float *prob;
    float *mask;
    float objectness;
};

/* ---- net life cycle ---- */
BCNN_API bcnn_status bcnn_init_net(bcnn_net **net, bcnn_mode mode);
BCNN_API void bcnn_end_net(bcnn_net **net);
BCNN_API void bcnn_set_log_context(bcnn_net *net, bcnn_log_callback fct, bcnn_log_level level);
BCNN_API bcnn_status bcnn_set_num_threads(bcnn_net *net, int num_threads, const int *cpu_ids);
BCNN_API int bcnn_get_num_threads(bcnn_net *net);
BCNN_API void bcnn_set_input_shape(bcnn_net *net, int width, int height, int channels, int batch_size);
BCNN_API bcnn_status bcnn_add_input(bcnn_net *net, int width, int height, int channels, const char *name);
BCNN_API int bcnn_get_batch_size(bcnn_net *net);
/* New input extent at batch 1; every node's first destination tensor is re-shaped and, with need_realloc, re-allocated.
 * A layer's private buffers (batch-norm workspaces, pooling indexes, saved activation inputs) follow by their allocated
 * capacity: a shape within it allocates nothing; past it they grow with need_realloc and the call is refused without.
 * Every refusal (BCNN_INVALID_PARAMETER) is found before anything changes: the net is left exactly as it was.
 * After BCNN_FAILED_ALLOC the net is only fit for bcnn_end_net. */
BCNN_API bcnn_status bcnn_resize_net(bcnn_net *net, int w, int h, int c, int need_realloc);
BCNN_API bcnn_status bcnn_compile_net(bcnn_net *net);
BCNN_API bcnn_status bcnn_load_weights(bcnn_net *net, const char *model_path);
BCNN_API bcnn_status bcnn_load_net(bcnn_net *net, const char *config_path, const char *model_path);
BCNN_API bcnn_status bcnn_save_weights(bcnn_net *net, const char *filename);

/* ---- data ---- */
BCNN_API bcnn_status bcnn_set_data_loader(bcnn_net *net, bcnn_loader_type type, const char *train_path_data,
                                          const char *train_path_extra, const char *test_path_data,
                                          const char *test_path_extra);
BCNN_API void bcnn_augment_data_with_shift(bcnn_net *net, int width_shift_range, int height_shift_range);
BCNN_API void bcnn_augment_data_with_scale(bcnn_net *net, float min_scale, float max_scale);
BCNN_API void bcnn_augment_data_with_rotation(bcnn_net *net, float rotation_range);
BCNN_API void bcnn_augment_data_with_flip(bcnn_net *net, int horizontal_flip, int vertical_flip);
BCNN_API void bcnn_augment_data_with_color_adjustment(bcnn_net *net, int min_brightness, int max_brightness,
                                                      float min_constrast, float max_contrast);
BCNN_API void bcnn_augment_data_with_blobs(bcnn_net *net, int max_blobs);
BCNN_API void bcnn_augment_data_with_distortion(bcnn_net *net, float distortion);
BCNN_API bcnn_status bcnn_fill_tensor_with_image(bcnn_net *net, const uint8_t *src, int w, int h, int c,
                                                 float norm_coeff, int swap_to_bgr, float mean_r, float mean_g,
                                                 float mean_b, int tensor_index, int batch_index);
/* New, without a reference counterpart: batch entries 0 .. num_images - 1 of tensor `tensor_index` from raw images, in
 * one call, prepared ON THE DEVICE (one host-to-device copy of the uint8 pixels and one kernel for the whole batch;
 * bcnn_fill_tensor_with_image uploads the whole float tensor once per image). Entries num_images .. n - 1 keep their
 * device content. images[b]: interleaved HWC uint8, widths[b] x heights[b] x c, rows strides[b] bytes apart (strides
 * NULL: widths[b] * c). With W x H the tensor's extent, image b becomes, bit for bit,
 *   STRETCH   : bip_resize_bilinear(images[b], widths[b], heights[b], strides[b], tmp, W, H, W * c, c), then
 *               bcnn_convert_img_to_float(tmp, W, H, c, norm_coeff, swap_to_bgr, mean_r, mean_g, mean_b, entry b);
 *               an image already W x H goes through the same arithmetic (the identity there);
 *   LETTERBOX : the rule of the reference's examples/yolo: if (float)W / w < (float)H / h then new_w = W,
 *               new_h = (h * W) / w, else new_h = H, new_w = (w * H) / h (integer divisions); resized to new_w x new_h,
 *               pasted at ((W - new_w) / 2, (H - new_h) / 2) onto a canvas whose every byte is 128, and the canvas
 *               converted. This is the geometry bcnn_yolo_get_detections[_batch] with netw = W, neth = H undoes.
 * As in bcnn_convert_img_to_float, the channel swap applies only when c == 3 and mean_r serves every channel when c != 3.
 * Returns BCNN_INVALID_PARAMETER with a log line, leaving the tensor as it was and queuing nothing, when tensor_index
 * is out of range or the tensor has no device buffer; num_images < 1 or above the batch size; c differs from the
 * tensor's or is outside 1..4; images, widths, heights or an images[b] is NULL; a width or height is below 1; a stride
 * is below widths[b] * c; fit is unknown; a letterbox extent comes out 0; or the pixels of the batch exceed 2 GiB.
 * The tensor's HOST data is not written: bcnn_download_tensor refreshes it, as for every tensor a kernel wrote. The work
 * is queued on the calling thread's stream; the images are copied to a staging buffer before the call returns, so the
 * caller may free or overwrite them at once. */
typedef enum { BCNN_IMAGE_FIT_STRETCH = 0, BCNN_IMAGE_FIT_LETTERBOX = 1 } bcnn_image_fit;
BCNN_API bcnn_status bcnn_fill_tensor_with_images(bcnn_net *net, int tensor_index, int num_images,
                                                  const uint8_t *const *images, const int *widths, const int *heights,
                                                  const int *strides, int c, bcnn_image_fit fit, float norm_coeff,
                                                  int swap_to_bgr, float mean_r, float mean_g, float mean_b);
/* New, without a reference counterpart: the same from COMPRESSED images. buffers[b] / lengths[b] hold one JPEG stream
 * each (what bip_load_image_from_memory decodes: 8-bit Huffman, baseline or progressive, 1 or 3 components). The host
 * only parses the headers and runs the entropy decoder, straight into the staging buffer; inverse DCT, chroma upsampling
 * and colour conversion run on the device, followed by the resize / letterbox / conversion above, so that decoded
 * pixels never exist on the host. Entry b equals, bit for bit, what bcnn_fill_tensor_with_images makes of the pixels
 * bip_load_image_from_memory returns for buffers[b]. `fit` is a bcnn_image_fit value; norm_coeff, swap_to_bgr and the
 * means are as above. With bcnn_set_num_threads(net, T, ...) and T > 1 the entropy decoding of the images is spread over T
 * host threads, created and joined inside the call; the result does not depend on T.
 * The call is refused as a whole -- BCNN_INVALID_PARAMETER, a log line, the tensor as it was, nothing queued -- when
 * tensor_index is out of range or the tensor has no device buffer; num_images < 1 or above the batch size; buffers,
 * lengths or a buffers[b] is NULL; fit is unknown; a stream cannot be decoded; its component count differs from the
 * tensor's c; its fitted extent is empty; or the staging block would pass 2 GiB. *failed_image (may be NULL) receives
 * the index of the image a refusal is about, -1 otherwise. Host data, stream and staging are as above: the buffers may
 * be freed or overwritten as soon as the call returns. */
BCNN_API bcnn_status bcnn_fill_tensor_with_jpegs(bcnn_net *net, int tensor_index, int num_images,
                                                 const uint8_t *const *buffers, const size_t *lengths, int fit,
                                                 float norm_coeff, int swap_to_bgr, float mean_r, float mean_g,
                                                 float mean_b, int *failed_image);

/* ---- training set-up ---- */
BCNN_API bcnn_status bcnn_set_mode(bcnn_net *net, bcnn_mode mode);
BCNN_API void bcnn_set_adam_optimizer(bcnn_net *net, float learning_rate, float beta1, float beta2);
BCNN_API void bcnn_set_sgd_optimizer(bcnn_net *net, float learning_rate, float momentum);
BCNN_API void bcnn_set_learning_rate_policy(bcnn_net *net, bcnn_lr_decay decay_type, float gamma, float scale,
                                            float power, int max_batches, int step);
BCNN_API void bcnn_set_weight_regularizer(bcnn_net *net, float weight_decay);

/* ---- execution ---- */
BCNN_API void bcnn_forward(bcnn_net *net);
BCNN_API void bcnn_backward(bcnn_net *net);
BCNN_API void bcnn_update(bcnn_net *net);
BCNN_API float bcnn_train_on_batch(bcnn_net *net);
BCNN_API float bcnn_predict_on_batch(bcnn_net *net, bcnn_tensor **out);
BCNN_API bcnn_output_detection *bcnn_yolo_get_detections(bcnn_net *net, int batch, int width, int height, int netw,
                                                         int neth, float thresh, int relative, int *num_dets);
BCNN_API int bcnn_get_tensor_index_by_name(bcnn_net *net, const char *name);
BCNN_API bcnn_tensor *bcnn_get_tensor_by_index(bcnn_net *net, int index);
BCNN_API bcnn_tensor *bcnn_get_tensor_by_name(bcnn_net *net, const char *name);

/* ---- layer builders ---- */
BCNN_API bcnn_status bcnn_add_convolutional_layer(bcnn_net *net, int num_filters, int size, int stride, int pad,
                                                  int num_groups, int batch_norm, bcnn_filler_type init,
                                                  bcnn_activation activation, int quantize, const char *src_id,
                                                  const char *dst_id);
BCNN_API bcnn_status bcnn_add_deconvolutional_layer(bcnn_net *net, int num_filters, int size, int stride, int pad,
                                                    bcnn_filler_type init, bcnn_activation activation,
                                                    const char *src_id, const char *dst_id);
/* Dilated (atrous) convolution: a size x size kernel whose taps sit `dilation` pixels apart, output extent
 * (h + 2 pad - dilation (size - 1) - 1) / stride + 1; weights "<src>_w" [num_filters][c / num_groups][size][size], biases
 * "<src>_b". dilation == 1 delegates to bcnn_add_convolutional_layer (no batch-norm) and builds an ordinary
 * BCNN_LAYER_CONV2D; dilation > 1 builds a BCNN_LAYER_DILATED_CONV2D node (fp32 in every precision mode; bcnn_resize_net
 * refuses a net that holds one). Refused with BCNN_INVALID_PARAMETER, nothing added: an unknown src, num_filters < 1,
 * size < 1, stride < 1, pad < 0, dilation < 1, num_groups < 1 or not dividing both channel counts, a non-positive output
 * extent, PReLU, and the activations that need the layer's input (hard-swish, swish, mish). */
BCNN_API bcnn_status bcnn_add_dilated_conv_layer(bcnn_net *net, int num_filters, int size, int stride, int pad,
                                                 int dilation, int num_groups, bcnn_filler_type init,
                                                 bcnn_activation activation, const char *src_id, const char *dst_id);
/* Dilated (atrous) depthwise convolution: one size x size filter per channel whose taps sit `dilation` pixels apart, output
 * extent (h + 2 pad - dilation (size - 1) - 1) / stride + 1; weights "<src>_w" (c * size * size floats laid out
 * [c][size][size]), biases "<src>_b", the depthwise node's tensors. dilation == 1 delegates to
 * bcnn_add_depthwise_conv_layer and builds an ordinary BCNN_LAYER_DEPTHWISE_CONV2D; dilation > 1 builds a
 * BCNN_LAYER_DILATED_DEPTHWISE_CONV2D node (fp32 in every precision mode, no batch-norm fusion; bcnn_resize_net refuses a
 * net that holds one). Refused with BCNN_INVALID_PARAMETER, nothing added: an unknown src, size < 1, stride < 1, pad < 0,
 * dilation < 1, a non-positive output extent, PReLU, and the activations that need the layer's input (hard-swish, swish,
 * mish). */
BCNN_API bcnn_status bcnn_add_dilated_depthwise_conv_layer(bcnn_net *net, int size, int stride, int pad, int dilation,
                                                           bcnn_filler_type init, bcnn_activation activation,
                                                           const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_depthwise_conv_layer(bcnn_net *net, int size, int stride, int pad, int batch_norm,
                                                   bcnn_filler_type init, bcnn_activation activation,
                                                   const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_batchnorm_layer(bcnn_net *net, const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_lrn_layer(bcnn_net *net, int local_size, float alpha, float beta, float k,
                                        const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_fullc_layer(bcnn_net *net, int output_size, bcnn_filler_type init,
                                          bcnn_activation activation, int quantize, const char *src_id,
                                          const char *dst_id);
BCNN_API bcnn_status bcnn_add_activation_layer(bcnn_net *net, bcnn_activation type, const char *id);
BCNN_API bcnn_status bcnn_add_softmax_layer(bcnn_net *net, const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_maxpool_layer(bcnn_net *net, int size, int stride, bcnn_padding padding,
                                            const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_avgpool_layer(bcnn_net *net, const char *src_id, const char *dst_id);
/* New, without a reference counterpart: max or average pooling over a square window of `size`, `stride` apart, with `pad`
 * on all four sides -- the rules of torch.nn.functional.max_pool2d / avg_pool2d, which are Caffe's. The two builders above
 * keep their meaning (max pooling padded at the bottom / right only, average pooling over the whole plane).
 *   out = floor_or_ceil((in + 2 pad - size) / stride) + 1 per axis; with ceil_mode, one less if the last window would start
 *   past the input and its leading padding. Window (i, j) covers rows i stride - pad .. + size - 1, clipped to the input.
 *   BCNN_POOL2D_MAX: the first maximum in row-major order wins, padding never does. BCNN_POOL2D_AVG: the sum of the real
 *   elements over the window's extent clipped to input + padding (count_include_pad != 0), or over the number of real
 *   elements (count_include_pad == 0); count_include_pad is ignored for max pooling.
 * Refused with BCNN_INVALID_PARAMETER and a log line, nothing added to the net: an unknown kind, size < 1, stride < 1,
 * pad < 0, pad > size / 2, in + 2 pad < size on either axis, an output extent <= 0. Works in TRAIN, VALID and PREDICT
 * mode, has no weights (model files skip it) and follows bcnn_resize_net. */
typedef enum { BCNN_POOL2D_MAX = 0, BCNN_POOL2D_AVG = 1 } bcnn_pool2d_kind;
BCNN_API bcnn_status bcnn_add_pool2d_layer(bcnn_net *net, bcnn_pool2d_kind kind, int size, int stride, int pad,
                                           int ceil_mode, int count_include_pad, const char *src_id, const char *dst_id);
/* New, without a reference counterpart: dst = src * gate, the last step of a squeeze-and-excitation block (Darknet's
 * [scale_channels]) or, with a gate of src's shape, of a spatial attention module (Darknet's [sam]).
 *   src is [N,C,H,W]; gate is [N,C,1,1] (one factor per plane) or [N,C,H,W] (the plain product); dst gets src's shape.
 *   Backward: dsrc += ddst * gate and dgate += sum over the plane of ddst * src (elementwise for the same-shape gate);
 *   both accumulate, and a source without a gradient buffer is skipped. The plane sums use no atomics: two runs give
 *   the same bits.
 * Refused with BCNN_INVALID_PARAMETER and a log line, nothing added to the net: an unknown src or gate name, a gate of
 * any other shape. Works in TRAIN, VALID and PREDICT mode, has no weights (model files skip it) and follows
 * bcnn_resize_net (dst is reshaped like src). */
BCNN_API bcnn_status bcnn_add_scale_channels_layer(bcnn_net *net, const char *src_id, const char *gate_id,
                                                   const char *dst_id);
/* New, without a reference counterpart: group normalisation of src [N,C,H,W] over num_groups groups of C / num_groups
 * consecutive channels, per image: dst = (src - mean) * rstd * scales[ch] + b[ch], mean and the biased variance over the
 * group's (C / num_groups) * H * W values, rstd = 1 / sqrt(var + eps). num_groups == 1 is layer norm over (C,H,W),
 * num_groups == C instance norm with affine. eps <= 0 selects 1e-5. The same function in TRAIN, VALID and PREDICT mode: no
 * running statistics.
 *   Parameters <src>_gn_scales (filled with 1) and <src>_gn_b (0), [1,1,1,C], trained like a layer's weights and biases
 *   (the scales take the weights' rule, weight decay included). Model files hold b then scales, C floats each; the
 *   Darknet reader skips the node.
 *   A net built in TRAIN or VALID mode keeps mean and rstd of the last forward, [2][N * num_groups] floats:
 *   bcnn_get_node_state(net, node, 0). The backward recomputes the normalised values from them. It adds into the source
 *   gradient (assigns when it is its sole writer); a source without a gradient buffer is skipped.
 * Refused with BCNN_INVALID_PARAMETER and a log line, nothing added to the net: an unknown src name, num_groups <= 0,
 * num_groups that does not divide C. May be the first node of a net. Follows bcnn_resize_net (dst is reshaped like src). */
BCNN_API bcnn_status bcnn_add_groupnorm_layer(bcnn_net *net, int num_groups, float eps, const char *src_id,
                                              const char *dst_id);
BCNN_API bcnn_status bcnn_add_concat_layer(bcnn_net *net, int num_src, char *const *src_ids, const char *dst_id);
BCNN_API bcnn_status bcnn_add_eltwise_layer(bcnn_net *net, bcnn_activation activation, const char *src_id1,
                                            const char *src_id2, const char *dst_id);
BCNN_API bcnn_status bcnn_add_dropout_layer(bcnn_net *net, float rate, const char *id);
BCNN_API bcnn_status bcnn_add_upsample_layer(bcnn_net *net, int size, const char *src_id, const char *dst_id);
/* New, without a reference counterpart: bilinear interpolation of every plane of src to a new extent, with a gradient --
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=...) with the extents given as size=; Caffe-DeepLab's
 * Interp layer is align_corners = 1. The upsample builder above keeps its meaning (nearest neighbour, integer factor).
 *   The output extent is given in exactly one of three forms, the other arguments 0:
 *     scale >= 1               out = in * scale
 *     zoom >= 1                out = (in - 1) * zoom + 1      (Interp's zoom_factor: 65 -> 513 with zoom 8)
 *     out_w > 0 && out_h > 0   out_w x out_h; downsampling is allowed
 *   Per axis (float32, every operation rounded on its own): align_corners != 0: src = o * (in - 1) / (out - 1), 0 for
 *   out == 1; align_corners == 0: src = max((o + 0.5) * in / out - 0.5, 0). i0 = min((int)src, in - 1), i1 = i0 + 1
 *   clipped to the axis, l1 = src - i0 clamped to [0, 1], l0 = 1 - l1; dst = h0 (w0 a + w1 b) + h1 (w0 c + w1 d).
 *   Backward: a gather without atomics, the same bits on every run. It adds into the source gradient (assigns when it is
 *   its sole writer); a source without a gradient buffer is skipped.
 * Refused with BCNN_INVALID_PARAMETER and a log line, nothing added to the net: an unknown src name, a negative argument,
 * no form or more than one, only one of out_w and out_h, an output extent of 2^31 - 1 or more. May be the first node of a
 * net (src_id is then the input tensor's name). Works in TRAIN, VALID and PREDICT mode in fp32, has no weights (model
 * files skip it) and follows bcnn_resize_net: scale and zoom follow the new source extent, the fixed form keeps its own. */
BCNN_API bcnn_status bcnn_add_interp_layer(bcnn_net *net, int out_w, int out_h, int scale, int zoom, int align_corners,
                                           const char *src_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_cost_layer(bcnn_net *net, bcnn_loss loss, bcnn_loss_metric loss_metric, float scale,
                                         const char *src_id, const char *label_id, const char *dst_id);
BCNN_API bcnn_status bcnn_add_yolo_layer(bcnn_net *net, int num_boxes_per_cell, int num_classes, int coords,
                                         int total, int *mask, float *anchors, const char *src_id,
                                         const char *dst_id);
/* New, without a reference counterpart: softmax over the channels of src ([n][C][h][w] logits) and cross-entropy against a
 * class-index label map -- torch's F.cross_entropy(src, label, ignore_index=ignore_label). The softmax and cost builders
 * above keep their meaning. dst is [n][C][h][w] and holds the probabilities; the label is tensor 1, which the builder
 * shapes and allocates as [n][1][h][w]: class indices stored as floats, written and uploaded by the caller
 * (bcnn_upload_tensor(net, 1, 0)). label_id is ignored like the cost builder's.
 *   One label value t is: ignored if ignore_label >= 0 and t == ignore_label; valid if it is an integer value in [0, C);
 *   out of range otherwise (negative, >= C, fractional, not finite) -- that pixel contributes nothing, like an ignored
 *   one, and is counted on its own. ignore_label < 0: nothing is ignored on purpose.
 *   loss = (sum over valid pixels of lse(x) - x[t]) / D and dx = scale / D * (p - [c == t]), exactly +0.0 on every other
 *   pixel, with D by `norm` (bcnn_loss_norm above). V = 0 gives loss 0 and a zero gradient. bcnn_update divides every
 *   gradient by the batch size again: BCNN_LOSS_NORM_VALID_PER_IMAGE makes the step the mean over the valid pixels.
 *   TRAIN and VALID forwards compute probabilities, loss and counts on the device without a host synchronisation;
 *   bcnn_train_on_batch / bcnn_predict_on_batch return the loss like a cost node's, read once at the end of the step.
 *   A PREDICT forward writes the probabilities only. The node's own dst gradient is never read or written.
 * Refused with BCNN_INVALID_PARAMETER and a log line, nothing added or allocated: the first node of a net, an unknown src
 * name, an unknown norm, ignore_label >= 2^24 (no float holds it as an index), a label tensor another node has already
 * shaped differently (a cost node, a YOLO head under detector training). Weightless (model files skip it); follows
 * bcnn_resize_net: dst follows src, the label becomes [n][1][h][w] -- re-allocated with need_realloc, refused in the plan
 * phase when it would outgrow its allocation without. */
BCNN_API bcnn_status bcnn_add_softmax_loss_layer(bcnn_net *net, int ignore_label, bcnn_loss_norm norm, float scale,
                                                 const char *src_id, const char *label_id, const char *dst_id);
/* What the latest TRAIN / VALID forward of softmax-loss node `node` left in its device record (one 24-byte read).
 * BCNN_INVALID_PARAMETER, *out zeroed: not such a node, or its latest forward computed no statistics (PREDICT mode, no
 * forward yet). */
typedef struct {
    float loss;
    int64_t valid, ignored, out_of_range, correct; /* correct: valid pixels whose first argmax of the logits is the label */
} bcnn_softmax_loss_stats;
BCNN_API bcnn_status bcnn_get_softmax_loss_stats(bcnn_net *net, int node, bcnn_softmax_loss_stats *out);
/* counts[t * C + a] = valid pixels with label t whose first argmax of the probabilities is a, from the probabilities and
 * the label the latest forward left on the device (one kernel, launched by this call; not on the training path). Its trace
 * is the record's `correct`, its total `valid`. BCNN_INVALID_PARAMETER: not such a node, counts NULL, no label on the device. */
BCNN_API bcnn_status bcnn_get_confusion_matrix(bcnn_net *net, int node, int64_t *counts);
/* New, without a reference counterpart: the output end of semantic segmentation. Tensor `tensor_index` -- any
 * [n][C][h][w] tensor with a device buffer, the logits or the softmax-loss node's probabilities -- becomes one class index
 * (a byte) per pixel of each of the first num_images images of the batch AT THAT IMAGE'S OWN SIZE widths[b] x heights[b],
 * on the device: the part of plane b that image b occupies is resampled bilinearly to the image's extent (the interp
 * node's rule for the given align_corners, bit for bit) and the label is the first maximum over the C classes. The
 * resampled floats are never stored and only the bytes are read back: one copy in, one kernel for the whole batch whatever
 * the sizes, one copy back. The call interpolates what it is given: the argmax of interpolated logits and of interpolated
 * probabilities can differ (softmax is not linear), so name the tensor you mean.
 *   fit is a bcnn_image_fit value (an int here, as in bcnn_fill_tensor_with_jpegs) and must be the one the batch was
 *   filled with (bcnn_fill_tensor_with_images / _jpegs):
 *     STRETCH   : the whole plane is the image, for a tensor of any extent -- a DeepLab head's 65 x 65 logits go straight
 *                 to image size;
 *     LETTERBOX : the image occupies the integer rectangle (x_off, y_off, new_w, new_h) documented at
 *                 bcnn_fill_tensor_with_images; accepted only when the tensor's h x w equals tensor 0's (resampling a
 *                 letterboxed low-resolution head needs a fractional rectangle and is out of scope).
 *   labels[b] receives heights[b] rows of widths[b] bytes, strides[b] bytes apart (strides NULL: widths[b]); the bytes
 *   between the width and the stride are not written. labels may be NULL when eval is given.
 *   eval (may be NULL) scores the labels against truth maps of the images' own sizes -- what VOC / Cityscapes / ADE20K
 *   call mIoU; bcnn_get_confusion_matrix counts at the net's extent against the augmented label tensor, a training
 *   statistic. truths[b]: heights[b] rows of widths[b] bytes, eval->strides[b] apart (NULL: widths[b]). A truth byte t is
 *   ignored (ignore_label >= 0 and t == ignore_label), valid (t < C) or out of range; a valid pixel labelled a adds 1 to
 *   counts[t * C + a]. counts (C * C), ignored and out_of_range are ADDED into: zero them before the first batch of a
 *   validation set. Integer arithmetic only: two runs give the same counts.
 * The results are complete when the call returns (it synchronises the calling thread's stream once).
 * Returns BCNN_INVALID_PARAMETER with a log line, every output untouched and nothing queued, when tensor_index is out of
 * range or the tensor has no device buffer; num_images < 1 or above the batch size; the tensor has more than 256 channels;
 * widths or heights is NULL or holds a value below 1; fit is unknown, or LETTERBOX on a tensor of another extent than
 * tensor 0's, or a letterbox extent comes out 0; labels and eval are both NULL; a labels[b] or truths[b] is NULL; a stride
 * is below widths[b]; eval has no truths or no counts; eval->ignore_label >= 256 (no byte equals it; negative: nothing is
 * ignored); or the label maps of the batch, with their truths, exceed 2 GiB. */
typedef struct {
    const uint8_t *const *truths;
    const int *strides;
    int ignore_label;
    int64_t *counts;
    int64_t ignored, out_of_range;
} bcnn_label_map_eval;
BCNN_API bcnn_status bcnn_get_label_maps_batch(bcnn_net *net, int tensor_index, int num_images, const int *widths,
                                               const int *heights, int fit, int align_corners,
                                               uint8_t *const *labels, const int *strides, bcnn_label_map_eval *eval);

/* ---------------------------------------------------------------------------------------------
 * Additions of the MI355X build (no reference counterpart).
 *  - bcnn_upload_tensor / bcnn_download_tensor: push a user-written host buffer to its device mirror
 *    and back (the reference has no public call for this; its CUDA build only syncs inside the
 *    data loader, bcnn_data.c:413-425).
 *  - data parallel: one process per GPU. After bcnn_compile_net every weight/bias gradient lives in
 *    ONE contiguous device arena; a launcher all-reduces (sum) that arena over RCCL between
 *    bcnn_backward and bcnn_update and tells the net the world size so the SGD step divides by the
 *    global batch and rescales the momentum carry ("data parallel").
 * ------------------------------------------------------------------------------------------- */
BCNN_API bcnn_status bcnn_upload_tensor(bcnn_net *net, int tensor_index, int with_grad);
BCNN_API bcnn_status bcnn_download_tensor(bcnn_net *net, int tensor_index, int with_grad);
BCNN_API bcnn_status bcnn_set_data_parallel(bcnn_net *net, int rank, int world_size);
/* The same, with the collective INSIDE the library (RCCL over xGMI, include/bcnn_hip.h): for a plain C program run as
 * one process per GPU (the reference's process model, src/cli/bcnn_cl.c:281-285). Call after bcnn_hip_set_device /
 * before training; `id_path` names a file every rank can reach, unique per job, through which rank 0 hands out the
 * RCCL id (world_size == 1 may pass NULL). From then on bcnn_backward all-reduces (sum) the weight-gradient arena
 * itself -- in ~8 MB buckets as the owning nodes finish, on the communicator's stream, overlapped with the rest of
 * backward -- and bcnn_update is ordered behind the last bucket; bcnn_train_on_batch needs no other change. The
 * communicator is destroyed by bcnn_end_net. A launcher that runs the collective itself (bench.py through
 * torch.distributed) keeps using bcnn_set_data_parallel + bcnn_get_gradient_arena. */
BCNN_API bcnn_status bcnn_set_data_parallel_comm(bcnn_net *net, int rank, int world_size, const char *id_path);
/* bcnn_backward queues the weight-gradient kernels of a pass on a second stream of the library, next to the sweeps and
 * data gradients of the layers in front, and joins it at the end of the pass (include/bcnn_hip.h:
 * bcnn_hip_conv_side_stream_mode). enable = 0 keeps everything on the caller's stream (a profiler
 * that wants every kernel alone, bench.py's `roofline.alone` leg); the results are the same bit for bit either way. */
BCNN_API void bcnn_set_weight_gradient_stream(bcnn_net *net, int enable);
BCNN_API float *bcnn_get_gradient_arena(bcnn_net *net, size_t *num_floats);  /* device pointer */
BCNN_API float *bcnn_get_parameter_arena(bcnn_net *net, size_t *num_floats); /* device pointer */
/* Overlap of the gradient all-reduce with backward. Parameters sit in the arena in node order and backward
 * visits the nodes in reverse, so the finished gradients always form a growing TAIL of the arena: `fn` is
 * called from inside bcnn_backward (same thread, after the owning node's work has been queued on the
 * stream) with the newly completed range [first_float, first_float + num_floats). The caller may queue a
 * collective on that range that depends on the stream's work so far. NULL removes the callback. */
typedef void (*bcnn_gradient_ready_fn)(size_t first_float, size_t num_floats, void *user);
BCNN_API void bcnn_set_gradient_ready_callback(bcnn_net *net, bcnn_gradient_ready_fn fn, void *user);
BCNN_API void bcnn_synchronize(bcnn_net *net);
/* borrowed pointer to tensor `index` WITHOUT the device->host refresh bcnn_get_tensor_by_index performs */
BCNN_API bcnn_tensor *bcnn_peek_tensor(bcnn_net *net, int index);
BCNN_API int bcnn_get_num_nodes(bcnn_net *net);
BCNN_API int bcnn_get_node_tensor(bcnn_net *net, int node, int is_dst, int slot); /* -1 if out of range */
/* layer-private device state needed by parity tests: which = 0 maxpool indexes (int*), 1 saved_mean,
 * 2 saved_variance, 3 d(saved_mean), 4 d(saved_variance), 5 the pre-normalisation values a batch-norm's backward works
 * from (the reference's param->workspace: a fused-BN convolution's raw output / a batch-norm node's kept input);
 * returns a DEVICE pointer or NULL */
BCNN_API void *bcnn_get_node_state(bcnn_net *net, int node, int which);
/* On a stand-alone activation node, which = 0 is the input the last TRAIN forward kept (hard-swish / swish / mish; NULL for
 * every other activation and in a net built in PREDICT mode).
 * The node's bcnn_layer_type, and the bcnn_activation of a node that has one (-1: it has none, or `node` is out of range) */
BCNN_API int bcnn_get_node_type(bcnn_net *net, int node);
BCNN_API int bcnn_get_node_activation(bcnn_net *net, int node);
/* Seed of the dropout masks (default 0). Node i of data-parallel rank r draws its mask from a Philox4x32-10 keyed by
 * (seed, i, r), counted by its TRAIN forwards (include/bcnn_hip.h): the same seed gives the same masks run after run.
 * Takes effect at the next TRAIN forward. */
BCNN_API void bcnn_set_dropout_seed(bcnn_net *net, uint64_t seed);
/* Loss value and number of positive pairs P of the latest forward of the LAST cost node with
 * BCNN_LOSS_LIFTED_STRUCT (the node's output holds the metric, as in the reference, so the loss is not visible
 * otherwise). An 8-byte read-back; either pointer may be NULL. BCNN_INVALID_PARAMETER if the net has no such node.
 * A batch without a positive pair gives loss 0 and P 0. */
BCNN_API bcnn_status bcnn_get_lifted_struct_loss(bcnn_net *net, float *loss, int *num_constraints);
/* Precision of the convolution nodes in an inference forward (default BCNN_PRECISION_FP32). With BCNN_PRECISION_BF16 every
 * convolution node of a forward pass in BCNN_MODE_PREDICT or BCNN_MODE_VALID runs on the bf16 matrix cores: activations and
 * weights stay fp32 in memory and are rounded to bf16 (round-to-nearest-even) inside the kernel, the accumulator is fp32,
 * bias / fused batch-norm / activation are computed as before. The output of a node then differs from the fp32 one by at
 * most about 2^-8 * sum |x| |w| per element, which is outside the 1e-4 parity the default path holds:
 * hence opt-in. Every convolution node takes it, whatever its shape, so that the numerics of a net are predictable.
 * Depthwise-convolution (dilated or not), deconvolution, dilated-convolution and full-connected nodes stay fp32. The value may be set in any mode and takes
 * effect only while the net's mode is PREDICT or VALID: a BCNN_MODE_TRAIN pass never uses it (its backward needs the fp32
 * forward). An unknown value returns BCNN_INVALID_PARAMETER and changes nothing. Config files: `inference_precision=bf16`
 * (or `fp32`) in the [net] section. */
typedef enum { BCNN_PRECISION_FP32 = 0, BCNN_PRECISION_BF16 = 1 } bcnn_precision;
BCNN_API bcnn_status bcnn_set_inference_precision(bcnn_net *net, bcnn_precision p);
BCNN_API bcnn_precision bcnn_get_inference_precision(const bcnn_net *net);
/* Where bcnn_loader_next makes the input batch (default 0: on the host, sample by sample, as the reference does). With
 * on != 0 the host still reads and decodes every sample, crops a list image to the net input and draws the sample's
 * augmentation parameters from rand() in the reference's order and number (net->data_aug holds the latest draws as
 * before; the draws of max_distortion / max_spots are consumed too), but touches no pixel: the raw uint8 samples of the
 * batch and one small record per sample go to the device in one copy, and two kernel launches (whatever the batch size)
 * flip, shift, scale, rotate, adjust contrast and brightness, centre-crop and convert them into the float input tensor.
 * The device tensor holds, bit for bit, what the host path writes for the same files, rand() seed and settings, in every
 * mode (outside BCNN_MODE_TRAIN: centre crop and conversion only) and for every loader type. Labels, skipped samples,
 * wrap-around and rewind are unchanged. tensors[0].data is NOT written and bcnn_loader_next does not upload it;
 * bcnn_get_tensor_by_index / bcnn_download_tensor refresh it from the device as usual. A scale draw that leaves an
 * extent below 1 pixel leaves the sample unscaled, as the host path does. A batch goes the host way regardless when the
 * input tensor has more than 4 channels or no device buffer, or an MNIST / CIFAR-10 record does not match the input's
 * channels, and always for BCNN_LOAD_DETECTION_LIST (this switch alone; bcnn_set_loader_detection_on_device below moves
 * that loader's letterbox to the device). May be called before or after bcnn_set_data_loader /
 * bcnn_compile_net and between batches; without a loader it has no effect. A NULL net returns BCNN_INVALID_PARAMETER.
 * Config files: `loader_on_device=1` in the [net] section. */
BCNN_API bcnn_status bcnn_set_loader_on_device(bcnn_net *net, int on);
BCNN_API int bcnn_get_loader_on_device(const bcnn_net *net);
/* Where the list loaders decode their JPEG entries (default 0: on the host, one file after the other). With on != 0,
 * and only for a batch that goes the device way (bcnn_set_loader_on_device, see above) of a BCNN_LOAD_CLASSIFICATION_LIST
 * or BCNN_LOAD_REGRESSION_LIST loader into an input of 1 or 3 channels, the host reads every file of the batch, parses the
 * JPEG headers and runs the entropy decoder on bcnn_get_num_threads(net) threads (created and joined inside
 * bcnn_loader_next; the batch does not depend on their number). Inverse DCT, chroma upsampling, colour conversion and
 * the crop to the net input (random origin in BCNN_MODE_TRAIN, centred otherwise, drawn on the host in the reference's
 * order) run on the device in front of the augmentation: decoded pixels never exist on the host. Entries that are not
 * JPEG streams the decoder covers, whose component count is not the input's channel count, or that fail to decode are
 * handled as before (PNG / BMP / PNM are decoded on the host; a failed entry repeats the previous sample). The device
 * tensor and the labels are, bit for bit, those of the host path for the same files, rand() seed and settings. A batch
 * whose staging block would pass 2 GiB is decoded on the host. Everywhere else the switch has no effect. Any non-zero
 * value is stored as 1; may be called before a loader exists and between batches; a NULL net returns
 * BCNN_INVALID_PARAMETER. Config files: `loader_decode_on_device=1` in the [net] section. */
BCNN_API bcnn_status bcnn_set_loader_decode_on_device(bcnn_net *net, int on);
BCNN_API int bcnn_get_loader_decode_on_device(const bcnn_net *net);
/* Number of samples of the latest bcnn_loader_next whose pixels were decoded on the device; 0 for a batch made any other
 * way, on a fresh net and for a NULL net. */
BCNN_API int bcnn_get_loader_device_decoded(const bcnn_net *net);
/* Where a BCNN_LOAD_DETECTION_LIST batch is letterboxed and augmented (default 0: on the host, image by image). With
 * on != 0, and only while bcnn_set_loader_on_device is on as well and the input tensor has a device buffer and 1 to 4
 * channels, the host reads the list, decodes every file (on bcnn_get_num_threads(net) threads, created and joined inside
 * bcnn_loader_next; the batch does not depend on their number), computes the letterbox extent, draws the offsets, the
 * flip and the augmentation parameters from rand() in the host path's order and number, and writes the labels -- but
 * touches no pixel: the decoded images of the batch go to the device in one copy, and three kernel launches (whatever the
 * batch size and the image sizes) resize them with bip_resize_bilinear's integer rule, paste them on the canvas of 128 at
 * the drawn offsets, augment the canvas and convert it into the float input tensor. The device tensor, the labels and
 * the state of rand() are, bit for bit, those of the host path for the same files, seed and settings, in every mode;
 * skipped entries, their warnings, the limit of 1000 failures in a row, wrap-around and rewind are unchanged.
 * tensors[0].data is NOT written and not uploaded. bcnn_set_loader_decode_on_device has no effect on this loader and
 * bcnn_get_loader_device_decoded stays 0 there. A batch whose staging block would pass 2 GiB, or that holds an image whose
 * letterbox is larger than the canvas (a non-square input only: the extent formula is the square input's, and the host
 * path's paste crops such an image), is made on the host from the images already decoded and the draws already made: no
 * draw is repeated, and bcnn_get_loader_device_letterboxed is 0 for it. Everywhere else the switch has no effect. Any non-zero value is
 * stored as 1; may be called before a loader exists and between batches; a NULL net returns BCNN_INVALID_PARAMETER.
 * Config files: `loader_detection_on_device=1` in the [net] section. */
BCNN_API bcnn_status bcnn_set_loader_detection_on_device(bcnn_net *net, int on);
BCNN_API int bcnn_get_loader_detection_on_device(const bcnn_net *net);
/* Number of samples of the latest bcnn_loader_next that were letterboxed on the device; 0 for a batch made any other
 * way, on a fresh net and for a NULL net. */
BCNN_API int bcnn_get_loader_device_letterboxed(const bcnn_net *net);
/* BCNN_LOAD_SEGMENTATION_LIST: number of label maps of the latest bcnn_loader_next that were made on the device (with
 * bcnn_set_loader_on_device the cropped masks of the batch go up in one copy and one kernel writes tensors[1]'s device
 * buffer from the image batch's own records; tensors[1].data is then not written and not uploaded). 0 on the host route,
 * for a batch whose image or labels the device side refused, and for every other loader type; 0 for a NULL net. */
BCNN_API int bcnn_get_loader_device_labels(const bcnn_net *net);
/* Whether bcnn_loader_next applies the augmenter's last two stages, Perlin distortion (config key `max_distortion`) and
 * random spotlights (`max_spots`, bcnn_augment_data_with_blobs), to TRAIN-mode samples (default 0: off). Off, a net whose
 * augmenter has one of the two ranges set draws their parameters from rand() exactly as the reference does (so every other
 * stage sees the reference's random stream) and leaves the pixels alone; one line on stderr says so. On, both effects
 * run after the brightness stage on the stored-size sample, as in the reference, and a run seeded like a reference run
 * sees the reference's samples bit for bit -- on the host path and on the three device routes
 * (bcnn_set_loader_on_device, bcnn_set_loader_decode_on_device, bcnn_set_loader_detection_on_device), which stay
 * bit-identical to the host path: the host draws and tabulates every cos and exp, the device does the per-pixel work in
 * the launch that converts the batch. The switch is independent of those three; the number of rand() calls does not
 * depend on it; outside TRAIN mode nothing is drawn or applied. At most 64 spotlights per sample: bcnn_loader_next returns
 * BCNN_INVALID_PARAMETER for a larger `max_spots` while the switch is on. Any non-zero value is stored as 1; may be
 * called before a loader exists and between batches; a NULL net returns BCNN_INVALID_PARAMETER.
 * Config files: `loader_effects=1` in the [net] section. */
BCNN_API bcnn_status bcnn_set_loader_effects(bcnn_net *net, int on);
BCNN_API int bcnn_get_loader_effects(const bcnn_net *net);
/* Detections of EVERY image of the batch from the latest forward, in one call. widths[b] / heights[b]: the original
 * size of image b (what bcnn_yolo_get_detections takes as w, h). dets[b] receives a malloc'ed array of num_dets[b]
 * boxes (NULL / 0 when image b has no candidate); per image, the result is what
 * bcnn_yolo_get_detections(net, b, widths[b], heights[b], netw, neth, thresh, relative, &n) returns: num_dets[b]
 * counts the boxes NMS suppressed too (objectness 0, prob zeroed), prob holds the classes of the head that produced the
 * box, mask is a zeroed coords - 4 array when coords > 4, the NMS threshold is 0.45, and prob, mask and the array can
 * each be released with free() (or all at once with bcnn_free_detections).
 * The one allowed difference is the place of boxes with EQUAL objectness: the per-image call sorts with qsort, which
 * leaves their order undefined; here boxes come by objectness, descending, and equal ones by candidate index,
 * ascending -- heads in node order, then cell row * w + col, then anchor. A suppressed box keeps the place of its
 * original objectness, as there.
 * Threshold, box decode, compaction and NMS run in kernels queued on the net's stream. The call reads back one block
 * (per-image counts, sort order and compact box records; its size follows the number of boxes kept, never the head
 * tensors, which are not read back) and synchronises once; the block has room for 256 boxes per image, or for 1.25 x
 * the most an image of the net's previous call had; a batch with more runs the kernels a second time with a larger block. Returns BCNN_INVALID_PARAMETER, writing nothing, when the net holds
 * no YOLO node or a pointer argument is NULL. */
BCNN_API bcnn_status bcnn_yolo_get_detections_batch(bcnn_net *net, const int *widths, const int *heights, int netw,
                                                    int neth, float thresh, int relative,
                                                    bcnn_output_detection **dets, int *num_dets);
BCNN_API void bcnn_free_detections(bcnn_output_detection *dets, int num_dets); /* prob, mask and the array */
/* Detector training (default 0: off, and then nothing below applies -- bcnn_add_yolo_layer on a TRAIN net,
 * bcnn_set_mode(TRAIN) on a net with a head and BCNN_LOAD_DETECTION_LIST on a net without one are refused). With on != 0:
 *   - bcnn_add_yolo_layer is accepted on a TRAIN net; in any mode it shapes tensors[1] (the label) as
 *     n x 1 x 1 x (BCNN_DETECTION_MAX_BOXES * 5) and allocates it when it has no data yet: per image up to 50 truths
 *     x, y, w, h, class (centre and extent relative to the input), the list ending at the first x == 0. Such a head
 *     needs coords = 4, a mask of at most 16 anchors and at most 32 anchors in all;
 *   - bcnn_set_mode(TRAIN) is accepted on a net whose heads were all built with the switch on and have gradient
 *     buffers (a net built in PREDICT mode has none and is still refused);
 *   - bcnn_set_data_loader(BCNN_LOAD_DETECTION_LIST) is accepted (also, without the switch, on a net that holds a head);
 *   - a TRAIN-mode forward of a head computes the YOLOv3 loss gradient of the reference (bcnn_yolo.c:250-415) into the
 *     head's output gradient on the device, bcnn_backward carries it on, and bcnn_train_on_batch counts every
 *     head's cost in its return value next to the cost nodes (the mean over all of them, as in the reference).
 * Set it before the heads are built. Config files: `train_detector=1` in the [net] section. A NULL net returns
 * BCNN_INVALID_PARAMETER (the getter: 0). */
BCNN_API bcnn_status bcnn_set_detector_training(bcnn_net *net, int on);
BCNN_API int bcnn_get_detector_training(const bcnn_net *net);
/* The statistics the reference prints on every TRAIN forward of a head ("Yolo Avg IOU: ..."), read on demand instead:
 * one 32-byte copy from the device, divided as there (a batch without an assigned truth gives 0 / 0 for the averages
 * over count). node_index: a YOLO node that has run a TRAIN forward (before one: zeros). Also refreshes the cost the
 * head reports to bcnn_train_on_batch. BCNN_INVALID_PARAMETER for a NULL net / out or a node that is no YOLO head. */
typedef struct bcnn_yolo_train_stats {
    float avg_iou, avg_class, avg_obj, avg_anyobj, recall50, recall75;
    int count;  /* truths that were assigned to an anchor of this head */
    float cost; /* sum of the squared elements of the head's output gradient */
} bcnn_yolo_train_stats;
BCNN_API bcnn_status bcnn_yolo_get_train_stats(bcnn_net *net, int node_index, bcnn_yolo_train_stats *out);
/* Run ONE node's forward / backward worker on whatever its tensors currently hold (no executor bookkeeping:
 * no zero fill of the dst gradients, no dead-fill elision -- a sole-writer gradient is accumulated like in the
 * reference). Used by the teacher-forced parity walk, which feeds every node the REFERENCE's inputs. */
BCNN_API bcnn_status bcnn_forward_node(bcnn_net *net, int node);
BCNN_API bcnn_status bcnn_backward_node(bcnn_net *net, int node);

#ifdef __cplusplus
}
#endif
#endif /* BCNN_H */
