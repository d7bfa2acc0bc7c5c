/*
 * bcnn_internal.h -- host-side (C99) runtime structures of the MI355X build.
 *
 * Struct tags and member names follow the reference's internal headers, because unchanged consumers
 * reach into them (src/cli/bcnn_cl.c:106-199 reads net->learner->max_batches, net->batch_size,
 * net->log_ctx, net->tensors[i], net->nodes[i].{dst,type,param}, net->data_loader->type):
 *   struct bcnn_net      reference src/bcnn_net.h:47-67
 *   struct bcnn_node     reference src/bcnn_node.h:36-48   (the operator plug-in signature)
 *   bcnn_learner         reference src/bcnn_learner.h:29-44
 *   bcnn_loader, bcnn_data_augmenter   reference src/bcnn_data.h:34-103
 *   bcnn_log_context + BCNN_CHECK_* macros   reference src/bcnn_utils.h:48-100
 * The headers bcnn_net.h, bcnn_node.h, bcnn_tensor.h, bcnn_utils.h, bcnn_learner.h, bcnn_data.h and the
 * per-layer headers in this directory are thin includes of this file so that `#include "bcnn_net.h"`
 * etc. keep working. Binary layout is free (consumers are recompiled).
 */
#ifndef BCNN_INTERNAL_H
#define BCNN_INTERNAL_H

#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include <bcnn/bcnn.h>
#include <bip/bip.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- logging / status macros ---------------------------------------------------------------- */
typedef struct {
    bcnn_log_callback fct;
    bcnn_log_level lvl;
} bcnn_log_context;

void bcnn_log(bcnn_log_context ctx, bcnn_log_level level, const char *fmt, ...);

#define BCNN_CHECK(exp, err) do { if (!(exp)) return (err); } while (0)
#define BCNN_CHECK_AND_LOG(ctx, exp, err, fmt, ...) \
    do { if (!(exp)) { bcnn_log((ctx), BCNN_LOG_ERROR, (fmt), ##__VA_ARGS__); return (err); } } while (0)
#define BCNN_CHECK_STATUS(s) do { bcnn_status ret_ = (s); if (ret_ != BCNN_SUCCESS) return ret_; } while (0)
#define BCNN_ERROR(ctx, err, fmt, ...) do { bcnn_log((ctx), BCNN_LOG_ERROR, (fmt), ##__VA_ARGS__); return (err); } while (0)
#define BCNN_INFO(ctx, fmt, ...) bcnn_log((ctx), BCNN_LOG_INFO, (fmt), ##__VA_ARGS__)
#define BCNN_WARNING(ctx, fmt, ...) bcnn_log((ctx), BCNN_LOG_WARNING, (fmt), ##__VA_ARGS__)

/* debugging switches of the host runtime exist only in an experiment build (-DBCNN_HIP_EXPERIMENT) */
#ifdef BCNN_HIP_EXPERIMENT
#define BCNN_EXP_ENV(name) getenv(name)
#else
#define BCNN_EXP_ENV(name) ((const char *)NULL)
#endif

typedef struct {
    int state;
    float r;
} bcnn_gauss_gen;
float bcnn_rng_gaussian(bcnn_gauss_gen *g);

/* ---- node: the operator plug-in --------------------------------------------------------------- */
struct bcnn_node {
    int num_src;
    int num_dst;
    bcnn_layer_type type;
    size_t param_size;
    int *src; /* indices into net->tensors (stable; pointers into the array are not) */
    int *dst;
    void *param;
    void (*forward)(struct bcnn_net *net, struct bcnn_node *node);
    void (*backward)(struct bcnn_net *net, struct bcnn_node *node);
    void (*update)(struct bcnn_net *net, struct bcnn_node *node);
    void (*release_param)(struct bcnn_node *node);
};
typedef struct bcnn_node bcnn_node;

/* ---- learner ------------------------------------------------------------------------------------ */
typedef struct {
    int step;
    int seen;
    int max_batches;
    float momentum;
    float decay;
    float base_learning_rate;
    float learning_rate;
    float gamma;
    float scale;
    float power;
    float beta1;
    float beta2;
    bcnn_optimizer optimizer;
    bcnn_lr_decay decay_type;
} bcnn_learner;

/* ---- data loader / augmenter (host only: bcnn_data.c; reference src/bcnn_data.h:34-131) ---------- */
typedef struct {
    int input_width;
    int input_height;
    int input_depth;
    bool has_extra_data;
    bcnn_loader_type type;
    uint8_t *input_uchar;
    uint8_t *input_net;
    FILE *f_train;
    FILE *f_train_extra;
    FILE *f_test;
    FILE *f_test_extra;
    FILE *f_current;
    FILE *f_current_extra;
} bcnn_loader;

typedef struct {
    int range_shift_x, range_shift_y, random_fliph, min_brightness, max_brightness, swap_to_bgr, no_input_norm,
        max_random_spots;
    float min_scale, max_scale, rotation_range, min_contrast, max_contrast, max_distortion, mean_r, mean_g, mean_b;
    int use_precomputed, brightness, apply_fliph, shift_x, shift_y;
    float rotation, scale, contrast, distortion, distortion_kx, distortion_ky;
} bcnn_data_augmenter;

struct bcnn_net;
bcnn_status bcnn_loader_next(struct bcnn_net *net);
void bcnn_convert_img_to_float(const uint8_t *src, int w, int h, int c, float norm_coeff, int swap_to_bgr, float mean_r,
                               float mean_g, float mean_b, float *dst);
/* The reference's function in full: all eight stages, the two effects included whenever max_distortion > 0 or
 * max_random_spots > 0 (it takes no net, so bcnn_set_loader_effects does not reach it). A max_random_spots above
 * BCNN_MAX_SPOTS is refused before any draw. */
#define BCNN_MAX_SPOTS 64 /* spotlights one sample can draw: what a sample's draws hold (bcnn_data.c) */
bcnn_status bcnn_apply_data_augmentation(unsigned char *img, int width, int height, int depth, bcnn_data_augmenter *param,
                                         unsigned char *buffer);
bcnn_status bcnn_open_dataset(bcnn_loader *iter, struct bcnn_net *net, const char *train_path, const char *train_path_extra,
                              const char *test_path, const char *test_path_extra, bool has_extra);
bcnn_status bcnn_switch_data_handles(struct bcnn_net *net, bcnn_loader *iter);
void bcnn_fill_input_tensor(struct bcnn_net *net, bcnn_loader *iter, char *path_img, int idx);
void bcnn_destroy_data_loader(struct bcnn_net *net);
void bcnn_free_loader_stage(struct bcnn_net *net);
/* bcnn_data.c, for the segmentation-list reader (bcnn_data_segmentation.c): doors onto its statics -- the list lines, the
 * crop, the effects switch, the device route's gather block, and augment_if_training with the record of its draws */
struct bcnn_hip_augment_record;
int bcnn_loader_line_tokens(FILE *f, char ***tok);
void bcnn_loader_free_tokens(char **tok, int n);
void bcnn_loader_crop_origin(struct bcnn_net *net, int wi, int hi, int w, int h, int *x_ul, int *y_ul);
bcnn_status bcnn_loader_crop_to_input(unsigned char *buf, int wi, int hi, int x_ul, int y_ul, unsigned char *img, int w, int h,
                                      int c);
int bcnn_loader_effects_on(const struct bcnn_net *net);
int bcnn_loader_staging(struct bcnn_net *net);
bcnn_status bcnn_loader_stage_sample(struct bcnn_net *net, bcnn_loader *it, int idx,
                                     const struct bcnn_hip_augment_record **record, const int32_t **taps);
void bcnn_loader_staged_records(struct bcnn_net *net, const struct bcnn_hip_augment_record **records, const int32_t **taps);
bcnn_status bcnn_loader_augment_recorded(struct bcnn_net *net, unsigned char *img, int w, int h, int c,
                                         struct bcnn_hip_augment_record *record, int32_t *taps);
void bcnn_loader_fill_record(int flip, int shift, int x_ul, int y_ul, int scale, float scale_factor, int rotate, float theta,
                             int w, int h, struct bcnn_hip_augment_record *record, int32_t *taps);
/* bcnn_data_segmentation.c: BCNN_LOAD_SEGMENTATION_LIST ("image-path mask-path" lines). _init sizes the mask buffer of a
 * loader list_init has opened; _check holds the refusals of bcnn_loader_next (label extents, distortion), made before any
 * draw; _next reads one sample into slot idx, or skips its line before any draw; _labels finishes a batch that was gathered
 * for the device: 1 when its label maps were made there (tensors[1].data is then not to be uploaded), 0 when they are in
 * tensors[1].data (device_ok 0: the image batch was made on the host, and so are they). */
bcnn_status bcnn_segmentation_init(bcnn_loader *it, struct bcnn_net *net);
bcnn_status bcnn_segmentation_check(struct bcnn_net *net);
bcnn_status bcnn_segmentation_next(bcnn_loader *it, struct bcnn_net *net, int idx);
int bcnn_segmentation_labels(struct bcnn_net *net, bcnn_loader *it, int device_ok);

/* ---- device context of a net (reference analogue: bcnn_cuda_context, src/bcnn_net.h:37-42) ------ */
typedef struct bcnn_hip_context {
    size_t workspace_size;  /* floats; shared conv backward scratch, sized at compile time */
    float *workspace_gpu;
    /* parameter / gradient arenas built by bcnn_compile_net (one all-reduce per step) */
    float *param_arena_gpu;
    float *grad_arena_gpu;
    size_t arena_size;  /* floats */
    int *param_ids;     /* tensor indices of trainable parameters, in creation order */
    int num_params;
    int arena_members; /* how many of param_ids[] already live inside the arenas (bcnn_compile_net re-packs when it grows) */
    int dp_rank;
    int dp_world;
    int compiled;
    /* update loop folded into one launch: table of (buffer, gradient, count, rule) chunks, built by the
     * first bcnn_update from what the nodes' update() workers ask for */
    /* gradient-ready callback (bcnn_set_gradient_ready_callback): node_grad_first[i] = arena offset of the first
     * parameter owned by node i, or (size_t)-1 */
    void (*grad_ready_fn)(size_t, size_t, void *);
    void *grad_ready_user;
    size_t *node_grad_first;
    /* per tensor: 1 = the zero-fill of its gradient before forward is dead (see mark_dead_grad_fills) */
    unsigned char *grad_fill_dead;
    int grad_fill_count; /* entries of grad_fill_dead[] (tensors that existed at compile time) */
    struct bcnn_hip_sgd_chunk *sgd_chunks_host;
    void *sgd_chunks_gpu;
    int num_sgd_chunks, cap_sgd_chunks;
    int sgd_collecting;
    /* the gradient zero fills of a TRAIN-mode forward pass gathered into one launch (built by the first forward after
     * a compile; dropped with the SGD table when the graph changes) */
    void *fill_chunks_gpu;
    int num_fill_chunks;
    /* RCCL inside the library (bcnn_set_data_parallel_comm): finished tail ranges of the gradient arena are gathered
     * into buckets of comm_bucket floats and all-reduced on the communicator's stream while backward continues */
    int comm_active;
    size_t comm_bucket, comm_lo, comm_hi;
    /* 1 inside bcnn_forward / 2 inside bcnn_backward: node workers may rely on their neighbours having run in this pass
     * (bcnn_forward_node / bcnn_backward_node run one worker alone: 0) */
    int in_pass;
    int no_side_stream; /* bcnn_set_weight_gradient_stream(net, 0) */
    uint64_t dropout_seed; /* bcnn_set_dropout_seed; 0 until set */
    int inference_precision; /* bcnn_set_inference_precision (a bcnn_precision); read by the convolution node outside TRAIN mode */
    int loader_on_device; /* bcnn_set_loader_on_device: bcnn_loader_next makes the input batch with bcnn_hip_augment_batch */
    void *loader_stage;   /* its host-side gather block (bcnn_data.c: loader_stage); freed by bcnn_free_loader_stage */
    int loader_decode_on_device; /* bcnn_set_loader_decode_on_device: JPEG entries of a list batch that goes the device way
                                  * are entropy-decoded on the host and become pixels on the device only */
    int loader_device_decoded;   /* samples of the latest bcnn_loader_next whose pixels were decoded on the device */
    int loader_detection_on_device; /* bcnn_set_loader_detection_on_device: a detection-list batch that goes the device way
                                     * is letterboxed and augmented by bcnn_hip_augment_letterbox_batch */
    int loader_device_letterboxed;  /* samples of the latest bcnn_loader_next that were letterboxed on the device */
    int loader_effects; /* bcnn_set_loader_effects: bcnn_loader_next applies Perlin distortion and random spotlights, on
                         * the host path and on every device route; off, their draws are made and dropped */
    int loader_device_labels; /* label maps of the latest bcnn_loader_next that were made on the device (segmentation list) */
    int detector_training; /* bcnn_set_detector_training: YOLO heads may be built on / switched to TRAIN, with their loss */
    int detect_capacity; /* 1.25 x the most boxes an image of the latest bcnn_yolo_get_detections_batch had: the next call's record capacity
                          * when above the default (0: never called) */
} bcnn_hip_context;

/* ---- net ------------------------------------------------------------------------------------------ */
struct bcnn_net {
    int batch_size;
    int num_nodes;
    int num_tensors;
    int num_inputs;
    int *inputs;
    bcnn_mode mode;
    bcnn_log_context log_ctx;
    bcnn_node *nodes;
    bcnn_tensor *tensors;
    bcnn_learner *learner;
    bcnn_loader *data_loader;
    bcnn_data_augmenter *data_aug;
    void *gemm_ctx; /* unused here (the reference's CPU gemm scratch) */
#ifdef BCNN_USE_HIP
    void *hip_ctx; /* bcnn_hip_context* */
#endif
    int num_threads;
};

/* ---- net / node / tensor helpers (reference: bcnn_net.h:69-76, bcnn_node.h:50-51, bcnn_tensor.h:37-63) */
bcnn_status bcnn_net_add_node(bcnn_net *net, bcnn_node node);
bcnn_status bcnn_net_add_tensor(bcnn_net *net, bcnn_tensor tensor);
bcnn_status bcnn_node_add_input(bcnn_net *net, bcnn_node *node, int index);
bcnn_status bcnn_node_add_output(bcnn_net *net, bcnn_node *node, int index);
/* new n x c x h x w tensor `dst_id` (with gradient, allocated for the net's mode) as the node's next output */
bcnn_status bcnn_node_new_output(bcnn_net *net, bcnn_node *node, int n, int c, int h, int w, const char *dst_id);
/* new [1,1,1,count] tensor `<src_id>_<suffix>`, filled with `fill`, as the node's next input; trainable ones join the arena */
bcnn_status bcnn_node_new_vector_param(bcnn_net *net, bcnn_node *node, int count, int has_grad, const char *src_id,
                                       const char *suffix, float fill, int trainable);

typedef struct tensor_filler {
    int range;
    float value;
    bcnn_filler_type type;
} bcnn_tensor_filler;

void bcnn_tensor_create(bcnn_tensor *t, int n, int c, int h, int w, int has_grad, const char *name, int net_state);
void bcnn_tensor_fill(bcnn_tensor *t, bcnn_tensor_filler filler);
void bcnn_tensor_destroy(bcnn_tensor *t);
void bcnn_tensor_set_shape(bcnn_tensor *t, int n, int c, int h, int w, int has_grad);
bcnn_status bcnn_tensor_allocate_buffer(bcnn_tensor *t, int net_state, size_t size);
bcnn_status bcnn_tensor_allocate(bcnn_tensor *t, int net_state);
/* The one rule for a layer's private device buffer whose size follows a tensor (bcnn_resize_net): `*capacity` is the number
 * of elements `*buf` was allocated with, set wherever the buffer is made. A NULL buffer stays NULL (PREDICT-built nets,
 * average pooling) and `elems <= *capacity` touches nothing: both BCNN_SUCCESS. Past the capacity: BCNN_INVALID_PARAMETER
 * with nothing touched when !may_grow; else the buffer is re-made (zero-filled) for `elems` elements of `elem_size` bytes, or
 * left NULL with capacity 0 and BCNN_FAILED_ALLOC. */
bcnn_status bcnn_reserve_device(void **buf, size_t *capacity, size_t elems, size_t elem_size, int may_grow);
void bcnn_tensor_free(bcnn_tensor *t);
int bcnn_tensor_size(const bcnn_tensor *t);
int bcnn_tensor_size3d(const bcnn_tensor *t);
int bcnn_tensor_size2d(const bcnn_tensor *t);

/* marks tensor `index` as a trainable parameter (member of the gradient arena) */
void bcnn_net_register_param(bcnn_net *net, int index);
/* finds the most recently created tensor called `name`; -1 if absent (reference builders scan newest-first) */
int bcnn_net_find_tensor(bcnn_net *net, const char *name);

bcnn_status bcnn_loader_next(bcnn_net *net);
void bcnn_convert_img_to_float(const uint8_t *src, int w, int h, int c, float norm_coeff, int swap_to_bgr,
                               float mean_r, float mean_g, float mean_b, float *dst);
void bcnn_draw_color_box(unsigned char *img, int w_img, int h_img, float cx_box, float cy_box, float w_box,
                         float h_box, unsigned char color[3]);

static inline const char *bcnn_act2str(bcnn_activation a) {
    switch (a) {
        case BCNN_ACT_TANH: return "Tanh";
        case BCNN_ACT_RELU: return "ReLU";
        case BCNN_ACT_RAMP: return "Ramp";
        case BCNN_ACT_SOFTPLUS: return "Softplus";
        case BCNN_ACT_LRELU: return "Leaky-ReLU";
        case BCNN_ACT_ABS: return "AbsVal";
        case BCNN_ACT_CLAMP: return "Clamp";
        case BCNN_ACT_PRELU: return "PReLU";
        case BCNN_ACT_LOGISTIC: return "Logistic";
        case BCNN_ACT_RELU6: return "ReLU6";
        case BCNN_ACT_HARD_SIGMOID: return "Hard-Sigmoid";
        case BCNN_ACT_HARD_SWISH: return "Hard-Swish";
        case BCNN_ACT_SWISH: return "Swish";
        case BCNN_ACT_MISH: return "Mish";
        default: return "None";
    }
}

/* hard-swish, swish, mish: the derivative is no function of the output, so only the stand-alone activation node (which
 * keeps its input) takes them */
static inline int bcnn_act_needs_input(bcnn_activation a) {
    return a == BCNN_ACT_HARD_SWISH || a == BCNN_ACT_SWISH || a == BCNN_ACT_MISH;
}
/* the refusal every builder with a fused activation starts with; nothing has been added to the net at that point */
#define BCNN_REFUSE_INPUT_ACTIVATION(net, a, layer)                                                                        \
    BCNN_CHECK_AND_LOG((net)->log_ctx, !bcnn_act_needs_input(a), BCNN_INVALID_PARAMETER,                                   \
                       "%s layer: %s takes its derivative from the layer's input and cannot be fused; build the layer "   \
                       "with BCNN_ACT_NONE and add bcnn_add_activation_layer on its output\n", layer, bcnn_act2str(a))

/* ---- layer parameter blocks (member names follow src/layers/<layer>.h of the reference) ---------- */
typedef struct bcnn_conv_param {
    int num, size, stride, pad, num_groups, batch_norm, post_func;
    size_t workspace_size;
    bcnn_activation activation;
    bcnn_tensor saved_mean;     /* batch statistics (data) and their gradients (grad_data) */
    bcnn_tensor saved_variance;
    float *conv_workspace;      /* unused on the device path (no materialised im2col) */
    float *workspace;
    float *x_norm;
    float *adam_m, *adam_v;
#ifdef BCNN_USE_HIP
    float *conv_workspace_gpu;  /* = net hip_ctx workspace (dW split-K partials) */
    float *bn_workspace_gpu;    /* pre-normalisation conv output, kept for backward */
    size_t bn_workspace_capacity; /* floats allocated (bcnn_reserve_device) */
    float *x_norm_gpu;          /* never allocated: recomputed in backward */
    float *adam_m_gpu, *adam_v_gpu; /* weight moments, allocated by the first Adam step */
    /* set by bcnn_compile_net when the node that follows is an eltwise node adding something to this node's (batch-norm,
     * no activation) output (bcnn_link_conv_eltwise): inside a whole pass the eltwise work rides on this node's
     * batch-norm sweeps */
    int elt_node;      /* index of that eltwise node, -1: none */
    int pool_node;     /* index of the max-pooling node that is this node's only consumer and normalises this node's
                        * pre-normalisation output on the fly inside a forward pass (bcnn_link_conv_maxpool), -1: none */
    int bnsums_node;   /* the stand-alone batch-norm node in front of this (1x1) node whose backward sums this node's
                        * data-gradient kernel emits inside a backward pass (bcnn_link_batchnorm_conv), -1: none */
    int dw_node;       /* index of the depthwise node that is this node's only consumer and normalises this node's
                        * pre-normalisation output while staging it (bcnn_link_conv_depthwise), -1: none */
    int apply_skipped; /* this node left its batch-norm apply sweep to its consumer in the running forward pass */
    int fold_bn;       /* the stand-alone batch-norm node in front of this (1x1) node that leaves its apply sweep to this node's
                        * packed weights inside a forward pass (bcnn_link_batchnorm_conv), -1: none */
    int folded;        /* the running pass's forward took that route: the backward reads the batch-norm's INPUT */
    int pool_bwd_pending; /* pool_node >= 0, inside a backward pass: that node left its backward to this node's (one kernel
                           * does the pooling backward and this node's batch-norm backward: bcnn_hip_maxpool_bn_backward) */
    float *insums_gpu;   /* dw_node >= 0: partial backward sums of this node's batch-norm, left by that depthwise node's */
    size_t insums_floats; /* backward kernel (bcnn_hip_depthwise_backward_bnin_sums) in the running backward pass */
    int insums_splits;   /* > 0: insums_gpu holds them (partials per channel) */
    int data_pending;  /* the last forward pass did not write this node's output tensor (nobody inside a pass reads it):
                        * bcnn_materialize_data produces it from bn_workspace_gpu on demand */
    int out_rewritten; /* another node rewrites this node's output in place (dropout; set by bcnn_compile_net): the
                        * backward reads the output tensor instead of recomputing it from bn_workspace_gpu */
#endif
} bcnn_conv_param;

typedef struct bcnn_depthwise_conv_param {
    int size, stride, pad, batch_norm;
    bcnn_activation activation;
    float *adam_m, *adam_v;
#ifdef BCNN_USE_HIP
    float *adam_m_gpu, *adam_v_gpu;
    /* set by bcnn_compile_net when this node's output feeds a stand-alone batch-norm node (bcnn_link_depthwise_batchnorm):
     * inside a whole forward / backward pass the two workers share work */
    int bn_node;         /* index of that batch-norm node, -1: none */
    int bn_fused_bwd;    /* the batch-norm node leaves its apply sweep to this node's backward kernel */
    float *stats_gpu;    /* per-channel statistics partials of the last forward (TRAIN) */
    size_t stats_floats;
    int stats_splits;    /* > 0: stats_gpu holds the statistics of the output written by the last forward of this pass */
    int conv_node;       /* the convolution node whose batch-norm this node applies to its input on the fly, -1: none */
    int raw_input;       /* the last forward pass read that node's pre-normalisation output: so must its backward */
    int grads_pending;   /* the last backward pass did not write the gradient of this node's output nor rewrite the
                          * batch-norm node's output gradient (nothing inside a pass reads them): they are produced on
                          * demand by bcnn_materialize_gradients, as the reference's two workers leave them */
#endif
} bcnn_depthwise_conv_param;

typedef struct bcnn_batchnorm_param {
    bcnn_tensor saved_mean;
    bcnn_tensor saved_variance;
    float *workspace;
    float *x_norm;
#ifdef BCNN_USE_HIP
    float *workspace_gpu;
    size_t workspace_capacity; /* floats allocated (bcnn_reserve_device); 0 while bcnn_link_depthwise_batchnorm keeps no copy */
    float *x_norm_gpu;   /* never allocated: recomputed in backward */
    int dw_node;         /* the depthwise node that produces this node's input (see bcnn_depthwise_conv_param), -1: none */
    int dw_fused_bwd;    /* that node applies this node's backward to the gradient it consumes */
    int sums_conv;       /* the 1x1 convolution node that is this node's only consumer: inside a backward pass its
                          * data-gradient kernel emits the partial sums this node's backward starts with, -1: none */
    float *bsums_gpu;    /* those partials (bcnn_hip_conv_bnsums_size floats) */
    size_t bsums_floats;
    int bsums_splits;    /* > 0: bsums_gpu holds the sums of the gradient written in the running backward pass */
    int input_kept;      /* the input tensor is not this node's output and has no other consumer: it IS the copy of the
                          * input the reference keeps in `workspace` (bcnn_batchnorm_layer.c:208) */
    int fold_conv;       /* the 1x1 convolution node that is this node's only consumer and folds this node's affine map into
                          * its weights inside a forward pass (bcnn_hip_conv_set_input_bnfold), -1: none */
    int apply_skipped;   /* the running forward pass left this node's output tensor unwritten for that node ... */
    int data_pending;    /* ... and nobody has asked for it since (bcnn_materialize_data produces it on demand) */
#endif
} bcnn_batchnorm_param;

typedef struct bcnn_maxpool_param {
    int size, stride;
    bcnn_padding padding;
    int *indexes;
#ifdef BCNN_USE_HIP
    int *indexes_gpu;
    size_t indexes_capacity; /* elements allocated, of indexes_gpu and of the host `indexes` (bcnn_reserve_device) */
    int conv_node;  /* the convolution node whose batch-norm this node applies on the fly (see bcnn_conv_param), -1: none */
    float *raw_at_max_gpu; /* conv_node >= 0: per pooled element the pre-normalisation value that won its window, kept by
                            * the forward pass for bcnn_hip_maxpool_bn_backward (the output tensor's shape) */
    size_t raw_at_max_capacity; /* floats allocated: bcnn_link_conv_maxpool makes it as large as the indexes */
    int raw_fwd;    /* the running pass's forward took that route (raw_at_max_gpu is current) */
#endif
} bcnn_maxpool_param;

typedef struct bcnn_activation_param {
    bcnn_activation activation;
#ifdef BCNN_USE_HIP
    float *x_saved_gpu;       /* hard-swish / swish / mish, nets built in TRAIN / VALID mode: the input of the last TRAIN forward */
    size_t x_saved_capacity;  /* floats allocated (bcnn_reserve_device) */
#endif
} bcnn_activation_param;

/* dst = src[0] * src[1] (bcnn_add_scale_channels_layer; no reference counterpart); the gate's form follows from the two
 * shapes at every call, so bcnn_resize_net has nothing to update here */
typedef struct bcnn_scale_channels_param {
    int same_shape; /* as built: 0 = [N,C,1,1] gate, 1 = a gate of the source's shape (log line only) */
} bcnn_scale_channels_param;

/* group normalisation (bcnn_add_groupnorm_layer; no reference counterpart): src[1] = scales, src[2] = b */
typedef struct bcnn_groupnorm_param {
    int num_groups;
    float eps;
#ifdef BCNN_USE_HIP
    float *stats_gpu;       /* nets built in TRAIN / VALID mode: mean [N * G] then rstd [N * G] of the last forward */
    size_t stats_capacity;  /* floats allocated (bcnn_reserve_device) */
    float *adam_m_gpu, *adam_v_gpu; /* moments of the scales, allocated by the first Adam step */
#endif
} bcnn_groupnorm_param;

typedef struct bcnn_eltwise_param {
    bcnn_activation activation;
    int stride[2];
    int min_dim[3];
#ifdef BCNN_USE_HIP
    int conv_node;     /* the convolution node that does this node's work inside a pass (see bcnn_conv_param), -1: none */
    int done_forward;  /* that node already wrote this node's output in the running forward pass */
    int deferred;      /* this node's backward was left to that node in the running backward pass */
    int grad_pending;  /* the last backward pass did not rewrite this node's output gradient (dy *= act'(y),
                        * bcnn_eltwise_layer.c:124-127): bcnn_materialize_gradients does on demand */
#endif
} bcnn_eltwise_param;

typedef struct bcnn_fullc_param {
    bcnn_activation activation;
    float *adam_m, *adam_v;
#ifdef BCNN_USE_HIP
    float *adam_m_gpu, *adam_v_gpu;
#endif
} bcnn_fullc_param;

typedef struct bcnn_cost_param {
    float scale;
    bcnn_loss loss;
    bcnn_loss_metric loss_metric;
    float num_constraints;           /* lifted-structure loss: positive pairs of the batch bcnn_get_lifted_struct_loss
                                        last read (the reference's field, bcnn_cost_layer.h:34) */
#ifdef BCNN_USE_HIP
    float *lifted_workspace_gpu;     /* bcnn_hip_lifted_struct_workspace_size(n, c) floats, the node's own */
    size_t lifted_workspace_size;
    void *lifted_record_gpu;         /* bcnn_hip_lifted_struct_record {loss, P}: backward scales by scale / P from it */
#endif
} bcnn_cost_param;

typedef struct bcnn_upsample_param {
    int size;
} bcnn_upsample_param;

/* transposed convolution (reference src/layers/bcnn_deconv_layer.h); weights [c_in][num][size][size] */
typedef struct bcnn_deconv_param {
    int num, size, stride, pad;
    bcnn_activation activation;
    float *conv_workspace;      /* unused on the device path (no materialised col2im / im2col) */
    float *adam_m, *adam_v;
#ifdef BCNN_USE_HIP
    float *conv_workspace_gpu;  /* the node's own dW split partials (bcnn_hip_deconv_workspace_size), first backward */
    size_t workspace_size;
    float *adam_m_gpu, *adam_v_gpu; /* weight moments, allocated by the first Adam step */
#endif
} bcnn_deconv_param;

/* dilated convolution (bcnn_add_dilated_conv_layer with dilation > 1; no reference counterpart); weights
 * [num][c / num_groups][size][size] */
typedef struct bcnn_dilated_conv_param {
    int num, size, stride, pad, dilation, num_groups;
    bcnn_activation activation;
    int section_bn; /* the config loader split one section into this node, a batch-norm node and an activation node: a
                       Darknet .weights file, which interleaves the section's values, cannot be loaded into them */
#ifdef BCNN_USE_HIP
    float *conv_workspace_gpu;  /* the node's own dW split partials (bcnn_hip_dilated_conv_workspace_size), first backward */
    size_t workspace_size;
    float *adam_m_gpu, *adam_v_gpu; /* weight moments, allocated by the first Adam step */
#endif
} bcnn_dilated_conv_param;

/* dilated depthwise convolution (bcnn_add_dilated_depthwise_conv_layer with dilation > 1; no reference counterpart);
 * weights [c][size][size], the depthwise node's layout */
typedef struct bcnn_dilated_depthwise_param {
    int size, stride, pad, dilation;
    bcnn_activation activation;
#ifdef BCNN_USE_HIP
    float *workspace_gpu; /* the node's own dW / dbias partials (bcnn_hip_dilated_depthwise_workspace_size), first backward */
    size_t workspace_size;
    float *adam_m_gpu, *adam_v_gpu; /* weight moments, allocated by the first Adam step */
#endif
} bcnn_dilated_depthwise_param;

/* local response normalisation across channels (reference src/layers/bcnn_lrn_layer.h); no buffers: the backward
 * recomputes the scale from the input */
typedef struct bcnn_lrn_param {
    int local_size;
    float alpha;
    float beta;
    float k;
} bcnn_lrn_param;

/* windowed pooling with symmetric padding (bcnn_add_pool2d_layer; no reference counterpart). A param block of its own:
 * nothing that keys on BCNN_LAYER_MAXPOOL / _AVGPOOL (the conv / batch-norm fusion links) ever sees this node */
typedef struct bcnn_pool2d_param {
    bcnn_pool2d_kind kind;
    int size, stride, pad, ceil_mode, count_include_pad;
#ifdef BCNN_USE_HIP
    int *indexes_gpu;        /* max, nets built in TRAIN / VALID mode: the winner of every window (the output's shape) */
    size_t indexes_capacity; /* elements allocated (bcnn_reserve_device) */
#endif
} bcnn_pool2d_param;

/* bilinear interpolation (bcnn_add_interp_layer; no reference counterpart). Exactly one of scale, zoom and
 * (out_w, out_h) is set; no device buffer of its own */
typedef struct bcnn_interp_param {
    int scale, zoom, out_w, out_h, align_corners;
} bcnn_interp_param;

/* softmax + cross-entropy against a class-index label map (bcnn_add_softmax_loss_layer; no reference counterpart) */
typedef struct bcnn_softmax_loss_param {
    int ignore_label;
    bcnn_loss_norm norm;
    float scale;
    int has_stats;         /* the latest forward wrote the record (TRAIN / VALID with a label on the device) */
    size_t label_capacity; /* floats the label tensor was allocated with by this node (bcnn_tensor has no capacity) */
#ifdef BCNN_USE_HIP
    float *record_gpu;     /* bcnn_hip_softmax_loss_record: 6 words */
#endif
} bcnn_softmax_loss_param;

/* in-place dropout (reference src/layers/bcnn_dropout_layer.h); the mask is regenerated from (key, step) of the last
 * TRAIN forward instead of being stored (include/bcnn_hip.h) */
typedef struct bcnn_dropout_param {
    float dropout_rate;
    float scale;
    uint64_t step;      /* TRAIN forwards run so far */
    uint64_t last_key;  /* key and step of the last TRAIN forward, for the backward */
    uint64_t last_step;
    int has_mask;       /* a TRAIN forward has run since the node was built */
} bcnn_dropout_param;

/* the YOLOv3 head (reference src/layers/bcnn_yolo.h); consumers read `classes` (src/cli/bcnn_cl.c:199) */
typedef struct bcnn_yolo_param {
    int num, classes, coords, total;
    int *mask;      /* num anchor indices of this head */
    float *biases;  /* host: total * 2 anchor extents (w, h) in input pixels */
    float *cost;    /* cost[0]: sum of the squared deltas of the latest TRAIN forward, as bcnn_yolo_get_train_stats last read it */
    int max_boxes, truths; /* detector training: BCNN_DETECTION_MAX_BOXES and floats per image of the label (0: built without) */
#ifdef BCNN_USE_HIP
    void *train_record_gpu;     /* bcnn_hip_yolo_train_record of the latest TRAIN forward */
    float *train_workspace_gpu; /* bcnn_hip_yolo_train_workspace_size floats, the node's own */
    size_t train_workspace_size;
#endif
} bcnn_yolo_param;

/* hot-path node workers (installed into bcnn_node) */
void bcnn_forward_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_conv_layer(bcnn_node *node);
void bcnn_forward_depthwise_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_depthwise_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_depthwise_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_depthwise_conv_layer(bcnn_node *node);
void bcnn_forward_batchnorm_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_batchnorm_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_batchnorm_layer(bcnn_node *node);
void bcnn_forward_maxpool_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_maxpool_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_maxpool_layer(bcnn_node *node);
void bcnn_forward_avgpool_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_avgpool_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_activation_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_activation_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_activation_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_eltwise_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_eltwise_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_fullc_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_fullc_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_fullc_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_fullc_layer(bcnn_node *node);
void bcnn_forward_softmax_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_softmax_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_cost_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_cost_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_cost_layer(bcnn_node *node);
void bcnn_forward_concat_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_concat_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_upsample_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_upsample_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_yolo_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_yolo_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_yolo_layer(bcnn_node *node);
/* bcnn_layers_detect.c: 1 when every head of the net can run its TRAIN forward (label and gradient buffers) */
int bcnn_yolo_heads_trainable(bcnn_net *net);
/* reads every head's record back (one small copy each) into param->cost[0]; returns the number of heads */
int bcnn_yolo_refresh_costs(bcnn_net *net);
/* bcnn_yolo_get_detections_batch with its capacities exposed (bcnn_layers_detect.c; exported for the tests) */
bcnn_status bcnn_yolo_detections_batch_worker(bcnn_net *net, const int *widths, const int *heights, int netw, int neth,
                                              float thresh, int relative, int record_cap, int nms_cap,
                                              bcnn_output_detection **dets, int *num_dets, int *passes);
void bcnn_forward_deconv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_deconv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_deconv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_deconv_layer(bcnn_node *node);
void bcnn_forward_dilated_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_dilated_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_dilated_conv_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_dilated_conv_layer(bcnn_node *node);
void bcnn_forward_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_dilated_depthwise_layer(bcnn_node *node);
void bcnn_forward_lrn_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_lrn_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_lrn_layer(bcnn_node *node);
void bcnn_forward_dropout_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_dropout_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_dropout_layer(bcnn_node *node);
uint64_t bcnn_dropout_key(uint64_t seed, int node, int rank);
void bcnn_forward_scale_channels_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_scale_channels_layer(bcnn_net *net, bcnn_node *node);
void bcnn_forward_groupnorm_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_groupnorm_layer(bcnn_net *net, bcnn_node *node);
void bcnn_update_groupnorm_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_groupnorm_layer(bcnn_node *node);
void bcnn_release_param_activation_layer(bcnn_node *node);
void bcnn_forward_pool2d_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_pool2d_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_pool2d_layer(bcnn_node *node);
/* bcnn_layers_pool2d.c: the node's output extents for an h x w source; 0 if the parameters refuse that source */
int bcnn_pool2d_out_extents(const bcnn_pool2d_param *p, int h, int w, int *out_h, int *out_w);
void bcnn_forward_interp_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_interp_layer(bcnn_net *net, bcnn_node *node);
/* bcnn_layers_interp.c: the node's output extents for an h x w source (the builder's rule); 0 if the extents are refused */
int bcnn_interp_out_extents(const bcnn_interp_param *p, int h, int w, int *out_h, int *out_w);
void bcnn_forward_softmax_loss_layer(bcnn_net *net, bcnn_node *node);
void bcnn_backward_softmax_loss_layer(bcnn_net *net, bcnn_node *node);
void bcnn_release_param_softmax_loss_layer(bcnn_node *node);
/* bcnn_layers_softmax_loss.c: the loss of the node's latest forward, read from its device record; 0 without statistics */
float bcnn_softmax_loss_read_loss(bcnn_net *net, bcnn_node *node);

/* SGD step on one node's parameters (bcnn_learner.c:67-104 in the reference) */
void bcnn_link_depthwise_batchnorm(bcnn_net *net); /* bcnn_layers_hot.c; called by bcnn_compile_net */
void bcnn_link_conv_eltwise(bcnn_net *net);        /* bcnn_layers_hot.c; called by bcnn_compile_net */
void bcnn_link_conv_maxpool(bcnn_net *net);
void bcnn_link_conv_depthwise(bcnn_net *net);
void bcnn_link_batchnorm_conv(bcnn_net *net);
/* bcnn_input_jpeg.c: the entropy decoding of a batch of JPEG streams into the caller's coefficient regions, spread over
 * num_threads host threads; lowest failing index, -1, or -2 (allocation). Not part of the public API: it is not static,
 * and so exported, only so that tests/test_jpeg_split.py can check on a plain heap block that the bytes do not depend on
 * the number of threads. */
int bcnn_jpeg_read_batch(int num_images, const uint8_t *const *buffers, const size_t *lengths, const bip_jpeg_info *infos,
                         int16_t *const *coeff, int num_threads);
struct bcnn_hip_jpeg_frame;
void bcnn_jpeg_frame_from_info(const bip_jpeg_info *info, struct bcnn_hip_jpeg_frame *f);
/* per-image form: coeff[b] == NULL skips image b; status[b] = 1 / 0 for the others; 0, or -2 (allocation) */
int bcnn_jpeg_read_batch_each(int num_images, const uint8_t *const *buffers, const size_t *lengths,
                              const bip_jpeg_info *infos, int16_t *const *coeff, int num_threads, int *status);
void bcnn_materialize_data(bcnn_net *net, int tensor);      /* tensor < 0: every pending one */
void bcnn_materialize_gradients(bcnn_net *net, int tensor); /* tensor < 0: every pending one */
void bcnn_drop_pending_gradients(bcnn_net *net);
void bcnn_prepack_conv_weights(bcnn_net *net, int data_gradient); /* bcnn_layers_hot.c */
int bcnn_grad_sole_writer(bcnn_net *net, int tensor); /* 1: this gradient's zero fill was skipped, assign instead of += */
void bcnn_node_sgd_step(bcnn_net *net, bcnn_tensor *weights, bcnn_tensor *biases);
void bcnn_node_optim_step(bcnn_net *net, bcnn_tensor *weights, bcnn_tensor *biases, float **adam_m_gpu,
                          float **adam_v_gpu); /* SGD or Adam according to net->learner->optimizer */

#ifdef __cplusplus
}
#endif
#endif /* BCNN_INTERNAL_H */
