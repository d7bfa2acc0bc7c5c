/*
 * bcnn_layers_softmax_loss.c -- the softmax-loss node: softmax over the channels and cross-entropy against a class-index
 * label map (torch's F.cross_entropy with ignore_index), with an ignore label, a normaliser, per-pixel statistics and an
 * on-demand confusion matrix. Builder, node workers and the two readers. One whole-batch call into the C-ABI per
 * direction (softmax_loss.hip).
 *
 * No reference counterpart: the reference's loss path is softmax -> cost (Euclidean) on a dense one-hot label
 * (bcnn_layers_next.c), which keeps its code. This node has a layer type and a param block of its own.
 *   - how a label value is classified and what a normaliser divides by is ../csrc/softmax_loss_rule.h, the header the
 *     kernels compile; the builder's own checks use its limits;
 *   - the builder checks every argument before it adds or allocates anything (INTEGRATION.md lists the refusals);
 *   - loss, counts and the factor scale / D live in a 24-byte device record: the forward does not synchronise, the backward
 *     reads the factor on the device, and the host reads the record only when asked (the two readers, and once per step
 *     for the loss that bcnn_train_on_batch returns);
 *   - the backward adds into the source gradient like every other node and assigns when it is the gradient's only writer
 *     (bcnn_grad_sole_writer): its overwrite form writes every element, +0.0 on pixels that are not valid;
 *   - the output tensor holds the probabilities; bcnn_node_new_output gives it a gradient buffer in TRAIN nets like every
 *     output, which this node neither reads nor writes;
 *   - no parameters: model files skip the node.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"
#include "../csrc/softmax_loss_rule.h"

bcnn_status bcnn_add_softmax_loss_layer(bcnn_net *net, int ignore_label, bcnn_loss_norm norm, float scale,
                                        const char *src_id, const char *label_id, const char *dst_id) {
    (void)label_id; /* the label is always tensor 1 */
    BCNN_CHECK_AND_LOG(net->log_ctx, net->num_nodes >= 1, BCNN_INVALID_PARAMETER,
                       "Softmax-loss layer can't be the first layer of the network\n");
    const int src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
    BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Softmax-loss layer: invalid input node name %s\n",
                       src_id ? src_id : "(null)");
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_softmax_loss_denominator((int)norm, 1, 1) != 0.0, BCNN_INVALID_PARAMETER,
                       "Softmax-loss layer %s: unknown normaliser %d\n", dst_id, (int)norm);
    BCNN_CHECK_AND_LOG(net->log_ctx, ignore_label < BCNN_SL_MAX_IGNORE_LABEL, BCNN_INVALID_PARAMETER,
                       "Softmax-loss layer %s: ignore_label %d is not below 2^24, no float holds it as an index\n", dst_id,
                       ignore_label);
    const bcnn_tensor s = net->tensors[src];
    bcnn_tensor *label = &net->tensors[1];
    BCNN_CHECK_AND_LOG(net->log_ctx,
                       label->data == NULL || (label->n == s.n && label->c == 1 && label->h == s.h && label->w == s.w),
                       BCNN_INVALID_PARAMETER,
                       "Softmax-loss layer %s: the label tensor is already %d x %d x %d x %d (another loss node shaped it), this "
                       "node needs %d x 1 x %d x %d\n", dst_id, label->n, label->c, label->h, label->w, s.n, s.h, s.w);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    if (label->data == NULL) {
        bcnn_tensor_set_shape(label, s.n, 1, s.h, s.w, 0);
        BCNN_CHECK_STATUS(bcnn_tensor_allocate(label, net->mode));
    }
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_SOFTMAX_LOSS;
    node.param_size = sizeof(bcnn_softmax_loss_param);
    bcnn_softmax_loss_param *param = (bcnn_softmax_loss_param *)calloc(1, node.param_size);
    node.param = param;
    param->ignore_label = ignore_label;
    param->norm = norm;
    param->scale = scale;
    param->label_capacity = (size_t)s.n * s.h * s.w;
    param->record_gpu = bcnn_hip_malloc_f32(sizeof(bcnn_hip_softmax_loss_record) / sizeof(float)); /* zero-filled */
    node.forward = bcnn_forward_softmax_loss_layer;
    node.backward = bcnn_backward_softmax_loss_layer;
    node.release_param = bcnn_release_param_softmax_loss_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Softmax loss] %-8s -> %-8s (%4d x%4d x%4d) ignore %d norm %s scale %g\n", src_id, dst_id, s.w,
              s.h, s.c, ignore_label,
              norm == BCNN_LOSS_NORM_NONE ? "none" : norm == BCNN_LOSS_NORM_VALID ? "valid" : "valid_per_image", scale);
    return BCNN_SUCCESS;
}

static bcnn_hip_softmax_loss_desc loss_desc(const bcnn_softmax_loss_param *p) {
    bcnn_hip_softmax_loss_desc d;
    d.ignore_label = p->ignore_label;
    d.norm = (int)p->norm;
    d.scale = p->scale;
    return d;
}

/* the label the kernels may read: on the device and of this node's shape */
static const float *label_gpu(const bcnn_net *net, const bcnn_tensor *x) {
    const bcnn_tensor *label = &net->tensors[1];
    return (label->n == x->n && label->c == 1 && label->h == x->h && label->w == x->w) ? label->data_gpu : NULL;
}

void bcnn_forward_softmax_loss_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_softmax_loss_param *p = (bcnn_softmax_loss_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const bcnn_hip_softmax_loss_desc d = loss_desc(p);
    const float *label = net->mode == BCNN_MODE_PREDICT ? NULL : label_gpu(net, x);
    p->has_stats = label != NULL && p->record_gpu != NULL;
    bcnn_hip_softmax_loss_forward(&d, x->data_gpu, p->has_stats ? label : NULL, y->data_gpu,
                                  (bcnn_hip_softmax_loss_record *)p->record_gpu, x->n, x->c, x->h * x->w);
}

void bcnn_backward_softmax_loss_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_softmax_loss_param *p = (const bcnn_softmax_loss_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const float *label = label_gpu(net, x);
    if (!x->grad_data_gpu || !label || !p->has_stats) return; /* no dX to write, or no forward that left a factor */
    const bcnn_hip_softmax_loss_desc d = loss_desc(p);
    bcnn_hip_softmax_loss_backward(&d, y->data_gpu, label, (const bcnn_hip_softmax_loss_record *)p->record_gpu,
                                   x->grad_data_gpu, x->n, x->c, x->h * x->w, bcnn_grad_sole_writer(net, node->src[0]));
}

void bcnn_release_param_softmax_loss_layer(bcnn_node *node) {
    bcnn_softmax_loss_param *p = (bcnn_softmax_loss_param *)node->param;
    bcnn_hip_free(p->record_gpu);
    p->record_gpu = NULL;
}

static int read_record(bcnn_node *node, bcnn_hip_softmax_loss_record *rec) {
    const bcnn_softmax_loss_param *p = (const bcnn_softmax_loss_param *)node->param;
    memset(rec, 0, sizeof(*rec));
    if (!p->has_stats || !p->record_gpu) return 0;
    bcnn_hip_memcpy_d2h(rec, p->record_gpu, sizeof(*rec)); /* waits for the forward that wrote it */
    return 1;
}

float bcnn_softmax_loss_read_loss(bcnn_net *net, bcnn_node *node) {
    (void)net;
    bcnn_hip_softmax_loss_record rec;
    read_record(node, &rec);
    return rec.loss;
}

static bcnn_node *loss_node(bcnn_net *net, int node) {
    if (!net || node < 0 || node >= net->num_nodes || net->nodes[node].type != BCNN_LAYER_SOFTMAX_LOSS) return NULL;
    return &net->nodes[node];
}

bcnn_status bcnn_get_softmax_loss_stats(bcnn_net *net, int node, bcnn_softmax_loss_stats *out) {
    if (!out) return BCNN_INVALID_PARAMETER;
    memset(out, 0, sizeof(*out));
    bcnn_node *nd = loss_node(net, node);
    bcnn_hip_softmax_loss_record rec;
    if (!nd || !read_record(nd, &rec)) return BCNN_INVALID_PARAMETER;
    out->loss = rec.loss;
    out->valid = rec.valid;
    out->ignored = rec.ignored;
    out->out_of_range = rec.out_of_range;
    out->correct = rec.correct;
    return BCNN_SUCCESS;
}

bcnn_status bcnn_get_confusion_matrix(bcnn_net *net, int node, int64_t *counts) {
    bcnn_node *nd = loss_node(net, node);
    if (!nd || !counts) return BCNN_INVALID_PARAMETER;
    const bcnn_tensor *x = &net->tensors[nd->src[0]], *y = &net->tensors[nd->dst[0]];
    const float *label = label_gpu(net, x);
    if (!label || !y->data_gpu) return BCNN_INVALID_PARAMETER;
    const size_t cells = (size_t)x->c * x->c;
    unsigned *counts_gpu = (unsigned *)bcnn_hip_malloc_f32(cells);
    unsigned *host = (unsigned *)malloc(cells * sizeof(unsigned));
    if (!counts_gpu || !host) {
        bcnn_hip_free(counts_gpu);
        free(host);
        return BCNN_FAILED_ALLOC;
    }
    const bcnn_hip_softmax_loss_desc d = loss_desc((const bcnn_softmax_loss_param *)nd->param);
    bcnn_hip_softmax_loss_confusion(&d, y->data_gpu, label, counts_gpu, x->n, x->c, x->h * x->w);
    bcnn_hip_memcpy_d2h(host, counts_gpu, cells * sizeof(unsigned));
    for (size_t i = 0; i < cells; ++i) counts[i] = (int64_t)host[i];
    bcnn_hip_free(counts_gpu);
    free(host);
    return BCNN_SUCCESS;
}
