/*
 * bcnn_layers_dice_loss.c -- the dice-loss node: softmax over the channels, cross-entropy and soft Dice against a
 * class-index label map, loss = ce_weight * CE + dice_weight * Dice (Swin-UNet's and TransUNet's objective). Builder, node
 * workers and the two readers. One whole-batch call into the C-ABI per direction (dice_loss.hip); the mathematics is in
 * include/bcnn_hip.h.
 *
 * No reference counterpart. The node stands beside the softmax-loss node (bcnn_layers_softmax_loss.c), which keeps its
 * code: the same inputs, the same output (the probabilities), the same label rule (../csrc/softmax_loss_rule.h).
 *   - the builder checks every argument before it adds or allocates anything (INTEGRATION.md lists the refusals);
 *   - record, per-class sums and gradient coefficients live in one device workspace: the forward does not synchronise,
 *     the backward reads the coefficients on the device, and the host reads the workspace only when asked (the two
 *     readers, and once per step for the loss that bcnn_train_on_batch returns). Its size depends on n and C alone,
 *     which bcnn_resize_net does not grow; a forward on a shape that needs more allocates it anew;
 *   - the backward adds into the source gradient like every other node and assigns when it is the gradient's only writer
 *     (bcnn_grad_sole_writer): its overwrite form writes every element, +0.0 on pixels that are not valid;
 *   - no parameters: model files skip the node.
 */
#include <math.h>
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"
#include "../csrc/softmax_loss_rule.h"

bcnn_status bcnn_add_dice_loss_layer(bcnn_net *net, int ignore_label, float ce_weight, float dice_weight, float smooth,
                                     int squared, bcnn_dice_reduce reduce, const char *src_id, const char *label_id,
                                     const char *dst_id) {
    (void)label_id; /* the label is always tensor 1 */
    BCNN_CHECK_AND_LOG(net->log_ctx, reduce == BCNN_DICE_REDUCE_BATCH || reduce == BCNN_DICE_REDUCE_IMAGE,
                       BCNN_INVALID_PARAMETER, "Dice-loss layer %s: unknown reduce %d\n", dst_id, (int)reduce);
    BCNN_CHECK_AND_LOG(net->log_ctx, ignore_label < BCNN_SL_MAX_IGNORE_LABEL, BCNN_INVALID_PARAMETER,
                       "Dice-loss layer %s: ignore_label %d is not below 2^24, no float holds it as an index\n", dst_id,
                       ignore_label);
    BCNN_CHECK_AND_LOG(net->log_ctx, smooth >= 0.0f && isfinite(smooth), BCNN_INVALID_PARAMETER,
                       "Dice-loss layer %s: smooth %g is negative or not finite\n", dst_id, smooth);
    BCNN_CHECK_AND_LOG(net->log_ctx, isfinite(ce_weight) && isfinite(dice_weight), BCNN_INVALID_PARAMETER,
                       "Dice-loss layer %s: a weight is not finite\n", dst_id);
    /* the node's own arguments are checked first; the line names them, so a config section's values can be read from it */
    BCNN_CHECK_AND_LOG(net->log_ctx, net->num_nodes >= 1, BCNN_INVALID_PARAMETER,
                       "Dice-loss layer (ignore %d ce %g dice %g smooth %g %s reduce %s) can't be the first layer of the network\n",
                       ignore_label, ce_weight, dice_weight, smooth, squared ? "squared" : "plain",
                       reduce == BCNN_DICE_REDUCE_BATCH ? "batch" : "image");
    const int src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
    BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Dice-loss layer: invalid input node name %s\n",
                       src_id ? src_id : "(null)");
    const bcnn_tensor s = net->tensors[src];
    const size_t ws = bcnn_hip_dice_loss_workspace_size(s.n, s.c, s.h * s.w, (int)reduce);
    BCNN_CHECK_AND_LOG(net->log_ctx, ws > 0, BCNN_INVALID_PARAMETER,
                       "Dice-loss layer %s: an empty source or one of 2^31 elements or more\n", dst_id);
    bcnn_tensor *label = &net->tensors[1];
    BCNN_CHECK_AND_LOG(net->log_ctx,
                       label->data == NULL || (label->n == s.n && label->c == 1 && label->h == s.h && label->w == s.w),
                       BCNN_INVALID_PARAMETER,
                       "Dice-loss layer %s: the label tensor is already %d x %d x %d x %d (another loss node shaped it), this "
                       "node needs %d x 1 x %d x %d\n", dst_id, label->n, label->c, label->h, label->w, s.n, s.h, s.w);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    if (label->data == NULL) {
        bcnn_tensor_set_shape(label, s.n, 1, s.h, s.w, 0);
        BCNN_CHECK_STATUS(bcnn_tensor_allocate(label, net->mode));
    }
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_DICE_LOSS;
    node.param_size = sizeof(bcnn_dice_loss_param);
    bcnn_dice_loss_param *param = (bcnn_dice_loss_param *)calloc(1, node.param_size);
    node.param = param;
    param->ignore_label = ignore_label;
    param->ce_weight = ce_weight;
    param->dice_weight = dice_weight;
    param->smooth = smooth;
    param->squared = squared != 0;
    param->reduce = reduce;
    param->label_capacity = (size_t)s.n * s.h * s.w;
    param->workspace_gpu = bcnn_hip_malloc_f32(ws); /* zero-filled */
    param->workspace_floats = ws;
    node.forward = bcnn_forward_dice_loss_layer;
    node.backward = bcnn_backward_dice_loss_layer;
    node.release_param = bcnn_release_param_dice_loss_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Dice loss] %-8s -> %-8s (%4d x%4d x%4d) ignore %d ce %g dice %g smooth %g %s reduce %s\n", src_id,
              dst_id, s.w, s.h, s.c, ignore_label, ce_weight, dice_weight, smooth, squared ? "squared" : "plain",
              reduce == BCNN_DICE_REDUCE_BATCH ? "batch" : "image");
    return BCNN_SUCCESS;
}

/* the label the kernels may read: on the device and of this node's shape */
static const float *label_gpu(const bcnn_net *net, const bcnn_tensor *x) {
    const bcnn_tensor *label = &net->tensors[1];
    return (label->n == x->n && label->c == 1 && label->h == x->h && label->w == x->w) ? label->data_gpu : NULL;
}

void bcnn_forward_dice_loss_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_dice_loss_param *p = (bcnn_dice_loss_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const float *label = net->mode == BCNN_MODE_PREDICT ? NULL : label_gpu(net, x);
    const size_t ws = bcnn_hip_dice_loss_workspace_size(x->n, x->c, x->h * x->w, (int)p->reduce);
    if (label != NULL && ws > p->workspace_floats) { /* a shape with more groups or classes than the node was built on */
        bcnn_hip_free(p->workspace_gpu);
        p->workspace_gpu = bcnn_hip_malloc_f32(ws);
        p->workspace_floats = p->workspace_gpu ? ws : 0;
        if (!p->workspace_gpu)
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Dice-loss layer: no memory for a workspace of %zu floats; this forward "
                                                   "computes no loss and its backward no gradient\n", ws);
    }
    p->has_stats = label != NULL && p->workspace_gpu != NULL && ws > 0 && ws <= p->workspace_floats;
    BcnnDiceLossFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x->data_gpu;
    a.label = p->has_stats ? label : NULL;
    a.p = y->data_gpu;
    a.workspace = p->has_stats ? p->workspace_gpu : NULL;
    a.n = x->n; a.c = x->c; a.hw = x->h * x->w;
    a.ignore_label = p->ignore_label; a.squared = p->squared; a.reduce = (int)p->reduce;
    a.ce_weight = p->ce_weight; a.dice_weight = p->dice_weight; a.smooth = p->smooth;
    bcnn_hip_dice_loss_forward(&a);
}

void bcnn_backward_dice_loss_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_dice_loss_param *p = (const bcnn_dice_loss_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const float *label = label_gpu(net, x);
    if (!x->grad_data_gpu || !label || !p->has_stats) return; /* no dX to write, or no forward that left coefficients */
    BcnnDiceLossBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.p = y->data_gpu;
    a.label = label;
    a.workspace = p->workspace_gpu;
    a.dx = x->grad_data_gpu;
    a.n = x->n; a.c = x->c; a.hw = x->h * x->w;
    a.ignore_label = p->ignore_label; a.squared = p->squared; a.reduce = (int)p->reduce;
    a.dice_weight = p->dice_weight;
    a.overwrite = bcnn_grad_sole_writer(net, node->src[0]);
    bcnn_hip_dice_loss_backward(&a);
}

void bcnn_release_param_dice_loss_layer(bcnn_node *node) {
    bcnn_dice_loss_param *p = (bcnn_dice_loss_param *)node->param;
    bcnn_hip_free(p->workspace_gpu);
    p->workspace_gpu = NULL;
}

static int read_record(bcnn_node *node, bcnn_hip_dice_loss_record *rec) {
    const bcnn_dice_loss_param *p = (const bcnn_dice_loss_param *)node->param;
    memset(rec, 0, sizeof(*rec));
    if (!p->has_stats || !p->workspace_gpu) return 0;
    bcnn_hip_memcpy_d2h(rec, p->workspace_gpu, sizeof(*rec)); /* waits for the forward that wrote it */
    return 1;
}

float bcnn_dice_loss_read_loss(bcnn_net *net, bcnn_node *node) {
    (void)net;
    bcnn_hip_dice_loss_record rec;
    read_record(node, &rec);
    return rec.loss;
}

static bcnn_node *loss_node(bcnn_net *net, int node) {
    if (!net || node < 0 || node >= net->num_nodes || net->nodes[node].type != BCNN_LAYER_DICE_LOSS) return NULL;
    return &net->nodes[node];
}

bcnn_status bcnn_get_dice_loss_stats(bcnn_net *net, int node, bcnn_dice_loss_stats *out) {
    if (!out) return BCNN_INVALID_PARAMETER;
    memset(out, 0, sizeof(*out));
    bcnn_node *nd = loss_node(net, node);
    bcnn_hip_dice_loss_record rec;
    if (!nd || !read_record(nd, &rec)) return BCNN_INVALID_PARAMETER;
    out->loss = rec.loss;
    out->ce = rec.ce;
    out->dice = rec.dice;
    out->valid = rec.valid;
    out->ignored = rec.ignored;
    out->out_of_range = rec.out_of_range;
    out->correct = rec.correct;
    return BCNN_SUCCESS;
}

int bcnn_get_dice_loss_groups(bcnn_net *net, int node) {
    bcnn_node *nd = loss_node(net, node);
    if (!nd) return -1;
    return ((const bcnn_dice_loss_param *)nd->param)->reduce == BCNN_DICE_REDUCE_IMAGE ? net->tensors[nd->src[0]].n : 1;
}

bcnn_status bcnn_get_dice_loss_sums(bcnn_net *net, int node, double *izy) {
    bcnn_node *nd = loss_node(net, node);
    if (!nd || !izy) return BCNN_INVALID_PARAMETER;
    const bcnn_dice_loss_param *p = (const bcnn_dice_loss_param *)nd->param;
    if (!p->has_stats || !p->workspace_gpu) return BCNN_INVALID_PARAMETER;
    const bcnn_tensor *x = &net->tensors[nd->src[0]];
    const size_t groups = p->reduce == BCNN_DICE_REDUCE_IMAGE ? (size_t)x->n : 1;
    bcnn_hip_memcpy_d2h(izy, p->workspace_gpu + sizeof(bcnn_hip_dice_loss_record) / sizeof(float),
                        groups * x->c * 3 * sizeof(double));
    return BCNN_SUCCESS;
}
