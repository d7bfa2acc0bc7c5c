/*
 * bcnn_layers_channelnorm.c -- the channel-norm node: every position of an NCHW tensor is normalised over its C channels
 * and mapped through a per-channel scale and bias (torch's LayerNorm(C) on tokens, LayerNorm2d). Builder, node workers,
 * update and release; one whole-batch call into the C-ABI per direction (channel_norm.hip). It stands beside the group-norm
 * node (bcnn_layers_groupnorm.c), whose one group normalises over (C,H,W).
 *
 * No reference counterpart.
 *   - the builder checks the source name and the tensor's size before it adds anything (INTEGRATION.md lists the refusals);
 *   - the same function in TRAIN, VALID and PREDICT mode. A net built in TRAIN / VALID mode keeps mean and rstd of the last
 *     forward (one [2][N * H * W] buffer, followed by bcnn_resize_net through its capacity); the backward recomputes the
 *     normalised values from them and the source;
 *   - the backward assigns the source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and
 *     adds otherwise; a source without a gradient (the net input) is skipped;
 *   - the scales train by the weights' rule (weight decay included), the biases by the biases'.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_channel_norm_layer(bcnn_net *net, float eps, const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Channel-norm layer: invalid input node name %s\n",
                           src_id ? src_id : "(null)");
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, (long long)s.n * s.c * s.h * s.w < 0x7fffffffLL, BCNN_INVALID_PARAMETER,
                       "Channel-norm layer %s: a source of 2^31 elements or more\n", dst_id);
    if (!src_id) src_id = s.name ? s.name : "input";

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, s.c, 1, src_id, "cn_scales", 1.0f, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, s.c, 1, src_id, "cn_b", 0.0f, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_CHANNEL_NORM;
    node.param_size = sizeof(bcnn_channel_norm_param);
    bcnn_channel_norm_param *param = (bcnn_channel_norm_param *)calloc(1, node.param_size);
    node.param = param;
    param->eps = eps > 0.f ? eps : 1e-5f;
    if (net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->stats_capacity = 2 * (size_t)s.n * (size_t)s.h * (size_t)s.w;
        param->stats_gpu = bcnn_hip_malloc_f32(param->stats_capacity);
    }
    node.forward = bcnn_forward_channel_norm_layer;
    node.backward = bcnn_backward_channel_norm_layer;
    node.update = bcnn_update_channel_norm_layer;
    node.release_param = bcnn_release_param_channel_norm_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[ChannelNorm] %-8s (%4d x%4d x%4d) -> %-8s eps= %g\n", src_id, s.w, s.h, s.c, dst_id, param->eps);
    return BCNN_SUCCESS;
}

void bcnn_forward_channel_norm_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_channel_norm_param *p = (const bcnn_channel_norm_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const size_t rows = (size_t)x->n * (size_t)x->h * (size_t)x->w;
    /* PREDICT stores no statistics; nor does a net whose buffer a resize without need_realloc could not follow */
    float *mean = (net->mode != BCNN_MODE_PREDICT && p->stats_gpu && 2 * rows <= p->stats_capacity) ? p->stats_gpu : NULL;
    const bcnn_hip_channel_norm_fwd_args a = {x->data_gpu, net->tensors[node->src[1]].data_gpu,
                                              net->tensors[node->src[2]].data_gpu, y->data_gpu, mean,
                                              mean ? mean + rows : NULL, x->n, x->c, x->h * x->w, p->eps};
    bcnn_hip_channel_norm_forward(&a);
}

void bcnn_backward_channel_norm_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_channel_norm_param *p = (const bcnn_channel_norm_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *g = &net->tensors[node->src[1]], *b = &net->tensors[node->src[2]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const size_t rows = (size_t)x->n * (size_t)x->h * (size_t)x->w;
    if (!y->grad_data_gpu) return; /* PREDICT-built */
    if (!p->stats_gpu || 2 * rows > p->stats_capacity) {
        /* no forward kept the statistics (see the group-norm node); said aloud, because under the sole-writer mark the source
         * gradient now holds nothing */
        BCNN_WARNING(net->log_ctx, "Channel-norm layer: no statistics of %zu positions kept (capacity %zu floats), backward skipped\n",
                     rows, p->stats_capacity);
        return;
    }
    /* the source may have no gradient (the net input): that half is skipped */
    const bcnn_hip_channel_norm_bwd_args a = {x->data_gpu, g->data_gpu, p->stats_gpu, p->stats_gpu + rows, y->grad_data_gpu,
                                              x->grad_data_gpu, g->grad_data_gpu, b->grad_data_gpu, x->n, x->c, x->h * x->w,
                                              bcnn_grad_sole_writer(net, node->src[0])};
    bcnn_hip_channel_norm_backward(&a);
}

void bcnn_update_channel_norm_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_channel_norm_param *p = (bcnn_channel_norm_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_channel_norm_layer(bcnn_node *node) {
    bcnn_channel_norm_param *p = (bcnn_channel_norm_param *)node->param;
    bcnn_hip_free(p->stats_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
