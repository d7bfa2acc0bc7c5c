/*
 * bcnn_layers_groupnorm.c -- the group-normalisation node: per image, groups of C / G consecutive channels are normalised
 * over their (C / G) * H * W values and mapped through a per-channel scale and bias. Layer norm over (C,H,W) is G = 1,
 * instance norm with affine G = C. Builder, node workers, update and release; one whole-batch call into the C-ABI per
 * direction (group_norm.hip).
 *
 * No reference counterpart (bcnn_load_net of the reference ends such a cfg with "Unknown Layer").
 *   - the builder checks the source name and the group count before it adds anything (INTEGRATION.md lists the refusals);
 *   - the same function in TRAIN, VALID and PREDICT mode: no running statistics. A net built in TRAIN / VALID mode keeps
 *     mean and rstd of the last forward (one [2][N * G] buffer, followed by bcnn_resize_net through its capacity); the
 *     backward recomputes the normalised values from them and the source;
 *   - the backward assigns the source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and
 *     adds otherwise; a source without a gradient (the net input) is skipped;
 *   - the scales train by the weights' rule (weight decay included), the biases by the biases'.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_groupnorm_layer(bcnn_net *net, int num_groups, float eps, const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Group-norm layer: invalid input node name %s\n",
                           src_id ? src_id : "(null)");
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, num_groups > 0, BCNN_INVALID_PARAMETER,
                       "Group-norm layer %s: the number of groups %d must be positive\n", dst_id, num_groups);
    BCNN_CHECK_AND_LOG(net->log_ctx, s.c % num_groups == 0, BCNN_INVALID_PARAMETER,
                       "Group-norm layer %s: %d groups do not divide the %d channels of %s\n", dst_id, num_groups, s.c,
                       src_id);
    if (!src_id) src_id = s.name ? s.name : "input";

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, s.c, 1, src_id, "gn_scales", 1.0f, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, s.c, 1, src_id, "gn_b", 0.0f, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_GROUPNORM;
    node.param_size = sizeof(bcnn_groupnorm_param);
    bcnn_groupnorm_param *param = (bcnn_groupnorm_param *)calloc(1, node.param_size);
    node.param = param;
    param->num_groups = num_groups;
    param->eps = eps > 0.f ? eps : 1e-5f;
    if (net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->stats_capacity = 2 * (size_t)s.n * (size_t)num_groups;
        param->stats_gpu = bcnn_hip_malloc_f32(param->stats_capacity);
    }
    node.forward = bcnn_forward_groupnorm_layer;
    node.backward = bcnn_backward_groupnorm_layer;
    node.update = bcnn_update_groupnorm_layer;
    node.release_param = bcnn_release_param_groupnorm_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[GroupNorm] %-8s (%4d x%4d x%4d) -> %-8s groups= %d eps= %g\n", src_id, s.w, s.h, s.c, dst_id,
              num_groups, param->eps);
    return BCNN_SUCCESS;
}

void bcnn_forward_groupnorm_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_groupnorm_param *p = (const bcnn_groupnorm_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const size_t rows = (size_t)x->n * (size_t)p->num_groups;
    /* PREDICT stores no statistics; nor does a net whose buffer a resize without need_realloc could not follow */
    float *mean = (net->mode != BCNN_MODE_PREDICT && p->stats_gpu && 2 * rows <= p->stats_capacity) ? p->stats_gpu : NULL;
    bcnn_hip_group_norm_forward(x->data_gpu, net->tensors[node->src[1]].data_gpu, net->tensors[node->src[2]].data_gpu,
                                y->data_gpu, mean, mean ? mean + rows : NULL, x->n, x->c, x->h * x->w, p->num_groups,
                                p->eps);
}

void bcnn_backward_groupnorm_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_groupnorm_param *p = (const bcnn_groupnorm_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *g = &net->tensors[node->src[1]], *b = &net->tensors[node->src[2]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const size_t rows = (size_t)x->n * (size_t)p->num_groups;
    if (!y->grad_data_gpu) return; /* PREDICT-built */
    if (!p->stats_gpu || 2 * rows > p->stats_capacity) {
        /* no forward kept the statistics. Unreachable today (a resize sets the batch to 1, a PREDICT net has no gradients);
         * said aloud, because under the sole-writer mark the source gradient now holds nothing */
        BCNN_WARNING(net->log_ctx, "Group-norm layer: no statistics of %zu rows kept (capacity %zu floats), backward skipped\n",
                     rows, p->stats_capacity);
        return;
    }
    /* the source may have no gradient (the net input): that half is skipped */
    bcnn_hip_group_norm_backward(x->data_gpu, g->data_gpu, p->stats_gpu, p->stats_gpu + rows, y->grad_data_gpu,
                                 x->grad_data_gpu, g->grad_data_gpu, b->grad_data_gpu, x->n, x->c, x->h * x->w,
                                 p->num_groups, bcnn_grad_sole_writer(net, node->src[0]));
}

void bcnn_update_groupnorm_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_groupnorm_param *p = (bcnn_groupnorm_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_groupnorm_layer(bcnn_node *node) {
    bcnn_groupnorm_param *p = (bcnn_groupnorm_param *)node->param;
    bcnn_hip_free(p->stats_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
