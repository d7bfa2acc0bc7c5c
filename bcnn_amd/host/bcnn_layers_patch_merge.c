/*
 * bcnn_layers_patch_merge.c -- the patch-merging node: the 2x2 neighbours of an NCHW tensor move to the channels
 * ([N,C,H,W] -> [N,4C,H/2,W/2], Swin's order) and, with norm, every output position is normalised over its 4C values and
 * mapped through a per-channel scale and bias -- the step between Swin stages, whose Linear(4C, 2C) is a 1x1 convolution
 * node behind this one; without norm it is space-to-depth (YOLOv5's Focus). Builder, node workers, update and release; one
 * whole-batch call into the C-ABI per direction (patch_merge.hip). It stands beside the channel-norm node
 * (bcnn_layers_channelnorm.c), whose rules for parameters, statistics and the source gradient it follows.
 *
 * No reference counterpart.
 *   - the builder checks the source name and the shape before it adds anything (INTEGRATION.md lists the refusals);
 *   - the same function in TRAIN, VALID and PREDICT mode. With norm, a net built in TRAIN / VALID mode keeps mean and rstd
 *     of the last forward (one [2][N * H/2 * W/2] buffer, followed by bcnn_resize_net through its capacity);
 *   - the backward assigns the source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and
 *     adds otherwise; a source without a gradient (the net input) is skipped;
 *   - the scales train by the weights' rule (weight decay included), the biases by the biases'.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_patch_merging_layer(bcnn_net *net, int norm, float eps, const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Patch-merging layer: invalid input node name %s\n",
                           src_id ? src_id : "(null)");
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, s.h > 0 && s.w > 0 && !(s.h & 1) && !(s.w & 1), BCNN_INVALID_PARAMETER,
                       "Patch-merging layer %s: a %d x %d source; height and width must be even (no padding is built)\n",
                       dst_id, s.w, s.h);
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_hip_patch_merge_path(s.n, s.c, s.h, s.w) >= 0, BCNN_INVALID_PARAMETER,
                       "Patch-merging layer %s: an empty source, or one of 2^31 elements or more\n", dst_id);
    if (!src_id) src_id = s.name ? s.name : "input";

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    if (norm) {
        BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, 4 * s.c, 1, src_id, "pm_scales", 1.0f, 1));
        BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, 4 * s.c, 1, src_id, "pm_b", 0.0f, 1));
    }
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, 4 * s.c, s.h / 2, s.w / 2, dst_id));
    node.type = BCNN_LAYER_PATCH_MERGING;
    node.param_size = sizeof(bcnn_patch_merging_param);
    bcnn_patch_merging_param *param = (bcnn_patch_merging_param *)calloc(1, node.param_size);
    node.param = param;
    param->norm = norm != 0;
    param->eps = eps > 0.f ? eps : 1e-5f;
    if (norm && net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->stats_capacity = 2 * (size_t)s.n * (size_t)(s.h / 2) * (size_t)(s.w / 2);
        param->stats_gpu = bcnn_hip_malloc_f32(param->stats_capacity);
    }
    node.forward = bcnn_forward_patch_merging_layer;
    node.backward = bcnn_backward_patch_merging_layer;
    if (norm) node.update = bcnn_update_patch_merging_layer;
    node.release_param = bcnn_release_param_patch_merging_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[PatchMerging] %-8s (%4d x%4d x%4d) -> %-8s (%4d x%4d x%4d) norm= %d eps= %g\n", src_id, s.w, s.h,
              s.c, dst_id, s.w / 2, s.h / 2, 4 * s.c, param->norm, param->eps);
    return BCNN_SUCCESS;
}

void bcnn_forward_patch_merging_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_patch_merging_param *p = (const bcnn_patch_merging_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!p->norm) {
        bcnn_hip_patch_merge_forward(x->data_gpu, NULL, NULL, y->data_gpu, NULL, NULL, x->n, x->c, x->h, x->w, p->eps);
        return;
    }
    const size_t rows = (size_t)y->n * (size_t)y->h * (size_t)y->w;
    /* PREDICT stores no statistics; nor does a net whose buffer a resize without need_realloc could not follow */
    float *mean = (net->mode != BCNN_MODE_PREDICT && p->stats_gpu && 2 * rows <= p->stats_capacity) ? p->stats_gpu : NULL;
    bcnn_hip_patch_merge_forward(x->data_gpu, net->tensors[node->src[1]].data_gpu, net->tensors[node->src[2]].data_gpu,
                                 y->data_gpu, mean, mean ? mean + rows : NULL, x->n, x->c, x->h, x->w, p->eps);
}

void bcnn_backward_patch_merging_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_patch_merging_param *p = (const bcnn_patch_merging_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const int sole = bcnn_grad_sole_writer(net, node->src[0]);
    if (!y->grad_data_gpu) return; /* PREDICT-built */
    if (!p->norm) { /* the source may have no gradient (the net input): nothing to do then */
        if (x->grad_data_gpu)
            bcnn_hip_patch_merge_backward(NULL, NULL, NULL, NULL, y->grad_data_gpu, x->grad_data_gpu, NULL, NULL, x->n, x->c, x->h,
                                          x->w, sole);
        return;
    }
    const size_t rows = (size_t)y->n * (size_t)y->h * (size_t)y->w;
    if (!p->stats_gpu || 2 * rows > p->stats_capacity) {
        /* no forward kept the statistics (see the channel-norm node); said aloud, because under the sole-writer mark the
         * source gradient now holds nothing */
        BCNN_WARNING(net->log_ctx, "Patch-merging layer: no statistics of %zu positions kept (capacity %zu floats), backward skipped\n",
                     rows, p->stats_capacity);
        return;
    }
    bcnn_tensor *g = &net->tensors[node->src[1]], *b = &net->tensors[node->src[2]];
    bcnn_hip_patch_merge_backward(x->data_gpu, g->data_gpu, p->stats_gpu, p->stats_gpu + rows, y->grad_data_gpu, x->grad_data_gpu,
                                  g->grad_data_gpu, b->grad_data_gpu, x->n, x->c, x->h, x->w, sole);
}

void bcnn_update_patch_merging_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_patch_merging_param *p = (bcnn_patch_merging_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_patch_merging_layer(bcnn_node *node) {
    bcnn_patch_merging_param *p = (bcnn_patch_merging_param *)node->param;
    bcnn_hip_free(p->stats_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
