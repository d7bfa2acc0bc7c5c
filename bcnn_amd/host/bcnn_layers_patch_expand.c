/*
 * bcnn_layers_patch_expand.c -- the patch-expanding node: the channels of an NCHW tensor move to block x block positions
 * ([N,p^2 c,H,W] -> [N,c,pH,pW], p = 2 or 4, in Swin-UNet's or in PixelShuffle's channel order) and, with norm, every output
 * position is normalised over its c values and mapped through a per-channel scale and bias -- the upward step of Swin-UNet's
 * decoder, whose Linear(C, 2C) is a 1x1 convolution node in front of this one; without norm it is depth-to-space / PixelShuffle.
 * Builder, node workers, update and release; one whole-batch call into the C-ABI per direction (patch_expand.hip). It stands
 * beside the patch-merging node (bcnn_layers_patch_merge.c), whose rules for parameters, statistics and the source gradient
 * it follows.
 *
 * No reference counterpart.
 *   - the builder checks the source name, the block, the order and the shape before it adds anything;
 *   - the same function in TRAIN, VALID and PREDICT mode. With norm, a net built in TRAIN / VALID mode keeps mean and rstd
 *     of the last forward (one [2][N * pH * pW] buffer, followed by bcnn_resize_net through its capacity);
 *   - the backward assigns the source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and
 *     adds otherwise; a source without a gradient (the net input) is skipped;
 *   - the scales train by the weights' rule (weight decay included), the biases by the biases'.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_patch_expanding_layer(bcnn_net *net, int block, bcnn_patch_expand_order order, int norm, float eps,
                                           const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Patch-expanding layer: invalid input node name %s\n",
                           src_id ? src_id : "(null)");
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, block == 2 || block == 4, BCNN_INVALID_PARAMETER,
                       "Patch-expanding layer %s: block %d; only 2 and 4 are built\n", dst_id, block);
    BCNN_CHECK_AND_LOG(net->log_ctx, order == BCNN_PATCH_EXPAND_BLOCKS || order == BCNN_PATCH_EXPAND_CHANNELS,
                       BCNN_INVALID_PARAMETER, "Patch-expanding layer %s: unknown order %d (blocks or channels)\n", dst_id, (int)order);
    BCNN_CHECK_AND_LOG(net->log_ctx, s.c > 0 && s.c % (block * block) == 0, BCNN_INVALID_PARAMETER,
                       "Patch-expanding layer %s: %d source channels are no multiple of block^2 = %d\n", dst_id, s.c, block * block);
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_hip_patch_expand_path(s.n, s.c, s.h, s.w, block) >= 0, BCNN_INVALID_PARAMETER,
                       "Patch-expanding layer %s: an empty source, or one of 2^31 elements or more\n", dst_id);
    if (!src_id) src_id = s.name ? s.name : "input";
    const int c = s.c / (block * block);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    if (norm) {
        BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, c, 1, src_id, "pe_scales", 1.0f, 1));
        BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, c, 1, src_id, "pe_b", 0.0f, 1));
    }
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, c, s.h * block, s.w * block, dst_id));
    node.type = BCNN_LAYER_PATCH_EXPANDING;
    node.param_size = sizeof(bcnn_patch_expanding_param);
    bcnn_patch_expanding_param *param = (bcnn_patch_expanding_param *)calloc(1, node.param_size);
    node.param = param;
    param->block = block;
    param->order = (int)order;
    param->norm = norm != 0;
    param->eps = eps > 0.f ? eps : 1e-5f;
    if (norm && net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->stats_capacity = 2 * (size_t)s.n * (size_t)(s.h * block) * (size_t)(s.w * block);
        param->stats_gpu = bcnn_hip_malloc_f32(param->stats_capacity);
    }
    node.forward = bcnn_forward_patch_expanding_layer;
    node.backward = bcnn_backward_patch_expanding_layer;
    if (norm) node.update = bcnn_update_patch_expanding_layer;
    node.release_param = bcnn_release_param_patch_expanding_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[PatchExpanding] %-8s (%4d x%4d x%4d) -> %-8s (%4d x%4d x%4d) block= %d order= %s norm= %d eps= %g\n",
              src_id, s.w, s.h, s.c, dst_id, s.w * block, s.h * block, c, block,
              order == BCNN_PATCH_EXPAND_BLOCKS ? "blocks" : "channels", param->norm, param->eps);
    return BCNN_SUCCESS;
}

void bcnn_forward_patch_expanding_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_patch_expanding_param *p = (const bcnn_patch_expanding_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    bcnn_hip_patch_expand_fwd_args a = {x->data_gpu, NULL, NULL, y->data_gpu, NULL, NULL, x->n, x->c, x->h, x->w,
                                        p->block, p->order, p->eps};
    if (p->norm) {
        const size_t rows = (size_t)y->n * (size_t)y->h * (size_t)y->w;
        a.scales = net->tensors[node->src[1]].data_gpu;
        a.b = net->tensors[node->src[2]].data_gpu;
        /* PREDICT stores no statistics; nor does a net whose buffer a resize without need_realloc could not follow */
        if (net->mode != BCNN_MODE_PREDICT && p->stats_gpu && 2 * rows <= p->stats_capacity) {
            a.mean = p->stats_gpu;
            a.rstd = p->stats_gpu + rows;
        }
    }
    bcnn_hip_patch_expand_forward(&a);
}

void bcnn_backward_patch_expanding_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_patch_expanding_param *p = (const bcnn_patch_expanding_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!y->grad_data_gpu) return; /* PREDICT-built */
    bcnn_hip_patch_expand_bwd_args a = {NULL, NULL, NULL, NULL, y->grad_data_gpu, x->grad_data_gpu, NULL, NULL, x->n, x->c, x->h,
                                        x->w, p->block, p->order, bcnn_grad_sole_writer(net, node->src[0])};
    if (p->norm) {
        const size_t rows = (size_t)y->n * (size_t)y->h * (size_t)y->w;
        if (!p->stats_gpu || 2 * rows > p->stats_capacity) {
            /* no forward kept the statistics (see the channel-norm node); said aloud, because under the sole-writer mark the
             * source gradient now holds nothing */
            BCNN_WARNING(net->log_ctx,
                         "Patch-expanding layer: no statistics of %zu positions kept (capacity %zu floats), backward skipped\n", rows,
                         p->stats_capacity);
            return;
        }
        bcnn_tensor *g = &net->tensors[node->src[1]], *b = &net->tensors[node->src[2]];
        a.x = x->data_gpu;
        a.scales = g->data_gpu;
        a.mean = p->stats_gpu;
        a.rstd = p->stats_gpu + rows;
        a.dscales = g->grad_data_gpu;
        a.db = b->grad_data_gpu;
    }
    bcnn_hip_patch_expand_backward(&a); /* (without norm and without a source gradient, the net input: nothing to do there) */
}

void bcnn_update_patch_expanding_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_patch_expanding_param *p = (bcnn_patch_expanding_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_patch_expanding_layer(bcnn_node *node) {
    bcnn_patch_expanding_param *p = (bcnn_patch_expanding_param *)node->param;
    bcnn_hip_free(p->stats_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
