/*
 * bcnn_layers_scale.c -- the scale-channels node: dst = src * gate, with one factor per (image, channel) plane (the last
 * step of a squeeze-and-excitation block, Darknet's [scale_channels]) or a gate of the source's shape (Darknet's [sam]).
 * Builder and node workers; one whole-batch call into the C-ABI per direction (scale_channels.hip).
 *
 * No reference counterpart (bcnn_load_net of the reference ends such a cfg with "Unknown Layer").
 *   - the builder checks both names and the gate's shape before it adds anything (INTEGRATION.md lists the refusals);
 *   - the backward ADDS into both source gradients, whoever else writes them: the node claims no sole-writer shortcut, so
 *     both fills stay unless another consumer's rule removes them (bcnn_core.c: mark_dead_grad_fills);
 *   - no parameters, no private buffers: model files skip the node, bcnn_resize_net reshapes dst like src, and the gate's
 *     form is read from the two shapes at every call.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

/* 0: one factor per plane, 1: the source's shape, -1: neither */
static int gate_form(const bcnn_tensor *x, const bcnn_tensor *g) {
    if (g->n != x->n || g->c != x->c) return -1;
    if (g->h == 1 && g->w == 1) return 0;
    return (g->h == x->h && g->w == x->w) ? 1 : -1;
}

bcnn_status bcnn_add_scale_channels_layer(bcnn_net *net, const char *src_id, const char *gate_id, const char *dst_id) {
    const int src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
    BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Scale-channels layer: invalid input node name %s\n",
                       src_id ? src_id : "(null)");
    const int gate = gate_id ? bcnn_net_find_tensor(net, gate_id) : -1;
    BCNN_CHECK_AND_LOG(net->log_ctx, gate >= 0, BCNN_INVALID_PARAMETER, "Scale-channels layer: invalid gate node name %s\n",
                       gate_id ? gate_id : "(null)");
    const bcnn_tensor s = net->tensors[src], g = net->tensors[gate];
    const int form = gate_form(&s, &g);
    BCNN_CHECK_AND_LOG(net->log_ctx, form >= 0, BCNN_INVALID_PARAMETER,
                       "Scale-channels layer %s: the gate %s is %d x %d x %d x %d; it must be %d x %d x 1 x 1 or the shape "
                       "of %s, %d x %d x %d x %d (n x c x h x w)\n", dst_id, gate_id, g.n, g.c, g.h, g.w, s.n, s.c, src_id, s.n,
                       s.c, s.h, s.w);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, gate));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_SCALE_CHANNELS;
    node.param_size = sizeof(bcnn_scale_channels_param);
    bcnn_scale_channels_param *param = (bcnn_scale_channels_param *)calloc(1, node.param_size);
    node.param = param;
    param->same_shape = form;
    node.forward = bcnn_forward_scale_channels_layer;
    node.backward = bcnn_backward_scale_channels_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[ScaleChannels%s] %-8s (%4d x%4d x%4d) * %-8s -> %-8s\n", form ? " same-shape" : "", src_id, s.w,
              s.h, s.c, gate_id, dst_id);
    return BCNN_SUCCESS;
}

void bcnn_forward_scale_channels_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_tensor *x = &net->tensors[node->src[0]], *g = &net->tensors[node->src[1]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const int form = gate_form(x, g);
    if (form < 0) return; /* a resize gave the two sources shapes that no longer fit (the builder refuses them) */
    bcnn_hip_scale_channels_forward(x->data_gpu, g->data_gpu, y->data_gpu, x->n, x->c, x->h * x->w, form);
}

void bcnn_backward_scale_channels_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_tensor *x = &net->tensors[node->src[0]], *g = &net->tensors[node->src[1]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    const int form = gate_form(x, g);
    if (form < 0 || !y->grad_data_gpu) return;
    /* either source may have no gradient (the net input): that half is skipped */
    bcnn_hip_scale_channels_backward(x->data_gpu, g->data_gpu, y->grad_data_gpu, x->grad_data_gpu, g->grad_data_gpu, x->n,
                                     x->c, x->h * x->w, form);
}
