/*
 * bcnn_layers_interp.c -- the interp node: bilinear interpolation of every plane to a new extent, with a gradient
 * (torch.nn.functional.interpolate(mode="bilinear") for both values of align_corners; Caffe-DeepLab's Interp layer is
 * align_corners = 1). Builder, node workers and the output-extent rule bcnn_resize_net uses. One whole-batch call into
 * the C-ABI per direction (interp.hip).
 *
 * No reference counterpart: the reference's only resampling node is the nearest-neighbour, integer-factor upsample
 * (bcnn_layers_next.c, detect.hip), which keeps its code. This node has a layer type and a param block of its own.
 *   - the output extent takes exactly one of three forms -- scale (in * scale), zoom ((in - 1) * zoom + 1) or fixed
 *     (out_w x out_h) -- by one function, bcnn_interp_out_extent (../csrc/interp_rule.h), which the builder and
 *     bcnn_resize_net both go through: scale and zoom follow a resized source, the fixed form keeps its extents;
 *   - the builder checks every parameter before it adds anything (INTEGRATION.md lists the refusals);
 *   - the backward adds into the source gradient like every other node and assigns when it is the gradient's only
 *     writer (bcnn_grad_sole_writer): its overwrite form touches every element, named by an output or not;
 *   - no parameters and no private buffers: model files skip the node, and it is fp32 in every inference-precision mode.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"
#include "../csrc/interp_rule.h"

int bcnn_interp_out_extents(const bcnn_interp_param *p, int h, int w, int *out_h, int *out_w) {
    *out_h = bcnn_interp_out_extent(h, p->scale, p->zoom, p->out_h);
    *out_w = bcnn_interp_out_extent(w, p->scale, p->zoom, p->out_w);
    return *out_h > 0 && *out_w > 0;
}

bcnn_status bcnn_add_interp_layer(bcnn_net *net, int out_w, int out_h, int scale, int zoom, int align_corners,
                                  const char *src_id, const char *dst_id) {
    const int src = src_id ? bcnn_net_find_tensor(net, src_id) : -1;
    BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Interp layer: invalid input node name %s\n",
                       src_id ? src_id : "(null)");
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, out_w >= 0 && out_h >= 0 && scale >= 0 && zoom >= 0, BCNN_INVALID_PARAMETER,
                       "Interp layer %s: out_w %d, out_h %d, scale %d and zoom %d must not be negative\n", dst_id, out_w, out_h,
                       scale, zoom);
    BCNN_CHECK_AND_LOG(net->log_ctx, (out_w > 0) == (out_h > 0), BCNN_INVALID_PARAMETER,
                       "Interp layer %s: the fixed form needs both out_w (%d) and out_h (%d)\n", dst_id, out_w, out_h);
    BCNN_CHECK_AND_LOG(net->log_ctx, (scale > 0) + (zoom > 0) + (out_w > 0) == 1, BCNN_INVALID_PARAMETER,
                       "Interp layer %s: exactly one of scale (%d), zoom (%d) and out_w x out_h (%d x %d) must be given "
                       "(align_corners %d)\n", dst_id, scale, zoom, out_w, out_h, align_corners ? 1 : 0);
    bcnn_interp_param proto;
    memset(&proto, 0, sizeof(proto));
    proto.scale = scale; proto.zoom = zoom; proto.out_w = out_w; proto.out_h = out_h;
    proto.align_corners = align_corners ? 1 : 0;
    int oh = 0, ow = 0;
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_interp_out_extents(&proto, s.h, s.w, &oh, &ow), BCNN_INVALID_PARAMETER,
                       "Interp layer %s: no valid output extent for a %d x %d input\n", dst_id, s.w, s.h);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, oh, ow, dst_id));
    node.type = BCNN_LAYER_INTERP;
    node.param_size = sizeof(bcnn_interp_param);
    bcnn_interp_param *param = (bcnn_interp_param *)calloc(1, node.param_size);
    node.param = param;
    *param = proto;
    node.forward = bcnn_forward_interp_layer;
    node.backward = bcnn_backward_interp_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Interp bilinear] %-8s (%4d x%4d x%4d) -> %-8s (%4d x%4d x%4d) %s %d%s\n", src_id, s.w, s.h, s.c,
              dst_id, ow, oh, s.c, scale ? "scale" : zoom ? "zoom" : "fixed", scale ? scale : zoom ? zoom : ow,
              align_corners ? " align-corners" : "");
    return BCNN_SUCCESS;
}

static bcnn_hip_interp_desc interp_desc(const bcnn_tensor *y, const bcnn_interp_param *p) {
    bcnn_hip_interp_desc d;
    d.out_h = y->h;
    d.out_w = y->w;
    d.align_corners = p->align_corners;
    return d;
}

void bcnn_forward_interp_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const bcnn_hip_interp_desc d = interp_desc(y, (const bcnn_interp_param *)node->param);
    bcnn_hip_interp_forward(&d, x->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w);
}

void bcnn_backward_interp_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!x->grad_data_gpu || !y->grad_data_gpu) return; /* the net input: no dX */
    const bcnn_hip_interp_desc d = interp_desc(y, (const bcnn_interp_param *)node->param);
    bcnn_hip_interp_backward(&d, y->grad_data_gpu, x->grad_data_gpu, x->n, x->c, x->h, x->w,
                             bcnn_grad_sole_writer(net, node->src[0]));
}
