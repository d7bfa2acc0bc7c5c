/*
 * bcnn_layers_pool2d.c -- the pool2d node: max or average pooling over a square window with the same padding on all four
 * sides (torch.nn.functional.max_pool2d / avg_pool2d, i.e. Caffe's rules). Builder, node workers, release and the
 * output-extent rule bcnn_resize_net uses. One whole-batch call into the C-ABI per direction (pool2d.hip).
 *
 * No reference counterpart: the reference's max pooling pads at the bottom / right only and its average pooling is
 * global; those two nodes (bcnn_layers_hot.c) keep their code, their dispatch and their fusions with the convolution and
 * batch-norm nodes. This node has a layer type and a param block of its own, so none of that code ever meets it.
 *   - the builder checks every parameter before it adds anything (INTEGRATION.md lists the refusals);
 *   - the backward adds into the source gradient like every other node and assigns when it is the gradient's only
 *     writer (bcnn_grad_sole_writer): its overwrite form touches every element, covered by a window or not;
 *   - a PREDICT-mode forward stores no indexes; a net built in PREDICT mode has no index buffer at all.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

static bcnn_hip_pool2d_desc pool2d_desc(const bcnn_pool2d_param *p) {
    bcnn_hip_pool2d_desc d;
    d.kind = p->kind == BCNN_POOL2D_AVG ? BCNN_HIP_POOL2D_AVG : BCNN_HIP_POOL2D_MAX;
    d.size = p->size;
    d.stride = p->stride;
    d.pad = p->pad;
    d.ceil_mode = p->ceil_mode;
    d.count_include_pad = p->count_include_pad;
    return d;
}

int bcnn_pool2d_out_extents(const bcnn_pool2d_param *p, int h, int w, int *out_h, int *out_w) {
    const bcnn_hip_pool2d_desc d = pool2d_desc(p);
    *out_h = bcnn_hip_pool2d_out_extent(&d, h);
    *out_w = bcnn_hip_pool2d_out_extent(&d, w);
    return *out_h > 0 && *out_w > 0;
}

bcnn_status bcnn_add_pool2d_layer(bcnn_net *net, bcnn_pool2d_kind kind, int size, int stride, int pad, int ceil_mode,
                                  int count_include_pad, const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Pool2d layer: invalid input node name %s\n",
                           src_id);
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, kind == BCNN_POOL2D_MAX || kind == BCNN_POOL2D_AVG, BCNN_INVALID_PARAMETER,
                       "Pool2d layer %s: unknown kind %d\n", dst_id, (int)kind);
    BCNN_CHECK_AND_LOG(net->log_ctx, size >= 1 && stride >= 1, BCNN_INVALID_PARAMETER,
                       "Pool2d layer %s: size %d and stride %d must be at least 1\n", dst_id, size, stride);
    BCNN_CHECK_AND_LOG(net->log_ctx, pad >= 0 && pad <= size / 2, BCNN_INVALID_PARAMETER,
                       "Pool2d layer %s: pad %d must lie in [0, size / 2 = %d]\n", dst_id, pad, size / 2);
    BCNN_CHECK_AND_LOG(net->log_ctx, s.h + 2 * pad >= size && s.w + 2 * pad >= size, BCNN_INVALID_PARAMETER,
                       "Pool2d layer %s: the padded input (%d + %d) x (%d + %d) is smaller than the %d x %d window\n", dst_id,
                       s.w, 2 * pad, s.h, 2 * pad, size, size);
    bcnn_pool2d_param proto;
    memset(&proto, 0, sizeof(proto));
    proto.kind = kind;
    proto.size = size; proto.stride = stride; proto.pad = pad;
    proto.ceil_mode = ceil_mode ? 1 : 0;
    proto.count_include_pad = count_include_pad ? 1 : 0;
    int oh = 0, ow = 0;
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_pool2d_out_extents(&proto, s.h, s.w, &oh, &ow), BCNN_INVALID_PARAMETER,
                       "Pool2d layer %s: empty output (%d x %d) for a %d x %d input\n", dst_id, ow, oh, s.w, s.h);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, oh, ow, dst_id));
    node.type = BCNN_LAYER_POOL2D;
    node.param_size = sizeof(bcnn_pool2d_param);
    bcnn_pool2d_param *param = (bcnn_pool2d_param *)calloc(1, node.param_size);
    node.param = param;
    *param = proto;
    if (kind == BCNN_POOL2D_MAX && net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->indexes_capacity = (size_t)s.n * s.c * oh * ow;
        param->indexes_gpu = bcnn_hip_malloc_i32(param->indexes_capacity);
    }
    node.forward = bcnn_forward_pool2d_layer;
    node.backward = bcnn_backward_pool2d_layer;
    node.release_param = bcnn_release_param_pool2d_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Pool2d %s] %-8s (%4d x%4d x%4d) -> %-8s (%4d x%4d x%4d) %d x %d / %d pad %d%s%s\n",
              kind == BCNN_POOL2D_MAX ? "max" : "avg", src_id, s.w, s.h, s.c, dst_id, ow, oh, s.c, size, size, stride, pad,
              ceil_mode ? " ceil" : "", kind == BCNN_POOL2D_AVG && !count_include_pad ? " exclude-pad" : "");
    return BCNN_SUCCESS;
}

void bcnn_forward_pool2d_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_pool2d_param *p = (const bcnn_pool2d_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const bcnn_hip_pool2d_desc d = pool2d_desc(p);
    /* PREDICT: no backward follows, the winners are not stored */
    bcnn_hip_pool2d_forward(&d, x->data_gpu, y->data_gpu, net->mode == BCNN_MODE_PREDICT ? NULL : p->indexes_gpu, x->n, x->c,
                            x->h, x->w);
}

void bcnn_backward_pool2d_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_pool2d_param *p = (const bcnn_pool2d_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!x->grad_data_gpu || !y->grad_data_gpu) return; /* the net input: no dX */
    if (p->kind == BCNN_POOL2D_MAX && !p->indexes_gpu) return; /* built in PREDICT mode: no forward stored any winner */
    const bcnn_hip_pool2d_desc d = pool2d_desc(p);
    bcnn_hip_pool2d_backward(&d, y->grad_data_gpu, p->indexes_gpu, x->grad_data_gpu, x->n, x->c, x->h, x->w,
                             bcnn_grad_sole_writer(net, node->src[0]));
}

void bcnn_release_param_pool2d_layer(bcnn_node *node) {
    bcnn_pool2d_param *p = (bcnn_pool2d_param *)node->param;
    bcnn_hip_free(p->indexes_gpu);
}
