/*
 * bcnn_layers_dwdilated.c -- the dilated (atrous) depthwise convolution node: builder, node workers, update and release.
 * One whole-batch call into the C-ABI per direction (bcnn_hip_dilated_depthwise_forward / _backward,
 * depthwise_dilated.hip).
 *
 * No reference counterpart. A node of its own beside the depthwise node, as the dilated convolution stands beside the
 * convolution node (bcnn_layers_dilated.c); it follows the depthwise node's conventions where the two meet: tensor names
 * "<src>_w" (c * size * size floats laid out [c][size][size]) and "<src>_b" [c], the filler's range size * size * c, a
 * weight gradient that accumulates unscaled, a source gradient that accumulates unless this node is its sole writer
 * (bcnn_grad_sole_writer: the overwrite form writes every element, those no tap reaches too), and bcnn_node_optim_step
 * on weights and biases. None of the depthwise node's batch-norm links (bn_node / conv_node) or fusions sees it.
 *   - dilation == 1 delegates to bcnn_add_depthwise_conv_layer: callers keep the depthwise ladder and its fusions;
 *   - refused with a log line, nothing added to the net: an unknown source, size < 1, stride < 1, pad < 0, dilation < 1,
 *     a non-positive output extent, PReLU and the activations that need the layer's input.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_dilated_depthwise_conv_layer(bcnn_net *net, int size, int stride, int pad, int dilation,
                                                  bcnn_filler_type init, bcnn_activation activation,
                                                  const char *src_id, const char *dst_id) {
    if (dilation == 1) return bcnn_add_depthwise_conv_layer(net, size, stride, pad, 0, init, activation, src_id, dst_id);
    int src = 0;
    if (net->num_nodes > 0) {
        src = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER,
                           "Dilated depthwise convolution layer: invalid input node name %s\n", src_id);
    } else {
        BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_tensor_size(&net->tensors[0]) > 0, BCNN_INVALID_PARAMETER,
                           "Invalid input size of the network. Hint: use 'bcnn_set_input_shape'\n");
    }
    BCNN_CHECK_AND_LOG(net->log_ctx, activation != BCNN_ACT_PRELU, BCNN_INVALID_PARAMETER,
                       "Dilated depthwise convolution layer %s: PReLU is not supported\n", dst_id);
    BCNN_REFUSE_INPUT_ACTIVATION(net, activation, "Dilated depthwise convolution");
    BCNN_CHECK_AND_LOG(net->log_ctx, size >= 1 && stride >= 1 && pad >= 0 && dilation >= 1, BCNN_INVALID_PARAMETER,
                       "Dilated depthwise convolution layer %s: invalid size %d / stride %d / pad %d / dilation %d\n",
                       dst_id, size, stride, pad, dilation);
    const bcnn_tensor s = net->tensors[src];
    const long long eh = (long long)s.h + 2LL * pad - (long long)dilation * (size - 1) - 1;
    const long long ew = (long long)s.w + 2LL * pad - (long long)dilation * (size - 1) - 1;
    BCNN_CHECK_AND_LOG(net->log_ctx, eh >= 0 && ew >= 0, BCNN_INVALID_PARAMETER,
                       "Dilated depthwise convolution layer %s: a %d x %d kernel at dilation %d does not fit %d x %d "
                       "inputs with pad %d\n", dst_id, size, size, dilation, s.w, s.h, pad);
    const int oh = (int)(eh / stride) + 1, ow = (int)(ew / stride) + 1;

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    char name[256];
    snprintf(name, sizeof(name), "%s_w", src_id);
    bcnn_tensor weights = {0};
    bcnn_tensor_create(&weights, 1, 1, 1, s.c * size * size, 1, name, net->mode); /* laid out [C][k][k] */
    bcnn_tensor_filler wf = {.range = size * size * s.c, .type = init};
    bcnn_tensor_fill(&weights, wf);
    BCNN_CHECK_STATUS(bcnn_net_add_tensor(net, weights));
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, net->num_tensors - 1));
    bcnn_net_register_param(net, net->num_tensors - 1);
    snprintf(name, sizeof(name), "%s_b", src_id);
    bcnn_tensor biases = {0};
    bcnn_tensor_create(&biases, 1, 1, 1, s.c, 1, name, net->mode);
    BCNN_CHECK_STATUS(bcnn_net_add_tensor(net, biases));
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, net->num_tensors - 1));
    bcnn_net_register_param(net, net->num_tensors - 1);
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, oh, ow, dst_id));

    node.type = BCNN_LAYER_DILATED_DEPTHWISE_CONV2D;
    node.param_size = sizeof(bcnn_dilated_depthwise_param);
    bcnn_dilated_depthwise_param *param = (bcnn_dilated_depthwise_param *)calloc(1, node.param_size);
    node.param = param;
    param->activation = activation;
    param->size = size; param->stride = stride; param->pad = pad; param->dilation = dilation;
    node.forward = bcnn_forward_dilated_depthwise_layer;
    node.backward = bcnn_backward_dilated_depthwise_layer;
    node.update = bcnn_update_dilated_depthwise_layer;
    node.release_param = bcnn_release_param_dilated_depthwise_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx,
              "[DilatedDepthwiseConv2D] input_shape= %dx%dx%d kernel_size= %d stride= %d padding= %d dilation= %d "
              "output_shape= %dx%dx%d\n", s.w, s.h, s.c, size, stride, pad, dilation, ow, oh, s.c);
    return BCNN_SUCCESS;
}

void bcnn_forward_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_dilated_depthwise_param *p = (const bcnn_dilated_depthwise_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    bcnn_hip_dilated_depthwise_forward(x->data_gpu, w->data_gpu, b->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w, p->size,
                                       p->stride, p->pad, p->dilation, (int)p->activation);
}

void bcnn_backward_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_dilated_depthwise_param *p = (bcnn_dilated_depthwise_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    const size_t need = bcnn_hip_dilated_depthwise_workspace_size(x->n, x->c, x->h, x->w, p->size, p->stride, p->pad,
                                                                  p->dilation);
    if (p->workspace_size < need) { /* the node's own partial sums, sized on the first backward */
        bcnn_hip_free(p->workspace_gpu);
        p->workspace_gpu = bcnn_hip_malloc_f32(need);
        p->workspace_size = need;
    }
    bcnn_hip_dilated_depthwise_backward(x->data_gpu, w->data_gpu, y->data_gpu, y->grad_data_gpu,
                                        x->grad_data_gpu /* NULL for the net input: no dX */, w->grad_data_gpu,
                                        b->grad_data_gpu, x->n, x->c, x->h, x->w, p->size, p->stride, p->pad, p->dilation,
                                        (int)p->activation, bcnn_grad_sole_writer(net, node->src[0]), p->workspace_gpu,
                                        p->workspace_size);
}

void bcnn_update_dilated_depthwise_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_dilated_depthwise_param *p = (bcnn_dilated_depthwise_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_dilated_depthwise_layer(bcnn_node *node) {
    bcnn_dilated_depthwise_param *p = (bcnn_dilated_depthwise_param *)node->param;
    bcnn_hip_free(p->workspace_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
