/*
 * bcnn_layers_dilated.c -- the dilated (atrous) convolution node: builder, node workers, update and release.
 * One whole-batch call into the C-ABI per direction (bcnn_hip_dilated_conv_forward / _backward, conv_dilated.hip).
 *
 * No reference counterpart. The node follows the convolution node's conventions where the two meet: tensor names
 * "<src>_w" [num][c / groups][size][size] and "<src>_b" [num], the filler's range size * size * c / groups, a weight
 * gradient that accumulates unscaled, a source gradient that is overwritten (quirk 3), and bcnn_node_optim_step on
 * weights and biases. It is a node of its own, like the transposed convolution (bcnn_layers_deconv.c): none of the
 * convolution node's fusions, tables or precision modes sees it.
 *   - dilation == 1 delegates to bcnn_add_convolutional_layer: callers keep the convolution ladder;
 *   - refused with a log line, nothing added to the net: an unknown source, num < 1, size < 1, stride < 1, pad < 0,
 *     dilation < 1, groups < 1 or not dividing both channel counts, a non-positive output extent, PReLU and the
 *     activations that need the layer's input.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_dilated_conv_layer(bcnn_net *net, int n, int size, int stride, int pad, int dilation,
                                        int num_groups, bcnn_filler_type init, bcnn_activation activation,
                                        const char *src_id, const char *dst_id) {
    if (dilation == 1)
        return bcnn_add_convolutional_layer(net, n, size, stride, pad, num_groups, 0, init, activation, 0, src_id, dst_id);
    int src = 0;
    if (net->num_nodes > 0) {
        src = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER,
                           "Dilated convolution layer: invalid input node name %s\n", src_id);
    } else {
        BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_tensor_size(&net->tensors[0]) > 0, BCNN_INVALID_PARAMETER,
                           "Invalid input size of the network. Hint: use 'bcnn_set_input_shape'\n");
    }
    BCNN_CHECK_AND_LOG(net->log_ctx, activation != BCNN_ACT_PRELU, BCNN_INVALID_PARAMETER,
                       "Dilated convolution layer %s: PReLU is not supported\n", dst_id);
    BCNN_REFUSE_INPUT_ACTIVATION(net, activation, "Dilated convolution");
    BCNN_CHECK_AND_LOG(net->log_ctx, n > 0 && size >= 1 && stride >= 1 && pad >= 0 && dilation >= 1,
                       BCNN_INVALID_PARAMETER,
                       "Dilated convolution layer %s: invalid filters %d / size %d / stride %d / pad %d / dilation %d\n",
                       dst_id, n, size, stride, pad, dilation);
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, num_groups > 0 && s.c % num_groups == 0 && n % num_groups == 0,
                       BCNN_INVALID_PARAMETER,
                       "Dilated convolution layer %s: %d groups have to divide %d input and %d output channels\n", dst_id,
                       num_groups, s.c, n);
    const long long eh = (long long)s.h + 2LL * pad - (long long)dilation * (size - 1) - 1;
    const long long ew = (long long)s.w + 2LL * pad - (long long)dilation * (size - 1) - 1;
    BCNN_CHECK_AND_LOG(net->log_ctx, eh >= 0 && ew >= 0, BCNN_INVALID_PARAMETER,
                       "Dilated convolution layer %s: a %d x %d kernel at dilation %d does not fit %d x %d inputs with "
                       "pad %d\n", dst_id, size, size, dilation, s.w, s.h, pad);
    const int oh = (int)(eh / stride) + 1, ow = (int)(ew / stride) + 1, cg = s.c / num_groups;

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    char name[256];
    snprintf(name, sizeof(name), "%s_w", src_id);
    bcnn_tensor weights = {0};
    bcnn_tensor_create(&weights, n, cg, size, size, 1, name, net->mode);
    bcnn_tensor_filler wf = {.range = size * size * cg, .type = init};
    bcnn_tensor_fill(&weights, wf);
    BCNN_CHECK_STATUS(bcnn_net_add_tensor(net, weights));
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, net->num_tensors - 1));
    bcnn_net_register_param(net, net->num_tensors - 1);
    snprintf(name, sizeof(name), "%s_b", src_id);
    bcnn_tensor biases = {0};
    bcnn_tensor_create(&biases, 1, 1, 1, n, 1, name, net->mode);
    BCNN_CHECK_STATUS(bcnn_net_add_tensor(net, biases));
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, net->num_tensors - 1));
    bcnn_net_register_param(net, net->num_tensors - 1);
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, n, oh, ow, dst_id));

    node.type = BCNN_LAYER_DILATED_CONV2D;
    node.param_size = sizeof(bcnn_dilated_conv_param);
    bcnn_dilated_conv_param *param = (bcnn_dilated_conv_param *)calloc(1, node.param_size);
    node.param = param;
    param->activation = activation;
    param->num = n; param->size = size; param->stride = stride; param->pad = pad;
    param->dilation = dilation; param->num_groups = num_groups;
    node.forward = bcnn_forward_dilated_conv_layer;
    node.backward = bcnn_backward_dilated_conv_layer;
    node.update = bcnn_update_dilated_conv_layer;
    node.release_param = bcnn_release_param_dilated_conv_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx,
              "[DilatedConvolutional] input_shape= %dx%dx%d nb_filters= %d kernel_size= %d stride= %d padding= %d "
              "dilation= %d groups= %d output_shape= %dx%dx%d\n",
              s.w, s.h, s.c, n, size, stride, pad, dilation, num_groups, ow, oh, n);
    return BCNN_SUCCESS;
}

void bcnn_forward_dilated_conv_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_dilated_conv_param *p = (const bcnn_dilated_conv_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    bcnn_hip_dilated_conv_forward(x->data_gpu, w->data_gpu, b->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w, p->num,
                                  p->size, p->stride, p->pad, p->dilation, p->num_groups, (int)p->activation);
}

void bcnn_backward_dilated_conv_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_dilated_conv_param *p = (bcnn_dilated_conv_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    const size_t need = bcnn_hip_dilated_conv_workspace_size(x->n, x->c, x->h, x->w, p->num, p->size, p->stride, p->pad,
                                                             p->dilation, p->num_groups);
    if (p->workspace_size < need) { /* the node's own: a convolution's weight gradient may still use the net's on the
                                     * side stream (bcnn_hip_conv_side_stream_mode) */
        bcnn_hip_free(p->conv_workspace_gpu);
        p->conv_workspace_gpu = bcnn_hip_malloc_f32(need);
        p->workspace_size = need;
    }
    bcnn_hip_dilated_conv_backward(x->data_gpu, w->data_gpu, y->data_gpu, y->grad_data_gpu,
                                   x->grad_data_gpu /* NULL for the net input: no dX */, w->grad_data_gpu,
                                   b->grad_data_gpu, x->n, x->c, x->h, x->w, p->num, p->size, p->stride, p->pad,
                                   p->dilation, p->num_groups, (int)p->activation, p->conv_workspace_gpu,
                                   p->workspace_size);
}

void bcnn_update_dilated_conv_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_dilated_conv_param *p = (bcnn_dilated_conv_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_dilated_conv_layer(bcnn_node *node) {
    bcnn_dilated_conv_param *p = (bcnn_dilated_conv_param *)node->param;
    bcnn_hip_free(p->conv_workspace_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
