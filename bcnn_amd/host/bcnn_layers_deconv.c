/*
 * bcnn_layers_deconv.c -- the transposed-convolution (deconvolution) node: builder, node workers, update and release.
 * One whole-batch call into the C-ABI per direction (bcnn_hip_deconv_forward / _backward, deconv.hip).
 *
 * Reference behaviour: bcnn_deconv_layer.c:40-147 (builder: tensor names "<src>_w", "<src>_b", weights
 * [c_in][num][size][size] drawn by the filler with range size * size * c_in), :150-246 (workers), :322-371 (update).
 * Deliberate deviations:
 *   - pad > 0 computes the transposed convolution the output shape describes (the full s (h - 1) + size result cropped
 *     by pad on each side); the reference reads its col2im / im2col workspace with the wrong extent there;
 *   - refused with a log line, nothing added to the net: PReLU (the reference passes NULL slopes and crashes),
 *     size < 1, stride < 1, pad < 0 and a non-positive output extent.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_deconvolutional_layer(bcnn_net *net, int n, int size, int stride, int pad, bcnn_filler_type init,
                                           bcnn_activation activation, const char *src_id, const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER,
                           "Deconvolution layer: invalid input node name %s\n", src_id);
    } else {
        BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_tensor_size(&net->tensors[0]) > 0, BCNN_INVALID_PARAMETER,
                           "Invalid input size of the network. Hint: use 'bcnn_set_input_shape'\n");
    }
    BCNN_CHECK_AND_LOG(net->log_ctx, activation != BCNN_ACT_PRELU, BCNN_INVALID_PARAMETER,
                       "Deconvolution layer %s: PReLU is not supported\n", dst_id);
    BCNN_REFUSE_INPUT_ACTIVATION(net, activation, "Deconvolution");
    BCNN_CHECK_AND_LOG(net->log_ctx, n > 0 && size >= 1 && stride >= 1 && pad >= 0, BCNN_INVALID_PARAMETER,
                       "Deconvolution layer %s: invalid filters %d / size %d / stride %d / pad %d\n", dst_id, n, size,
                       stride, pad);
    const bcnn_tensor s = net->tensors[src];
    const int oh = stride * (s.h - 1) + size - 2 * pad, ow = stride * (s.w - 1) + size - 2 * pad;
    BCNN_CHECK_AND_LOG(net->log_ctx, oh > 0 && ow > 0, BCNN_INVALID_PARAMETER,
                       "Deconvolution layer %s: output extent %d x %d from %d x %d inputs\n", dst_id, ow, oh, s.w, s.h);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    char name[256];
    snprintf(name, sizeof(name), "%s_w", src_id);
    bcnn_tensor weights = {0};
    bcnn_tensor_create(&weights, 1, 1, 1, s.c * n * size * size, 1, name, net->mode);
    bcnn_tensor_filler wf = {.range = size * size * s.c, .type = init};
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

    node.type = BCNN_LAYER_TRANSPOSE_CONV2D;
    node.param_size = sizeof(bcnn_deconv_param);
    bcnn_deconv_param *param = (bcnn_deconv_param *)calloc(1, node.param_size);
    node.param = param;
    param->activation = activation;
    param->num = n; param->size = size; param->stride = stride; param->pad = pad;
    node.forward = bcnn_forward_deconv_layer;
    node.backward = bcnn_backward_deconv_layer;
    node.update = bcnn_update_deconv_layer;
    node.release_param = bcnn_release_param_deconv_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx,
              "[Deconvolutional] input_shape= %dx%dx%d nb_filters= %d kernel_size= %d stride= %d output_shape= %dx%dx%d\n",
              s.w, s.h, s.c, n, size, stride, ow, oh, n);
    return BCNN_SUCCESS;
}

void bcnn_forward_deconv_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_deconv_param *p = (const bcnn_deconv_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    bcnn_hip_deconv_forward(x->data_gpu, w->data_gpu, b->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w, p->num, p->size,
                            p->stride, p->pad, (int)p->activation);
}

void bcnn_backward_deconv_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_deconv_param *p = (bcnn_deconv_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *w = &net->tensors[node->src[1]];
    bcnn_tensor *b = &net->tensors[node->src[2]], *y = &net->tensors[node->dst[0]];
    const size_t need =
        bcnn_hip_deconv_workspace_size(x->n, x->c, x->h, x->w, p->num, p->size, p->stride, p->pad);
    if (p->workspace_size < need) { /* the node's own: a convolution's weight gradient may still use the net's on the
                                     * side stream (bcnn_hip_conv_side_stream_mode) */
        bcnn_hip_free(p->conv_workspace_gpu);
        p->conv_workspace_gpu = bcnn_hip_malloc_f32(need);
        p->workspace_size = need;
    }
    bcnn_hip_deconv_backward(x->data_gpu, w->data_gpu, y->data_gpu, y->grad_data_gpu,
                             x->grad_data_gpu /* NULL for the net input: no dX */, w->grad_data_gpu, b->grad_data_gpu,
                             x->n, x->c, x->h, x->w, p->num, p->size, p->stride, p->pad, (int)p->activation,
                             p->conv_workspace_gpu, p->workspace_size);
}

void bcnn_update_deconv_layer(bcnn_net *net, bcnn_node *node) { /* reference bcnn_deconv_layer.c:322-371 */
    bcnn_deconv_param *p = (bcnn_deconv_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[1]], &net->tensors[node->src[2]], &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_deconv_layer(bcnn_node *node) {
    bcnn_deconv_param *p = (bcnn_deconv_param *)node->param;
    bcnn_hip_free(p->conv_workspace_gpu);
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
