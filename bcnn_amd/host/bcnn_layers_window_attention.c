/*
 * bcnn_layers_window_attention.c -- the window-attention node: the attention of Swin blocks. The map is rolled by `shift`, cut
 * into window x window windows, and every window attends to itself per image and head, with a learned relative position bias
 * and, under a shift, Swin's region mask. Builder, node workers, update and release; one whole-batch call into the C-ABI per
 * direction (attention_window.hip). It stands beside the attention node (bcnn_layers_attention.c), which attends globally.
 *
 * No reference counterpart.
 *   - src[0] = q [N][Cqk][H][W], src[1] = k [N][Cqk][H][W], src[2] = v [N][Cv][H][W]; dst [N][Cv][H][W]. The three may be one
 *     tensor or alias in pairs. With rel_bias, src[3] = <dst>_relbias [heads][(2 window - 1)^2], a registered parameter;
 *   - the builder checks the names and the shapes before it adds anything (INTEGRATION.md lists the refusals);
 *     bcnn_resize_net asks the same shape rules of the new extents (bcnn_window_attention_fits);
 *   - nothing is kept between forward and backward: the backward recomputes the softmax from q, k and the table and does not
 *     read dst, so an in-place node behind this one needs no copy;
 *   - the backward assigns a source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and adds
 *     otherwise -- always when two of q, k, v are one tensor; a source without a gradient (the net input) is skipped. The
 *     table's gradient accumulates like every parameter gradient;
 *   - the table trains by the weights' rule.
 */
#include <stdio.h>
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

int bcnn_window_attention_fits(const bcnn_window_attention_param *p, const bcnn_tensor *q, const bcnn_tensor *k,
                               const bcnn_tensor *v, char *why, size_t why_size) {
    const int heads = p->num_heads;
    why[0] = '\0';
    if (q->n != k->n || q->n != v->n)
        snprintf(why, why_size, "the batch sizes %d, %d, %d differ", q->n, k->n, v->n);
    else if (q->h != k->h || q->w != k->w || q->h != v->h || q->w != v->w)
        snprintf(why, why_size, "q, k, v have different extents (%d x %d, %d x %d, %d x %d)", q->w, q->h, k->w, k->h, v->w, v->h);
    else if (q->c != k->c)
        snprintf(why, why_size, "q has %d channels, k has %d", q->c, k->c);
    else if (heads < 1 || q->c % heads != 0 || v->c % heads != 0)
        snprintf(why, why_size, "%d heads do not divide %d and %d channels", heads, q->c, v->c);
    else {
        switch (bcnn_hip_window_attention_check(q->n, heads, q->c / heads, v->c / heads, q->h, q->w, p->window, p->shift)) {
            case 0: return 1;
            case BCNN_HIP_WINDOW_ATTN_BAD_WINDOW:
                snprintf(why, why_size, "a window of %d is outside 1 .. 8 (64 positions)", p->window);
                break;
            case BCNN_HIP_WINDOW_ATTN_RAGGED_MAP:
                snprintf(why, why_size, "a %d x %d map is not whole windows of %d", q->w, q->h, p->window);
                break;
            case BCNN_HIP_WINDOW_ATTN_BAD_SHIFT:
                snprintf(why, why_size, "a shift of %d is outside [0, %d)", p->shift, p->window);
                break;
            case BCNN_HIP_WINDOW_ATTN_BAD_HEAD_DIM:
                snprintf(why, why_size, "a head of %d / %d channels is above the limit of 64", q->c / heads, v->c / heads);
                break;
            case BCNN_HIP_WINDOW_ATTN_TOO_LARGE:
                snprintf(why, why_size, "q, k, v or the output would hold 2^31 elements or more");
                break;
            default: snprintf(why, why_size, "an empty tensor"); break;
        }
    }
    return 0;
}

bcnn_status bcnn_add_window_attention_layer(bcnn_net *net, int num_heads, int window, int shift, int rel_bias, float scale,
                                            const char *q_id, const char *k_id, const char *v_id, const char *dst_id) {
    const char *ids[3] = {q_id, k_id, v_id};
    int src[3];
    for (int i = 0; i < 3; ++i) {
        src[i] = ids[i] ? bcnn_net_find_tensor(net, ids[i]) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src[i] >= 0, BCNN_INVALID_PARAMETER,
                           "Window-attention layer: invalid input node name %s\n", ids[i] ? ids[i] : "(null)");
    }
    const bcnn_tensor q = net->tensors[src[0]], k = net->tensors[src[1]], v = net->tensors[src[2]];
    bcnn_window_attention_param want = {0};
    want.num_heads = num_heads;
    want.window = window;
    want.shift = shift;
    want.rel_bias = rel_bias != 0;
    want.scale = scale;
    want.out_channels = v.c;
    char why[256];
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_window_attention_fits(&want, &q, &k, &v, why, sizeof(why)), BCNN_INVALID_PARAMETER,
                       "Window-attention layer %s: %s\n", dst_id, why);

    bcnn_node node = {0};
    for (int i = 0; i < 3; ++i) BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src[i]));
    if (want.rel_bias) /* zero-filled: the node starts as plain window attention */
        BCNN_CHECK_STATUS(bcnn_node_new_vector_param(net, &node, num_heads * (2 * window - 1) * (2 * window - 1), 1, dst_id,
                                                     "relbias", 0.0f, 1));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, q.n, v.c, q.h, q.w, dst_id));
    node.type = BCNN_LAYER_WINDOW_ATTENTION;
    node.param_size = sizeof(bcnn_window_attention_param);
    bcnn_window_attention_param *param = (bcnn_window_attention_param *)calloc(1, node.param_size);
    *param = want;
    node.param = param;
    node.forward = bcnn_forward_window_attention_layer;
    node.backward = bcnn_backward_window_attention_layer;
    if (want.rel_bias) node.update = bcnn_update_window_attention_layer;
    node.release_param = bcnn_release_param_window_attention_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[WindowAttention] %-8s %-8s %-8s (%4d x%4d x%4d) -> %-8s heads= %d window= %d shift= %d bias= %d\n",
              q_id, k_id, v_id, q.w, q.h, q.c, dst_id, num_heads, window, shift, want.rel_bias);
    return BCNN_SUCCESS;
}

void bcnn_forward_window_attention_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_window_attention_param *p = (const bcnn_window_attention_param *)node->param;
    const bcnn_tensor *q = &net->tensors[node->src[0]], *k = &net->tensors[node->src[1]], *v = &net->tensors[node->src[2]];
    const BcnnWindowAttnFwdArgs a = {q->data_gpu, k->data_gpu, v->data_gpu,
                                     p->rel_bias ? net->tensors[node->src[3]].data_gpu : NULL,
                                     net->tensors[node->dst[0]].data_gpu, q->n, p->num_heads, q->c / p->num_heads,
                                     v->c / p->num_heads, q->h, q->w, p->window, p->shift, p->scale};
    /* bf16 inference (never a TRAIN pass): the same call on the bf16 matrix cores, whatever the shape */
    (bcnn_bf16_inference(net) ? bcnn_hip_window_attention_forward_bf16 : bcnn_hip_window_attention_forward)(&a);
}

void bcnn_backward_window_attention_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_window_attention_param *p = (const bcnn_window_attention_param *)node->param;
    bcnn_tensor *q = &net->tensors[node->src[0]], *k = &net->tensors[node->src[1]], *v = &net->tensors[node->src[2]];
    const bcnn_tensor *o = &net->tensors[node->dst[0]];
    if (!o->grad_data_gpu) return; /* PREDICT-built */
    /* a source may have no gradient (the net input): that part is skipped */
    const BcnnWindowAttnBwdArgs a = {q->data_gpu, k->data_gpu, v->data_gpu,
                                     p->rel_bias ? net->tensors[node->src[3]].data_gpu : NULL, o->grad_data_gpu,
                                     q->grad_data_gpu, k->grad_data_gpu, v->grad_data_gpu,
                                     p->rel_bias ? net->tensors[node->src[3]].grad_data_gpu : NULL, q->n, p->num_heads,
                                     q->c / p->num_heads, v->c / p->num_heads, q->h, q->w, p->window, p->shift, p->scale,
                                     bcnn_grad_sole_writer(net, node->src[0]), bcnn_grad_sole_writer(net, node->src[1]),
                                     bcnn_grad_sole_writer(net, node->src[2])};
    bcnn_hip_window_attention_backward(&a);
}

void bcnn_update_window_attention_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_window_attention_param *p = (bcnn_window_attention_param *)node->param;
    bcnn_node_optim_step(net, &net->tensors[node->src[3]], NULL, &p->adam_m_gpu, &p->adam_v_gpu);
}

void bcnn_release_param_window_attention_layer(bcnn_node *node) {
    bcnn_window_attention_param *p = (bcnn_window_attention_param *)node->param;
    bcnn_hip_free(p->adam_m_gpu);
    bcnn_hip_free(p->adam_v_gpu);
}
