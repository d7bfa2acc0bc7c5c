/*
 * bcnn_layers_attention.c -- the multi-head attention node: dst = V softmax(scale Q^T K)^T over the positions of three feature
 * maps, per image and head. Builder, node workers and release; no parameters, no update. One whole-batch call into the C-ABI
 * per direction (attention.hip).
 *
 * No reference counterpart (bcnn_load_net of the reference ends such a cfg with "Unknown Layer").
 *   - src[0] = q [N][Cqk][Hq][Wq], src[1] = k [N][Cqk][Hk][Wk], src[2] = v [N][Cv][Hk][Wk]; dst [N][Cv][Hq][Wq]. The three
 *     may be one tensor or alias in pairs;
 *   - the builder checks the names and the shapes before it adds anything (INTEGRATION.md lists the refusals);
 *   - a net built in TRAIN / VALID mode keeps the log-sum-exp of every (image, head, query) of the last forward (one
 *     [N][heads][Lq] buffer, followed by bcnn_resize_net through its capacity); the backward recomputes the softmax from it;
 *   - the backward assigns a source gradient when this node is its sole writer (bcnn_core.c: mark_dead_grad_fills) and adds
 *     otherwise -- always when two of q, k, v are one tensor; a source without a gradient (the net input) is skipped;
 *   - the backward reads the node's own output (Dl = sum_r dO O). A node that works in place on dst (an activation, a
 *     dropout) rewrites it between forward and backward: in such a net the forward keeps a copy of what it wrote in a buffer
 *     of the node, and the backward reads that.
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

bcnn_status bcnn_add_attention_layer(bcnn_net *net, int num_heads, float scale, const char *q_id, const char *k_id,
                                     const char *v_id, const char *dst_id) {
    const char *ids[3] = {q_id, k_id, v_id};
    int src[3];
    for (int i = 0; i < 3; ++i) {
        src[i] = ids[i] ? bcnn_net_find_tensor(net, ids[i]) : -1;
        BCNN_CHECK_AND_LOG(net->log_ctx, src[i] >= 0, BCNN_INVALID_PARAMETER, "Attention layer: invalid input node name %s\n",
                           ids[i] ? ids[i] : "(null)");
    }
    const bcnn_tensor q = net->tensors[src[0]], k = net->tensors[src[1]], v = net->tensors[src[2]];
    BCNN_CHECK_AND_LOG(net->log_ctx, q.n == k.n && q.n == v.n, BCNN_INVALID_PARAMETER,
                       "Attention layer %s: the batch sizes %d, %d, %d of %s, %s, %s differ\n", dst_id, q.n, k.n, v.n, q_id,
                       k_id, v_id);
    BCNN_CHECK_AND_LOG(net->log_ctx, q.c == k.c, BCNN_INVALID_PARAMETER,
                       "Attention layer %s: %s has %d channels, %s has %d\n", dst_id, q_id, q.c, k_id, k.c);
    BCNN_CHECK_AND_LOG(net->log_ctx, k.h * k.w == v.h * v.w, BCNN_INVALID_PARAMETER,
                       "Attention layer %s: %s has %d x %d positions, %s has %d x %d\n", dst_id, k_id, k.w, k.h, v_id, v.w,
                       v.h);
    BCNN_CHECK_AND_LOG(net->log_ctx, num_heads > 0, BCNN_INVALID_PARAMETER,
                       "Attention layer %s: the number of heads %d must be positive\n", dst_id, num_heads);
    BCNN_CHECK_AND_LOG(net->log_ctx, q.c % num_heads == 0 && v.c % num_heads == 0, BCNN_INVALID_PARAMETER,
                       "Attention layer %s: %d heads do not divide %d and %d channels\n", dst_id, num_heads, q.c, v.c);
    BCNN_CHECK_AND_LOG(net->log_ctx, bcnn_attention_fits(&q, &k, &v), BCNN_INVALID_PARAMETER,
                       "Attention layer %s: q, k, v or the output would hold 2^31 elements or more\n", dst_id);
    BCNN_CHECK_AND_LOG(net->log_ctx, q.c / num_heads <= BCNN_ATTENTION_MAX_HEAD_DIM && v.c / num_heads <= BCNN_ATTENTION_MAX_HEAD_DIM,
                       BCNN_INVALID_PARAMETER, "Attention layer %s: a head of %d / %d channels is above the limit of %d\n",
                       dst_id, q.c / num_heads, v.c / num_heads, BCNN_ATTENTION_MAX_HEAD_DIM);

    bcnn_node node = {0};
    for (int i = 0; i < 3; ++i) BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src[i]));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, q.n, v.c, q.h, q.w, dst_id));
    node.type = BCNN_LAYER_ATTENTION;
    node.param_size = sizeof(bcnn_attention_param);
    bcnn_attention_param *param = (bcnn_attention_param *)calloc(1, node.param_size);
    node.param = param;
    param->num_heads = num_heads;
    param->scale = scale;
    param->out_channels = v.c;
    if (net->mode != BCNN_MODE_PREDICT) { /* the backward's input; a PREDICT net has no backward */
        param->lse_capacity = bcnn_hip_attention_lse_size(q.n, num_heads, q.h * q.w);
        param->lse_gpu = bcnn_hip_malloc_f32(param->lse_capacity);
    }
    node.forward = bcnn_forward_attention_layer;
    node.backward = bcnn_backward_attention_layer;
    node.release_param = bcnn_release_param_attention_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Attention] %-8s %-8s %-8s (%4d x%4d x%4d) -> %-8s heads= %d scale= %g\n", q_id, k_id, v_id, q.w,
              q.h, q.c, dst_id, num_heads, scale);
    return BCNN_SUCCESS;
}

int bcnn_attention_fits(const bcnn_tensor *q, const bcnn_tensor *k, const bcnn_tensor *v) {
    const long long lq = (long long)q->h * q->w, lk = (long long)k->h * k->w, limit = 0x7fffffffLL;
    return lk == (long long)v->h * v->w && (long long)q->n * q->c * lq < limit && (long long)k->n * k->c * lk < limit &&
           (long long)v->n * v->c * lk < limit && (long long)q->n * v->c * lq < limit;
}

/* some other node writes this node's dst too: an in-place activation or dropout behind it */
static int dst_rewritten(const bcnn_net *net, const bcnn_node *node) {
    for (int i = 0; i < net->num_nodes; ++i) {
        const bcnn_node *nd = &net->nodes[i];
        if (nd == node) continue;
        for (int k = 0; k < nd->num_dst; ++k)
            if (nd->dst[k] == node->dst[0]) return 1;
    }
    return 0;
}

void bcnn_forward_attention_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_attention_param *p = (bcnn_attention_param *)node->param;
    const bcnn_tensor *q = &net->tensors[node->src[0]], *k = &net->tensors[node->src[1]], *v = &net->tensors[node->src[2]];
    bcnn_tensor *o = &net->tensors[node->dst[0]];
    const size_t rows = bcnn_hip_attention_lse_size(q->n, p->num_heads, q->h * q->w);
    /* PREDICT stores no log-sum-exp; nor does a net whose buffer a resize without need_realloc could not follow */
    float *lse = (net->mode != BCNN_MODE_PREDICT && p->lse_gpu && rows <= p->lse_capacity) ? p->lse_gpu : NULL;
    /* bf16 inference (never a TRAIN pass): the same call on the bf16 matrix cores, whatever the shape */
    (bcnn_bf16_inference(net) ? bcnn_hip_attention_forward_bf16 : bcnn_hip_attention_forward)(
        q->data_gpu, k->data_gpu, v->data_gpu, o->data_gpu, lse, q->n, p->num_heads, q->c / p->num_heads,
        v->c / p->num_heads, q->h * q->w, k->h * k->w, p->scale);
    p->out_kept = 0;
    if (lse && dst_rewritten(net, node)) { /* the backward's O, out of the in-place node's reach */
        const size_t elems = (size_t)bcnn_tensor_size(o);
        if (!p->out_gpu) { /* from here on bcnn_resize_net follows it like the log-sum-exp */
            p->out_gpu = bcnn_hip_malloc_f32(elems);
            p->out_capacity = p->out_gpu ? elems : 0;
        }
        if (elems <= p->out_capacity) {
            bcnn_hip_memcpy_d2d(p->out_gpu, o->data_gpu, elems * sizeof(float));
            p->out_kept = 1;
        }
    }
}

void bcnn_backward_attention_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_attention_param *p = (const bcnn_attention_param *)node->param;
    bcnn_tensor *q = &net->tensors[node->src[0]], *k = &net->tensors[node->src[1]], *v = &net->tensors[node->src[2]];
    const bcnn_tensor *o = &net->tensors[node->dst[0]];
    const size_t rows = bcnn_hip_attention_lse_size(q->n, p->num_heads, q->h * q->w);
    if (!o->grad_data_gpu) return; /* PREDICT-built */
    if (!p->lse_gpu || rows > p->lse_capacity) {
        /* no forward kept the log-sum-exp; said aloud, because under the sole-writer mark a source gradient now holds nothing */
        BCNN_WARNING(net->log_ctx, "Attention layer: no log-sum-exp of %zu rows kept (capacity %zu floats), backward skipped\n",
                     rows, p->lse_capacity);
        return;
    }
    if (!p->out_kept && dst_rewritten(net, node)) { /* (a resize without need_realloc past the copy's capacity) */
        BCNN_WARNING(net->log_ctx, "Attention layer: the output was rewritten in place and no copy of it kept, backward skipped\n");
        return;
    }
    /* a source may have no gradient (the net input): that third is skipped */
    bcnn_hip_attention_backward(q->data_gpu, k->data_gpu, v->data_gpu, p->out_kept ? p->out_gpu : o->data_gpu, p->lse_gpu, o->grad_data_gpu,
                                q->grad_data_gpu, k->grad_data_gpu, v->grad_data_gpu, q->n, p->num_heads, q->c / p->num_heads,
                                v->c / p->num_heads, q->h * q->w, k->h * k->w, p->scale,
                                bcnn_grad_sole_writer(net, node->src[0]), bcnn_grad_sole_writer(net, node->src[1]),
                                bcnn_grad_sole_writer(net, node->src[2]));
}

void bcnn_release_param_attention_layer(bcnn_node *node) {
    bcnn_hip_free(((bcnn_attention_param *)node->param)->lse_gpu);
    bcnn_hip_free(((bcnn_attention_param *)node->param)->out_gpu);
}
