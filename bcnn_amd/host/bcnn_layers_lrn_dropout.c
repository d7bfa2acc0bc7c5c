/*
 * bcnn_layers_lrn_dropout.c -- the local response normalisation node and the in-place dropout node: builders, node
 * workers and release. One whole-batch call into the C-ABI per direction (lrn_dropout.hip).
 *
 * Reference behaviour: bcnn_lrn_layer.c:35-101 (builder), bcnn_dropout_layer.c:32-126 (builder, workers).
 * Deliberate deviations:
 *   - LRN computes s_c = k + alpha/n sum x^2 over the window [c - (n-1)/2, c + n/2] exactly (the reference's running
 *     sums drop and re-subtract channel n/2, never store k, and its backward overwrites dx from a truncated window);
 *     its backward adds into the source gradient like every other node (assigns when it is the sole writer);
 *   - LRN refuses local_size < 1, local_size >= c and negative alpha / beta / k before it adds anything;
 *   - dropout draws its mask from a counter-based generator keyed by the net's dropout seed, the node index and the
 *     data-parallel rank (bcnn_set_dropout_seed; include/bcnn_hip.h), reproducible from run to run, and refuses
 *     rates outside [0, 1).
 */
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

static bcnn_hip_context *hctx(bcnn_net *net) { return (bcnn_hip_context *)net->hip_ctx; }

bcnn_status bcnn_add_lrn_layer(bcnn_net *net, int local_size, float alpha, float beta, float k, const char *src_id,
                               const char *dst_id) {
    int src = 0;
    if (net->num_nodes > 0) {
        src = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "LRN layer: invalid input node name %s\n",
                           src_id);
    }
    const bcnn_tensor s = net->tensors[src];
    BCNN_CHECK_AND_LOG(net->log_ctx, local_size >= 1 && local_size < s.c, BCNN_INVALID_PARAMETER,
                       "LRN layer %s: local size %d must be at least 1 and inferior to the number of channels %d\n",
                       dst_id, local_size, s.c);
    BCNN_CHECK_AND_LOG(net->log_ctx, alpha >= 0.f && beta >= 0.f && k >= 0.f, BCNN_INVALID_PARAMETER,
                       "LRN layer %s: alpha %g, beta %g and k %g must not be negative\n", dst_id, alpha, beta, k);

    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    node.type = BCNN_LAYER_LRN;
    node.param_size = sizeof(bcnn_lrn_param);
    bcnn_lrn_param *param = (bcnn_lrn_param *)calloc(1, node.param_size);
    node.param = param;
    param->local_size = local_size;
    param->alpha = alpha;
    param->beta = beta;
    param->k = k;
    node.forward = bcnn_forward_lrn_layer;
    node.backward = bcnn_backward_lrn_layer;
    node.release_param = bcnn_release_param_lrn_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[LRNorm] input_shape= %dx%dx%d local_size= %d alpha= %g beta= %g k= %g\n", s.w, s.h, s.c,
              local_size, alpha, beta, k);
    return BCNN_SUCCESS;
}

void bcnn_forward_lrn_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_lrn_param *p = (const bcnn_lrn_param *)node->param;
    const bcnn_tensor *x = &net->tensors[node->src[0]];
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    bcnn_hip_lrn_forward(x->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w, p->local_size, p->alpha, p->beta, p->k);
}

void bcnn_backward_lrn_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_lrn_param *p = (const bcnn_lrn_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!x->grad_data_gpu || !y->grad_data_gpu) return; /* the net input: no dX */
    bcnn_hip_lrn_backward(x->data_gpu, y->grad_data_gpu, x->grad_data_gpu, x->n, x->c, x->h, x->w, p->local_size,
                          p->alpha, p->beta, p->k, bcnn_grad_sole_writer(net, node->src[0]));
}

void bcnn_release_param_lrn_layer(bcnn_node *node) { (void)node; }

/* ---- dropout ------------------------------------------------------------------------------------------------------ */
static uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* the Philox key of dropout node `node` on data-parallel rank `rank` */
uint64_t bcnn_dropout_key(uint64_t seed, int node, int rank) {
    return splitmix64(seed ^ splitmix64(((uint64_t)(uint32_t)rank << 32) | (uint32_t)node));
}

void bcnn_set_dropout_seed(bcnn_net *net, uint64_t seed) {
    if (net && net->hip_ctx) hctx(net)->dropout_seed = seed;
}

bcnn_status bcnn_add_dropout_layer(bcnn_net *net, float rate, const char *src_id) {
    BCNN_CHECK_AND_LOG(net->log_ctx, net->num_nodes >= 1, BCNN_INVALID_PARAMETER,
                       "Dropout layer can't be the first layer of the network\n");
    const int src = bcnn_net_find_tensor(net, src_id);
    BCNN_CHECK_AND_LOG(net->log_ctx, src >= 0, BCNN_INVALID_PARAMETER, "Dropout layer: invalid input node name %s\n",
                       src_id);
    BCNN_CHECK_AND_LOG(net->log_ctx, rate >= 0.f && rate < 1.f, BCNN_INVALID_PARAMETER,
                       "Dropout layer %s: rate %g must lie in [0, 1)\n", src_id, rate);
    bcnn_node node = {0};
    BCNN_CHECK_STATUS(bcnn_node_add_input(net, &node, src));
    BCNN_CHECK_STATUS(bcnn_node_add_output(net, &node, src));
    node.type = BCNN_LAYER_DROPOUT;
    node.param_size = sizeof(bcnn_dropout_param);
    bcnn_dropout_param *param = (bcnn_dropout_param *)calloc(1, node.param_size);
    node.param = param;
    param->dropout_rate = rate;
    param->scale = 1.0f / (1.0f - rate);
    node.forward = bcnn_forward_dropout_layer;
    node.backward = bcnn_backward_dropout_layer;
    node.release_param = bcnn_release_param_dropout_layer;
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    const bcnn_tensor *t = &net->tensors[src];
    BCNN_INFO(net->log_ctx, "[Dropout] %s (%dx%dx%d) in place rate= %f\n", t->name, t->w, t->h, t->c, rate);
    return BCNN_SUCCESS;
}

void bcnn_forward_dropout_layer(bcnn_net *net, bcnn_node *node) {
    if (net->mode != BCNN_MODE_TRAIN) return; /* VALID / PREDICT: identity (bcnn_dropout_layer.c:78-80) */
    bcnn_dropout_param *p = (bcnn_dropout_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    p->last_key = bcnn_dropout_key(hctx(net)->dropout_seed, (int)(node - net->nodes), hctx(net)->dp_rank);
    p->last_step = p->step++;
    p->has_mask = 1;
    bcnn_hip_dropout_forward(x->data_gpu, (size_t)bcnn_tensor_size(x), p->dropout_rate, p->last_key, p->last_step);
}

void bcnn_backward_dropout_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_dropout_param *p = (const bcnn_dropout_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]];
    if (!x->grad_data_gpu || !p->has_mask) return;
    bcnn_hip_dropout_backward(x->grad_data_gpu, (size_t)bcnn_tensor_size(x), p->dropout_rate, p->last_key,
                              p->last_step);
}

void bcnn_release_param_dropout_layer(bcnn_node *node) { (void)node; }
