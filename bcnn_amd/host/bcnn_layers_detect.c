/*
 * bcnn_layers_detect.c -- the nodes a Darknet detector graph (yolov3-tiny) needs besides the hot path: concat
 * ([route]), nearest-neighbour upsample, the YOLOv3 head, and bcnn_yolo_get_detections.
 *
 * Reference behaviour: bcnn_concat_layer.c:33-146, bcnn_upsample_layer.c:28-147, bcnn_yolo.c:15-107, 207-215, 417-468,
 * 470-639. Deliberate deviations:
 *   - detector training is opt-in (bcnn_set_detector_training, INI train_detector=1): without the switch
 *     bcnn_add_yolo_layer on a TRAIN net and bcnn_set_mode(TRAIN) on a net holding a head are refused, as before the
 *     loss was built; with it the head's TRAIN forward (bcnn_yolo.c:250-415) runs on the device, the per-step
 *     statistics line is not printed (bcnn_yolo_get_train_stats reads them on demand), and a truth whose cell or class
 *     lies outside the head is skipped where the reference writes out of bounds;
 *   - bcnn_yolo_get_detections prints nothing per box and sizes `prob` from the classes of the YOLO nodes (the
 *     reference reads them from the LAST node of the net, right only when that node is a head);
 *   - a head whose mask names an anchor outside [0, total) is refused (the reference reads past its anchor table).
 */
#include <math.h>
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

/* ================================================================================================
 * concat: dst = [src_0 | src_1 | ...] along the channels, image by image. A single source is a copy (Darknet
 * `[route] layers=-4`). Backward src_grad += slice of dst_grad for every source with a gradient; the sources'
 * gradient fills stay live (mark_dead_grad_fills: a concat consumer is never a sole writer).
 * ============================================================================================== */
bcnn_status bcnn_add_concat_layer(bcnn_net *net, int num_src, char *const *src_ids, const char *dst_id) {
    BCNN_CHECK_AND_LOG(net->log_ctx, net->num_nodes >= 1, BCNN_INVALID_PARAMETER,
                       "Concat layer can't be the first layer of the network\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, num_src >= 1 && src_ids && dst_id, BCNN_INVALID_PARAMETER,
                       "Concat layer: needs at least one source and a destination\n");
    bcnn_node node = {0};
    int out_c = 0;
    for (int i = 0; i < num_src; ++i) {
        const int idx = bcnn_get_tensor_index_by_name(net, src_ids[i]);
        if (idx < 0) {
            free(node.src);
            BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER, "Concat layer: invalid input node name %s\n", src_ids[i]);
        }
        bcnn_node_add_input(net, &node, idx);
        const bcnn_tensor *s0 = &net->tensors[node.src[0]], *si = &net->tensors[idx];
        if (si->w != s0->w || si->h != s0->h) {
            free(node.src);
            BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER,
                       "Concat layer: inconsistent spatial sizes between node %s (%dx%d) and node %s (%dx%d)\n",
                       src_ids[0], s0->w, s0->h, src_ids[i], si->w, si->h);
        }
        out_c += si->c;
    }
    const bcnn_tensor s = net->tensors[node.src[0]];
    node.type = BCNN_LAYER_CONCAT;
    node.forward = bcnn_forward_concat_layer;
    node.backward = bcnn_backward_concat_layer;
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, out_c, s.h, s.w, dst_id));
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Concat] %d sources -> %-8s (%4d x%4d x%4d)\n", num_src, dst_id, s.w, s.h, out_c);
    return BCNN_SUCCESS;
}

void bcnn_forward_concat_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    const float **src = (const float **)malloc((size_t)node->num_src * sizeof(*src));
    int *size = (int *)malloc((size_t)node->num_src * sizeof(int));
    for (int i = 0; i < node->num_src; ++i) {
        const bcnn_tensor *x = &net->tensors[node->src[i]];
        src[i] = x->data_gpu;
        size[i] = bcnn_tensor_size3d(x);
    }
    bcnn_hip_concat_forward(node->num_src, src, size, y->data_gpu, bcnn_tensor_size3d(y), y->n);
    free(src);
    free(size);
}

void bcnn_backward_concat_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_tensor *y = &net->tensors[node->dst[0]];
    if (!y->grad_data_gpu) return;
    float **grad = (float **)malloc((size_t)node->num_src * sizeof(*grad));
    int *size = (int *)malloc((size_t)node->num_src * sizeof(int));
    for (int i = 0; i < node->num_src; ++i) {
        const bcnn_tensor *x = &net->tensors[node->src[i]];
        grad[i] = x->grad_data_gpu; /* NULL (the net input, PREDICT nets): skipped */
        size[i] = bcnn_tensor_size3d(x);
    }
    bcnn_hip_concat_backward(node->num_src, grad, size, y->grad_data_gpu, bcnn_tensor_size3d(y), y->n);
    free(grad);
    free(size);
}

/* ================================================================================================
 * upsample: nearest neighbour by an integer factor
 * ============================================================================================== */
bcnn_status bcnn_add_upsample_layer(bcnn_net *net, int size, const char *src_id, const char *dst_id) {
    BCNN_CHECK_AND_LOG(net->log_ctx, size >= 1, BCNN_INVALID_PARAMETER, "Upsample layer: invalid factor %d\n", size);
    bcnn_node node = {0};
    if (net->num_nodes > 0) {
        const int idx = bcnn_net_find_tensor(net, src_id);
        BCNN_CHECK_AND_LOG(net->log_ctx, idx >= 0, BCNN_INVALID_PARAMETER, "Upsample layer: invalid input node name %s\n",
                           src_id);
        bcnn_node_add_input(net, &node, idx);
    } else {
        bcnn_node_add_input(net, &node, 0);
    }
    const bcnn_tensor s = net->tensors[node.src[0]];
    node.type = BCNN_LAYER_UPSAMPLE;
    node.param_size = sizeof(bcnn_upsample_param);
    bcnn_upsample_param *param = (bcnn_upsample_param *)calloc(1, node.param_size);
    node.param = param;
    param->size = size;
    node.forward = bcnn_forward_upsample_layer;
    node.backward = bcnn_backward_upsample_layer;
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h * size, s.w * size, dst_id));
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Upsample] %-8s (%4d x%4d x%4d) -> %-8s (%4d x%4d x%4d)\n", s.name, s.w, s.h, s.c, dst_id,
              s.w * size, s.h * size, s.c);
    return BCNN_SUCCESS;
}

void bcnn_forward_upsample_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_upsample_param *p = (const bcnn_upsample_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *y = &net->tensors[node->dst[0]];
    bcnn_hip_upsample_forward(x->data_gpu, y->data_gpu, x->n, x->c, x->h, x->w, p->size);
}

void bcnn_backward_upsample_layer(bcnn_net *net, bcnn_node *node) {
    const bcnn_upsample_param *p = (const bcnn_upsample_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *y = &net->tensors[node->dst[0]];
    if (x->grad_data_gpu && y->grad_data_gpu)
        bcnn_hip_upsample_backward(x->grad_data_gpu, y->grad_data_gpu, x->n, x->c, x->h, x->w, p->size);
}

/* ================================================================================================
 * YOLOv3 head (inference): dst = src with the logistic on x, y, objectness and the class scores
 * ============================================================================================== */
bcnn_status bcnn_add_yolo_layer(bcnn_net *net, int num_boxes_per_cell, int classes, int coords, int total, int *mask,
                                float *anchors, const char *src_id, const char *dst_id) {
    BCNN_CHECK_AND_LOG(net->log_ctx, net->num_nodes >= 1, BCNN_INVALID_PARAMETER,
                       "Yolo layer can't be the first layer of the network\n");
    const int train_detector = bcnn_get_detector_training(net);
    BCNN_CHECK_AND_LOG(net->log_ctx, net->mode != BCNN_MODE_TRAIN || train_detector, BCNN_INVALID_PARAMETER,
                       "Yolo layer: the TRAIN-mode loss of the YOLO head is not built (PREDICT / VALID nets only)\n");
    const int idx = bcnn_net_find_tensor(net, src_id);
    BCNN_CHECK_AND_LOG(net->log_ctx, idx >= 0, BCNN_INVALID_PARAMETER, "Yolo layer: invalid input node name %s\n", src_id);
    const bcnn_tensor s = net->tensors[idx];
    BCNN_CHECK_AND_LOG(net->log_ctx, num_boxes_per_cell * (classes + coords + 1) == s.c, BCNN_INVALID_PARAMETER,
                       "Yolo layer: inconsistent number of channels %d\n", num_boxes_per_cell * (classes + coords + 1));
    for (int i = 0; mask && i < num_boxes_per_cell; ++i)
        BCNN_CHECK_AND_LOG(net->log_ctx, mask[i] >= 0 && mask[i] < total, BCNN_INVALID_PARAMETER,
                           "Yolo layer: mask entry %d names anchor %d of %d\n", i, mask[i], total);
    if (train_detector) { /* what the device loss takes (include/bcnn_hip.h), and the label tensor every head shares */
        BCNN_CHECK_AND_LOG(net->log_ctx,
                           coords == 4 && num_boxes_per_cell >= 1 && num_boxes_per_cell <= BCNN_HIP_YOLO_MAX_ANCHORS &&
                               total >= 1 && total <= BCNN_HIP_YOLO_TRAIN_MAX_TOTAL && mask,
                           BCNN_INVALID_PARAMETER,
                           "Yolo layer: detector training needs coords = 4, a mask of 1 to %d anchors and 1 to %d anchors in all\n",
                           BCNN_HIP_YOLO_MAX_ANCHORS, BCNN_HIP_YOLO_TRAIN_MAX_TOTAL);
        bcnn_tensor *label = &net->tensors[1];
        if (label->data == NULL) { /* reference bcnn_yolo.c:68-73 (there: outside PREDICT mode only) */
            bcnn_tensor_set_shape(label, s.n, 1, 1, BCNN_DETECTION_MAX_BOXES * 5, 0);
            BCNN_CHECK_STATUS(bcnn_tensor_allocate(label, net->mode));
        }
        BCNN_CHECK_AND_LOG(net->log_ctx, label->n >= s.n && bcnn_tensor_size3d(label) >= BCNN_DETECTION_MAX_BOXES * 5,
                           BCNN_INVALID_PARAMETER, "Yolo layer: the label tensor holds %d x %d floats, a detector needs %d x %d\n",
                           label->n, bcnn_tensor_size3d(label), s.n, BCNN_DETECTION_MAX_BOXES * 5);
    }
    bcnn_node node = {0};
    bcnn_node_add_input(net, &node, idx);
    node.type = BCNN_LAYER_YOLOV3;
    node.param_size = sizeof(bcnn_yolo_param);
    bcnn_yolo_param *param = (bcnn_yolo_param *)calloc(1, node.param_size);
    node.param = param;
    param->num = num_boxes_per_cell;
    param->classes = classes;
    param->coords = coords;
    param->total = total;
    param->mask = (int *)calloc((size_t)(num_boxes_per_cell > 0 ? num_boxes_per_cell : 1), sizeof(int));
    for (int i = 0; i < num_boxes_per_cell; ++i) param->mask[i] = mask ? mask[i] : i;
    param->biases = (float *)malloc((size_t)(total > 0 ? 2 * total : 1) * sizeof(float));
    for (int i = 0; i < 2 * total; ++i) param->biases[i] = 0.5f;
    if (anchors) memcpy(param->biases, anchors, (size_t)(2 * total) * sizeof(float));
    param->cost = (float *)calloc(1, sizeof(float));
    if (train_detector) {
        param->max_boxes = BCNN_DETECTION_MAX_BOXES;
        param->truths = param->max_boxes * (coords + 1);
    }
    node.forward = bcnn_forward_yolo_layer;
    node.backward = bcnn_backward_yolo_layer;
    node.release_param = bcnn_release_param_yolo_layer;
    BCNN_CHECK_STATUS(bcnn_node_new_output(net, &node, s.n, s.c, s.h, s.w, dst_id));
    BCNN_CHECK_STATUS(bcnn_net_add_node(net, node));
    BCNN_INFO(net->log_ctx, "[Yolo] %-8s (%4d x%4d x%4d) -> %-8s %5d classes\n", src_id, s.w, s.h, s.c, dst_id, classes);
    return BCNN_SUCCESS;
}

/* what bcnn_hip_yolo_train_forward needs of a head; 0 when the head cannot train (built without the switch, no label or
 * gradient buffer) */
static int yolo_train_head(const bcnn_net *net, const bcnn_node *node, bcnn_hip_yolo_train_head *hd) {
    const bcnn_yolo_param *p = (const bcnn_yolo_param *)node->param;
    const bcnn_tensor *y = &net->tensors[node->dst[0]], *label = &net->tensors[1];
    if (p->truths <= 0 || !label->data_gpu || label->n < y->n || bcnn_tensor_size3d(label) < p->truths || !y->grad_data_gpu)
        return 0;
    memset(hd, 0, sizeof(*hd));
    hd->n = y->n; hd->h = y->h; hd->w = y->w;
    hd->num = p->num; hd->coords = p->coords; hd->classes = p->classes; hd->total = p->total;
    hd->in_w = net->tensors[0].w; hd->in_h = net->tensors[0].h;
    hd->label_stride = bcnn_tensor_size3d(label);
    for (int i = 0; i < p->num; ++i) hd->mask[i] = p->mask[i];
    memcpy(hd->biases, p->biases, (size_t)(2 * p->total) * sizeof(float));
    return 1;
}

int bcnn_yolo_heads_trainable(bcnn_net *net) {
    bcnn_hip_yolo_train_head hd;
    for (int i = 0; i < net->num_nodes; ++i)
        if (net->nodes[i].type == BCNN_LAYER_YOLOV3 && !yolo_train_head(net, &net->nodes[i], &hd)) return 0;
    return 1;
}

void bcnn_forward_yolo_layer(bcnn_net *net, bcnn_node *node) {
    bcnn_yolo_param *p = (bcnn_yolo_param *)node->param;
    bcnn_tensor *x = &net->tensors[node->src[0]], *y = &net->tensors[node->dst[0]];
    if (net->mode == BCNN_MODE_TRAIN) { /* reference bcnn_yolo.c:250-415, on the device; the statistics stay there */
        bcnn_hip_yolo_train_head hd;
        if (!yolo_train_head(net, node, &hd)) { /* bcnn_set_mode and the builder refuse such a net */
            fprintf(stderr, "[bcnn] YOLO head %s: TRAIN forward without a label or gradient buffer\n", y->name);
            exit(1);
        }
        const size_t need = bcnn_hip_yolo_train_workspace_size(&hd);
        if (p->train_workspace_size < need) { /* first TRAIN forward */
            bcnn_hip_sync();
            bcnn_hip_free(p->train_workspace_gpu);
            p->train_workspace_gpu = bcnn_hip_malloc_f32(need);
            p->train_workspace_size = need;
        }
        if (!p->train_record_gpu) p->train_record_gpu = bcnn_hip_malloc_f32(sizeof(bcnn_hip_yolo_train_record) / sizeof(float));
        if (bcnn_hip_yolo_train_forward(&hd, x->data_gpu, net->tensors[1].data_gpu, y->data_gpu, y->grad_data_gpu,
                                        (bcnn_hip_yolo_train_record *)p->train_record_gpu, p->train_workspace_gpu) != 0) {
            fprintf(stderr, "[bcnn] YOLO head %s: shape outside the device loss\n", y->name);
            exit(1);
        }
        return;
    }
    bcnn_hip_yolo_activate(x->data_gpu, y->data_gpu, y->n, p->num, p->coords, p->classes, y->h * y->w);
}

void bcnn_backward_yolo_layer(bcnn_net *net, bcnn_node *node) { /* reference bcnn_yolo.c:441-447 */
    bcnn_tensor *x = &net->tensors[node->src[0]], *y = &net->tensors[node->dst[0]];
    if (x->grad_data_gpu && y->grad_data_gpu)
        bcnn_hip_axpy((size_t)bcnn_tensor_size(x), 1.0f, y->grad_data_gpu, x->grad_data_gpu);
}

void bcnn_release_param_yolo_layer(bcnn_node *node) {
    bcnn_yolo_param *p = (bcnn_yolo_param *)node->param;
    free(p->mask);
    free(p->biases);
    free(p->cost);
    bcnn_hip_free(p->train_record_gpu);
    bcnn_hip_free(p->train_workspace_gpu);
}

/* The reference prints these on every TRAIN forward (bcnn_yolo.c:408-414), which here would cost a synchronisation per
 * head and step: the sums stay in a 32-byte device record and are read, and divided as there, on demand. */
static bcnn_status yolo_read_stats(bcnn_net *net, bcnn_node *node, bcnn_yolo_train_stats *out) {
    bcnn_yolo_param *p = (bcnn_yolo_param *)node->param;
    const bcnn_tensor *y = &net->tensors[node->dst[0]];
    bcnn_hip_yolo_train_record rec;
    memset(&rec, 0, sizeof(rec));
    if (p->train_record_gpu) bcnn_hip_memcpy_d2h(&rec, p->train_record_gpu, sizeof(rec));
    p->cost[0] = rec.cost;
    if (!out) return BCNN_SUCCESS;
    out->avg_iou = rec.avg_iou / rec.count;
    out->avg_class = rec.avg_cat / rec.count;
    out->avg_obj = rec.avg_obj / rec.count;
    out->avg_anyobj = rec.avg_anyobj / (y->w * y->h * p->num * y->n);
    out->recall50 = rec.recall / rec.count;
    out->recall75 = rec.recall75 / rec.count;
    out->count = rec.count;
    out->cost = rec.cost;
    return BCNN_SUCCESS;
}

bcnn_status bcnn_yolo_get_train_stats(bcnn_net *net, int node_index, bcnn_yolo_train_stats *out) {
    if (!net || !out || node_index < 0 || node_index >= net->num_nodes || net->nodes[node_index].type != BCNN_LAYER_YOLOV3)
        return BCNN_INVALID_PARAMETER;
    return yolo_read_stats(net, &net->nodes[node_index], out);
}

int bcnn_yolo_refresh_costs(bcnn_net *net) {
    int heads = 0;
    for (int i = 0; i < net->num_nodes; ++i)
        if (net->nodes[i].type == BCNN_LAYER_YOLOV3) {
            yolo_read_stats(net, &net->nodes[i], NULL);
            ++heads;
        }
    return heads;
}

/* ================================================================================================
 * detections (host; a few thousand candidate boxes at most), reference bcnn_yolo.c:99-145, 470-639
 * ============================================================================================== */
typedef struct {
    float x, y, w, h;
} yolo_box;

static float overlap(float x1, float w1, float x2, float w2) {
    const float l1 = x1 - w1 / 2, l2 = x2 - w2 / 2;
    const float left = l1 > l2 ? l1 : l2;
    const float r1 = x1 + w1 / 2, r2 = x2 + w2 / 2;
    const float right = r1 < r2 ? r1 : r2;
    return right - left;
}

static float box_iou(yolo_box a, yolo_box b) {
    const float w = overlap(a.x, a.w, b.x, b.w), h = overlap(a.y, a.h, b.y, b.h);
    const float inter = (w < 0 || h < 0) ? 0 : w * h;
    return inter / (a.w * a.h + b.w * b.h - inter);
}

static int entry_index(const bcnn_yolo_param *p, const bcnn_tensor *t, int batch, int location, int entry) {
    const int n = location / (t->w * t->h), loc = location % (t->w * t->h);
    return batch * bcnn_tensor_size3d(t) + n * t->w * t->h * (p->coords + p->classes + 1) + entry * t->w * t->h + loc;
}

static void correct_region_boxes(bcnn_output_detection *dets, int n, int w, int h, int netw, int neth, int relative) {
    int new_w, new_h;
    if (((float)netw / w) < ((float)neth / h)) {
        new_w = netw;
        new_h = (h * netw) / w;
    } else {
        new_h = neth;
        new_w = (w * neth) / h;
    }
    for (int i = 0; i < n; ++i) {
        dets[i].x = (dets[i].x - (netw - new_w) / 2. / netw) / ((float)new_w / netw);
        dets[i].y = (dets[i].y - (neth - new_h) / 2. / neth) / ((float)new_h / neth);
        dets[i].w *= (float)netw / new_w;
        dets[i].h *= (float)neth / new_h;
        if (!relative) {
            dets[i].x *= w;
            dets[i].w *= w;
            dets[i].y *= h;
            dets[i].h *= h;
        }
    }
}

static int by_objectness_desc(const void *pa, const void *pb) {
    const float diff = ((const bcnn_output_detection *)pa)->objectness - ((const bcnn_output_detection *)pb)->objectness;
    return diff < 0 ? 1 : (diff > 0 ? -1 : 0);
}

static void suppress_sorted(bcnn_output_detection *dets, int num_dets, float thresh);

static void do_nms_obj(bcnn_output_detection *dets, int num_dets, float thresh) {
    int k = num_dets - 1;
    for (int i = 0; i <= k; ++i) { /* zero-objectness boxes to the end, outside the sort */
        if (dets[i].objectness == 0) {
            const bcnn_output_detection swap = dets[i];
            dets[i] = dets[k];
            dets[k] = swap;
            --k;
            --i;
        }
    }
    num_dets = k + 1;
    qsort(dets, (size_t)num_dets, sizeof(bcnn_output_detection), by_objectness_desc);
    suppress_sorted(dets, num_dets, thresh);
}

/* the greedy walk of do_nms_obj over boxes already in their final order */
static void suppress_sorted(bcnn_output_detection *dets, int num_dets, float thresh) {
    for (int i = 0; i < num_dets; ++i) {
        if (dets[i].objectness == 0) continue;
        const yolo_box a = {dets[i].x, dets[i].y, dets[i].w, dets[i].h};
        for (int j = i + 1; j < num_dets; ++j) {
            if (dets[j].objectness == 0) continue;
            const yolo_box b = {dets[j].x, dets[j].y, dets[j].w, dets[j].h};
            if (box_iou(a, b) > thresh) {
                dets[j].objectness = 0;
                for (int c = 0; c < dets[j].num_classes; ++c) dets[j].prob[c] = 0;
            }
        }
    }
}

bcnn_output_detection *bcnn_yolo_get_detections(bcnn_net *net, int batch, int w, int h, int netw, int neth,
                                                float thresh, int relative, int *num_dets) {
    int count = 0;
    if (num_dets) *num_dets = 0;
    for (int k = 0; k < net->num_nodes; ++k) { /* one read-back per head, then count the candidates */
        if (net->nodes[k].type != BCNN_LAYER_YOLOV3) continue;
        bcnn_download_tensor(net, net->nodes[k].dst[0], 0);
    }
    bcnn_synchronize(net);
    for (int k = 0; k < net->num_nodes; ++k) {
        if (net->nodes[k].type != BCNN_LAYER_YOLOV3) continue;
        const bcnn_yolo_param *p = (const bcnn_yolo_param *)net->nodes[k].param;
        const bcnn_tensor *dst = &net->tensors[net->nodes[k].dst[0]];
        if (batch < 0 || batch >= dst->n || !dst->data) return NULL;
        for (int i = 0; i < dst->w * dst->h; ++i)
            for (int n = 0; n < p->num; ++n)
                count += dst->data[entry_index(p, dst, batch, n * dst->w * dst->h + i, p->coords)] > thresh;
    }
    if (count == 0) return NULL;
    bcnn_output_detection *dets = (bcnn_output_detection *)calloc((size_t)count, sizeof(bcnn_output_detection));
    count = 0;
    for (int k = 0; k < net->num_nodes; ++k) {
        if (net->nodes[k].type != BCNN_LAYER_YOLOV3) continue;
        const bcnn_yolo_param *p = (const bcnn_yolo_param *)net->nodes[k].param;
        const bcnn_tensor *dst = &net->tensors[net->nodes[k].dst[0]];
        const int hw = dst->w * dst->h;
        for (int i = 0; i < hw; ++i) {
            const int row = i / dst->w, col = i % dst->w;
            for (int n = 0; n < p->num; ++n) {
                const float objectness = dst->data[entry_index(p, dst, batch, n * hw + i, p->coords)];
                if (objectness <= thresh) continue;
                const float *x = dst->data + entry_index(p, dst, batch, n * hw + i, 0);
                const float *anchor = p->biases + 2 * p->mask[n];
                bcnn_output_detection *d = &dets[count++];
                /* get_yolo_box, reference bcnn_yolo.c:137-145 */
                d->x = (col + x[0]) / dst->w;
                d->y = (row + x[hw]) / dst->h;
                d->w = expf(x[2 * hw]) * anchor[0] / net->tensors[0].w;
                d->h = expf(x[3 * hw]) * anchor[1] / net->tensors[0].h;
                d->objectness = objectness;
                d->num_classes = p->classes;
                d->prob = (float *)calloc((size_t)(p->classes > 0 ? p->classes : 1), sizeof(float));
                if (p->coords > 4) d->mask = (float *)calloc((size_t)(p->coords - 4), sizeof(float));
                for (int j = 0; j < p->classes; ++j) {
                    const float prob = objectness * x[(p->coords + 1 + j) * hw];
                    d->prob[j] = (prob > thresh) ? prob : 0;
                }
            }
        }
    }
    correct_region_boxes(dets, count, w, h, netw, neth, relative);
    do_nms_obj(dets, count, 0.45f);
    if (num_dets) *num_dets = count;
    return dets;
}

/* ================================================================================================
 * detections of the whole batch, decoded / filtered / suppressed on the device (detect.hip: bcnn_hip_yolo_detect_batch).
 * What comes back is one block -- the counts, the sort order and the compact box records -- whose size depends on the
 * record capacity, not on the head tensors; the head tensors are never read back.
 * ============================================================================================== */
#define DETECT_RECORD_CAPACITY 256 /* boxes per image the first pass has room for, until a batch needed more */
#define DETECT_NMS_THRESH 0.45f    /* reference bcnn_yolo.c:637 */

typedef struct {
    float objectness;
    int index;
} det_key;

static int by_objectness_then_index(const void *pa, const void *pb) {
    const det_key *a = (const det_key *)pa, *b = (const det_key *)pb;
    if (a->objectness != b->objectness) return a->objectness < b->objectness ? 1 : -1;
    return a->index < b->index ? -1 : (a->index > b->index ? 1 : 0);
}

/* one record -> one detection (prob and mask calloc'ed like bcnn_yolo_get_detections does); 0 on failure */
static int detection_from_record(bcnn_output_detection *d, const float *rec, const bcnn_hip_yolo_head *heads,
                                 int num_heads) {
    int g, first = 0, k = 0;
    memcpy(&g, &rec[5], sizeof(g));
    for (; k < num_heads; ++k) {
        const int cnt = heads[k].h * heads[k].w * heads[k].num;
        if (g >= first && g < first + cnt) break;
        first += cnt;
    }
    if (k == num_heads) return 0;
    const int classes = heads[k].classes, coords = heads[k].coords;
    d->x = rec[0];
    d->y = rec[1];
    d->w = rec[2];
    d->h = rec[3];
    d->objectness = rec[4];
    d->num_classes = classes;
    d->prob = (float *)calloc((size_t)(classes > 0 ? classes : 1), sizeof(float));
    if (!d->prob) return 0;
    memcpy(d->prob, rec + BCNN_HIP_YOLO_RECORD_HEAD, (size_t)classes * sizeof(float));
    if (coords > 4) {
        d->mask = (float *)calloc((size_t)(coords - 4), sizeof(float));
        if (!d->mask) return 0;
    }
    return 1;
}

void bcnn_free_detections(bcnn_output_detection *dets, int num_dets) {
    if (!dets) return;
    for (int i = 0; i < num_dets; ++i) {
        free(dets[i].prob);
        free(dets[i].mask);
    }
    free(dets);
}

/* bcnn_yolo_get_detections_batch with its two capacities as arguments (<= 0: the defaults), so that a test can drive
 * the grow-and-rerun path and the host-NMS path with a dozen boxes. record_cap: boxes per image the first pass has room
 * for; nms_cap: boxes per image the device NMS takes (at most bcnn_hip_yolo_nms_capacity()). *passes (may be NULL)
 * receives how many times the kernels ran (1, or 2 after a grow). */
bcnn_status bcnn_yolo_detections_batch_worker(bcnn_net *net, const int *widths, const int *heights, int netw, int neth,
                                              float thresh, int relative, int record_cap, int nms_cap,
                                              bcnn_output_detection **dets, int *num_dets, int *passes) {
    if (!net || !widths || !heights || !dets || !num_dets || netw <= 0 || neth <= 0) return BCNN_INVALID_PARAMETER;
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    bcnn_hip_yolo_head heads[BCNN_HIP_YOLO_MAX_HEADS];
    int num_heads = 0, n = 0, max_classes = 0;
    memset(heads, 0, sizeof(heads));
    for (int k = 0; k < net->num_nodes; ++k) {
        if (net->nodes[k].type != BCNN_LAYER_YOLOV3) continue;
        const bcnn_yolo_param *p = (const bcnn_yolo_param *)net->nodes[k].param;
        BCNN_CHECK_AND_LOG(net->log_ctx, num_heads < BCNN_HIP_YOLO_MAX_HEADS && p->num <= BCNN_HIP_YOLO_MAX_ANCHORS,
                           BCNN_INVALID_PARAMETER, "Batched detections: at most %d heads of %d anchors each\n",
                           BCNN_HIP_YOLO_MAX_HEADS, BCNN_HIP_YOLO_MAX_ANCHORS);
        bcnn_materialize_data(net, net->nodes[k].dst[0]);
        const bcnn_tensor *dst = &net->tensors[net->nodes[k].dst[0]];
        BCNN_CHECK_AND_LOG(net->log_ctx, dst->data_gpu && dst->n > 0 && (num_heads == 0 || dst->n == n),
                           BCNN_INVALID_PARAMETER, "Batched detections: head %s has no device output\n", dst->name);
        n = dst->n;
        bcnn_hip_yolo_head *hd = &heads[num_heads++];
        hd->out_d = dst->data_gpu;
        hd->h = dst->h;
        hd->w = dst->w;
        hd->num = p->num;
        hd->coords = p->coords;
        hd->classes = p->classes;
        for (int i = 0; i < p->num; ++i) {
            hd->anchor_w[i] = p->biases[2 * p->mask[i]];
            hd->anchor_h[i] = p->biases[2 * p->mask[i] + 1];
        }
        if (p->classes > max_classes) max_classes = p->classes;
    }
    if (num_heads == 0) return BCNN_INVALID_PARAMETER;
    int *geom = (int *)malloc((size_t)n * 4 * sizeof(int));
    if (!geom) return BCNN_FAILED_ALLOC;
    for (int b = 0; b < n; ++b) { /* correct_region_boxes: the letter-boxed extent of image b */
        const int w = widths[b], h = heights[b];
        if (w <= 0 || h <= 0) {
            free(geom);
            return BCNN_INVALID_PARAMETER;
        }
        int new_w, new_h;
        if (((float)netw / w) < ((float)neth / h)) {
            new_w = netw;
            new_h = (h * netw) / w;
        } else {
            new_h = neth;
            new_w = (w * neth) / h;
        }
        geom[4 * b] = w;
        geom[4 * b + 1] = h;
        geom[4 * b + 2] = new_w;
        geom[4 * b + 3] = new_h;
    }
    const int stride = BCNN_HIP_YOLO_RECORD_HEAD + max_classes;
    const int nms_max = bcnn_hip_yolo_nms_capacity();
    const int nms_eff = (nms_cap <= 0 || nms_cap > nms_max) ? nms_max : nms_cap;
    int cap = record_cap > 0 ? record_cap
                             : (hc->detect_capacity > DETECT_RECORD_CAPACITY ? hc->detect_capacity : DETECT_RECORD_CAPACITY);
    int *result = NULL;
    bcnn_status st = BCNN_SUCCESS;
    int pass = 0, most = 0;
    for (;;) { /* the counts are exact, so one grow is enough */
        result = (int *)malloc(bcnn_hip_yolo_detect_result_words(n, cap, max_classes) * sizeof(int));
        if (!result) {
            st = BCNN_FAILED_ALLOC;
            break;
        }
        ++pass;
        if (bcnn_hip_yolo_detect_batch(heads, num_heads, n, geom, net->tensors[0].w, net->tensors[0].h, netw, neth, thresh,
                                       relative, DETECT_NMS_THRESH, cap, nms_eff, result) != 0) {
            st = BCNN_INVALID_PARAMETER;
            break;
        }
        bcnn_hip_sync(); /* the one synchronisation of the call (two after a grow) */
        most = 0;
        for (int b = 0; b < n; ++b) most = result[b] > most ? result[b] : most;
        if (most <= cap) break;
        if (pass == 2) {
            st = BCNN_INTERNAL_ERROR;
            break;
        }
        free(result);
        result = NULL;
        cap = most + most / 4;
    }
    free(geom);
    if (passes) *passes = pass;
    if (st != BCNN_SUCCESS) {
        free(result);
        return st;
    }
    if (record_cap <= 0) hc->detect_capacity = most + most / 4; /* follows the latest batch: it shrinks again too */

    const int *count = result, *order = result + n;
    const float *records = (const float *)(result + n + (size_t)n * cap);
    bcnn_output_detection **out = (bcnn_output_detection **)calloc((size_t)n, sizeof(*out));
    if (!out) st = BCNN_FAILED_ALLOC;
    for (int b = 0; st == BCNN_SUCCESS && b < n; ++b) {
        const int cnt = count[b];
        if (cnt <= 0) continue;
        const float *rec = records + (size_t)b * cap * stride;
        out[b] = (bcnn_output_detection *)calloc((size_t)cnt, sizeof(bcnn_output_detection));
        det_key *keys = NULL;
        if (cnt > nms_eff) { /* too many for the device NMS: the same order, then the host's greedy walk */
            keys = (det_key *)malloc((size_t)cnt * sizeof(det_key));
            for (int r = 0; keys && r < cnt; ++r) {
                keys[r].objectness = rec[(size_t)r * stride + 4];
                keys[r].index = r;
            }
            if (keys) qsort(keys, (size_t)cnt, sizeof(det_key), by_objectness_then_index);
        }
        if (!out[b] || (cnt > nms_eff && !keys)) {
            st = BCNN_FAILED_ALLOC;
            free(keys);
            break;
        }
        for (int r = 0; r < cnt; ++r) {
            const int slot = keys ? keys[r].index : (int)((unsigned)order[(size_t)b * cap + r] & 0x7fffffffu);
            if (slot >= cnt || !detection_from_record(&out[b][r], rec + (size_t)slot * stride, heads, num_heads)) {
                st = BCNN_INTERNAL_ERROR;
                break;
            }
        }
        if (keys && st == BCNN_SUCCESS) suppress_sorted(out[b], cnt, DETECT_NMS_THRESH);
        free(keys);
    }
    if (st != BCNN_SUCCESS) {
        for (int b = 0; out && b < n; ++b) bcnn_free_detections(out[b], out[b] ? count[b] : 0);
    } else {
        for (int b = 0; b < n; ++b) {
            dets[b] = out[b];
            num_dets[b] = count[b] > 0 ? count[b] : 0;
        }
    }
    free(out);
    free(result);
    return st;
}

bcnn_status bcnn_yolo_get_detections_batch(bcnn_net *net, const int *widths, const int *heights, int netw, int neth,
                                           float thresh, int relative, bcnn_output_detection **dets, int *num_dets) {
    return bcnn_yolo_detections_batch_worker(net, widths, heights, netw, neth, thresh, relative, 0, 0, dets, num_dets,
                                             NULL);
}
