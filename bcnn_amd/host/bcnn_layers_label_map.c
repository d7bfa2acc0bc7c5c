/*
 * bcnn_layers_label_map.c -- bcnn_get_label_maps_batch: what a segmentation net predicts, as one class index per pixel of
 * every image of the batch at that image's own size, and on request the confusion counts against truth maps of those
 * sizes. The output end of semantic segmentation, as bcnn_yolo_get_detections_batch is the detector's: the geometry
 * bcnn_fill_tensor_with_images put in is undone on the device and only bytes come back (label_map.hip: one copy in, one
 * kernel for the whole batch, one copy back). No reference counterpart and no node: the call reads a tensor.
 *
 * This file only checks the arguments against the net and turns (widths, heights, fit) into the rectangles of the C-ABI;
 * the rule itself (rectangle, resampling, argmax, counts) is ../csrc/label_map_rule.h behind bcnn_hip_label_map_fit and
 * bcnn_hip_label_maps_batch, which repeats every check that needs no net before it stages or queues anything.
 */
#include <stdlib.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

/* the counts cross the C-ABI as long long */
typedef char bcnn_label_map_int64_is_long_long[sizeof(int64_t) == sizeof(long long) ? 1 : -1];

bcnn_status bcnn_get_label_maps_batch(bcnn_net *net, int tensor_index, int num_images, const int *widths,
                                      const int *heights, int fit, int align_corners, uint8_t *const *labels,
                                      const int *strides, bcnn_label_map_eval *eval) {
    if (!net) return BCNN_INVALID_PARAMETER;
    BCNN_CHECK_AND_LOG(net->log_ctx, tensor_index >= 0 && tensor_index < net->num_tensors, BCNN_INVALID_PARAMETER,
                       "Label maps: invalid tensor index %d\n", tensor_index);
    const bcnn_tensor *t = &net->tensors[tensor_index];
    BCNN_CHECK_AND_LOG(net->log_ctx, t->data_gpu != NULL, BCNN_INVALID_PARAMETER,
                       "Label maps: tensor %d has no device buffer\n", tensor_index);
    BCNN_CHECK_AND_LOG(net->log_ctx, num_images >= 1 && num_images <= t->n, BCNN_INVALID_PARAMETER,
                       "Label maps: %d images for a batch of %d\n", num_images, t->n);
    BCNN_CHECK_AND_LOG(net->log_ctx, t->c >= 1 && t->c <= 256 && t->h >= 1 && t->w >= 1, BCNN_INVALID_PARAMETER,
                       "Label maps: tensor %d has %d channels (a label is a byte: 1 to 256 classes)\n", tensor_index, t->c);
    BCNN_CHECK_AND_LOG(net->log_ctx, widths && heights, BCNN_INVALID_PARAMETER, "Label maps: NULL widths or heights\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, fit == BCNN_IMAGE_FIT_STRETCH || fit == BCNN_IMAGE_FIT_LETTERBOX,
                       BCNN_INVALID_PARAMETER, "Label maps: unknown fit %d\n", fit);
    BCNN_CHECK_AND_LOG(net->log_ctx,
                       fit != BCNN_IMAGE_FIT_LETTERBOX || (t->h == net->tensors[0].h && t->w == net->tensors[0].w),
                       BCNN_INVALID_PARAMETER,
                       "Label maps: letterbox needs a tensor of the input's extent %d x %d (tensor %d is %d x %d): the "
                       "rectangle of a resampled head would be fractional\n",
                       net->tensors[0].w, net->tensors[0].h, tensor_index, t->w, t->h);
    BCNN_CHECK_AND_LOG(net->log_ctx, labels || eval, BCNN_INVALID_PARAMETER, "Label maps: neither labels nor eval\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, !eval || (eval->truths && eval->counts), BCNN_INVALID_PARAMETER,
                       "Label maps: eval without truths or counts\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, !eval || eval->ignore_label < 256, BCNN_INVALID_PARAMETER,
                       "Label maps: ignore label %d is no byte (negative: none)\n", eval ? eval->ignore_label : 0);
    bcnn_hip_label_map_image *imgs = (bcnn_hip_label_map_image *)calloc((size_t)num_images, sizeof(*imgs));
    if (!imgs) return BCNN_FAILED_ALLOC;
    for (int b = 0; b < num_images; ++b) {
        const int bad_ptr = (labels && !labels[b]) || (eval && !eval->truths[b]);
        const int bad_stride = (labels && strides && strides[b] < widths[b]) ||
                               (eval && eval->strides && eval->strides[b] < widths[b]);
        if (bad_ptr || bad_stride || bcnn_hip_label_map_fit(fit, t->w, t->h, widths[b], heights[b], &imgs[b]) != 0) {
            free(imgs);
            BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER,
                       "Label maps: image %d: a NULL buffer, a stride below the width, an extent below 1 or a letterbox "
                       "extent of 0 (%d x %d in %d x %d)\n", b, widths[b], heights[b], t->w, t->h);
        }
    }
    /* values a fused forward left pending for this tensor are produced first, as in bcnn_download_tensor */
    bcnn_materialize_data(net, tensor_index);
    long long ignored = 0, out_of_range = 0;
    const int st = bcnn_hip_label_maps_batch(t->data_gpu, t->n, t->c, t->h, t->w, align_corners ? 1 : 0, imgs, num_images,
                                             labels, strides, eval ? eval->truths : NULL, eval ? eval->strides : NULL,
                                             eval ? eval->ignore_label : -1, eval ? (long long *)eval->counts : NULL,
                                             &ignored, &out_of_range);
    free(imgs);
    if (st != 0)
        BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER,
                   "Label maps: the label maps of the batch (with their truths) exceed 2 GiB\n");
    if (eval) {
        eval->ignored += (int64_t)ignored;
        eval->out_of_range += (int64_t)out_of_range;
    }
    return BCNN_SUCCESS;
}
