/*
 * bcnn_data_segmentation.c -- BCNN_LOAD_SEGMENTATION_LIST: "image-path mask-path" lines into tensors[0] (the image, as the
 * classification list makes it) and tensors[1] (a class-index label map [n][1][h][w], what the softmax-loss node reads).
 * No reference counterpart. bcnn_data.c opens the streams, runs the batch loop and the uploads; this file reads one sample.
 *
 * One sample: image and mask are decoded FIRST; a line whose image or mask does not decode, whose extents differ or whose
 * image has other channels than the input is skipped with a log line BEFORE ANY DRAW, and the next line takes the slot
 * (bcnn_loader_next gives up after 1000 skips in a row). So this loader has no "buffer as it was" state, and leaves none
 * behind for the reference-compatible list loaders. Then the crop origin is drawn (two draws in TRAIN mode when the file
 * does not have the input's extents, the centre otherwise), then the augmentation once (draw_augmentation). The image is
 * cropped and augmented by bcnn_data.c's own code; the mask is cropped at the same origin, with F outside the file, and
 * warped by bip_label_warp.h from the record and taps that fill_record makes of the same draws. The mask adds no rand()
 * call: the input batch is what BCNN_LOAD_CLASSIFICATION_LIST produces for the same image files, seed and settings, bit
 * for bit. Outside TRAIN mode the record is the identity. In PREDICT mode the mask path may be missing and is not read.
 *
 * F, the fill byte (where the image gets its canvas): the ignore_label of the first softmax-loss node in node order when
 * that lies in 0 ... 255, else 255.
 *
 * Routes: on the host the labels go into tensors[1].data as (float)byte, sample by sample. With
 * bcnn_set_loader_on_device the cropped raw masks of the batch are gathered in it->input_net beside the image batch's
 * block, and bcnn_segmentation_labels makes the label tensor with one call of bcnn_hip_augment_label_batch from the image
 * batch's own records; tensors[1].data is then not written. If the device side refused the image batch's effects, or
 * refuses that call, the same records make the labels here and they are uploaded as ever.
 */
#include <string.h>

#include <bcnn_hip.h>
#include <bip/bip.h>

#include "bcnn_internal.h"
#include "bip_label_warp.h"

static int fill_byte(const bcnn_net *net) {
    for (int i = 0; i < net->num_nodes; ++i) {
        if (net->nodes[i].type != BCNN_LAYER_SOFTMAX_LOSS) continue;
        const int ignore = ((const bcnn_softmax_loss_param *)net->nodes[i].param)->ignore_label;
        return (ignore >= 0 && ignore <= 255) ? ignore : 255;
    }
    return 255;
}

/* it->input_net: the cropped raw masks of one batch, w x h bytes each (list_init leaves it unused) */
bcnn_status bcnn_segmentation_init(bcnn_loader *it, bcnn_net *net) {
    const bcnn_tensor *in = &net->tensors[0];
    const size_t batch = net->batch_size > 0 ? (size_t)net->batch_size : 1;
    it->input_net = (uint8_t *)calloc(batch * in->w * in->h, 1);
    return it->input_net ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
}

bcnn_status bcnn_segmentation_check(bcnn_net *net) {
    const bcnn_tensor *in = &net->tensors[0], *lab = &net->tensors[1];
    if (!in->data) /* the input tensor gets its buffers when the net is compiled */
        BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER, "bcnn_loader_next: the input tensor is not allocated (bcnn_compile_net)\n");
    if (net->mode != BCNN_MODE_PREDICT &&
        (net->num_tensors < 2 || !lab->data || lab->n < net->batch_size || lab->c != 1 || lab->h != in->h || lab->w != in->w))
        BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER,
                   "bcnn_loader_next: the segmentation list fills a [n][1][%d][%d] label map, the extents of the net input; a "
                   "net that predicts at a lower resolution ends in an [interp]\n", in->h, in->w);
    if (bcnn_loader_effects_on(net) && net->mode == BCNN_MODE_TRAIN && net->data_aug && net->data_aug->max_distortion > 0.0f)
        BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER,
                   "bcnn_loader_next: the Perlin distortion (max_distortion) moves pixels and has no label form: a "
                   "segmentation list cannot run with loader_effects and max_distortion > 0\n");
    return BCNN_SUCCESS;
}

/* the label plane of slot idx from its cropped mask */
static void labels_of(bcnn_net *net, const uint8_t *mask, const bcnn_hip_augment_record *r, const int32_t *taps, int idx) {
    const bcnn_tensor *in = &net->tensors[0];
    const int w = in->w, h = in->h;
    const bip_label_sample s = {mask, taps, taps + 2 * (size_t)w, w, h, r->flags, r->x_ul, r->y_ul, r->ca, r->sa, fill_byte(net)};
    float *y = net->tensors[1].data + (size_t)idx * w * h;
    for (int32_t py = 0; py < h; ++py)
        for (int32_t px = 0; px < w; ++px) y[(size_t)py * w + px] = (float)bip_label_warp(&s, px, py);
}

bcnn_status bcnn_segmentation_next(bcnn_loader *it, bcnn_net *net, int idx) {
    bcnn_tensor *in = &net->tensors[0];
    const int w = in->w, h = in->h, c = in->c, with_mask = net->mode != BCNN_MODE_PREDICT;
    char **tok = NULL;
    const int n = bcnn_loader_line_tokens(it->f_current, &tok);
    if (n <= 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid segmentation list format\n");
        return BCNN_INVALID_DATA;
    }
    bcnn_status st = BCNN_SUCCESS;
    unsigned char *img = NULL, *mask = NULL;
    int wi = 0, hi = 0, ci = 0, wm = 0, hm = 0;
    /* ---- everything that can skip the line, before any draw */
    if (with_mask && n != 2) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip line %s: found %d tokens, expected an image path and a mask path\n", tok[0], n);
        st = BCNN_INVALID_DATA;
    }
    if (st == BCNN_SUCCESS) {
        bip_load_image(tok[0], &img, &wi, &hi, &ci);
        if (!(img && wi > 0 && hi > 0)) {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip invalid image %s\n", tok[0]);
            st = BCNN_INVALID_DATA;
        } else if (ci != c) {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: unexpected number of channels\n", tok[0]);
            st = BCNN_INVALID_DATA;
        }
    }
    if (st == BCNN_SUCCESS && with_mask) {
        bip_load_index_map(tok[1], &mask, &wm, &hm);
        if (!(mask && wm > 0 && hm > 0)) {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: its mask %s is not a class-index map\n", tok[0], tok[1]);
            st = BCNN_INVALID_DATA;
        } else if (wm != wi || hm != hi) {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: it is %d x %d, its mask %s is %d x %d\n", tok[0], wi, hi,
                     tok[1], wm, hm);
            st = BCNN_INVALID_DATA;
        }
    }
    /* ---- the draws: the crop origin, then the augmentation, as the classification list makes them */
    int x_ul = 0, y_ul = 0;
    if (st == BCNN_SUCCESS) {
        bcnn_loader_crop_origin(net, wi, hi, w, h, &x_ul, &y_ul);
        st = bcnn_loader_crop_to_input(img, wi, hi, x_ul, y_ul, it->input_uchar, w, h, c);
    }
    if (st == BCNN_SUCCESS) {
        if (net->data_aug) {
            net->data_aug->shift_x = x_ul;
            net->data_aug->shift_y = y_ul;
        }
        uint8_t *cropped = it->input_net + (size_t)idx * w * h;
        if (with_mask) { /* the same window of the mask, F outside the file */
            const int F = fill_byte(net);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const long long X = (long long)x + x_ul, Y = (long long)y + y_ul;
                    cropped[(size_t)y * w + x] = (X >= 0 && X < wi && Y >= 0 && Y < hi) ? mask[(size_t)Y * wi + (size_t)X] : (uint8_t)F;
                }
        }
        if (bcnn_loader_staging(net)) { /* the device route: image and draws into the block; the labels follow per batch */
            const bcnn_hip_augment_record *r;
            const int32_t *taps;
            st = bcnn_loader_stage_sample(net, it, idx, &r, &taps);
        } else {
            bcnn_hip_augment_record r;
            int32_t *taps = (int32_t *)calloc(((size_t)w + h) * 2, sizeof(int32_t));
            st = taps ? bcnn_loader_augment_recorded(net, it->input_uchar, w, h, c, &r, taps) : BCNN_FAILED_ALLOC;
            if (st == BCNN_SUCCESS) {
                bcnn_convert_img_to_float(it->input_uchar, w, h, c, 1 / 127.5f, net->data_aug ? net->data_aug->swap_to_bgr : 0,
                                          127.5f, 127.5f, 127.5f, in->data + (size_t)idx * bcnn_tensor_size3d(in));
                if (with_mask) labels_of(net, cropped, &r, taps, idx);
            }
            free(taps);
        }
    }
    free(img);
    free(mask);
    bcnn_loader_free_tokens(tok, n);
    return st;
}

int bcnn_segmentation_labels(bcnn_net *net, bcnn_loader *it, int device_ok) {
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    bcnn_tensor *in = &net->tensors[0], *lab = &net->tensors[1];
    if (net->mode == BCNN_MODE_PREDICT) return 0;
    const bcnn_hip_augment_record *records;
    const int32_t *taps;
    bcnn_loader_staged_records(net, &records, &taps);
    if (!records || !taps) return 0;
    if (device_ok && lab->data_gpu &&
        bcnn_hip_augment_label_batch(lab->data_gpu, lab->n, in->h, in->w, net->batch_size, it->input_net, records, taps,
                                     fill_byte(net)) == 0) {
        hc->loader_device_labels = net->batch_size;
        return 1;
    }
    const size_t sample_taps = ((size_t)in->w + in->h) * 2, map_bytes = (size_t)in->w * in->h;
    for (int i = 0; i < net->batch_size; ++i)
        labels_of(net, it->input_net + (size_t)i * map_bytes, &records[i], taps + (size_t)i * sample_taps, i);
    return 0;
}
