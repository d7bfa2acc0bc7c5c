/* bcnn_input_jpeg.c -- bcnn_fill_tensor_with_jpegs: the input tensor of a batch from compressed JPEG buffers. The serial
 * half of the decoder (headers, entropy decoding) runs here through libbip.so, straight into the pinned staging block
 * that libbcnn_hip.so hands out; inverse DCT, upsampling, colour conversion, resize and float conversion run on the
 * device (bcnn_amd/csrc/jpeg_pixels.hip). Decoded pixels never exist on the host. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "bcnn_internal.h"
#include "../../include/bcnn_hip.h"

typedef struct {
    const uint8_t *const *buffers;
    const size_t *lengths;
    const bip_jpeg_info *infos;
    int16_t *const *coeff;
    int num_images, first, step;
    int failed; /* lowest index of this worker's images that failed, or num_images */
    int *status; /* per image (bcnn_jpeg_read_batch_each), or NULL */
} jpeg_worker;

static void *jpeg_worker_run(void *arg) {
    jpeg_worker *w = (jpeg_worker *)arg;
    /* no early exit: what each coeff[b] holds afterwards does not depend on the number of workers */
    for (int b = w->first; b < w->num_images; b += w->step) {
        if (w->status && !w->coeff[b]) continue; /* not this routine's image */
        const int ok = bip_jpeg_read_coefficients(w->buffers[b], w->lengths[b], &w->infos[b], w->coeff[b]) == BIP_SUCCESS;
        if (w->status) w->status[b] = ok;
        if (!ok && b < w->failed) w->failed = b;
    }
    return NULL;
}

/* Entropy-decodes image b of the batch into coeff[b] (infos[b].num_coefficients int16 each), images b = t, t + T, ... on
 * thread t of T = num_threads; with T <= 1 on the calling thread alone. Returns the lowest index that failed to decode,
 * -1 when all decoded, or -2 when the routine's own bookkeeping could not be allocated (nothing was decoded). The bytes
 * written are the same for every T. */
static int read_batch(int num_images, const uint8_t *const *buffers, const size_t *lengths, const bip_jpeg_info *infos,
                      int16_t *const *coeff, int num_threads, int *status) {
    int T = num_threads < 1 ? 1 : (num_threads > num_images ? num_images : num_threads);
    jpeg_worker *workers = (jpeg_worker *)calloc((size_t)T, sizeof(jpeg_worker));
    pthread_t *threads = (pthread_t *)calloc((size_t)T, sizeof(pthread_t));
    if (!workers || !threads) { free(workers); free(threads); return -2; }
    for (int t = 0; t < T; ++t) {
        jpeg_worker w = {buffers, lengths, infos, coeff, num_images, t, T, num_images, status};
        workers[t] = w;
    }
    int started = 0;
    for (int t = 1; t < T; ++t) { /* a thread that cannot be created: its images are decoded below */
        if (pthread_create(&threads[t], NULL, jpeg_worker_run, &workers[t]) != 0) break;
        started = t;
    }
    jpeg_worker_run(&workers[0]);
    for (int t = started + 1; t < T; ++t) jpeg_worker_run(&workers[t]);
    int failed = num_images;
    for (int t = 0; t < T; ++t) {
        if (t >= 1 && t <= started) pthread_join(threads[t], NULL);
        if (workers[t].failed < failed) failed = workers[t].failed;
    }
    free(workers);
    free(threads);
    return failed < num_images ? failed : -1;
}

int bcnn_jpeg_read_batch(int num_images, const uint8_t *const *buffers, const size_t *lengths, const bip_jpeg_info *infos,
                         int16_t *const *coeff, int num_threads) {
    return read_batch(num_images, buffers, lengths, infos, coeff, num_threads, NULL);
}

/* The same with a status PER IMAGE, for a caller that goes on with the images that decoded (the list loaders): images
 * with coeff[b] == NULL are skipped and keep their status[b]; the others get status[b] = 1 (decoded) or 0. Returns 0, or
 * -2 when the bookkeeping could not be allocated (nothing was decoded, status untouched). */
int bcnn_jpeg_read_batch_each(int num_images, const uint8_t *const *buffers, const size_t *lengths,
                              const bip_jpeg_info *infos, int16_t *const *coeff, int num_threads, int *status) {
    if (!status || num_images < 1) return num_images < 1 ? 0 : -2;
    return read_batch(num_images, buffers, lengths, infos, coeff, num_threads, status) == -2 ? -2 : 0;
}

/* what libbcnn_hip.so needs of a parsed frame header (it does not depend on libbip.so) */
void bcnn_jpeg_frame_from_info(const bip_jpeg_info *info, bcnn_hip_jpeg_frame *f) {
    memset(f, 0, sizeof(*f));
    f->width = info->width; f->height = info->height; f->ncomp = info->ncomp;
    f->hmax = info->hmax; f->vmax = info->vmax;
    for (int k = 0; k < info->ncomp && k < 3; ++k) {
        const bip_jpeg_component *s = &info->comp[k];
        bcnn_hip_jpeg_component *d = &f->comp[k];
        d->h = s->h; d->v = s->v; d->width = s->width; d->height = s->height; d->pitch = s->pitch; d->rows = s->rows;
        d->blocks_w = s->blocks_w; d->blocks_h = s->blocks_h; d->idct_w = s->idct_w; d->idct_h = s->idct_h;
    }
}

bcnn_status bcnn_fill_tensor_with_jpegs(bcnn_net *net, int tensor_index, int num_images, const uint8_t *const *buffers,
                                        const size_t *lengths, int fit, float norm_coeff, int swap_to_bgr, float mean_r,
                                        float mean_g, float mean_b, int *failed_image) {
    if (failed_image) *failed_image = -1;
    if (!net) return BCNN_INVALID_PARAMETER;
    BCNN_CHECK_AND_LOG(net->log_ctx, tensor_index >= 0 && tensor_index < net->num_tensors, BCNN_INVALID_PARAMETER,
                       "Fill with JPEGs: invalid tensor index %d\n", tensor_index);
    bcnn_tensor *t = &net->tensors[tensor_index];
    BCNN_CHECK_AND_LOG(net->log_ctx, t->data_gpu != NULL, BCNN_INVALID_PARAMETER,
                       "Fill with JPEGs: tensor %d has no device buffer\n", tensor_index);
    BCNN_CHECK_AND_LOG(net->log_ctx, num_images >= 1 && num_images <= t->n, BCNN_INVALID_PARAMETER,
                       "Fill with JPEGs: %d images for a batch of %d\n", num_images, t->n);
    BCNN_CHECK_AND_LOG(net->log_ctx, t->c == 1 || t->c == 3, BCNN_INVALID_PARAMETER,
                       "Fill with JPEGs: the tensor has %d channels (a JPEG stream has 1 or 3)\n", t->c);
    BCNN_CHECK_AND_LOG(net->log_ctx, buffers && lengths, BCNN_INVALID_PARAMETER,
                       "Fill with JPEGs: NULL buffers or lengths\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, fit == BCNN_IMAGE_FIT_STRETCH || fit == BCNN_IMAGE_FIT_LETTERBOX,
                       BCNN_INVALID_PARAMETER, "Fill with JPEGs: unknown fit %d\n", fit);
    bip_jpeg_info *infos = (bip_jpeg_info *)calloc((size_t)num_images, sizeof(bip_jpeg_info));
    bcnn_hip_jpeg_frame *frames = (bcnn_hip_jpeg_frame *)calloc((size_t)num_images, sizeof(bcnn_hip_jpeg_frame));
    int16_t **coeff = (int16_t **)calloc((size_t)num_images, sizeof(int16_t *));
    bcnn_status st = BCNN_INVALID_PARAMETER;
    int failed = -1;
    if (!infos || !frames || !coeff) { st = BCNN_FAILED_ALLOC; goto done; }
    /* ---- headers: sizes and offsets of the whole batch are known before any coefficient is decoded */
    for (int b = 0; b < num_images; ++b) {
        if (!buffers[b] || bip_jpeg_frame_info(buffers[b], lengths[b], &infos[b]) != BIP_SUCCESS) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Fill with JPEGs: image %d is not a JPEG stream the decoder covers\n", b);
            failed = b;
            goto done;
        }
        if (infos[b].ncomp != t->c) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Fill with JPEGs: image %d has %d components, the tensor %d channels\n",
                     b, infos[b].ncomp, t->c);
            failed = b;
            goto done;
        }
        bcnn_jpeg_frame_from_info(&infos[b], &frames[b]);
    }
    /* ---- the staging block: refused as a whole when an extent comes out empty or the block would pass 2 GiB */
    if (bcnn_hip_jpeg_stage_begin(t->n, t->c, t->h, t->w, num_images, frames, fit, coeff, &failed) != 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Fill with JPEGs: image %d does not fit the %d x %d input (letterbox extent "
                 "of 0, or more than 2 GiB to stage)\n", failed, t->w, t->h);
        goto done;
    }
    /* ---- entropy decoding, straight into the pinned block */
    failed = bcnn_jpeg_read_batch(num_images, buffers, lengths, infos, coeff, net->num_threads);
    if (failed == -2) {
        bcnn_hip_jpeg_stage_cancel();
        failed = -1;
        st = BCNN_FAILED_ALLOC;
        goto done;
    }
    if (failed >= 0) {
        bcnn_hip_jpeg_stage_cancel();
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Fill with JPEGs: image %d cannot be decoded\n", failed);
        goto done;
    }
    /* Values a fused forward left pending for this tensor go in first (see bcnn_fill_tensor_with_images); nothing can
     * refuse the batch from here on. */
    bcnn_materialize_data(net, tensor_index);
    st = bcnn_hip_jpeg_stage_run(t->data_gpu, norm_coeff, swap_to_bgr, mean_r, mean_g, mean_b) == 0 ? BCNN_SUCCESS
                                                                                                    : BCNN_INTERNAL_ERROR;
done:
    if (failed_image) *failed_image = failed;
    free(infos);
    free(frames);
    free(coeff);
    return st;
}
