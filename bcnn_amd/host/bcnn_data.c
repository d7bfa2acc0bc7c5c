/*
 * bcnn_data.c -- dataset readers and online augmentation: the caller side of the hot path (what feeds tensors[0] / tensors[1]
 * before bcnn_forward). Reference: src/bcnn_data.c and src/data_loader/bcnn_{mnist,cifar10,classif,regression}_loader.c.
 *
 *   bcnn_set_data_loader      opens the train / test streams of one of the formats below and sizes the sample buffers
 *   bcnn_loader_next          fills one batch on the host, sample by sample, then uploads inputs (+ labels) to the device
 *                             (the reference's H2D hook, bcnn_data.c:413-425)
 *                             with bcnn_set_loader_on_device the host only reads, decodes and draws; the raw samples and one
 *                             record each go up in one copy and ../csrc/augment.hip makes the float batch (same bits);
 *                             with bcnn_set_loader_decode_on_device as well, the JPEG entries of a list batch go up as
 *                             coefficient blocks and are decoded and cropped there too (list_batch_decoded below);
 *                             with bcnn_set_loader_detection_on_device a detection-list batch goes up as the decoded images
 *                             (decoded on the net's host threads) and is resized, pasted on its canvas and augmented there
 *                             (detection_batch_device below). Nothing reads it->input_net / it->input_uchar for that loader
 *                             type between samples, so that path writes neither of them, nor tensors[0].data
 *   bcnn_augment_data_with_*  augmentation ranges; bcnn_apply_data_augmentation draws the parameters of one sample from
 *                             libc rand() in the reference's order (flip, shift, scale, rotation, contrast, brightness,
 *                             distortion, spotlights), so that a run seeded like a reference run sees the same samples byte
 *                             for byte
 *   bcnn_set_loader_effects   (bcnn_core.c) whether bcnn_loader_next applies the last two of them, or only makes their draws
 *   formats: BCNN_LOAD_MNIST (idx3 images + idx1 labels, big-endian headers), BCNN_LOAD_CIFAR10 (1 + 3072 byte records,
 *            planar RGB), BCNN_LOAD_CLASSIFICATION_LIST ("path label" lines), BCNN_LOAD_REGRESSION_LIST ("path v0 v1 ..").
 *            BCNN_LOAD_DETECTION_LIST ("path (class x y w h)*" lines: bcnn_detection_loader.c) letterboxes the image onto a
 *            canvas of 128 and moves the boxes with it; it needs detector training or a net that holds a YOLO head.
 *            BCNN_LOAD_SEGMENTATION_LIST ("image-path mask-path" lines, no reference counterpart) is read by
 *            bcnn_data_segmentation.c through the doors near the end of this file; it needs a softmax-loss node.
 *   class-index labels: on a net that holds a softmax-loss node and whose label slot is one float, the classification
 *            readers write the class index itself instead of a one-hot row (write_class_label).
 *
 * Behaviours of the reference that are kept on purpose (each is visible to a consumer that compares runs):
 *   - bcnn_augment_data_with_flip stores its flag in `apply_fliph`, the flip only happens when the INI key `flip_h` has set
 *     `random_fliph` as well, and it is then applied to EVERY sample (no draw);
 *   - bcnn_augment_data_with_distortion stores `distortion`, not `max_distortion`: it enables nothing;
 *   - a shifted or rotated sample is composed over a buffer filled with 128 / 0 respectively;
 *   - the readers wrap around at end of file, and switching to VALID / PREDICT mode rewinds the test streams.
 * One deliberate difference in the detection-list reader: the reference forms the image's aspect ratio w / h in INTEGER
 * arithmetic (bcnn_detection_loader.c:103), which gives a portrait image width 0 and stretches a 4:3 image square; here
 * the ratio is the float one. Batches and labels are the reference's whenever the height divides the width.
 * Perlin distortion and random spotlights (INI keys max_distortion / max_spots, bcnn_augment_data_with_blobs) are applied
 * by the loader behind a switch that is off by default, bcnn_set_loader_effects (`loader_effects=1`): stages 7 and 8 of
 * augment_pixels on the host, the effects kernel of ../csrc/augment.hip on the three device routes. With the switch off
 * their draws still consume rand() call for call like the reference (parameters, the distortion's own seed, four values per
 * spot), so that the other augmentations stay aligned; the image is left untouched and a warning is printed once.
 * bcnn_apply_data_augmentation, which takes no net, always applies them, like the reference's.
 */
#include <math.h>
#include <pthread.h>
#include <string.h>

#include <bh/bh_string.h>
#include <bcnn_hip.h>
#include <bip/bip.h>

#include "bcnn_internal.h"
#include "bip_resize_tap.h" /* the taps of the scale stage, tabulated here for the device path */

/* ---- augmentation ranges (reference bcnn_data.c:144-209) ---------------------------------------------------------- */
void bcnn_augment_data_with_shift(bcnn_net *net, int width_shift_range, int height_shift_range) {
    if (!net->data_aug) return;
    net->data_aug->range_shift_x = width_shift_range;
    net->data_aug->range_shift_y = height_shift_range;
}
void bcnn_augment_data_with_scale(bcnn_net *net, float min_scale, float max_scale) {
    if (!net->data_aug) return;
    net->data_aug->min_scale = min_scale;
    net->data_aug->max_scale = max_scale;
}
void bcnn_augment_data_with_rotation(bcnn_net *net, float rotation_range) {
    if (net->data_aug) net->data_aug->rotation_range = rotation_range;
}
void bcnn_augment_data_with_flip(bcnn_net *net, int horizontal_flip, int vertical_flip) {
    (void)vertical_flip;
    if (net->data_aug) net->data_aug->apply_fliph = horizontal_flip; /* sic: see the file header */
}
void bcnn_augment_data_with_color_adjustment(bcnn_net *net, int min_brightness, int max_brightness, float min_contrast,
                                             float max_contrast) {
    if (!net->data_aug) return;
    net->data_aug->min_brightness = min_brightness;
    net->data_aug->max_brightness = max_brightness;
    net->data_aug->min_contrast = min_contrast;
    net->data_aug->max_contrast = max_contrast;
}
void bcnn_augment_data_with_blobs(bcnn_net *net, int max_blobs) {
    if (net->data_aug) net->data_aug->max_random_spots = max_blobs;
}
void bcnn_augment_data_with_distortion(bcnn_net *net, float distortion) {
    if (net->data_aug) net->data_aug->distortion = distortion; /* sic */
}

/* uniform integer in [lo, hi] from one rand() draw, rounded to nearest (reference bcnn_utils.h:119-124) */
static int rand_between(int lo, int hi) {
    if (lo > hi) return 0;
    return (int)(((float)rand() / RAND_MAX * (hi - lo)) + lo + 0.5f);
}
/* one draw mapped to [-1/2, 1/2) * range and [0, 1] * (b - a) + a, in float like the reference */
static float rand_centred(float range) { return (float)(rand() - RAND_MAX / 2) / RAND_MAX * range; }
static float rand_span(float a, float b) { return ((float)rand() / RAND_MAX) * (b - a) + a; }

/* What the draws of one sample decide. The pixel work reads nothing else: augment_pixels below on the host, the kernels of
 * ../csrc/augment.hip on the device (bcnn_set_loader_on_device). */
typedef struct {
    int flip, shift, scale, rotate, contrast, brighten; /* which stages run */
    int x_ul, y_ul;                                     /* shift origin; (0, 0) without a shift */
    float scale_factor, theta, contrast_factor;
    int brightness;
    int distort;                 /* Perlin distortion runs: its offsets, its strength and the seed of its lattice */
    float kx, ky, distortion;
    int32_t seed;
    int spots;                   /* spotlights that run, in this order (0: the stage is the identity) */
    bip_spot spot[BCNN_MAX_SPOTS];
} aug_draw;

/* Draws the parameters of one sample from rand() in the reference's order and number (shift x, shift y, scale, rotation,
 * contrast, brightness, then the two effects: kx, ky, distortion, the seed bip_image_perlin_distortion draws for itself;
 * the spot count and four values per spot), leaves them in `p` as the reference does, and touches no pixel. With
 * use_precomputed the values already in `p` are taken instead. `effects` (bcnn_set_loader_effects): the draws of the two
 * effects are kept in `d` for a width x height sample; without it they are made and dropped, and the sample keeps its
 * pixels. */
static void draw_augmentation(bcnn_data_augmenter *p, aug_draw *d, int effects, int width, int height) {
    memset(d, 0, offsetof(aug_draw, spot)); /* spot[0 .. spots) is all that is read of the list */
    d->flip = p->random_fliph && p->apply_fliph;
    if (p->range_shift_x || p->range_shift_y) {
        d->shift = 1;
        if (p->use_precomputed) {
            d->x_ul = p->shift_x;
            d->y_ul = p->shift_y;
        } else {
            d->x_ul = p->shift_x = (int)rand_centred((float)p->range_shift_x);
            d->y_ul = p->shift_y = (int)rand_centred((float)p->range_shift_y);
        }
    }
    if (p->max_scale > 0.0f || p->min_scale > 0.0f) {
        d->scale = 1;
        d->scale_factor = p->use_precomputed ? p->scale : (p->scale = rand_span(p->min_scale, p->max_scale));
    }
    if (p->rotation_range > 0.0f) {
        d->rotate = 1;
        d->theta = p->use_precomputed ? p->rotation : (p->rotation = bip_deg2rad(rand_centred(p->rotation_range)));
    }
    if (p->min_contrast > 0.0f || p->max_contrast > 0.0f) {
        d->contrast = 1;
        d->contrast_factor = p->use_precomputed ? p->contrast : (p->contrast = rand_span(p->min_contrast, p->max_contrast));
    }
    if (p->min_brightness != 0 || p->max_brightness != 0) {
        d->brighten = 1;
        d->brightness = p->use_precomputed
                            ? p->brightness
                            : (p->brightness = (int)rand_span((float)p->min_brightness, (float)p->max_brightness));
    }
    /* Perlin distortion and random spotlights. Their draws are consumed exactly as the reference consumes them, kept or
     * not, so that the samples behind this one see the generator in the reference's state: three parameters (when not
     * precomputed) plus the seed bip_image_perlin_distortion draws for itself on every call (bip.c:212); the spot count
     * plus four values per spot (mu_x, mu_y, sigma_x, sigma_y: bip.c:294-298). */
    if (p->max_distortion > 0.0f) {
        if (!p->use_precomputed) {
            p->distortion_kx = ((float)rand() - RAND_MAX / 2) / RAND_MAX;
            p->distortion_ky = ((float)rand() - RAND_MAX / 2) / RAND_MAX;
            p->distortion = ((float)rand() / RAND_MAX) * p->max_distortion;
        }
        const int32_t seed = rand();
        if (effects) {
            d->distort = 1;
            d->kx = p->distortion_kx;
            d->ky = p->distortion_ky;
            d->distortion = p->distortion;
            d->seed = seed;
        }
    }
    if (p->max_random_spots > 0) {
        const int spots = rand_between(0, p->max_random_spots);
        for (int i = 0; i < spots; ++i) {
            bip_spot s; /* the callers refuse a range above BCNN_MAX_SPOTS before they draw */
            if (effects) bip_draw_spot((size_t)width, (size_t)height, 0.3f, 3.0f, 0.3f, 3.0f, i < BCNN_MAX_SPOTS ? &d->spot[i] : &s);
            else for (int k = 0; k < 4; ++k) (void)rand();
        }
        if (effects) d->spots = spots < BCNN_MAX_SPOTS ? spots : BCNN_MAX_SPOTS;
    }
    static int warned = 0;
    if (!effects && (p->max_distortion > 0.0f || p->max_random_spots > 0) && !warned) {
        warned = 1;
        fprintf(stderr, "[bcnn] max_distortion / max_spots: Perlin distortion and random spotlights are off "
                        "(bcnn_set_loader_effects, or loader_effects=1 in the [net] section, turns them on); samples keep "
                        "their pixels (the random stream stays aligned with the reference)\n");
    }
}

/* The drawn augmentation of one sample, in place. `scratch` (same size as the image) is needed by flip / shift / rotation. */
static bcnn_status augment_pixels(unsigned char *img, int width, int height, int depth, const aug_draw *d,
                                  unsigned char *scratch) {
    const size_t stride = (size_t)width * depth, bytes = stride * height;
    if (d->flip) {
        bip_fliph_image(img, width, height, depth, stride, scratch, stride);
        memcpy(img, scratch, bytes);
    }
    if (d->shift) {
        memset(scratch, 128, bytes);
        bip_crop_image(img, width, height, stride, d->x_ul, d->y_ul, scratch, width, height, stride, depth);
        memcpy(img, scratch, bytes);
    }
    if (d->scale) {
        const int ws = (int)(width * d->scale_factor), hs = (int)(height * d->scale_factor);
        unsigned char *scaled = (unsigned char *)calloc((size_t)ws * hs * depth, 1);
        if (!scaled) return BCNN_FAILED_ALLOC;
        bip_resize_bilinear(img, width, height, stride, scaled, ws, hs, (size_t)ws * depth, depth);
        /* cropped back at the shift's origin, over the unscaled image */
        bip_crop_image(scaled, ws, hs, (size_t)ws * depth, d->x_ul, d->y_ul, img, width, height, stride, depth);
        free(scaled);
    }
    if (d->rotate) {
        memset(scratch, 128, bytes);
        bip_rotate_image(img, width, height, stride, scratch, width, height, stride, depth, d->theta, width / 2, height / 2,
                         BILINEAR);
        memcpy(img, scratch, bytes);
    }
    if (d->contrast) bip_contrast_stretch(img, stride, width, height, depth, img, stride, d->contrast_factor);
    if (d->brighten) bip_image_brightness(img, stride, width, height, depth, img, stride, d->brightness);
    if (d->distort) { /* reads img, writes another image: into the scratch and back */
        unsigned char *out = scratch ? scratch : (unsigned char *)malloc(bytes);
        if (!out) return BCNN_FAILED_ALLOC;
        bip_perlin_distortion_seeded(img, stride, width, height, depth, out, stride, d->distortion, d->kx, d->ky, d->seed);
        memcpy(img, out, bytes);
        if (!scratch) free(out);
    }
    if (d->spots > 0) bip_add_spotlights(img, stride, width, height, depth, img, stride, d->spot, (uint32_t)d->spots);
    return BCNN_SUCCESS;
}

/* One sample, in place: the draws, then the pixels. The reference's function in full: it takes no net, so both effects
 * run whenever their range is set. The loader does not come through here (augment_if_training). */
bcnn_status bcnn_apply_data_augmentation(unsigned char *img, int width, int height, int depth, bcnn_data_augmenter *p,
                                         unsigned char *scratch) {
    if (p->max_random_spots > BCNN_MAX_SPOTS) return BCNN_INVALID_PARAMETER; /* before any draw */
    aug_draw d;
    draw_augmentation(p, &d, 1, width, height);
    return augment_pixels(img, width, height, depth, &d, scratch);
}

/* ---- streams ------------------------------------------------------------------------------------------------------ */
static FILE *open_stream(bcnn_net *net, const char *path, bcnn_status *st) {
    if (!path) return NULL;
    FILE *f = fopen(path, "rb");
    if (!f) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Could not open file %s\n", path);
        *st = BCNN_INVALID_PARAMETER;
    }
    return f;
}

/* TRAIN mode reads the train streams, every other mode the test streams (reference bcnn_data.c:493-543) */
static bcnn_status select_streams(bcnn_net *net, bcnn_loader *it, int rewind_test) {
    const int train = net->mode == BCNN_MODE_TRAIN;
    if (!train && rewind_test) { /* every evaluation run sees the same samples */
        if (!it->f_test || fseek(it->f_test, 0L, SEEK_SET) != 0) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Could not rewind test dataset file\n");
            return BCNN_INVALID_DATA;
        }
        if (it->has_extra_data && (!it->f_test_extra || fseek(it->f_test_extra, 0L, SEEK_SET) != 0)) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Could not rewind extra test dataset file\n");
            return BCNN_INVALID_DATA;
        }
    }
    it->f_current = train ? it->f_train : it->f_test;
    it->f_current_extra = it->has_extra_data ? (train ? it->f_train_extra : it->f_test_extra) : NULL;
    if (!it->f_current || (it->has_extra_data && !it->f_current_extra)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "A %s dataset must be provided\n", train ? "training" : "testing");
        return BCNN_INVALID_DATA;
    }
    return BCNN_SUCCESS;
}

bcnn_status bcnn_open_dataset(bcnn_loader *it, bcnn_net *net, const char *train_path, const char *train_path_extra,
                              const char *test_path, const char *test_path_extra, bool has_extra) {
    bcnn_status st = BCNN_SUCCESS;
    it->f_train = open_stream(net, train_path, &st);
    it->f_test = open_stream(net, test_path, &st);
    if (has_extra) {
        it->f_train_extra = open_stream(net, train_path_extra, &st);
        it->f_test_extra = open_stream(net, test_path_extra, &st);
    }
    if (st != BCNN_SUCCESS) return st;
    it->has_extra_data = has_extra;
    return select_streams(net, it, 0);
}

bcnn_status bcnn_switch_data_handles(bcnn_net *net, bcnn_loader *it) { return select_streams(net, it, 1); }

/* at end of file start over; otherwise stay where we are (the readers peek one byte) */
static void wrap_at_eof(FILE *f) {
    unsigned char probe;
    if (fread(&probe, 1, 1, f) == 0) rewind(f);
    else fseek(f, -1, SEEK_CUR);
}

/* ---- the batch on the device (bcnn_set_loader_on_device) ------------------------------------------------------------ */
/* While a device-mode bcnn_loader_next runs, the readers below hand each raw sample and its draws to this block instead of
 * augmenting and converting it; bcnn_hip_augment_batch then makes the float batch on the device. Grow-only, owned by the
 * net's device context. */
typedef struct {
    uint8_t *pixels;                  /* batch x (w * h * c) raw samples */
    bcnn_hip_augment_record *records; /* batch */
    int32_t *taps;                    /* batch x (w + h) (index, fraction) pairs; written for samples that scale */
    aug_draw *draws;                  /* batch: what the records were made from (the effects' tables, the host fallback) */
    size_t cap_bytes, cap_records, cap_taps;
    int w, h, c;                      /* the stored sample of the batch being gathered */
    int active;                       /* inside a device-mode bcnn_loader_next */
    /* List loaders: a file that fails to decode leaves the sample buffer as it was, and the reference then augments and
     * converts that buffer again. On the host path the buffer holds the previous sample AUGMENTED; on the device path it
     * holds it raw, and `owed` remembers the pixel work that makes the two equal should a decode fail next. */
    int owed;
    aug_draw owed_draw;
    int refused; /* the device side refused this batch's effects: bcnn_loader_next makes it on the host */
    /* bcnn_set_loader_decode_on_device. Per sample of the batch being gathered: 1 = its pixels are made on the device, and
     * the origin of its crop window there. A device-decoded sample leaves no pixels on the host, so `lazy` keeps what
     * rebuilds the latest one in it->input_uchar should a decode fail next: the file's bytes and the crop origin. */
    uint8_t *decoded;
    int32_t *origins;
    uint8_t *lazy;
    size_t lazy_len;
    int lazy_x, lazy_y;
} loader_stage;

static loader_stage *stage_of(bcnn_net *net) { return (loader_stage *)((bcnn_hip_context *)net->hip_ctx)->loader_stage; }

void bcnn_free_loader_stage(bcnn_net *net) {
    loader_stage *ls = stage_of(net);
    if (!ls) return;
    free(ls->pixels); free(ls->records); free(ls->taps); free(ls->draws); free(ls->decoded); free(ls->origins); free(ls->lazy);
    free(ls);
    ((bcnn_hip_context *)net->hip_ctx)->loader_stage = NULL;
}

/* w x h x c window of the decoded wi x hi image at (x_ul, y_ul) into img, zero outside the image; a plain copy when the
 * extents are equal (reference bcnn_data.c:352-372) */
static bcnn_status crop_to_input(unsigned char *buf, int wi, int hi, int x_ul, int y_ul, unsigned char *img, int w, int h,
                                 int c) {
    if (wi == w && hi == h) {
        memcpy(img, buf, (size_t)w * h * c);
        return BCNN_SUCCESS;
    }
    unsigned char *crop = (unsigned char *)calloc((size_t)w * h * c, 1);
    if (!crop) return BCNN_FAILED_ALLOC;
    bip_crop_image(buf, wi, hi, (size_t)wi * c, x_ul, y_ul, crop, w, h, (size_t)w * c, c);
    memcpy(img, crop, (size_t)w * h * c);
    free(crop);
    return BCNN_SUCCESS;
}

static void drop_lazy(loader_stage *ls) {
    free(ls->lazy);
    ls->lazy = NULL;
    ls->lazy_len = 0;
}

/* Before the sample buffer is used "as it was": the pixels a device-decoded sample would have left in it, then the pixel
 * work owed to it. */
static void settle_owed(bcnn_net *net, bcnn_loader *it) {
    loader_stage *ls = stage_of(net);
    if (!ls) return;
    bcnn_tensor *in = &net->tensors[0];
    if (ls->lazy) {
        int wi = 0, hi = 0, ci = 0;
        unsigned char *buf = NULL;
        bip_load_image_from_memory(ls->lazy, (int)ls->lazy_len, &buf, &wi, &hi, &ci);
        if (buf && wi > 0 && hi > 0 && ci == in->c)
            crop_to_input(buf, wi, hi, ls->lazy_x, ls->lazy_y, it->input_uchar, in->w, in->h, in->c);
        free(buf);
        drop_lazy(ls);
    }
    if (!ls->owed) return;
    ls->owed = 0;
    unsigned char *scratch = (unsigned char *)calloc((size_t)bcnn_tensor_size3d(in), 1);
    if (scratch) augment_pixels(it->input_uchar, in->w, in->h, in->c, &ls->owed_draw, scratch);
    free(scratch);
}

/* Sizes the block for one batch of w x h x c samples; NULL when this batch has to go the host way: no device input
 * tensor, more than 4 channels (bip_resize_bilinear's limit, and the kernels'), or a stored sample that does not match
 * the net input. */
static loader_stage *stage_begin(bcnn_net *net, bcnn_loader *it) {
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    bcnn_tensor *in = &net->tensors[0];
    if (it->type == BCNN_LOAD_DETECTION_LIST) return NULL; /* no block of equal samples: detection_batch_device, or the host */
    if (!hc->loader_on_device || !in->data_gpu || in->c < 1 || in->c > 4 || net->batch_size < 1 || in->n < net->batch_size)
        return NULL;
    const int stored = it->type == BCNN_LOAD_MNIST || it->type == BCNN_LOAD_CIFAR10;
    if (stored && (it->input_depth != in->c || it->input_width < in->w || it->input_height < in->h)) return NULL;
    if (!hc->loader_stage) hc->loader_stage = calloc(1, sizeof(loader_stage));
    loader_stage *ls = (loader_stage *)hc->loader_stage;
    if (!ls) return NULL;
    ls->w = stored ? it->input_width : in->w;
    ls->h = stored ? it->input_height : in->h;
    ls->c = in->c;
    const size_t n = (size_t)net->batch_size, bytes = n * ls->w * ls->h * ls->c, taps = n * ((size_t)ls->w + ls->h) * 2;
    if (ls->cap_bytes < bytes) {
        free(ls->pixels);
        ls->pixels = (uint8_t *)calloc(bytes, 1);
        ls->cap_bytes = ls->pixels ? bytes : 0;
    }
    if (ls->cap_records < n) {
        free(ls->records); free(ls->decoded); free(ls->origins); free(ls->draws);
        ls->records = (bcnn_hip_augment_record *)calloc(n, sizeof(bcnn_hip_augment_record));
        ls->decoded = (uint8_t *)calloc(n, 1);
        ls->origins = (int32_t *)calloc(2 * n, sizeof(int32_t));
        ls->draws = (aug_draw *)calloc(n, sizeof(aug_draw));
        ls->cap_records = (ls->records && ls->decoded && ls->origins && ls->draws) ? n : 0;
    }
    if (ls->cap_taps < taps) {
        free(ls->taps);
        ls->taps = (int32_t *)calloc(taps, sizeof(int32_t));
        ls->cap_taps = ls->taps ? taps : 0;
    }
    if (!ls->pixels || !ls->cap_records || !ls->taps) return NULL;
    ls->active = 1;
    return ls;
}

/* What the device needs of one sample's draws. Every float -> integer step is the host's own expression: ws / hs as
 * bcnn_apply_data_augmentation forms them, the taps of bip_resize_bilinear, ca / sa of bip_rotate_image, the gain of
 * bip_contrast_stretch. A scale draw that leaves ws < 1 or hs < 1 resizes to nothing on the host (calloc(0), then
 * bip_resize_bilinear refuses the empty extent and the paste copies no byte): the stage is left out. */
static void fill_record(bcnn_hip_augment_record *r, int32_t *taps, const aug_draw *d, int w, int h) {
    memset(r, 0, sizeof(*r));
    if (d->flip) r->flags |= BCNN_HIP_AUG_FLIP;
    if (d->shift) {
        r->flags |= BCNN_HIP_AUG_SHIFT;
        r->x_ul = d->x_ul;
        r->y_ul = d->y_ul;
    }
    if (d->scale) {
        const int ws = (int)(w * d->scale_factor), hs = (int)(h * d->scale_factor);
        if (ws >= 1 && hs >= 1) {
            r->flags |= BCNN_HIP_AUG_SCALE;
            /* the resized image is pasted back at (x_ul, y_ul): column x of the sample shows its column x + x_ul */
            const float xs = bip_resize_scale((size_t)w, (size_t)ws), ys = bip_resize_scale((size_t)h, (size_t)hs);
            for (int x = 0; x < w; ++x) {
                const long long X = (long long)x + d->x_ul;
                taps[2 * x] = -1;
                taps[2 * x + 1] = 0;
                if (X >= 0 && X < ws) bip_resize_tap((size_t)X, xs, (size_t)w, &taps[2 * x], &taps[2 * x + 1]);
            }
            int32_t *ty = taps + 2 * (size_t)w;
            for (int y = 0; y < h; ++y) {
                const long long Y = (long long)y + d->y_ul;
                ty[2 * y] = -1;
                ty[2 * y + 1] = 0;
                if (Y >= 0 && Y < hs) bip_resize_tap((size_t)Y, ys, (size_t)h, &ty[2 * y], &ty[2 * y + 1]);
            }
        }
    }
    if (d->rotate) {
        r->flags |= BCNN_HIP_AUG_ROTATE;
        r->ca = (int32_t)(cos(d->theta) * 65536);
        r->sa = (int32_t)(sin(d->theta) * 65536);
    }
    if (d->contrast) {
        r->flags |= BCNN_HIP_AUG_CONTRAST;
        r->gain = (int32_t)(d->contrast_factor * (1 << 12) + 0.5);
    }
    if (d->brighten) r->brightness = d->brightness;
}

static int effects_on(const bcnn_net *net) { return ((const bcnn_hip_context *)net->hip_ctx)->loader_effects; }

/* How far from its centre a spotlight of the loader can change a byte. The loader draws sigma in [0.3 + 0.5, 3.0 + 0.5]
 * (bip_draw_spot; the float sums may round up by an ulp: sigma^2 <= 12.2500015). At |dx| >= 12 or |dy| >= 12 the exponent is
 * <= -0.5 * 144 / 12.2500015 = -5.877, so val <= exp(-5.877) = 0.00281 and 255 * val <= 0.716: added to a byte d in fp32
 * (ulp <= 2^-16 there) the sum stays below d + 1 and truncates to d again, and a sum above 255 is clamped to 255 = d. The
 * farthest pixel that does change is at distance 11 (255 * exp(-0.5 * 121 / 12.25) = 1.83). So the device gets `val` over
 * the box of radius 12 only; tests/test_augment_effects.py holds the table form to the full-image form. */
#define BCNN_SPOT_RADIUS 12
#define BCNN_SPOT_BOX ((2 * BCNN_SPOT_RADIUS + 1) * (2 * BCNN_SPOT_RADIUS + 1))

/* Stages the effects of the batch whose n draws lie `stride` bytes apart from `first` on, for the batch call that follows
 * (bcnn_hip_augment_effects_begin): every cos and exp is made here, with libm. 0: no sample of the batch has an effect,
 * nothing is staged; 1: staged; -1: refused -- the caller makes this batch on the host from the same draws. */
static int stage_effects(const void *first, size_t stride, int n, int w, int h) {
    size_t spots = 0, distorted = 0;
    for (int i = 0; i < n; ++i) {
        const aug_draw *d = (const aug_draw *)((const char *)first + (size_t)i * stride);
        spots += (size_t)d->spots;
        distorted += d->distort ? 1 : 0;
    }
    if (spots == 0 && distorted == 0) return 0;
    const size_t axis = (size_t)w + h;
    bcnn_hip_augment_effect *fx = (bcnn_hip_augment_effect *)calloc((size_t)n, sizeof(*fx));
    float *perlin = (float *)calloc(distorted ? (size_t)n * axis * 2 : 1, sizeof(float));
    int32_t *cells = (int32_t *)calloc(distorted ? (size_t)n * axis : 1, sizeof(int32_t));
    bcnn_hip_augment_spot *sp = (bcnn_hip_augment_spot *)calloc(spots ? spots : 1, sizeof(*sp));
    float *tables = (float *)calloc(spots ? spots * BCNN_SPOT_BOX : 1, sizeof(float));
    int rc = (fx && perlin && cells && sp && tables) ? 1 : -1;
    size_t at = 0, floats = 0;
    for (int i = 0; rc == 1 && i < n; ++i) {
        const aug_draw *d = (const aug_draw *)((const char *)first + (size_t)i * stride);
        if (d->distort) {
            fx[i].flags |= BCNN_HIP_AUG_DISTORT;
            fx[i].seed = d->seed;
            fx[i].distortion = d->distortion;
            float *norm = perlin + (size_t)i * axis * 2, *weight = norm + axis;
            bip_perlin_axis((size_t)w, d->kx, norm, weight, cells + (size_t)i * axis);
            bip_perlin_axis((size_t)h, d->ky, norm + w, weight + w, cells + (size_t)i * axis + w);
        }
        if (d->spots > 0) {
            fx[i].flags |= BCNN_HIP_AUG_SPOTS;
            fx[i].first_spot = (int32_t)at;
            fx[i].num_spots = d->spots;
            for (int s = 0; s < d->spots; ++s, ++at) {
                int32_t box[4];
                if (bip_spot_table(&d->spot[s], (size_t)w, (size_t)h, BCNN_SPOT_RADIUS, box, tables + floats) != BIP_SUCCESS) {
                    rc = -1;
                    break;
                }
                sp[at].x0 = box[0]; sp[at].y0 = box[1]; sp[at].bw = box[2]; sp[at].bh = box[3];
                sp[at].table = (uint32_t)floats;
                floats += (size_t)box[2] * box[3];
            }
        }
    }
    if (rc == 1 && bcnn_hip_augment_effects_begin(n, w, h, fx, perlin, cells, sp, (int)spots, tables, floats) != 0) rc = -1;
    free(fx); free(perlin); free(cells); free(sp); free(tables);
    return rc;
}

/* Slot idx of the block gets this sample's draws (TRAIN mode) or the identity record. */
static void stage_draws(bcnn_net *net, loader_stage *ls, int idx, int w, int h, int list_loader) {
    bcnn_hip_augment_record *r = &ls->records[idx];
    memset(r, 0, sizeof(*r));
    ls->owed = 0;
    if (!(net->mode == BCNN_MODE_TRAIN && net->data_aug)) {
        memset(&ls->draws[idx], 0, offsetof(aug_draw, spot)); /* the identity */
    } else {
        aug_draw *d = &ls->draws[idx];
        draw_augmentation(net->data_aug, d, effects_on(net), w, h);
        fill_record(r, ls->taps + (size_t)idx * ((size_t)w + h) * 2, d, w, h);
        if (list_loader) {
            ls->owed = 1;
            ls->owed_draw = *d;
        }
    }
}

/* The loader's sample buffer into slot idx of the block, with its draws. */
static bcnn_status stage_sample(bcnn_net *net, bcnn_loader *it, loader_stage *ls, int idx, int w, int h, int c,
                                int list_loader) {
    if (w != ls->w || h != ls->h || c != ls->c || idx < 0 || (size_t)idx >= ls->cap_records) return BCNN_INVALID_DATA;
    const size_t bytes = (size_t)w * h * c;
    memcpy(ls->pixels + (size_t)idx * bytes, it->input_uchar, bytes);
    stage_draws(net, ls, idx, w, h, list_loader);
    return BCNN_SUCCESS;
}

/* ---- sample -> tensors ---------------------------------------------------------------------------------------------- */
static int needs_scratch(const bcnn_data_augmenter *a, int list_loader, int effects) {
    if (a->range_shift_x != 0 || a->range_shift_y != 0 || a->random_fliph != 0) return 1;
    if (list_loader) return a->rotation_range > 0.0f || a->max_random_spots > 0 || a->max_distortion > 0.0f;
    if (effects && (a->max_random_spots > 0 || a->max_distortion > 0.0f)) return 1;
    return a->rotation_range != 0;
}

/* The loader's own pair of steps: the draws, with the net's effects switch, then the pixels. */
static bcnn_status augment_if_training(bcnn_net *net, unsigned char *img, int w, int h, int c, int list_loader) {
    if (net->mode != BCNN_MODE_TRAIN || !net->data_aug) return BCNN_SUCCESS;
    unsigned char *scratch = NULL;
    if (needs_scratch(net->data_aug, list_loader, effects_on(net))) {
        scratch = (unsigned char *)calloc((size_t)w * h * c, 1);
        if (!scratch) return BCNN_FAILED_ALLOC;
    }
    aug_draw d;
    draw_augmentation(net->data_aug, &d, effects_on(net), w, h);
    const bcnn_status st = augment_pixels(img, w, h, c, &d, scratch);
    free(scratch);
    return st;
}

/* The batch the device side refused (bcnn_hip_augment_effects_begin), made on the host from the raw samples and the draws
 * the block holds: pixel step, centre crop of a stored-size sample, conversion into tensors[0].data, which the caller
 * then uploads. */
static bcnn_status host_batch_from_stage(bcnn_net *net, loader_stage *ls, int list_loader) {
    bcnn_tensor *in = &net->tensors[0];
    const size_t bytes = (size_t)ls->w * ls->h * ls->c, out = (size_t)bcnn_tensor_size3d(in);
    unsigned char *scratch = (unsigned char *)calloc(bytes + out, 1);
    if (!scratch) return BCNN_FAILED_ALLOC;
    bcnn_status st = BCNN_SUCCESS;
    for (int i = 0; i < net->batch_size && st == BCNN_SUCCESS; ++i) {
        unsigned char *img = ls->pixels + (size_t)i * bytes;
        st = augment_pixels(img, ls->w, ls->h, ls->c, &ls->draws[i], scratch);
        if (in->w < ls->w || in->h < ls->h) {
            bip_crop_image(img, ls->w, ls->h, (size_t)ls->w * ls->c, (ls->w - in->w) / 2, (ls->h - in->h) / 2, scratch + bytes,
                           in->w, in->h, (size_t)in->w * in->c, in->c);
            img = scratch + bytes;
        }
        bcnn_convert_img_to_float(img, in->w, in->h, in->c, 1 / 127.5f,
                                  list_loader && net->data_aug ? net->data_aug->swap_to_bgr : 0, 127.5f, 127.5f, 127.5f,
                                  in->data + (size_t)i * out);
    }
    free(scratch);
    return st;
}

/* the stored-size sample (MNIST / CIFAR) into input slot idx: centre crop when the net input is smaller, [-1, 1] floats */
static void sample_to_input(bcnn_net *net, bcnn_loader *it, int idx) {
    bcnn_tensor *in = &net->tensors[0];
    float *x = in->data + (size_t)idx * bcnn_tensor_size3d(in);
    const unsigned char *img = it->input_uchar;
    if (in->w < it->input_width || in->h < it->input_height) {
        bip_crop_image(it->input_uchar, it->input_width, it->input_height, (size_t)it->input_width * it->input_depth,
                       (it->input_width - in->w) / 2, (it->input_height - in->h) / 2, it->input_net, in->w, in->h,
                       (size_t)in->w * in->c, in->c);
        img = it->input_net;
    }
    bcnn_convert_img_to_float(img, in->w, in->h, in->c, 1 / 127.5f, 0, 127.5f, 127.5f, 127.5f, x);
}

static float *label_slot(bcnn_net *net, int idx, int *label_sz) {
    bcnn_tensor *lab = &net->tensors[1];
    *label_sz = bcnn_tensor_size3d(lab);
    float *y = lab->data + (size_t)idx * *label_sz;
    memset(y, 0, (size_t)*label_sz * sizeof(float));
    return y;
}

static int has_softmax_loss(const bcnn_net *net) {
    for (int i = 0; i < net->num_nodes; ++i)
        if (net->nodes[i].type == BCNN_LAYER_SOFTMAX_LOSS) return 1;
    return 0;
}

/* The label of a classification sample into slot idx: a one-hot row (a class outside the row leaves it zero), or, on a net
 * that holds a softmax-loss node and whose slot is one float ([n][1][1][1]), the class index itself, as that node reads it
 * (a negative class is written as is: the node counts it as out of range). */
static void write_class_label(bcnn_net *net, int idx, int cls) {
    int sz;
    float *y = label_slot(net, idx, &sz);
    const bcnn_tensor *lab = &net->tensors[1];
    if (sz == 1 && lab->c == 1 && lab->h == 1 && lab->w == 1 && has_softmax_loss(net)) y[0] = (float)cls;
    else if (cls >= 0 && cls < sz) y[cls] = 1;
}

static bcnn_status check_input_shape(bcnn_net *net) {
    if (net->tensors[0].w > 0 && net->tensors[0].h > 0 && net->tensors[0].c > 0) return BCNN_SUCCESS;
    bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Input's width, height and channels must be > 0\n");
    return BCNN_INVALID_PARAMETER;
}

/* ---- MNIST: idx3-ubyte images + idx1-ubyte labels (bcnn_mnist_loader.c) ------------------------------------------- */
static uint32_t be32(const unsigned char *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

static bcnn_status mnist_header(bcnn_net *net, bcnn_loader *it) {
    unsigned char h[16];
    if (fread(h, 1, 16, it->f_current) != 16) goto corrupt;
    const uint32_t images = be32(h + 4);
    it->input_height = (int)be32(h + 8);
    it->input_width = (int)be32(h + 12);
    /* the sample buffer is sized from these two and the network input is cut out of it: neither can be empty or absurd, and
     * the input cannot be larger than the stored sample (the reference reads past the sample there) */
    if (it->input_height < 1 || it->input_width < 1 || it->input_height > 4096 || it->input_width > 4096 ||
        net->tensors[0].h > it->input_height || net->tensors[0].w > it->input_width) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Mnist header: %d x %d samples do not fit the %d x %d network input\n",
                 it->input_width, it->input_height, net->tensors[0].w, net->tensors[0].h);
        return BCNN_INVALID_DATA;
    }
    if (fread(h, 1, 8, it->f_current_extra) != 8) goto corrupt;
    if (images != be32(h + 4)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR,
                 "Inconsistent MNIST data: number of images and labels must be the same\n");
        return BCNN_INVALID_DATA;
    }
    return BCNN_SUCCESS;
corrupt:
    bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Corrupted Mnist data\n");
    return BCNN_INVALID_DATA;
}

static bcnn_status mnist_init(bcnn_loader *it, bcnn_net *net, const char *a, const char *b, const char *c, const char *d) {
    BCNN_CHECK_STATUS(bcnn_open_dataset(it, net, a, b, c, d, true));
    BCNN_CHECK_STATUS(check_input_shape(net));
    BCNN_CHECK_STATUS(mnist_header(net, it));
    it->input_depth = 1;
    it->input_uchar = (uint8_t *)calloc((size_t)it->input_width * it->input_height, 1);
    it->input_net = (uint8_t *)calloc((size_t)bcnn_tensor_size3d(&net->tensors[0]), 1);
    rewind(it->f_current);
    rewind(it->f_current_extra);
    return (it->input_uchar && it->input_net) ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
}

static bcnn_status mnist_next(bcnn_loader *it, bcnn_net *net, int idx) {
    wrap_at_eof(it->f_current);
    wrap_at_eof(it->f_current_extra);
    if (ftell(it->f_current) == 0 && ftell(it->f_current_extra) == 0) BCNN_CHECK_STATUS(mnist_header(net, it));
    unsigned char label;
    const size_t sz = (size_t)it->input_width * it->input_height;
    if (fread(&label, 1, 1, it->f_current_extra) != 1 || fread(it->input_uchar, 1, sz, it->f_current) != sz) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Corrupted Mnist data\n");
        return BCNN_INVALID_DATA;
    }
    loader_stage *ls = stage_of(net);
    if (ls && ls->active) {
        BCNN_CHECK_STATUS(stage_sample(net, it, ls, idx, it->input_width, it->input_height, it->input_depth, 0));
    } else {
        BCNN_CHECK_STATUS(augment_if_training(net, it->input_uchar, it->input_width, it->input_height, it->input_depth, 0));
        sample_to_input(net, it, idx);
    }
    if (net->mode != BCNN_MODE_PREDICT) write_class_label(net, idx, (int)label);
    return BCNN_SUCCESS;
}

/* ---- CIFAR-10 binary batches: {label, 1024 R, 1024 G, 1024 B} records (bcnn_cifar10_loader.c) --------------------- */
static bcnn_status cifar10_init(bcnn_loader *it, bcnn_net *net, const char *a, const char *b, const char *c,
                                const char *d) {
    BCNN_CHECK_STATUS(bcnn_open_dataset(it, net, a, b, c, d, false));
    it->input_width = it->input_height = 32;
    it->input_depth = 3;
    it->input_uchar = (uint8_t *)calloc(32 * 32 * 3, 1);
    BCNN_CHECK_STATUS(check_input_shape(net));
    it->input_net = (uint8_t *)calloc((size_t)bcnn_tensor_size3d(&net->tensors[0]), 1);
    return (it->input_uchar && it->input_net) ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
}

static bcnn_status cifar10_next(bcnn_loader *it, bcnn_net *net, int idx) {
    unsigned char rec[1 + 3072];
    wrap_at_eof(it->f_current);
    if (fread(rec, 1, sizeof(rec), it->f_current) != sizeof(rec)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Corrupted Cifar data\n");
        return BCNN_INVALID_DATA;
    }
    for (int k = 0; k < 3; ++k) /* planar -> interleaved */
        for (int p = 0; p < 1024; ++p) it->input_uchar[p * 3 + k] = rec[1 + k * 1024 + p];
    loader_stage *ls = stage_of(net);
    if (ls && ls->active) {
        BCNN_CHECK_STATUS(stage_sample(net, it, ls, idx, 32, 32, 3, 0));
    } else {
        BCNN_CHECK_STATUS(augment_if_training(net, it->input_uchar, 32, 32, 3, 0));
        sample_to_input(net, it, idx);
    }
    if (net->mode != BCNN_MODE_PREDICT) write_class_label(net, idx, (int)rec[0]);
    return BCNN_SUCCESS;
}

/* ---- list files: one "image-path label..." line per sample (bcnn_classif_loader.c, bcnn_regression_loader.c) ----- */
static bcnn_status list_init(bcnn_loader *it, bcnn_net *net, const char *a, const char *b, const char *c, const char *d) {
    BCNN_CHECK_STATUS(bcnn_open_dataset(it, net, a, b, c, d, false));
    BCNN_CHECK_STATUS(check_input_shape(net));
    it->input_uchar = (uint8_t *)calloc((size_t)bcnn_tensor_size3d(&net->tensors[0]), 1);
    return it->input_uchar ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
}

/* where a decoded wi x hi image is cropped to the w x h net input: at a random origin for training (two draws, or none
 * where the range is negative), centred for evaluation; (0, 0) and no draw when the extents are equal */
static void crop_origin(bcnn_net *net, int wi, int hi, int w, int h, int *x_ul, int *y_ul) {
    *x_ul = *y_ul = 0;
    if (wi == w && hi == h) return;
    if (net->mode == BCNN_MODE_TRAIN) {
        *x_ul = rand_between(0, wi - w);
        *y_ul = rand_between(0, hi - h);
    } else {
        *x_ul = (wi - w) / 2;
        *y_ul = (hi - h) / 2;
    }
}

/* the decoded file (buf is freed here) cropped to the net input */
static bcnn_status place_decoded(bcnn_net *net, const char *path, unsigned char *buf, int wi, int hi, int ci, int w, int h,
                                 int c, unsigned char *img, int *x_shift, int *y_shift) {
    int x_ul = 0, y_ul = 0;
    if (!(wi > 0 && hi > 0 && buf)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid image %s\n", path);
        free(buf);
        return BCNN_INVALID_DATA;
    }
    if (c != ci) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Unexpected number of channels of image %s\n", path);
        free(buf);
        return BCNN_INVALID_DATA;
    }
    crop_origin(net, wi, hi, w, h, &x_ul, &y_ul);
    const bcnn_status st = crop_to_input(buf, wi, hi, x_ul, y_ul, img, w, h, c);
    free(buf);
    if (st != BCNN_SUCCESS) return st;
    if (x_shift && y_shift) { *x_shift = x_ul; *y_shift = y_ul; }
    return BCNN_SUCCESS;
}

/* decodes the file, crops it to the net input (centred for evaluation, at a random origin for training) */
static bcnn_status load_image(bcnn_net *net, char *path, int w, int h, int c, unsigned char *img, int *x_shift,
                              int *y_shift) {
    int wi = 0, hi = 0, ci = 0;
    unsigned char *buf = NULL;
    bip_load_image(path, &buf, &wi, &hi, &ci);
    return place_decoded(net, path, buf, wi, hi, ci, w, h, c, img, x_shift, y_shift);
}

/* reference bcnn_fill_input_tensor (bcnn_data.c:336-377): a sample that fails to decode leaves the buffer as it was */
void bcnn_fill_input_tensor(bcnn_net *net, bcnn_loader *it, char *path_img, int idx) {
    bcnn_tensor *in = &net->tensors[0];
    loader_stage *ls = stage_of(net);
    if (load_image(net, path_img, in->w, in->h, in->c, it->input_uchar, net->data_aug ? &net->data_aug->shift_x : NULL,
                   net->data_aug ? &net->data_aug->shift_y : NULL) != BCNN_SUCCESS)
        settle_owed(net, it); /* the buffer as the host path would have left it */
    else if (ls) {
        ls->owed = 0;
        drop_lazy(ls);
    }
    if (ls && ls->active) {
        stage_sample(net, it, ls, idx, in->w, in->h, in->c, 1);
        return;
    }
    if (net->data_aug) augment_if_training(net, it->input_uchar, in->w, in->h, in->c, 1);
    bcnn_convert_img_to_float(it->input_uchar, in->w, in->h, in->c, 1 / 127.5f, net->data_aug ? net->data_aug->swap_to_bgr : 0,
                              127.5f, 127.5f, 127.5f, in->data + (size_t)idx * bcnn_tensor_size3d(in));
}

static void free_tokens(char **tok, int n) {
    for (int i = 0; i < n; ++i) free(tok[i]);
    free(tok);
}

/* next line split at blanks, wrapping around once at end of file (reference bh_fsplitline) */
static int next_line_tokens(FILE *f, char ***tok) {
    char *line = bh_fgetline(f);
    if (!line) {
        rewind(f);
        line = bh_fgetline(f);
        if (!line) return 0;
    }
    char **t = NULL;
    const int n = bh_strsplit(line, ' ', &t);
    free(line);
    if (!t || n == 0) { free(t); return 0; }
    *tok = t;
    return n;
}

static bcnn_status list_classif_next(bcnn_loader *it, bcnn_net *net, int idx) {
    char **tok = NULL;
    const int n = next_line_tokens(it->f_current, &tok);
    if (n <= 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid regression format\n"); /* the reference's wording */
        return BCNN_INVALID_DATA;
    }
    if (net->mode != BCNN_MODE_PREDICT && n != 2) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unexpected classif format. Found label size of %d, expected %d.\n", n - 1, 1);
        free_tokens(tok, n);
        return BCNN_INVALID_DATA;
    }
    bcnn_fill_input_tensor(net, it, tok[0], idx);
    if (net->mode != BCNN_MODE_PREDICT) write_class_label(net, idx, atoi(tok[1]));
    free_tokens(tok, n);
    return BCNN_SUCCESS;
}

static bcnn_status list_reg_next(bcnn_loader *it, bcnn_net *net, int idx) {
    char **tok = NULL;
    const int n = next_line_tokens(it->f_current, &tok);
    if (n <= 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid regression format\n");
        return BCNN_INVALID_DATA;
    }
    bcnn_fill_input_tensor(net, it, tok[0], idx);
    if (net->mode != BCNN_MODE_PREDICT) {
        int sz;
        float *y = label_slot(net, idx, &sz);
        if (n - 1 != sz)
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unexpected label format. Found label size of %d, expected %d.\n", n - 1, sz);
        for (int i = 0; i < n - 1 && i < sz; ++i) y[i] = (float)atof(tok[i + 1]);
    }
    free_tokens(tok, n);
    return BCNN_SUCCESS;
}

/* ---- a list batch whose JPEG entries are decoded on the device (bcnn_set_loader_decode_on_device) --------------------- */
/* The batch in three phases instead of sample by sample, because the number of rand() draws of a sample depends on
 * whether its file decoded, and the entropy decoding of the whole batch runs in parallel in between:
 *   1 (serial)   lines are accepted or skipped by their token count as list_classif_next / list_reg_next do, labels are
 *                written, every file is read whole and its JPEG header parsed; a stream whose component count is the
 *                input's and whose frame fits the staging block is a device candidate;
 *   2 (parallel) the candidates' coefficients straight into the pinned staging block, a status per image;
 *   3 (serial)   in batch order, per sample: a file that is no candidate, or whose coefficients failed, is decoded here
 *                as load_image does; a decoded sample draws its crop origin, then the augmentation; a failed one goes
 *                the "buffer as it was" way. Only the pixels of a device-decoded sample stay away from the host.
 * One copy and at most four launches follow (bcnn_hip_augment_jpeg_run); *launched is 0 when no sample ended up decoded
 * on the device and the caller stages the batch as usual. */
typedef struct {
    char **paths;
    uint8_t **bytes; /* the files, whole; NULL: unreadable */
    size_t *lengths;
    bip_jpeg_info *infos;
    bcnn_hip_jpeg_frame *frames; /* ncomp 0: not a device candidate */
    int16_t **coeff;
    int *status;
} list_batch;

static void list_batch_free(list_batch *lb, int n) {
    for (int i = 0; i < n; ++i) {
        if (lb->paths) free(lb->paths[i]);
        if (lb->bytes) free(lb->bytes[i]);
    }
    free(lb->paths); free(lb->bytes); free(lb->lengths); free(lb->infos); free(lb->frames); free(lb->coeff); free(lb->status);
}

/* the whole file as bip_load_image reads it; NULL when it cannot be read */
static uint8_t *read_file(const char *path, size_t *len) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return NULL;
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t *buf = (size > 0 && size < (1L << 30)) ? (uint8_t *)malloc((size_t)size) : NULL;
    if (buf && fread(buf, 1, (size_t)size, fp) != (size_t)size) {
        free(buf);
        buf = NULL;
    }
    fclose(fp);
    *len = buf ? (size_t)size : 0;
    return buf;
}

static bcnn_status list_batch_decoded(bcnn_net *net, bcnn_loader *it, loader_stage *ls, int *launched) {
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    bcnn_tensor *in = &net->tensors[0];
    const int n = net->batch_size, w = in->w, h = in->h, c = in->c;
    const int classif = it->type == BCNN_LOAD_CLASSIFICATION_LIST;
    *launched = 0;
    list_batch lb;
    lb.paths = (char **)calloc((size_t)n, sizeof(char *));
    lb.bytes = (uint8_t **)calloc((size_t)n, sizeof(uint8_t *));
    lb.lengths = (size_t *)calloc((size_t)n, sizeof(size_t));
    lb.infos = (bip_jpeg_info *)calloc((size_t)n, sizeof(bip_jpeg_info));
    lb.frames = (bcnn_hip_jpeg_frame *)calloc((size_t)n, sizeof(bcnn_hip_jpeg_frame));
    lb.coeff = (int16_t **)calloc((size_t)n, sizeof(int16_t *));
    lb.status = (int *)calloc((size_t)n, sizeof(int));
    if (!lb.paths || !lb.bytes || !lb.lengths || !lb.infos || !lb.frames || !lb.coeff || !lb.status) {
        list_batch_free(&lb, n);
        return BCNN_FAILED_ALLOC;
    }
    /* ---- phase 1: lines, labels, files, headers */
    int count = 0, failures = 0, candidates = 0, gave_up = 0;
    while (count < n) {
        char **tok = NULL;
        const int nt = next_line_tokens(it->f_current, &tok);
        int accepted = nt > 0;
        if (nt <= 0) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid regression format\n");
        } else if (classif && net->mode != BCNN_MODE_PREDICT && nt != 2) {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unexpected classif format. Found label size of %d, expected %d.\n", nt - 1, 1);
            free_tokens(tok, nt);
            accepted = 0;
        }
        if (!accepted) {
            if (++failures >= 1000) {
                bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "bcnn_loader_next: 1000 samples in a row could not be read\n");
                gave_up = 1; /* the samples accepted so far still make their draws, as they have on the host path */
                break;
            }
            continue;
        }
        failures = 0;
        if (net->mode != BCNN_MODE_PREDICT && classif) {
            write_class_label(net, count, atoi(tok[1]));
        } else if (net->mode != BCNN_MODE_PREDICT) {
            int sz;
            float *y = label_slot(net, count, &sz);
            if (nt - 1 != sz)
                bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unexpected label format. Found label size of %d, expected %d.\n", nt - 1, sz);
            for (int i = 0; i < nt - 1 && i < sz; ++i) y[i] = (float)atof(tok[i + 1]);
        }
        lb.paths[count] = tok[0];
        tok[0] = NULL;
        free_tokens(tok, nt);
        lb.bytes[count] = read_file(lb.paths[count], &lb.lengths[count]);
        if (lb.bytes[count] && bip_jpeg_frame_info(lb.bytes[count], lb.lengths[count], &lb.infos[count]) == BIP_SUCCESS &&
            lb.infos[count].ncomp == c) {
            bcnn_jpeg_frame_from_info(&lb.infos[count], &lb.frames[count]);
            ++candidates;
        }
        ++count;
    }
    /* ---- phase 2: entropy decoding into the staging block. A batch that does not fit it (2 GiB) and a frame the device
     * side refuses get no coeff[] and are decoded below like every other file. */
    int staged = candidates > 0 && !gave_up &&
                 bcnn_hip_augment_jpeg_begin(in->n, c, h, w, count, lb.frames, lb.coeff) == 0;
    if (staged && bcnn_jpeg_read_batch_each(count, (const uint8_t *const *)lb.bytes, lb.lengths, lb.infos, lb.coeff,
                                            net->num_threads, lb.status) != 0) {
        bcnn_hip_augment_jpeg_cancel();
        staged = 0;
    }
    /* ---- phase 3: the draws, in the reference's order */
    int on_device = 0;
    const int keep_bytes = effects_on(net) && net->mode == BCNN_MODE_TRAIN && net->data_aug;
    memset(ls->decoded, 0, (size_t)n);
    for (int i = 0; i < count; ++i) {
        int *x_shift = net->data_aug ? &net->data_aug->shift_x : NULL, *y_shift = net->data_aug ? &net->data_aug->shift_y : NULL;
        if (staged && lb.coeff[i] && lb.status[i]) {
            int x_ul, y_ul;
            crop_origin(net, lb.infos[i].width, lb.infos[i].height, w, h, &x_ul, &y_ul);
            if (x_shift) { *x_shift = x_ul; *y_shift = y_ul; }
            ls->decoded[i] = 1;
            ls->origins[2 * i] = x_ul;
            ls->origins[2 * i + 1] = y_ul;
            drop_lazy(ls); /* the bytes that rebuild this sample on the host, should the next one fail */
            uint8_t *copy = keep_bytes ? (uint8_t *)malloc(lb.lengths[i]) : NULL;
            if (copy) { /* the batch keeps its own: should the effects be refused, every sample is decoded here (below) */
                memcpy(copy, lb.bytes[i], lb.lengths[i]);
                ls->lazy = copy;
            } else {
                ls->lazy = lb.bytes[i];
                lb.bytes[i] = NULL;
            }
            ls->lazy_len = lb.lengths[i];
            ls->lazy_x = x_ul;
            ls->lazy_y = y_ul;
            ls->owed = 0;
            stage_draws(net, ls, i, w, h, 1);
            ++on_device;
            continue;
        }
        int wi = 0, hi = 0, ci = 0;
        unsigned char *buf = NULL;
        if (lb.bytes[i]) bip_load_image_from_memory(lb.bytes[i], (int)lb.lengths[i], &buf, &wi, &hi, &ci);
        if (place_decoded(net, lb.paths[i], buf, wi, hi, ci, w, h, c, it->input_uchar, x_shift, y_shift) != BCNN_SUCCESS) {
            settle_owed(net, it); /* the buffer as the host path would have left it */
        } else {
            ls->owed = 0;
            drop_lazy(ls);
        }
        stage_sample(net, it, ls, i, w, h, c, 1);
    }
    bcnn_status st = BCNN_SUCCESS;
    if (gave_up) {
        st = BCNN_INVALID_DATA;
    } else if (staged && on_device == 0) {
        bcnn_hip_augment_jpeg_cancel();
    } else if (staged && stage_effects(ls->draws, sizeof(aug_draw), count, w, h) < 0) {
        /* the effects were refused: the batch is made on the host (bcnn_loader_next), so the samples that were to be
         * decoded on the device are decoded here after all, from the files' bytes, which are still held */
        bcnn_hip_augment_jpeg_cancel();
        ls->refused = 1;
        for (int i = 0; i < count; ++i) {
            if (!ls->decoded[i]) continue;
            uint8_t *bytes = lb.bytes[i] ? lb.bytes[i] : ls->lazy; /* the latest one's have moved to `lazy` */
            const size_t len = lb.bytes[i] ? lb.lengths[i] : ls->lazy_len;
            int wi = 0, hi = 0, ci = 0;
            unsigned char *buf = NULL;
            if (bytes) bip_load_image_from_memory(bytes, (int)len, &buf, &wi, &hi, &ci);
            if (buf && wi > 0 && hi > 0 && ci == c)
                crop_to_input(buf, wi, hi, ls->origins[2 * i], ls->origins[2 * i + 1], ls->pixels + (size_t)i * w * h * c, w, h, c);
            else
                st = BCNN_INVALID_DATA;
            free(buf);
        }
    } else if (staged) {
        if (bcnn_hip_augment_jpeg_run(in->data_gpu, ls->decoded, ls->pixels, ls->records, ls->taps, ls->origins,
                                      net->data_aug ? net->data_aug->swap_to_bgr : 0) != 0) {
            bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "bcnn_loader_next: the batch does not fit the device loader path\n");
            st = BCNN_INVALID_PARAMETER;
        } else {
            *launched = 1;
            hc->loader_device_decoded = on_device;
        }
    }
    list_batch_free(&lb, n);
    return st;
}

/* ---- detection list: "image-path (class x y w h)*" lines (bcnn_detection_loader.c) --------------------------------- */
static bcnn_status list_detection_init(bcnn_loader *it, bcnn_net *net, const char *a, const char *b, const char *c,
                                       const char *d) {
    BCNN_CHECK_STATUS(list_init(it, net, a, b, c, d));
    it->input_net = (uint8_t *)calloc((size_t)bcnn_tensor_size3d(&net->tensors[0]), 1);
    return it->input_net ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
}

/* One entry of the list, split so that the pixel work is separable: the host path (list_detection_next) and the device
 * path (detection_batch_device) run the same steps in the same order and differ only in who makes the pixels. */
typedef struct {
    char **tok;
    int n;               /* tokens of the line; <= 0: no line */
    unsigned char *pimg; /* the decoded file, or NULL */
    int w_img, h_img, c_img;
    int nw, nh, dx, dy;  /* letterbox extent and canvas offsets */
    int augmented;       /* `draw` holds this sample's augmentation (TRAIN mode with an augmenter) */
    aug_draw draw;
} det_entry;

static void det_entry_free(det_entry *e) {
    free(e->pimg);
    if (e->n > 0) free_tokens(e->tok, e->n);
    memset(e, 0, sizeof(*e));
}

static void det_read_line(bcnn_loader *it, det_entry *e) {
    memset(e, 0, sizeof(*e));
    e->n = next_line_tokens(it->f_current, &e->tok);
}

/* Decodes the file of a well-formed row. Reads and writes nothing but the entry (bip_load_image keeps no state), so the
 * entries of a batch may be decoded on several threads. */
static void det_decode(det_entry *e) {
    if (e->n > 0 && (e->n - 1) % 5 == 0) bip_load_image(e->tok[0], &e->pimg, &e->w_img, &e->h_img, &e->c_img);
}

/* The skips, none of which consumes a draw, with their warnings; then the letterbox extent. */
static bcnn_status det_accept(bcnn_net *net, det_entry *e) {
    bcnn_tensor *in = &net->tensors[0];
    if (e->n <= 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid detection format\n");
        return BCNN_INVALID_DATA;
    }
    if ((e->n - 1) % 5 != 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING,
                 "Wrong data format for detection %s. Found %d labels but expected multiple of 5\n", e->tok[0], e->n - 1);
        return BCNN_INVALID_DATA;
    }
    if (!(e->w_img > 0 && e->h_img > 0 && e->pimg)) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip invalid image %s\n", e->tok[0]);
        return BCNN_INVALID_DATA;
    }
    if (in->c != e->c_img) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: unexpected number of channels\n", e->tok[0]);
        return BCNN_INVALID_DATA;
    }
    /* the letterbox: the float ratio (file header), the reference's truncations otherwise */
    const float wh_ratio = (float)e->w_img / (float)e->h_img;
    if (wh_ratio < 1) {
        e->nh = in->h;
        e->nw = (int)(e->nh * wh_ratio);
    } else {
        e->nw = in->w;
        e->nh = (int)(e->nw / wh_ratio);
    }
    if (e->nw < 1 || e->nh < 1) { /* an image so narrow that nothing of it is left at this input size */
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: %d x %d leaves no pixel at the input size\n", e->tok[0],
                 e->w_img, e->h_img);
        return BCNN_INVALID_DATA;
    }
    return BCNN_SUCCESS;
}

/* The draws of an accepted entry, in the reference's order: the canvas offsets, the flip (:130-140), the augmentation. */
static void det_draw(bcnn_net *net, det_entry *e) {
    bcnn_tensor *in = &net->tensors[0];
    if (net->mode == BCNN_MODE_TRAIN) {
        e->dx = rand_between(0, in->w - e->nw);
        e->dy = rand_between(0, in->h - e->nh);
    } else {
        e->dx = (in->w - e->nw) / 2;
        e->dy = (in->h - e->nh) / 2;
    }
    bcnn_data_augmenter *aug = net->data_aug;
    e->augmented = net->mode == BCNN_MODE_TRAIN && aug;
    if (e->augmented) {
        aug->apply_fliph = 0;
        if (aug->random_fliph) aug->apply_fliph = ((float)rand() / RAND_MAX > 0.5f);
        draw_augmentation(aug, &e->draw, effects_on(net), in->w, in->h);
    }
}

/* The letterboxed, augmented sample into input slot idx on the host. `buf` (nw x nh x c, freed here) takes the resized
 * image. */
static void det_pixels_host(bcnn_net *net, bcnn_loader *it, const det_entry *e, unsigned char *buf, int idx) {
    bcnn_tensor *in = &net->tensors[0];
    const int c = e->c_img;
    bip_resize_bilinear(e->pimg, e->w_img, e->h_img, (size_t)e->w_img * c, buf, e->nw, e->nh, (size_t)e->nw * c, c);
    const size_t bytes = (size_t)bcnn_tensor_size3d(in);
    memset(it->input_net, 128, bytes);
    bip_crop_image(buf, e->nw, e->nh, (size_t)e->nw * c, -e->dx, -e->dy, it->input_net, in->w, in->h, (size_t)in->w * in->c,
                   in->c);
    free(buf);
    if (e->augmented) augment_pixels(it->input_net, in->w, in->h, in->c, &e->draw, it->input_uchar);
    memcpy(it->input_uchar, it->input_net, bytes);
    bcnn_convert_img_to_float(it->input_uchar, in->w, in->h, in->c, 1 / 127.5f, net->data_aug ? net->data_aug->swap_to_bgr : 0,
                              127.5f, 127.5f, 127.5f, in->data + (size_t)idx * bytes);
}

static void det_labels(bcnn_net *net, const det_entry *e, int idx) {
    if (net->mode == BCNN_MODE_PREDICT) return;
    bcnn_tensor *in = &net->tensors[0];
    const bcnn_data_augmenter *aug = net->data_aug;
    char **tok = e->tok;
    int sz;
    float *y = label_slot(net, idx, &sz);
    int num_boxes = (e->n - 1) / 5;
    if (num_boxes > BCNN_DETECTION_MAX_BOXES) num_boxes = BCNN_DETECTION_MAX_BOXES;
    if (num_boxes > sz / 5) num_boxes = sz / 5; /* a label tensor some other builder shaped */
    const float scale_x = (float)e->nw / (float)in->w, scale_y = (float)e->nh / (float)in->h;
    const float scale_dx = (float)e->dx / (float)in->w, scale_dy = (float)e->dy / (float)in->h;
    for (int i = 0; i < num_boxes; ++i) { /* box centre (x, y), extent (w, h), class */
        y[i * 5 + 0] = (float)atof(tok[5 * i + 2]) * scale_x + scale_dx;
        y[i * 5 + 1] = (float)atof(tok[5 * i + 3]) * scale_y + scale_dy;
        y[i * 5 + 2] = (float)atof(tok[5 * i + 4]) * scale_x;
        y[i * 5 + 3] = (float)atof(tok[5 * i + 5]) * scale_y;
        if (aug && aug->apply_fliph) y[i * 5 + 0] = 1.0f - y[i * 5 + 0];
        y[i * 5 + 4] = (float)atoi(tok[5 * i + 1]);
    }
}

static bcnn_status list_detection_next(bcnn_loader *it, bcnn_net *net, int idx) {
    det_entry e;
    det_read_line(it, &e);
    det_decode(&e);
    bcnn_status st = det_accept(net, &e);
    unsigned char *buf = NULL;
    if (st == BCNN_SUCCESS && !(buf = (unsigned char *)calloc((size_t)e.nw * e.nh * e.c_img, 1))) {
        bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Skip image %s: %d x %d leaves no pixel at the input size\n", e.tok[0], e.w_img,
                 e.h_img);
        st = BCNN_INVALID_DATA;
    }
    if (st == BCNN_SUCCESS) {
        det_draw(net, &e);
        det_pixels_host(net, it, &e, buf, idx);
        det_labels(net, &e, idx);
    }
    det_entry_free(&e);
    return st;
}

/* ---- a detection batch letterboxed on the device (bcnn_set_loader_detection_on_device) ------------------------------- */
/* Entries first .. first + count - 1 on up to `threads` threads, entry first + t, first + t + T, ... on thread t. */
typedef struct { det_entry *entries; int count, first, step; } det_worker;

static void *det_worker_run(void *arg) {
    det_worker *w = (det_worker *)arg;
    for (int i = w->first; i < w->count; i += w->step) det_decode(&w->entries[i]);
    return NULL;
}

static void det_decode_group(det_entry *entries, int count, int threads) {
    const int T = threads > count ? count : threads;
    det_worker *workers = T > 1 ? (det_worker *)calloc((size_t)T, sizeof(det_worker)) : NULL;
    pthread_t *ids = T > 1 ? (pthread_t *)calloc((size_t)T, sizeof(pthread_t)) : NULL;
    if (!workers || !ids) { /* one thread: the sequential path */
        free(workers);
        free(ids);
        for (int i = 0; i < count; ++i) det_decode(&entries[i]);
        return;
    }
    for (int t = 0; t < T; ++t) {
        det_worker w = {entries, count, t, T};
        workers[t] = w;
    }
    int started = 0;
    for (int t = 1; t < T; ++t) { /* a thread that cannot be created: its entries are decoded below */
        if (pthread_create(&ids[t], NULL, det_worker_run, &workers[t]) != 0) break;
        started = t;
    }
    det_worker_run(&workers[0]);
    for (int t = started + 1; t < T; ++t) det_worker_run(&workers[t]);
    for (int t = 1; t <= started; ++t) pthread_join(ids[t], NULL);
    free(workers);
    free(ids);
}

/* The batch in rounds, because a skipped entry consumes no draw and reading a file consumes none: as many lines as slots
 * are still empty are read (each fills a slot or is skipped, so no line is read that the host path would not have read),
 * their files are decoded in parallel, and the results are walked in list order with the skips, warnings, draws, records
 * and labels of list_detection_next. The decoded images are kept until the batch is complete and go up in one copy;
 * tensors[0].data and the loader's two sample buffers are not written. Should the device side refuse the batch (2 GiB),
 * it is made on the host from the images already decoded and the draws already made. *on_device: the input tensor was
 * made on the device. */
static bcnn_status detection_batch_device(bcnn_net *net, bcnn_loader *it, int *on_device) {
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    bcnn_tensor *in = &net->tensors[0];
    const int n = net->batch_size, w = in->w, h = in->h;
    const size_t sample_taps = ((size_t)w + h) * 2;
    *on_device = 0;
    det_entry *kept = (det_entry *)calloc((size_t)n, sizeof(det_entry)), *group = (det_entry *)calloc((size_t)n, sizeof(det_entry));
    bcnn_hip_letterbox_image *images = (bcnn_hip_letterbox_image *)calloc((size_t)n, sizeof(bcnn_hip_letterbox_image));
    bcnn_hip_augment_record *records = (bcnn_hip_augment_record *)calloc((size_t)n, sizeof(bcnn_hip_augment_record));
    int32_t *taps = (int32_t *)calloc((size_t)n * sample_taps, sizeof(int32_t));
    bcnn_status st = (kept && group && images && records && taps) ? BCNN_SUCCESS : BCNN_FAILED_ALLOC;
    int count = 0, failures = 0;
    while (st == BCNN_SUCCESS && count < n) {
        const int want = n - count;
        for (int i = 0; i < want; ++i) det_read_line(it, &group[i]);
        det_decode_group(group, want, net->num_threads);
        for (int i = 0; i < want; ++i) {
            det_entry *e = &group[i];
            if (st != BCNN_SUCCESS || det_accept(net, e) != BCNN_SUCCESS) {
                det_entry_free(e);
                if (st == BCNN_SUCCESS && ++failures >= 1000) {
                    bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "bcnn_loader_next: 1000 samples in a row could not be read\n");
                    st = BCNN_INVALID_DATA; /* the entries behind this one are dropped unseen */
                }
                continue;
            }
            failures = 0;
            det_draw(net, e);
            if (e->augmented) fill_record(&records[count], taps + (size_t)count * sample_taps, &e->draw, w, h);
            det_labels(net, e, count);
            kept[count++] = *e;
            memset(e, 0, sizeof(*e));
        }
    }
    if (st == BCNN_SUCCESS) {
        for (int i = 0; i < n; ++i) {
            const bcnn_hip_letterbox_image im = {kept[i].pimg, kept[i].w_img, kept[i].h_img, kept[i].nw, kept[i].nh,
                                                 kept[i].dx, kept[i].dy};
            images[i] = im;
        }
        /* the effects first: a refusal there sends the batch the host way as well */
        if (stage_effects(&kept[0].draw, sizeof(det_entry), n, w, h) >= 0 &&
            bcnn_hip_augment_letterbox_batch(in->data_gpu, in->n, in->c, h, w, n, images, records, taps,
                                             net->data_aug ? net->data_aug->swap_to_bgr : 0) == 0) {
            *on_device = 1;
            hc->loader_device_letterboxed = n;
        } else { /* the host way, from what is already decoded and drawn */
            for (int i = 0; i < n && st == BCNN_SUCCESS; ++i) {
                unsigned char *buf = (unsigned char *)calloc((size_t)kept[i].nw * kept[i].nh * kept[i].c_img, 1);
                if (buf) det_pixels_host(net, it, &kept[i], buf, i);
                else st = BCNN_FAILED_ALLOC;
            }
        }
    }
    for (int i = 0; kept && i < n; ++i) det_entry_free(&kept[i]);
    free(kept); free(group); free(images); free(records); free(taps);
    return st;
}

/* ---- what bcnn_data_segmentation.c uses of this file (bcnn_internal.h) ------------------------------------------------ */
/* Thin doors onto the statics above, which do what they did: the segmentation-list reader decodes, skips and crops by its
 * own rules and takes the draws, the pixel work and the staging from here, so that its input batch is the classification
 * list's bit for bit. */
int bcnn_loader_line_tokens(FILE *f, char ***tok) { return next_line_tokens(f, tok); }
void bcnn_loader_free_tokens(char **tok, int n) { free_tokens(tok, n); }
void bcnn_loader_crop_origin(bcnn_net *net, int wi, int hi, int w, int h, int *x_ul, int *y_ul) {
    crop_origin(net, wi, hi, w, h, x_ul, y_ul);
}
bcnn_status bcnn_loader_crop_to_input(unsigned char *buf, int wi, int hi, int x_ul, int y_ul, unsigned char *img, int w, int h,
                                      int c) {
    return crop_to_input(buf, wi, hi, x_ul, y_ul, img, w, h, c);
}
int bcnn_loader_effects_on(const bcnn_net *net) { return effects_on(net); }
int bcnn_loader_staging(bcnn_net *net) {
    loader_stage *ls = stage_of(net);
    return ls && ls->active;
}
/* The loader's sample buffer into slot idx of the block with its draws (stage_sample, with no pixel work owed to a later
 * sample); *record and *taps then point at what fill_record made of them. */
bcnn_status bcnn_loader_stage_sample(bcnn_net *net, bcnn_loader *it, int idx, const bcnn_hip_augment_record **record,
                                     const int32_t **taps) {
    loader_stage *ls = stage_of(net);
    bcnn_tensor *in = &net->tensors[0];
    if (!ls || !ls->active) return BCNN_INVALID_PARAMETER;
    BCNN_CHECK_STATUS(stage_sample(net, it, ls, idx, in->w, in->h, in->c, 0));
    *record = &ls->records[idx];
    *taps = ls->taps + (size_t)idx * ((size_t)in->w + in->h) * 2;
    return BCNN_SUCCESS;
}
/* The records and tap tables of the batch gathered last (batch x 2 (w + h) taps). */
void bcnn_loader_staged_records(bcnn_net *net, const bcnn_hip_augment_record **records, const int32_t **taps) {
    loader_stage *ls = stage_of(net);
    *records = ls ? ls->records : NULL;
    *taps = ls ? ls->taps : NULL;
}
/* augment_if_training, which also leaves the record and the w + h tap pairs of the draws it made (the identity outside
 * TRAIN mode): the draws once, then the pixels of `img` in place. */
bcnn_status bcnn_loader_augment_recorded(bcnn_net *net, unsigned char *img, int w, int h, int c,
                                         bcnn_hip_augment_record *record, int32_t *taps) {
    memset(record, 0, sizeof(*record));
    if (net->mode != BCNN_MODE_TRAIN || !net->data_aug) return BCNN_SUCCESS;
    unsigned char *scratch = (unsigned char *)calloc((size_t)w * h * c, 1);
    if (!scratch) return BCNN_FAILED_ALLOC;
    aug_draw d;
    draw_augmentation(net->data_aug, &d, effects_on(net), w, h);
    fill_record(record, taps, &d, w, h);
    const bcnn_status st = augment_pixels(img, w, h, c, &d, scratch);
    free(scratch);
    return st;
}

/* fill_record for a caller that holds the draws as numbers (tests and tools restate the label rule from them): the record
 * and the w + h tap pairs of one w x h sample. */
void bcnn_loader_fill_record(int flip, int shift, int x_ul, int y_ul, int scale, float scale_factor, int rotate, float theta,
                             int w, int h, bcnn_hip_augment_record *record, int32_t *taps) {
    aug_draw d;
    memset(&d, 0, offsetof(aug_draw, spot));
    d.flip = flip;
    d.shift = shift;
    d.x_ul = shift ? x_ul : 0;
    d.y_ul = shift ? y_ul : 0;
    d.scale = scale;
    d.scale_factor = scale_factor;
    d.rotate = rotate;
    d.theta = theta;
    fill_record(record, taps, &d, w, h);
}

/* ---- public entry points ------------------------------------------------------------------------------------------ */
static void loader_close(bcnn_loader *it) {
    FILE **fs[4] = {&it->f_train, &it->f_train_extra, &it->f_test, &it->f_test_extra};
    for (int i = 0; i < 4; ++i)
        if (*fs[i]) { fclose(*fs[i]); *fs[i] = NULL; }
    free(it->input_uchar);
    free(it->input_net);
    it->input_uchar = it->input_net = NULL;
}

void bcnn_destroy_data_loader(bcnn_net *net) {
    if (!net->data_loader) return;
    loader_close(net->data_loader);
    free(net->data_loader);
    net->data_loader = NULL;
}

bcnn_status bcnn_set_data_loader(bcnn_net *net, bcnn_loader_type type, const char *train_path_data,
                                 const char *train_path_extra, const char *test_path_data, const char *test_path_extra) {
    bcnn_destroy_data_loader(net);
    if (stage_of(net)) drop_lazy(stage_of(net)); /* a sample of the loader that is gone */
    int detector = bcnn_get_detector_training(net); /* or a net that already holds a head (bcnn-cl in PREDICT / VALID mode) */
    for (int i = 0; !detector && i < net->num_nodes; ++i) detector = net->nodes[i].type == BCNN_LAYER_YOLOV3;
    if (type == BCNN_LOAD_SEGMENTATION_LIST && !has_softmax_loss(net)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR,
                 "bcnn_set_data_loader: the segmentation-list format fills a class-index label map, which only the "
                 "softmax-loss node reads; the net holds none\n");
        return BCNN_INVALID_PARAMETER;
    }
    if ((type == BCNN_LOAD_DETECTION_LIST && !detector) || (int)type < 0 ||
        ((int)type >= BCNN_NUM_LOADERS && type != BCNN_LOAD_SEGMENTATION_LIST)) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR,
                 "bcnn_set_data_loader: the detection-list format belongs to the YOLO head, which is outside the MI355X "
                 "hot-path build (see INTEGRATION.md)\n");
        return BCNN_INVALID_PARAMETER;
    }
    bcnn_loader *it = (bcnn_loader *)calloc(1, sizeof(bcnn_loader));
    if (!it) return BCNN_FAILED_ALLOC;
    it->type = type;
    net->data_loader = it;
    bcnn_status st;
    switch (type) {
        case BCNN_LOAD_MNIST: st = mnist_init(it, net, train_path_data, train_path_extra, test_path_data, test_path_extra); break;
        case BCNN_LOAD_CIFAR10: st = cifar10_init(it, net, train_path_data, train_path_extra, test_path_data, test_path_extra); break;
        case BCNN_LOAD_DETECTION_LIST: st = list_detection_init(it, net, train_path_data, train_path_extra, test_path_data, test_path_extra); break;
        default: st = list_init(it, net, train_path_data, train_path_extra, test_path_data, test_path_extra); break;
    }
    if (st == BCNN_SUCCESS && type == BCNN_LOAD_SEGMENTATION_LIST) st = bcnn_segmentation_init(it, net);
    if (st != BCNN_SUCCESS) bcnn_destroy_data_loader(net); /* no half-opened loader for a later bcnn_loader_next to trip over */
    return st;
}

/* One batch: samples on the host, then the reference's host -> device hook (bcnn_data.c:398-427). A sample that cannot be
 * read is skipped and the next one takes its slot like in the reference -- but after 1000 failures in a row the batch is
 * given up (the reference retries forever, e.g. on a truncated file). Without a loader the caller has filled the host
 * tensors itself and only the upload happens. */
bcnn_status bcnn_loader_next(bcnn_net *net) {
    bcnn_loader *it = net->data_loader;
    if (it && effects_on(net) && net->mode == BCNN_MODE_TRAIN && net->data_aug && net->data_aug->max_random_spots > BCNN_MAX_SPOTS)
        BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER, "bcnn_loader_next: loader_effects draws at most %d spotlights per sample\n",
                   BCNN_MAX_SPOTS);
    const int segmentation = it && it->type == BCNN_LOAD_SEGMENTATION_LIST;
    if (segmentation) BCNN_CHECK_STATUS(bcnn_segmentation_check(net)); /* before any draw as well */
    loader_stage *ls = it ? stage_begin(net, it) : NULL; /* non-NULL: the input batch is made on the device */
    if (ls) ls->refused = 0;
    bcnn_hip_context *hc = (bcnn_hip_context *)net->hip_ctx;
    int launched = 0; /* list_batch_decoded has queued the batch already */
    hc->loader_device_decoded = 0;
    hc->loader_device_letterboxed = 0;
    hc->loader_device_labels = 0;
    int letterboxed = 0; /* detection_batch_device has made the input batch on the device */
    bcnn_tensor *in0 = &net->tensors[0];
    if (it && it->type == BCNN_LOAD_DETECTION_LIST && hc->loader_on_device && hc->loader_detection_on_device && in0->data_gpu &&
        in0->c >= 1 && in0->c <= 4 && net->batch_size >= 1 && in0->n >= net->batch_size) {
        BCNN_CHECK_STATUS(detection_batch_device(net, it, &letterboxed));
    } else if (ls && hc->loader_decode_on_device && (net->tensors[0].c == 1 || net->tensors[0].c == 3) &&
        (it->type == BCNN_LOAD_CLASSIFICATION_LIST || it->type == BCNN_LOAD_REGRESSION_LIST)) {
        const bcnn_status st = list_batch_decoded(net, it, ls, &launched);
        if (st != BCNN_SUCCESS) {
            ls->active = 0;
            return st;
        }
    } else if (it) {
        int failures = 0;
        for (int i = 0; i < net->batch_size; ++i) {
            bcnn_status st;
            switch (it->type) {
                case BCNN_LOAD_MNIST: st = mnist_next(it, net, i); break;
                case BCNN_LOAD_CIFAR10: st = cifar10_next(it, net, i); break;
                case BCNN_LOAD_CLASSIFICATION_LIST: st = list_classif_next(it, net, i); break;
                case BCNN_LOAD_DETECTION_LIST: st = list_detection_next(it, net, i); break;
                case BCNN_LOAD_REGRESSION_LIST: st = list_reg_next(it, net, i); break;
                default: st = bcnn_segmentation_next(it, net, i); break; /* BCNN_LOAD_SEGMENTATION_LIST, behind the enumerators */
            }
            if (st != BCNN_SUCCESS) {
                if (++failures >= 1000) {
                    bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "bcnn_loader_next: 1000 samples in a row could not be read\n");
                    if (ls) ls->active = 0;
                    return BCNN_INVALID_DATA;
                }
                --i;
                continue;
            }
            failures = 0;
        }
    }
    if (ls) ls->active = 0;
    int host_made = 0; /* the device side refused the effects of a batch gathered for it: made on the host after all */
    if (ls && !launched) { /* one copy of the raw samples and their records, two launches; tensors[0].data is not written */
        bcnn_tensor *in = &net->tensors[0];
        const int list_loader = it->type != BCNN_LOAD_MNIST && it->type != BCNN_LOAD_CIFAR10;
        if (ls->refused || stage_effects(ls->draws, sizeof(aug_draw), net->batch_size, ls->w, ls->h) < 0) {
            BCNN_CHECK_STATUS(host_batch_from_stage(net, ls, list_loader));
            host_made = 1;
        } else if (bcnn_hip_augment_batch(in->data_gpu, in->n, in->c, in->h, in->w, net->batch_size, ls->w, ls->h, ls->pixels,
                                          ls->records, ls->taps,
                                          list_loader && net->data_aug ? net->data_aug->swap_to_bgr : 0) != 0)
            BCNN_ERROR(net->log_ctx, BCNN_INVALID_PARAMETER, "bcnn_loader_next: the batch does not fit the device loader path\n");
    }
    for (int i = 0; i < net->num_inputs; ++i) {
        if (((ls && !host_made) || letterboxed) && net->inputs[i] == 0) continue; /* the host copy is stale in this mode */
        bcnn_tensor *t = &net->tensors[net->inputs[i]];
        if (t->data && t->data_gpu) bcnn_hip_memcpy_h2d(t->data_gpu, t->data, (size_t)bcnn_tensor_size(t) * sizeof(float));
    }
    /* a segmentation batch gathered for the device: its label maps are made there from the staged masks and the batch's
     * records (bcnn_data_segmentation.c), and tensors[1].data is then neither written nor uploaded */
    if (segmentation && ls && bcnn_segmentation_labels(net, it, !host_made) != 0) return BCNN_SUCCESS;
    bcnn_tensor *lab = &net->tensors[1];
    if (net->mode != BCNN_MODE_PREDICT && lab->data && lab->data_gpu)
        bcnn_hip_memcpy_h2d(lab->data_gpu, lab->data, (size_t)bcnn_tensor_size(lab) * sizeof(float));
    return BCNN_SUCCESS;
}
