/* label_map_rule.h -- the ONE definition of how a predicted [n][C][h][w] tensor becomes one class index per pixel of an
 * image of another size (label_map.hip, bcnn_hip_label_maps_batch): the source rectangle of an image inside the tensor
 * plane, the value of a class at an output pixel, the argmax step, the class of a truth byte, and the layout of the
 * result block. Plain C99 / C++ that also compiles as HIP; every function is static inline, so nothing is exported.
 * The kernel, the host entry points of label_map.hip and a stand-alone host program under a sanitizer
 * (tools/label_map_rule_check.c) all compile this one definition.
 *
 * Source rectangle. Image b has a rectangle (roi_x, roi_y, roi_w, roi_h) of the w x h tensor plane that is resampled to
 * the image's out_w x out_h. Two fits produce it, mirroring bcnn_image_fit:
 *   STRETCH   : the whole plane, (0, 0, W, H);
 *   LETTERBOX : the rule documented at bcnn_fill_tensor_with_images (include/bcnn/bcnn.h): if (float)W / iw < (float)H / ih
 *               then new_w = W, new_h = (ih * W) / iw, else new_h = H, new_w = (iw * H) / ih (integer divisions), pasted
 *               at ((W - new_w) / 2, (H - new_h) / 2): the rectangle is (x_off, y_off, new_w, new_h). fitted_extent
 *               (image_fill.h) computes the same extents in C++ and stays the fill's; tests/test_label_map_rule.py holds
 *               the two together.
 * Value. Inside the rectangle the value of class c at output pixel (ox, oy) is interp_rule.h's rule applied to the
 * rectangle as if it were a tensor of extent roi_w x roi_h: bcnn_interp_step / bcnn_interp_tap per axis, and
 *   v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
 * in float32, every operation rounded on its own: a translation unit that calls bcnn_label_map_value must be compiled with
 * contraction off (-ffp-contract=off), as csrc/ is. v is therefore, bit for bit, what bcnn_hip_interp_forward writes for
 * the cropped rectangle.
 * Argmax. Start at class 0 and replace on strict > in ascending class order: the first maximum wins, as in the
 * softmax-loss node. NaN is whatever that rule gives: a NaN never replaces anything (v > best is false) and a NaN at class
 * 0 is never replaced (nothing compares greater than it), so an all-NaN pixel and a pixel whose class 0 is NaN are both
 * labelled 0. Nothing is promised about numpy's argmax on such input.
 * Label type. uint8_t, so C <= 256.
 * Evaluation. A truth byte t is classified by softmax_loss_rule.h's bcnn_softmax_loss_classify on (float)t with the
 * call's ignore_label: ignored, valid, or out of range (t >= C). A valid pixel adds 1 to counts[t * C + a].
 * Result block. Image b's labels occupy out_h rows of round_up(out_w, 4) bytes; each image's block starts on a 16-byte
 * boundary; the truths of an evaluating call are staged in a second block of the same layout. A call whose total, truths
 * included, would pass 2^31 bytes is refused. */
#ifndef BCNN_LABEL_MAP_RULE_H
#define BCNN_LABEL_MAP_RULE_H

#include "interp_rule.h"
#include "softmax_loss_rule.h"

#define BCNN_LABEL_MAP_FIT_STRETCH 0   /* the values of bcnn_image_fit (include/bcnn/bcnn.h) */
#define BCNN_LABEL_MAP_FIT_LETTERBOX 1
#define BCNN_LABEL_MAP_MAX_CLASSES 256
#define BCNN_LABEL_MAP_MAX_BYTES 0x80000000ULL

/* one image of a call; the layout of bcnn_hip_label_map_image (include/bcnn_hip.h) */
typedef struct bcnn_label_map_geom {
    int out_w, out_h;                 /* the image's own extent: the extent of its label map */
    int roi_x, roi_y, roi_w, roi_h;   /* the rectangle of the tensor plane that is resampled to it */
} bcnn_label_map_geom;

/* The rectangle of an iw x ih image inside the W x H plane. 0, or 1 with *out untouched: an extent below 1, an unknown
 * fit, a letterbox extent that comes out 0. */
BCNN_INTERP_INLINE int bcnn_label_map_fit(int fit, int W, int H, int iw, int ih, bcnn_label_map_geom *out) {
    if (W < 1 || H < 1 || iw < 1 || ih < 1) return 1;
    int new_w = W, new_h = H;
    if (fit == BCNN_LABEL_MAP_FIT_LETTERBOX) {
        if ((float)W / (float)iw < (float)H / (float)ih) {
            new_h = (int)(((long long)ih * W) / iw);
        } else {
            new_w = (int)(((long long)iw * H) / ih);
        }
    } else if (fit != BCNN_LABEL_MAP_FIT_STRETCH) {
        return 1;
    }
    if (new_w < 1 || new_h < 1 || new_w > W || new_h > H) return 1;
    out->out_w = iw;
    out->out_h = ih;
    out->roi_x = (W - new_w) / 2;
    out->roi_y = (H - new_h) / 2;
    out->roi_w = new_w;
    out->roi_h = new_h;
    return 0;
}

/* An image a call can run: output extents of at least 1 and a non-empty rectangle inside the w x h plane. */
BCNN_INTERP_INLINE int bcnn_label_map_geom_ok(const bcnn_label_map_geom *g, int h, int w) {
    return g->out_w >= 1 && g->out_h >= 1 && g->roi_w >= 1 && g->roi_h >= 1 && g->roi_x >= 0 && g->roi_y >= 0 &&
           g->roi_w <= w && g->roi_h <= h && g->roi_x <= w - g->roi_w && g->roi_y <= h - g->roi_h;
}

/* The value of one class at one output pixel: a, b the two column taps on the row of the first row tap, c, d on the
 * second; seven roundings in the interp node's association. */
BCNN_INTERP_INLINE float bcnn_label_map_value(float a, float b, float c, float d, float w0, float w1, float h0, float h1) {
    return h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d);
}

/* One step of the argmax, for classes 1 .. C - 1 in ascending order after (*best, *arg) = (value of class 0, 0). */
BCNN_INTERP_INLINE void bcnn_label_map_argmax_step(float v, int cls, float *best, int *arg) {
    if (v > *best) {
        *best = v;
        *arg = cls;
    }
}

/* The class of a truth byte: BCNN_SL_VALID (*cls = t), BCNN_SL_IGNORED or BCNN_SL_OUT_OF_RANGE (*cls = -1). */
BCNN_INTERP_INLINE int bcnn_label_map_truth(unsigned char t, int ignore_label, int classes, int *cls) {
    return bcnn_softmax_loss_classify((float)t, ignore_label, classes, cls);
}

/* bytes between two label rows of an image out_w wide */
BCNN_INTERP_INLINE unsigned bcnn_label_map_row_stride(int out_w) { return ((unsigned)out_w + 3u) & ~3u; }

/* The result block of a call, host only (no device attribute under HIP): row_strides[b] and offsets[b] of every image
 * (either may be NULL) and the bytes of the label block in *total_bytes (may be NULL). 0, or 1 with nothing written: imgs
 * NULL, num_images < 1, an extent below 1, or a total -- twice the label block when truths are staged beside it -- past
 * 2^31 bytes. */
static inline int bcnn_label_map_plan(const bcnn_label_map_geom *imgs, int num_images, int with_truths,
                                      unsigned *row_strides, unsigned long long *offsets,
                                      unsigned long long *total_bytes) {
    if (!imgs || num_images < 1) return 1;
    const unsigned long long limit = BCNN_LABEL_MAP_MAX_BYTES / (with_truths ? 2u : 1u);
    unsigned long long at = 0;
    for (int b = 0; b < num_images; ++b) {
        if (imgs[b].out_w < 1 || imgs[b].out_h < 1 || imgs[b].out_w > 0x7ffffffc) return 1;
        const unsigned long long bytes = (unsigned long long)bcnn_label_map_row_stride(imgs[b].out_w) * imgs[b].out_h;
        at += (bytes + 15u) & ~15ULL;   /* at most 2^31 + 2^62: no wrap */
        if (at > limit) return 1;
    }
    at = 0;
    for (int b = 0; b < num_images; ++b) {
        const unsigned stride = bcnn_label_map_row_stride(imgs[b].out_w);
        if (row_strides) row_strides[b] = stride;
        if (offsets) offsets[b] = at;
        at += ((unsigned long long)stride * imgs[b].out_h + 15u) & ~15ULL;
    }
    if (total_bytes) *total_bytes = at;
    return 0;
}

#endif /* BCNN_LABEL_MAP_RULE_H */
