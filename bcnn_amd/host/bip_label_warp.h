/* bip_label_warp.h -- the ONE definition of how a class-index label map follows the geometry of its augmented image,
 * shared by the host warp (bip_warp_label_map, bip_augment.c), the segmentation-list loader (bcnn_data_segmentation.c) and
 * the device kernel (../csrc/augment_label.hip). Plain C that also compiles as HIP; every function is static inline, so
 * nothing is exported.
 *
 * The label of output pixel (x, y) of a w x h sample is ONE byte of the cropped mask, or the fill byte F: a pull-back
 * through the image's geometry stages, with nearest-neighbour picks where the image blends. It reads the record and the
 * tap table the loader makes for the image (fill_record in bcnn_data.c; bcnn_hip_augment_record in bcnn_hip.h), so image
 * and label agree on where every pixel comes from and on what is canvas:
 *   L0(x, y)  byte (x, y) of the cropped mask
 *   FLIP      L1(x, y) = L0(w - 1 - x, y)
 *   SHIFT     L2(x, y) = L1(x + x_ul, y + y_ul) inside the sample, else F                       (the image gets 128)
 *   SCALE     where both taps have an index >= 0 (covered by the resized image): L3(x, y) = L2(ix, iy), with per axis
 *             i = index + 1 if frac >= 8 (sixteenths: a tie goes up) and the extent is > 1, else index; a pixel that is
 *             not covered falls through to L2(x, y), as the image falls through to its unscaled self
 *   ROTATE    px, py as bip_rotate_image forms them (16.16 fixed point, uint32 wrap-around, centre (w / 2, h / 2));
 *             mx = px >> 16, my = py >> 16; covered iff 0 <= mx < w - 1 and 0 <= my < h - 1 (the image's own test);
 *             L4(x, y) = L3(mx + ((px & 0xffff) >= 0x8000), my + ((py & 0xffff) >= 0x8000)) if covered, else F
 *                                                                                               (the image gets 0)
 * A stage whose flag is clear is the identity. Contrast, brightness and the effects do not touch a label.
 * The caller guarantees what taps_in_range (../csrc/augment.hip) guarantees for the image: with SCALE every tap index is
 * in [-1, max(extent - 2, 0)], so index + 1 stays inside the sample. */
#ifndef BIP_LABEL_WARP_H
#define BIP_LABEL_WARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BIP_LABEL_INLINE __host__ __device__ static inline
#else
#define BIP_LABEL_INLINE static inline
#endif

/* the flag bits of bcnn_hip_augment_record that move pixels (bcnn_hip.h: BCNN_HIP_AUG_FLIP ... _ROTATE) */
#define BIP_LABEL_FLIP 1
#define BIP_LABEL_SHIFT 2
#define BIP_LABEL_SCALE 4
#define BIP_LABEL_ROTATE 8

/* One sample as the rule sees it. tapx / tapy: w and h (index, fraction) int32 pairs; read only with SCALE. */
typedef struct bip_label_sample {
    const uint8_t *map; /* w x h bytes, dense */
    const int32_t *tapx, *tapy;
    int32_t w, h;
    int32_t flags, x_ul, y_ul, ca, sa;
    int32_t fill; /* F, 0 ... 255 */
} bip_label_sample;

/* Every stage moves a label and none changes it, so the rule is a map from the output pixel to ONE source byte: the
 * functions below return its offset in the map, or -1 for the fill byte. (The device kernel forms the offsets of a lane's
 * pixels first and loads afterwards.) */

/* L2: flip and shift of the cropped mask. (x, y) inside the sample. */
BIP_LABEL_INLINE int64_t bip_label_shifted(const bip_label_sample *s, int32_t x, int32_t y) {
    if (s->flags & BIP_LABEL_SHIFT) {
        const long long X = (long long)x + s->x_ul, Y = (long long)y + s->y_ul;
        if (X < 0 || X >= s->w || Y < 0 || Y >= s->h) return -1;
        x = (int32_t)X;
        y = (int32_t)Y;
    }
    if (s->flags & BIP_LABEL_FLIP) x = s->w - 1 - x;
    return (int64_t)y * s->w + x;
}

/* L3: the nearer of the resize's two taps per axis. (x, y) inside the sample. */
BIP_LABEL_INLINE int64_t bip_label_scaled(const bip_label_sample *s, int32_t x, int32_t y) {
    if (s->flags & BIP_LABEL_SCALE) {
        const int32_t ix = s->tapx[2 * x], iy = s->tapy[2 * y];
        if (ix >= 0 && iy >= 0) /* covered by the resized image */
            return bip_label_shifted(s, ix + ((s->tapx[2 * x + 1] >= 8 && s->w > 1) ? 1 : 0),
                                     iy + ((s->tapy[2 * y + 1] >= 8 && s->h > 1) ? 1 : 0));
    }
    return bip_label_shifted(s, x, y);
}

/* L4: where the label of output pixel (x, y) comes from: an offset into the map, or -1 for the fill byte. */
BIP_LABEL_INLINE int64_t bip_label_source(const bip_label_sample *s, int32_t x, int32_t y) {
    if (!(s->flags & BIP_LABEL_ROTATE)) return bip_label_scaled(s, x, y);
    const int32_t cxr = s->w / 2, cyr = s->h / 2;
    const uint32_t u = (uint32_t)(x - cxr), v = (uint32_t)(y - cyr);
    const uint32_t upx = (uint32_t)s->ca * u - (uint32_t)s->sa * v + ((uint32_t)cxr << 16);
    const uint32_t upy = (uint32_t)s->sa * u + (uint32_t)s->ca * v + ((uint32_t)cyr << 16);
    /* px >> 16 of the int32 the image path forms: the sign-extended upper half */
    const int32_t mx = (int32_t)(int16_t)(uint16_t)(upx >> 16), my = (int32_t)(int16_t)(uint16_t)(upy >> 16);
    if (mx < 0 || mx >= s->w - 1 || my < 0 || my >= s->h - 1) return -1;
    return bip_label_scaled(s, mx + ((upx & 0xffffu) >= 0x8000u ? 1 : 0), my + ((upy & 0xffffu) >= 0x8000u ? 1 : 0));
}

/* The label of output pixel (x, y). */
BIP_LABEL_INLINE int32_t bip_label_warp(const bip_label_sample *s, int32_t x, int32_t y) {
    const int64_t at = bip_label_source(s, x, y);
    return at < 0 ? s->fill : (int32_t)s->map[at];
}

/* 1 when the taps of a SCALE sample keep every read of the rule inside it (the test of taps_in_range), or no SCALE. */
static inline int bip_label_taps_ok(int32_t flags, const int32_t *tapx, const int32_t *tapy, int32_t w, int32_t h) {
    if (!(flags & BIP_LABEL_SCALE)) return 1;
    if (!tapx || !tapy) return 0;
    for (int32_t x = 0; x < w; ++x)
        if (tapx[2 * x] < -1 || tapx[2 * x] > (w >= 2 ? w - 2 : 0)) return 0;
    for (int32_t y = 0; y < h; ++y)
        if (tapy[2 * y] < -1 || tapy[2 * y] > (h >= 2 ? h - 2 : 0)) return 0;
    return 1;
}

/* The whole map: out[y * w + x] = L4(x, y). The double loop the host function and the loader's host route are. */
static inline void bip_label_warp_map(const bip_label_sample *s, uint8_t *out) {
    for (int32_t y = 0; y < s->h; ++y)
        for (int32_t x = 0; x < s->w; ++x) out[(size_t)y * (size_t)s->w + (size_t)x] = (uint8_t)bip_label_warp(s, x, y);
}

#endif
