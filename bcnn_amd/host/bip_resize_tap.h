/* bip_resize_tap.h -- the ONE definition of bip_resize_bilinear's sampling rule, shared by the host resize (bip_min.c)
 * and by the device input fill (../csrc/image_fill.hip), whose host side tabulates the taps for its kernel. Plain C
 * that also compiles as HIP; every function is static inline, so nothing is exported. */
#ifndef BIP_RESIZE_TAP_H
#define BIP_RESIZE_TAP_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BIP_TAP_INLINE __host__ __device__ static inline
#else
#define BIP_TAP_INLINE static inline
#endif

/* Source position of destination sample i: half-pixel centres, then clamped so that (index, index + 1) stays
 * inside the image; the fraction is quantised to 1/16 (reference bip.c:1118-1156). Host only. */
static inline void bip_resize_tap(size_t i, float scale, size_t src_extent, int32_t *index, int32_t *frac) {
    float alpha = (float)((i + 0.5) * scale - 0.5);
    long idx = (long)floor(alpha);
    alpha -= idx;
    if (idx < 0) { idx = 0; alpha = 0; }
    if (idx > (long)src_extent - 2) { idx = (long)src_extent - 2; alpha = 1; }
    if (idx < 0) { idx = 0; alpha = 0; } /* one-sample axis: replicate (the reference reads out of bounds here) */
    *index = (int32_t)idx;
    *frac = (int32_t)(alpha * 16 + 0.5);
}

/* The scale of one axis, as bip_resize_bilinear forms it. */
static inline float bip_resize_scale(size_t src_extent, size_t dst_extent) { return (float)src_extent / dst_extent; }

/* One output sample from its four neighbours (a0, a1 on the upper row, b0, b1 on the lower one): horizontal pass in
 * 1/16 units on both rows, vertical pass in 1/256 units, round to nearest. */
BIP_TAP_INLINE uint8_t bip_resize_blend(int32_t a0, int32_t a1, int32_t b0, int32_t b1, int32_t ax, int32_t ay) {
    const int32_t h0 = (a0 << 4) + (a1 - a0) * ax;
    const int32_t h1 = (b0 << 4) + (b1 - b0) * ax;
    return (uint8_t)(((h0 << 4) + (h1 - h0) * ay + 128) >> 8);
}

#endif
