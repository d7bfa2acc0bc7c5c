/* bip_effects.h -- the ONE definition of the per-pixel arithmetic of the augmenter's two effects, Perlin distortion and
 * random spotlights (reference src/bip/src/bip.c:154-316), shared by the host functions (bip_effects.c) and by the device
 * loader's convert kernel (../csrc/augment.hip). Plain C that also compiles as HIP; every function is static inline, so
 * nothing is exported. Nothing here calls cos, exp or a division whose divisor is no power of two: those steps are made
 * once, on the host, with libm (bip_perlin_axis and bip_spot_table in bip_effects.c), and reach the device as tables. What
 * is left is integer work and fp32 products and sums in the reference's order, which both sides must compile uncontracted
 * (no FMA: -ffp-contract=off for the kernels; the host build targets baseline x86-64). */
#ifndef BIP_EFFECTS_H
#define BIP_EFFECTS_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BIP_FX_INLINE __host__ __device__ static inline
#else
#define BIP_FX_INLINE static inline
#endif

/* The lattice value of octave 0 at (x, y): the reference's integer hash (_bip_noise2d) overflows a signed int, which its
 * compiler wraps; the same bits in uint32_t here. The quotient is exact (a 31-bit integer rounded to float once, then
 * divided by 2^30). */
BIP_FX_INLINE float bip_perlin_lattice(int32_t x, int32_t y, int32_t seed) {
    const uint32_t i = (uint32_t)x * 1619u + (uint32_t)y * 31337u + (uint32_t)seed * 13397u;
    const uint32_t n = (i << 13) ^ i;
    const uint32_t m = (n * (n * n * 15731u + 789221u) + 1376312589u) & 0x7fffffffu;
    return 1.0f - (float)(int32_t)m / 1073741824.0f;
}

BIP_FX_INLINE float bip_perlin_mix(float v1, float v2, float t) { return v1 * (1.0f - t) + v2 * t; }

/* One octave, persistence 0 (_bip_perlin_noise2d with octaves = 1): the smoothed noise of the cell (ix, iy) at the cosine
 * weights (tx, ty) of the fractions. ix and tx depend on the column alone, iy and ty on the row alone (bip_perlin_axis). */
BIP_FX_INLINE float bip_perlin_noise(int32_t ix, int32_t iy, float tx, float ty, int32_t seed) {
    const float v1 = bip_perlin_lattice(ix, iy, seed);
    const float v2 = bip_perlin_lattice((int32_t)((uint32_t)ix + 1u), iy, seed);
    const float v3 = bip_perlin_lattice(ix, (int32_t)((uint32_t)iy + 1u), seed);
    const float v4 = bip_perlin_lattice((int32_t)((uint32_t)ix + 1u), (int32_t)((uint32_t)iy + 1u), seed);
    const float i1 = bip_perlin_mix(v1, v2, tx);
    const float i2 = bip_perlin_mix(v3, v4, tx);
    float total = 0.0f;
    total += bip_perlin_mix(i1, i2, ty) * 1.0f;
    return total;
}

/* (int)p as the reference's x86-64 code converts it: INT32_MIN for a value that has no int (too large, NaN). Such a
 * position fails the range test below on every target. */
BIP_FX_INLINE int32_t bip_trunc_i32(float p) {
    return (p >= -2147483648.0f && p < 2147483648.0f) ? (int32_t)p : INT32_MIN;
}

/* Where destination pixel (x, y) of a width x height image reads: norm_x = (float)x / width, norm_y likewise, fw / fh the
 * extents as floats; the SAME noise value moves both coordinates. *ix / *iy truncate towards zero while the fractions come
 * from floor(): for -1 < p < 0 the two disagree, as in the reference. Returns 1 when the four taps (ix, iy) .. (ix + 1,
 * iy + 1) lie inside the image -- the reference's unsigned compare against extent - 1, which no pixel of an image of
 * width or height 1 passes; the pixel is 0 otherwise. */
BIP_FX_INLINE int bip_distort_map(float norm_x, float norm_y, float noise, float distortion, float fw, float fh, int32_t width,
                                  int32_t height, int32_t *ix, int32_t *iy, float *x_diff, float *y_diff) {
    const float px = (norm_x + noise * distortion) * fw;
    const float py = (norm_y + noise * distortion) * fh;
    *ix = bip_trunc_i32(px);
    *iy = bip_trunc_i32(py);
    *x_diff = px - floorf(px);
    *y_diff = py - floorf(py);
    return (uint32_t)*ix < (uint32_t)(width - 1) && (uint32_t)*iy < (uint32_t)(height - 1);
}

/* The four taps blended: four products of three fp32 factors, summed left to right, truncated to 8 bits. */
BIP_FX_INLINE uint8_t bip_distort_blend(float p00, float p01, float p10, float p11, float x_diff, float y_diff) {
    const float level = p00 * (1 - x_diff) * (1 - y_diff) + p01 * (x_diff) * (1 - y_diff) + p10 * (1 - x_diff) * (y_diff) +
                        p11 * (x_diff) * (y_diff);
    return (uint8_t)level;
}

/* The exponent of one spot at offset (dx, dy) from its centre, before exp(): the inner sum in fp32, in this association. */
BIP_FX_INLINE float bip_spot_exponent(float inv_sigma2_x, float inv_sigma2_y, int32_t dx, int32_t dy) {
    return -0.5f * (inv_sigma2_x * dx * dx + inv_sigma2_y * dy * dy);
}

/* One spot on one byte: val = (float)exp((double)bip_spot_exponent(..)). Truncated per spot. */
BIP_FX_INLINE uint8_t bip_spot_add(float val, uint8_t level) {
    const float v = 255.0f * val + level;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

#endif
