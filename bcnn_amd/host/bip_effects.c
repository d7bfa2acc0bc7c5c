/* bip_effects.c -- libbip.so: the last two operations of the online data augmenter, Perlin distortion and random
 * spotlights (reference src/bip/src/bip.c:154-316), byte for byte like the reference for the same rand() state
 * (tests/test_augment_effects.py compares against the compiled reference).
 *   bip_image_perlin_distortion / bip_add_random_spotlights  the reference's signatures: they make the reference's rand()
 *        draws (the distortion's seed; mu_x, mu_y, sigma_x, sigma_y per spot) and call the forms below
 *   bip_perlin_distortion_seeded / bip_add_spotlights        the same pixels from draws the caller made: what the data
 *        loader's pixel step calls (bcnn_data.c)
 *   bip_perlin_axis / bip_spot_table / bip_apply_spot_table  what the device loader path sends up instead of calling cos
 *        and exp there: per column and per row of a sample the cell, the cosine weight and the normalised coordinate of
 *        the noise argument; per spot the table of `val` over a box around its centre. The seeded distortion above is
 *        written on bip_perlin_axis, so the tables are checked whenever the host function is.
 * The per-pixel arithmetic is bip_effects.h's, which ../csrc/augment.hip includes as well. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bip/bip.h"
#include "bip_effects.h"

#define BIP_PI 3.14159265358979f /* a float, like the reference's */

/* The noise argument along one axis of `extent` samples, offset k: for sample i, norm[i] = (float)i / extent, and of
 * norm[i] + k the integer part cell[i] (floor) and the cosine weight of the fraction, weight[i] = (1 - cos(frac * pi)) / 2
 * with a float pi, a double cos and float arithmetic around it (_bip_smooth2d, _bip_interpolate). */
void bip_perlin_axis(size_t extent, float k, float *norm, float *weight, int32_t *cell) {
    for (size_t i = 0; i < extent; ++i) {
        const float n = (float)i / extent;
        const float arg = n + k;
        const double fl = floor(arg);
        const int32_t c = (fl >= -2147483648.0 && fl < 2147483648.0) ? (int32_t)fl : INT32_MIN; /* (int) on x86-64 */
        const float frac = arg - c;
        norm[i] = n;
        cell[i] = c;
        weight[i] = (1.0f - (float)cos(frac * BIP_PI)) * 0.5f;
    }
}

bip_status bip_perlin_distortion_seeded(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth,
                                        uint8_t *dst, size_t dst_stride, float distortion, float kx, float ky, int32_t seed) {
    (void)src_stride; /* like the reference, both images are addressed as dense width x depth rows */
    (void)dst_stride;
    if (width == 0 || height == 0) return BIP_INVALID_SIZE;
    if (!src || !dst) return BIP_INVALID_PTR;
    float *tab = (float *)malloc((width + height) * (2 * sizeof(float) + sizeof(int32_t)));
    if (!tab) return BIP_UNKNOWN_ERROR;
    float *norm_x = tab, *norm_y = tab + width, *wx = norm_y + height, *wy = wx + width;
    int32_t *cx = (int32_t *)(wy + height), *cy = cx + width;
    bip_perlin_axis(width, kx, norm_x, wx, cx);
    bip_perlin_axis(height, ky, norm_y, wy, cy);
    const float fw = (float)width, fh = (float)height;
    for (size_t y = 0; y < height; ++y) {
        uint8_t *row = dst + y * depth * width;
        for (size_t x = 0; x < width; ++x) {
            const float noise = bip_perlin_noise(cx[x], cy[y], wx[x], wy[y], seed);
            int32_t ix, iy;
            float xd, yd;
            if (!bip_distort_map(norm_x[x], norm_y[y], noise, distortion, fw, fh, (int32_t)width, (int32_t)height, &ix, &iy,
                                 &xd, &yd)) {
                memset(row + x * depth, 0, depth);
                continue;
            }
            const uint8_t *p00 = src + ((size_t)iy * width + (size_t)ix) * depth;
            const uint8_t *p01 = p00 + depth, *p10 = p00 + width * depth, *p11 = p10 + depth;
            for (size_t k = 0; k < depth; ++k)
                row[x * depth + k] = bip_distort_blend((float)p00[k], (float)p01[k], (float)p10[k], (float)p11[k], xd, yd);
        }
    }
    free(tab);
    return BIP_SUCCESS;
}

bip_status bip_image_perlin_distortion(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth,
                                       uint8_t *dst, size_t dst_stride, float distortion, float kx, float ky) {
    const int32_t seed = rand(); /* before the checks, like the reference */
    return bip_perlin_distortion_seeded(src, src_stride, width, height, depth, dst, dst_stride, distortion, kx, ky, seed);
}

bip_status bip_add_spotlights(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                              size_t dst_stride, const bip_spot *spots, uint32_t num_spots) {
    (void)src_stride; /* the reference copies width * height * depth dense bytes */
    if (width == 0 || height == 0) return BIP_INVALID_SIZE;
    if (!src || !dst || (num_spots && !spots)) return BIP_INVALID_PTR;
    if (dst != src) memcpy(dst, src, width * height * depth);
    for (uint32_t i = 0; i < num_spots; ++i) {
        const float isx = 1 / (spots[i].sigma_x * spots[i].sigma_x), isy = 1 / (spots[i].sigma_y * spots[i].sigma_y);
        for (int y = 0; y < (int)height; ++y) {
            uint8_t *row = dst + (size_t)y * dst_stride;
            for (int x = 0; x < (int)width; ++x) {
                const float val = (float)exp(bip_spot_exponent(isx, isy, x - spots[i].mu_x, y - spots[i].mu_y));
                for (size_t c = 0; c < depth; ++c) row[depth * x + c] = bip_spot_add(val, row[depth * x + c]);
            }
        }
    }
    return BIP_SUCCESS;
}

/* the reference's two static helpers: one rand() each, + 0.5 in DOUBLE */
static int spot_rand_between(int min, int max) {
    if (min > max) return 0;
    return (int)(((float)rand() / RAND_MAX * (max - min)) + min + 0.5);
}
static float spot_frand_between(float min, float max) {
    if (min > max) return 0.f;
    return (float)(((float)rand() / RAND_MAX * (max - min)) + min + 0.5);
}

void bip_draw_spot(size_t width, size_t height, float min_spot_width, float max_spot_width, float min_spot_height,
                   float max_spot_height, bip_spot *spot) {
    spot->mu_x = spot_rand_between(0, (int)(width - 1));
    spot->mu_y = spot_rand_between(0, (int)(height - 1));
    spot->sigma_x = spot_frand_between(min_spot_width, max_spot_width);
    spot->sigma_y = spot_frand_between(min_spot_height, max_spot_height);
}

bip_status bip_add_random_spotlights(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                                     size_t dst_stride, uint32_t num_spots, float min_spot_width, float max_spot_width,
                                     float min_spot_height, float max_spot_height) {
    if (width == 0 || height == 0) return BIP_INVALID_SIZE;
    if (!src || !dst) return BIP_INVALID_PTR;
    if (dst != src) memcpy(dst, src, width * height * depth);
    for (uint32_t i = 0; i < num_spots; ++i) { /* draw, apply, draw, apply: any number of spots, no list */
        bip_spot s;
        bip_draw_spot(width, height, min_spot_width, max_spot_width, min_spot_height, max_spot_height, &s);
        bip_add_spotlights(dst, dst_stride, width, height, depth, dst, dst_stride, &s, 1);
    }
    return BIP_SUCCESS;
}

/* `val` of one spot over the box of `radius` around its centre, clipped to the width x height image: box = {x0, y0, bw,
 * bh}, val[(y - y0) * bw + (x - x0)] for the pixels inside. `val` has room for (2 radius + 1)^2 floats. */
bip_status bip_spot_table(const bip_spot *spot, size_t width, size_t height, int32_t radius, int32_t box[4], float *val) {
    if (!spot || !box || !val) return BIP_INVALID_PTR;
    if (width == 0 || height == 0 || width > 0x7fffffff || height > 0x7fffffff) return BIP_INVALID_SIZE;
    if (radius < 0 || radius > (1 << 12) || spot->mu_x < 0 || spot->mu_x >= (int32_t)width || spot->mu_y < 0 ||
        spot->mu_y >= (int32_t)height)
        return BIP_INVALID_PARAMETER;
    const int32_t x0 = spot->mu_x - radius < 0 ? 0 : spot->mu_x - radius, y0 = spot->mu_y - radius < 0 ? 0 : spot->mu_y - radius;
    const int32_t x1 = spot->mu_x + radius >= (int32_t)width ? (int32_t)width - 1 : spot->mu_x + radius;
    const int32_t y1 = spot->mu_y + radius >= (int32_t)height ? (int32_t)height - 1 : spot->mu_y + radius;
    const float isx = 1 / (spot->sigma_x * spot->sigma_x), isy = 1 / (spot->sigma_y * spot->sigma_y);
    box[0] = x0; box[1] = y0; box[2] = x1 - x0 + 1; box[3] = y1 - y0 + 1;
    for (int32_t y = y0; y <= y1; ++y)
        for (int32_t x = x0; x <= x1; ++x)
            val[(size_t)(y - y0) * box[2] + (x - x0)] = (float)exp(bip_spot_exponent(isx, isy, x - spot->mu_x, y - spot->mu_y));
    return BIP_SUCCESS;
}

/* One spot from its table, in place: what the device does with it. Pixels outside the box keep their bytes. */
bip_status bip_apply_spot_table(uint8_t *img, size_t stride, size_t width, size_t height, size_t depth, const int32_t box[4],
                                const float *val) {
    if (!img || !box || !val) return BIP_INVALID_PTR;
    if (box[0] < 0 || box[1] < 0 || box[2] < 1 || box[3] < 1 || (size_t)box[0] + box[2] > width || (size_t)box[1] + box[3] > height)
        return BIP_INVALID_PARAMETER;
    for (int32_t y = 0; y < box[3]; ++y) {
        uint8_t *row = img + (size_t)(y + box[1]) * stride + (size_t)box[0] * depth;
        for (int32_t x = 0; x < box[2]; ++x)
            for (size_t c = 0; c < depth; ++c) row[depth * x + c] = bip_spot_add(val[(size_t)y * box[2] + x], row[depth * x + c]);
    }
    return BIP_SUCCESS;
}
