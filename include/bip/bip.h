/* bip/bip.h -- the slice of the reference's image library (src/bip/inc/bip/bip.h) that unchanged consumers of
 * the public API call: src/cli/bcnn_cl.c dumps detection overlays with bip_write_image (:1872);
 * examples/inference_benchmark loads its test image with bip_load_image (:530) and fits it to the net input
 * with bip_resize_bilinear (:338). Own dependency-free implementations in bcnn_amd/host/bip_min.c and
 * bip_decode.c / bip_jpeg.c (libbip.so): PNG writer (stored deflate blocks), JPEG / PNG / PNM / BMP reader (JPEG with the
 * reference's -- stb_image's -- exact pixels, PNG with a full inflate),
 * and the reference's fixed-point bilinear resize (bit-identical, tests/test_bip.py); bip_augment.c holds the operations
 * of the online data augmenter (crop / shift, horizontal flip, rotation, contrast, brightness: bcnn_data.c:211-334),
 * byte for byte like the reference (tests/test_data_loader.py); bip_effects.c holds its last two, Perlin distortion and
 * random spotlights (tests/test_augment_effects.py). */
#ifndef BIP_H
#define BIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef enum { BIP_SUCCESS, BIP_INVALID_PTR, BIP_INVALID_SIZE, BIP_INVALID_PARAMETER, BIP_UNKNOWN_ERROR } bip_status;
typedef enum { NEAREST_NEIGHBOR, BILINEAR } bip_interpolation;
#define bip_deg2rad(x) (x) * 0.01745329252f

/* writes `src` (src_height rows of src_stride bytes, src_depth = 1, 3 or 4 interleaved channels) as a PNG file */
bip_status bip_write_image(char *filename, uint8_t *src, int32_t src_width, int32_t src_height, int32_t src_depth,
                           int32_t src_stride);
/* decodes an image file / buffer into a malloc'ed interleaved 8-bit image with the file's own channel count
 * (reference: stbi_load(..., 0)); the caller frees *src */
bip_status bip_load_image(char *filename, uint8_t **src, int32_t *src_width, int32_t *src_height, int32_t *src_depth);
bip_status bip_load_image_from_memory(unsigned char *buffer, int buffer_size, uint8_t **src, int32_t *src_width,
                                      int32_t *src_height, int32_t *src_depth);
/* A class-index mask: *map gets width x height bytes (malloc), one class index per pixel. Accepted: 8-bit grey PNG (its
 * values), 8-bit palette PNG (the INDICES, not the colours: VOC's SegmentationClass files), PNM P5 / P2 with maxval <= 255
 * (its values). Everything else -- RGB / RGBA / grey+alpha PNG, JPEG, BMP, colour PNM -- fails with BIP_UNKNOWN_ERROR and a
 * line on stderr that names the reason: a lossy or coloured mask has no class indices. */
bip_status bip_load_index_map(char *filename, uint8_t **map, int32_t *width, int32_t *height);
bip_status bip_load_index_map_from_memory(unsigned char *buffer, int buffer_size, uint8_t **map, int32_t *width,
                                          int32_t *height);
/* ---- the JPEG decoder split at the coefficient boundary (bip_jpeg.c): entropy decoding on one side, pixel arithmetic
 * (bcnn_amd/host/bip_jpeg_pixels.h) on the other; bip_load_image* is the three calls below in a row ---- */
typedef struct {
    int32_t h, v;               /* sampling factors */
    int32_t width, height;      /* samples that carry image content */
    int32_t pitch, rows;        /* the component's plane: whole MCUs */
    int32_t blocks_w, blocks_h; /* its 8 x 8 blocks; block (bx, by) is the 64 int16 at 64 * (by * blocks_w + bx) */
    int32_t idct_w, idct_h;     /* blocks (bx < idct_w, by < idct_h) that the pixel stage transforms: every block of a
                                   baseline stream, the ((width + 7) >> 3) x ((height + 7) >> 3) with content of a
                                   progressive one */
} bip_jpeg_component;
typedef struct {
    int32_t width, height, ncomp; /* ncomp: 1 (grey) or 3 (Y Cb Cr) */
    int32_t hmax, vmax, progressive;
    size_t num_coefficients;      /* int16 the caller provides: the components' blocks one after the other */
    bip_jpeg_component comp[3];
} bip_jpeg_info;
/* parses the stream up to and including its frame header; BIP_SUCCESS only for a stream the decoder covers so far */
bip_status bip_jpeg_frame_info(const uint8_t *buf, size_t len, bip_jpeg_info *info);
/* runs every scan and leaves the DEQUANTISED coefficient blocks in coeff[0 .. info->num_coefficients), row-major, 64 per
 * block. `info` is what bip_jpeg_frame_info returned for the same buffer (anything else is refused). Fails on everything
 * bip_load_image_from_memory fails on; writes nothing outside coeff. */
bip_status bip_jpeg_read_coefficients(const uint8_t *buf, size_t len, const bip_jpeg_info *info, int16_t *coeff);
/* the host pixel stage: inverse DCT, chroma upsampling, colour conversion into image[height][width][ncomp] */
bip_status bip_jpeg_pixels_from_coefficients(const bip_jpeg_info *info, const int16_t *coeff, uint8_t *image);
/* bilinear resize with half-pixel centres and 4-bit fixed-point weights per axis, depth 1..4 interleaved
 * channels, strides in bytes (reference src/bip/src/bip.c:1077-1200) */
bip_status bip_resize_bilinear(uint8_t *src, size_t src_width, size_t src_height, size_t src_stride, uint8_t *dst,
                               size_t dst_width, size_t dst_height, size_t dst_stride, size_t depth);
/* ---- the data augmenter's operations (interleaved 8-bit images, strides in bytes) ---- */
/* copies the overlap of the source rectangle at (x_ul, y_ul) into dst; negative origins shift the image right / down and
 * leave the uncovered part of dst as it was (reference bip.h:219) */
bip_status bip_crop_image(uint8_t *src, size_t src_width, size_t src_height, size_t src_stride, int32_t x_ul, int32_t y_ul,
                          uint8_t *dst, size_t dst_width, size_t dst_height, size_t dst_stride, size_t depth);
bip_status bip_fliph_image(uint8_t *src, size_t width, size_t height, size_t depth, size_t src_stride, uint8_t *dst,
                           size_t dst_stride);
/* rotation by `angle` radians around (center_x, center_y); pixels that map outside the source become 0 (bip.h:361) */
bip_status bip_rotate_image(uint8_t *src, size_t src_width, size_t src_height, size_t src_stride, uint8_t *dst,
                            size_t dst_width, size_t dst_height, size_t dst_stride, size_t depth, float angle,
                            int32_t center_x, int32_t center_y, bip_interpolation interpolation);
/* The label map that belongs to an augmented image: out[y * width + x] is one byte of `map` (width x height, dense) or
 * `fill`, by the rule of bcnn_amd/host/bip_label_warp.h -- the pull-back through horizontal flip, shift, scale and
 * rotation as the loader's record describes them (flags: bits 1 / 2 / 4 / 8; x_ul, y_ul; ca, sa = cos, sin * 65536; tapx /
 * tapy: width / height (index, fraction) int32 pairs of bip_resize_bilinear's rule, index -1 where the resized image does
 * not cover the column or row; read only with the scale bit). BIP_INVALID_PTR for a NULL map / out (or taps with the scale
 * bit), BIP_INVALID_SIZE for an extent < 1, BIP_INVALID_PARAMETER for fill outside 0 ... 255 or a tap index outside
 * [-1, max(extent - 2, 0)]; nothing is written then. */
bip_status bip_warp_label_map(const uint8_t *map, int32_t width, int32_t height, int32_t flags, int32_t x_ul, int32_t y_ul,
                              int32_t ca, int32_t sa, const int32_t *tapx, const int32_t *tapy, int32_t fill, uint8_t *out);
bip_status bip_contrast_stretch(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                                size_t dst_stride, float contrast);
bip_status bip_image_brightness(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                                size_t dst_stride, int32_t brightness);
/* ---- the augmenter's two effects (bip_effects.c; per-pixel arithmetic in bcnn_amd/host/bip_effects.h) ---- */
/* One octave of cosine-interpolated lattice noise, seeded by ONE rand() call made on entry, moves every pixel's source
 * position by noise * distortion (in units of the image extent) along both axes; four-tap float blend, truncated. A pixel
 * whose taps leave the image becomes 0: the last row and column always do, and an image of width or height 1 becomes
 * all 0. Both images are dense width x depth rows (the strides are not used), and may not overlap (bip.c:205-266). */
bip_status bip_image_perlin_distortion(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth,
                                       uint8_t *dst, size_t dst_stride, float distortion, float kx, float ky);
/* num_spots Gaussian spots one after the other, each drawn with FOUR rand() calls (centre x, centre y in the image; sigma
 * x, sigma y in [min + 0.5, max + 0.5]): every byte becomes (uint8)clamp(255 * exp(-(dx^2 / sx^2 + dy^2 / sy^2) / 2) +
 * byte, 0, 255), truncated per spot. src == dst works in place (bip.c:268-316). */
bip_status bip_add_random_spotlights(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                                     size_t dst_stride, uint32_t num_spots, float min_spot_width, float max_spot_width,
                                     float min_spot_height, float max_spot_height);
/* The same pixels from draws the caller has made (not in the reference): the seed; the spot list. bip_draw_spot makes the
 * four draws of one spot. */
typedef struct { int32_t mu_x, mu_y; float sigma_x, sigma_y; } bip_spot;
bip_status bip_perlin_distortion_seeded(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth,
                                        uint8_t *dst, size_t dst_stride, float distortion, float kx, float ky, int32_t seed);
bip_status bip_add_spotlights(uint8_t *src, size_t src_stride, size_t width, size_t height, size_t depth, uint8_t *dst,
                              size_t dst_stride, const bip_spot *spots, uint32_t num_spots);
void bip_draw_spot(size_t width, size_t height, float min_spot_width, float max_spot_width, float min_spot_height,
                   float max_spot_height, bip_spot *spot);
/* What a device needs instead of cos and exp. bip_perlin_axis: for the `extent` columns (rows) of an image and the
 * offset kx (ky), the normalised coordinate, the cosine weight and the lattice cell of the noise argument, `extent`
 * values each. bip_spot_table: `val` of one spot over the box of `radius` around its centre clipped to the image,
 * box = {x0, y0, bw, bh}, row-major bw x bh floats (room for (2 radius + 1)^2); bip_apply_spot_table applies one such
 * table in place and leaves every pixel outside the box alone. */
void bip_perlin_axis(size_t extent, float k, float *norm, float *weight, int32_t *cell);
bip_status bip_spot_table(const bip_spot *spot, size_t width, size_t height, int32_t radius, int32_t box[4], float *val);
bip_status bip_apply_spot_table(uint8_t *img, size_t stride, size_t width, size_t height, size_t depth, const int32_t box[4],
                                const float *val);
#ifdef __cplusplus
}
#endif
#endif
