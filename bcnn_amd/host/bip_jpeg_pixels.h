/* bip_jpeg_pixels.h -- the ONE definition of the JPEG decoder's pixel arithmetic: everything behind the dequantised
 * coefficient blocks. Shared by the host decoder (bip_jpeg.c) and by the device pixel stage (../csrc/jpeg_pixels.hip), so
 * that both return the same bytes: the inverse DCT (Loeffler-Ligtenberg-Moschytz, 12-bit constants, 2 extra bits between
 * the column and the row pass), the chroma upsampling ("triangle" filters, nearest neighbour for the other ratios) with
 * the rule that picks the two source rows of an output row, and Y Cb Cr -> R G B in 20-bit fixed point. Plain C that also
 * compiles as HIP; every function is static inline, so nothing is exported.
 * All of it is integer arithmetic on independent blocks / output samples. The transform works modulo 2^32 (unsigned),
 * which is what the reference's int arithmetic amounts to on every target it runs on and keeps a corrupt stream's
 * oversized coefficients from being undefined behaviour. */
#ifndef BIP_JPEG_PIXELS_H
#define BIP_JPEG_PIXELS_H

#include <stdint.h>

#ifdef __HIPCC__
#define BIP_JPEG_INLINE __host__ __device__ static inline
#else
#define BIP_JPEG_INLINE static inline
#endif

typedef uint32_t bip_u32;
#define BIP_JPEG_FIX(x) ((int)((x) * 4096 + 0.5))
#define BIP_JPEG_UMUL(a, k) ((bip_u32)(a) * (bip_u32)(int32_t)(k))

BIP_JPEG_INLINE uint8_t bip_jpeg_clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

/* arithmetic shift right of the two's-complement value */
BIP_JPEG_INLINE int32_t bip_jpeg_sar(bip_u32 v, int n) {
    return (int32_t)(v >> n) | ((v & 0x80000000u) ? (int32_t)(~0u << (32 - n)) : 0);
}

/* one 8-point pass: even part in e[0..3], odd part in o[0..3] (both scaled by 4096); the caller combines e[i] +- o[3-i] */
BIP_JPEG_INLINE void bip_jpeg_idct8(int32_t s0, int32_t s1, int32_t s2, int32_t s3, int32_t s4, int32_t s5, int32_t s6,
                                    int32_t s7, bip_u32 e[4], bip_u32 o[4]) {
    const bip_u32 z = BIP_JPEG_UMUL((bip_u32)s2 + (bip_u32)s6, BIP_JPEG_FIX(0.5411961f));
    const bip_u32 a = z + BIP_JPEG_UMUL(s6, BIP_JPEG_FIX(-1.847759065f)), b = z + BIP_JPEG_UMUL(s2, BIP_JPEG_FIX(0.765366865f));
    const bip_u32 c = ((bip_u32)s0 + (bip_u32)s4) * 4096u, dd = ((bip_u32)s0 - (bip_u32)s4) * 4096u;
    e[0] = c + b; e[3] = c - b; e[1] = dd + a; e[2] = dd - a;
    const bip_u32 p3 = (bip_u32)s7 + (bip_u32)s3, p4 = (bip_u32)s5 + (bip_u32)s1, p1 = (bip_u32)s7 + (bip_u32)s1,
                  p2 = (bip_u32)s5 + (bip_u32)s3;
    const bip_u32 p5 = BIP_JPEG_UMUL(p3 + p4, BIP_JPEG_FIX(1.175875602f));
    const bip_u32 q1 = p5 + BIP_JPEG_UMUL(p1, BIP_JPEG_FIX(-0.899976223f)), q2 = p5 + BIP_JPEG_UMUL(p2, BIP_JPEG_FIX(-2.562915447f));
    const bip_u32 q3 = BIP_JPEG_UMUL(p3, BIP_JPEG_FIX(-1.961570560f)), q4 = BIP_JPEG_UMUL(p4, BIP_JPEG_FIX(-0.390180644f));
    o[3] = BIP_JPEG_UMUL(s1, BIP_JPEG_FIX(1.501321110f)) + q1 + q4;
    o[2] = BIP_JPEG_UMUL(s3, BIP_JPEG_FIX(3.072711026f)) + q2 + q3;
    o[1] = BIP_JPEG_UMUL(s5, BIP_JPEG_FIX(2.053119869f)) + q2 + q4;
    o[0] = BIP_JPEG_UMUL(s7, BIP_JPEG_FIX(0.298631336f)) + q1 + q3;
}

/* Column pass of one column: coefficients c[0], c[stride], ... c[7 * stride] -> mid[0..7], 2 extra bits of precision kept.
 * With all seven AC coefficients 0 every output is c[0] * 4: then e[i] = c[0] * 4096, o[i] = 0 and
 * sar(c[0] * 4096 + 512, 10) = c[0] * 4 because c[0] * 4096 is a multiple of 1024 and 512 < 1024. A caller may take that
 * shortcut (the host does, for speed) or not (the device does not): the values are the same. */
BIP_JPEG_INLINE void bip_jpeg_idct_column(const int16_t *c, int stride, int32_t mid[8]) {
    bip_u32 e[4], o[4];
    bip_jpeg_idct8(c[0], c[stride], c[2 * stride], c[3 * stride], c[4 * stride], c[5 * stride], c[6 * stride], c[7 * stride],
                   e, o);
    for (int i = 0; i < 4; ++i) {
        mid[i] = bip_jpeg_sar(e[i] + 512u + o[3 - i], 10);
        mid[7 - i] = bip_jpeg_sar(e[i] + 512u - o[3 - i], 10);
    }
}

/* Row pass of one row: removes 12 + 2 + 3 bits, re-centres on 128 and clamps. */
BIP_JPEG_INLINE void bip_jpeg_idct_row(const int32_t m[8], uint8_t row[8]) {
    bip_u32 e[4], o[4];
    bip_jpeg_idct8(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], e, o);
    for (int i = 0; i < 4; ++i) {
        const bip_u32 base = e[i] + 65536u + (128u << 17);
        row[i] = bip_jpeg_clamp255(bip_jpeg_sar(base + o[3 - i], 17));
        row[7 - i] = bip_jpeg_clamp255(bip_jpeg_sar(base - o[3 - i], 17));
    }
}

/* The coefficient block whose transform is 64 bytes of 0 (DC only: mid = -4096 in column 0, every row sums to
 * -2^24 + 65536 + 2^24 >> 17 = 0). bip_jpeg_read_coefficients leaves it where a baseline scan ended before it reached a
 * block, because the one-pass decoder left such a block of its zeroed plane untouched. */
#define BIP_JPEG_DC_OF_ZERO_BLOCK (-1024)

/* The two source rows of output row y for a component subsampled vs times vertically with `rows` content rows: the
 * nearer and the farther one. It is the closed form of stepping through the rows with a phase that starts at vs / 2:
 * in the lower half of a source row the next row is the nearer one, and the next row stops at the last content row. */
BIP_JPEG_INLINE void bip_jpeg_up_source_rows(int y, int vs, int rows, int *near_row, int *far_row) {
    const int t = y + (vs >> 1), q = t / vs;
    const int r1 = q < rows - 1 ? q : rows - 1;
    const int r0 = q < 1 ? 0 : (q - 1 < rows - 1 ? q - 1 : rows - 1);
    const int lower = t - q * vs >= (vs >> 1);
    *near_row = lower ? r1 : r0;
    *far_row = lower ? r0 : r1;
}

/* The blends of the "triangle" upsampling filters: two samples 3 : 1 (scaled by 4), its rounded quotient, and the blend
 * 3 : 1 of two such sums along the other axis (rounded, by 16). */
#define BIP_JPEG_UP_3TO1(a, b) (3 * (a) + (b))
#define BIP_JPEG_UP_DIV4(t) ((uint8_t)(((t) + 2) >> 2))
#define BIP_JPEG_UP_DIV16(t3, t1) ((uint8_t)((3 * (t3) + (t1) + 8) >> 4))

/* Sample x of the upsampled row (0 <= x < w * hs) from the nearer and the farther source row of w samples: the five
 * cases (1x1, vertical 2, horizontal 2, both, everything else), with the first / last column forms and the w == 1 forms
 * of the reference. The device calls it for every sample; the host calls it for the columns at the two ends of a row and
 * runs the same blends over the columns between them with the sums of a column kept for its neighbour. */
BIP_JPEG_INLINE uint8_t bip_jpeg_up_sample(const uint8_t *near_row, const uint8_t *far_row, int w, int hs, int vs, int x) {
    if (hs == 1 && vs == 1) return near_row[x];
    if (hs == 1 && vs == 2) return BIP_JPEG_UP_DIV4(BIP_JPEG_UP_3TO1(near_row[x], far_row[x]));
    if (hs == 2 && vs == 1) {
        if (w == 1 || x == 0) return near_row[0];
        if (x == 2 * w - 1) return near_row[w - 1];
        if (x == 2 * w - 2) return BIP_JPEG_UP_DIV4(BIP_JPEG_UP_3TO1(near_row[w - 2], near_row[w - 1])); /* sic: not the mirror of x == 1 */
        const int i = x >> 1;
        return BIP_JPEG_UP_DIV4(BIP_JPEG_UP_3TO1(near_row[i], near_row[(x & 1) ? i + 1 : i - 1]));
    }
    if (hs == 2 && vs == 2) { /* vertical blend (4x) of the two columns the sample lies between, then the horizontal one */
        const int i = x >> 1;
        const int cur = BIP_JPEG_UP_3TO1(near_row[i], far_row[i]);
        if (w == 1 || x == 0 || x == 2 * w - 1) return BIP_JPEG_UP_DIV4(cur);
        const int j = (x & 1) ? i + 1 : i - 1;
        return BIP_JPEG_UP_DIV16(cur, BIP_JPEG_UP_3TO1(near_row[j], far_row[j]));
    }
    return near_row[x / hs]; /* other ratios: nearest neighbour along the row, the nearer row vertically */
}

#define BIP_JPEG_CFIX(x) (((int)((x) * 4096.0f + 0.5f)) << 8)
BIP_JPEG_INLINE void bip_jpeg_ycc_to_rgb(int y, int cb, int cr, uint8_t out[3]) {
    const int yf = (y << 20) + (1 << 19), r_ = cr - 128, b_ = cb - 128;
    const int r = (yf + r_ * BIP_JPEG_CFIX(1.40200f)) >> 20;
    const int g = (int)(yf + (r_ * -BIP_JPEG_CFIX(0.71414f)) +
                        (int)(((unsigned)(b_ * -BIP_JPEG_CFIX(0.34414f))) & 0xffff0000u)) >> 20;
    const int b = (yf + b_ * BIP_JPEG_CFIX(1.77200f)) >> 20;
    out[0] = bip_jpeg_clamp255(r); out[1] = bip_jpeg_clamp255(g); out[2] = bip_jpeg_clamp255(b);
}

#endif
