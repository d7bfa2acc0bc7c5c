/* bip_jpeg.c -- libbip.so: JPEG decoding for bip_load_image / bip_load_image_from_memory.
 *
 * The reference decodes images through stb_image 2.08 (src/bip/thirdparty/stb_image/stb_image.h, called from
 * src/bip/src/bip.c:1837-1870 with req_comp = 0), and its list-file dataset readers and examples/inference_benchmark are
 * normally fed .jpg files. A JPEG decoder is only a drop-in here if it returns the SAME PIXELS, because the decoded bytes
 * go straight into the augmenter and the input tensor: the lossy part of JPEG -- inverse DCT, chroma upsampling,
 * YCbCr -> RGB -- is implementation-defined, so this file follows that library's published arithmetic step by step:
 *   - 8-bit Huffman JPEG, baseline / extended sequential (SOF0, SOF1) and progressive (SOF2), 1 or 3 components,
 *     sampling factors 1..4, restart intervals, 8-bit quantisation tables; everything else is refused;
 *   - coefficients are dequantised in 16-bit arithmetic; the inverse DCT is the Loeffler-Ligtenberg-Moschytz integer
 *     transform with 12-bit constants, 2 extra bits kept between the column and the row pass, rounding constants
 *     512 / 65536 + (128 << 17), shifts 10 / 17;
 *   - chroma planes are brought to full resolution row by row with the "triangle" filters (3 near + 1 far) / 4
 *     (one axis) and (9, 3, 3, 1) / 16 (both axes), nearest neighbour for the other ratios;
 *   - Y, Cb, Cr -> R, G, B in 20-bit fixed point with the constants 1.402, 0.71414, 0.34414, 1.772 rounded to 12 bits
 *     and the Cb term of green truncated to its upper 16 bits; a one-component file yields one channel.
 * tests/test_bip.py compares every supported variant (subsampling 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 / 4:1:1, grey,
 * progressive, restart markers, odd sizes, qualities 5..100) byte for byte with the reference's loader. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bip/bip.h"
#include "bip_jpeg_pixels.h"

/* zig-zag position -> row-major index of the 8 x 8 block */
static const uint8_t k_unzig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

typedef struct {
    /* canonical Huffman code: symbols in code order, first code / first symbol index per length, and a 9-bit prefix table */
    uint8_t symbols[256];
    int32_t first_code[18]; /* first code of length L, left-justified to 16 bits; [17] = sentinel */
    int32_t first_index[17];
    int32_t end_code[18]; /* one past the last code of length L, left-justified */
    uint16_t quick[512];  /* (length << 8) | symbol for codes of <= 9 bits, 0 = longer */
    int defined;
} jhuff;

typedef struct {
    int id, h, v, tq, dc_table, ac_table;
    int dc_pred;
    int width, height;     /* samples that carry image content */
    int pitch, rows;       /* allocated plane: whole MCUs */
    int blocks_w, blocks_h;
    int16_t *coeff; /* all coefficient blocks of the component, in the caller's memory */
} jcomp;

typedef struct {
    const uint8_t *p, *end;
    uint32_t bits;  /* left-justified bit reservoir */
    int nbits;
    int marker;     /* marker met while refilling (0 = none); after it the reservoir is fed zeros */
    uint8_t qt[4][64]; /* row-major */
    jhuff dc[4], ac[4];
    jcomp comp[3];
    int ncomp, width, height, hmax, vmax, mcus_x, mcus_y;
    int progressive, restart_interval;
    /* current scan */
    int scan_n, scan_comp[3], ss, se, ah, al, eob_run, todo;
} jdec;

/* ---- byte / bit input ------------------------------------------------------------------------------------------------ */
static int get8(jdec *d) { return d->p < d->end ? *d->p++ : 0; }
static int get16(jdec *d) { const int a = get8(d); return (a << 8) | get8(d); }

static void refill(jdec *d) {
    while (d->nbits <= 24) {
        int b = 0;
        if (!d->marker) {
            b = get8(d);
            if (b == 0xff) {
                const int c = get8(d);
                if (c != 0) { /* a marker ends the entropy-coded segment: zeros from here on */
                    d->marker = c;
                    b = 0;
                }
            }
        }
        d->bits |= (uint32_t)b << (24 - d->nbits);
        d->nbits += 8;
    }
}

static int take_bits(jdec *d, int n) { /* n in 1..16 */
    if (d->nbits < n) refill(d);
    const uint32_t v = d->bits >> (32 - n);
    d->bits <<= n;
    d->nbits -= n;
    return (int)v;
}
static int take_bit(jdec *d) { return take_bits(d, 1); }

/* n magnitude bits -> signed value (the "extend" procedure of the standard, F.2.2.1) */
static int take_signed(jdec *d, int n) {
    const int v = take_bits(d, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

static int huff_build(jhuff *h, const int counts[16], const uint8_t *symbols, int nsym) {
    int code = 0, k = 0;
    memset(h->quick, 0, sizeof(h->quick));
    memcpy(h->symbols, symbols, (size_t)nsym);
    for (int len = 1; len <= 16; ++len) {
        h->first_index[len] = k;
        h->first_code[len] = code << (16 - len);
        for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
            if (code >= (1 << len) || k >= nsym) return 0; /* more codes than the length can hold / than symbols given */
            if (len <= 9)
                for (int fill = 0; fill < (1 << (9 - len)); ++fill)
                    h->quick[(code << (9 - len)) + fill] = (uint16_t)((len << 8) | symbols[k]);
        }
        h->end_code[len] = code << (16 - len);
        code <<= 1;
    }
    h->end_code[17] = 0x7fffffff;
    h->defined = 1;
    return 1;
}

static int huff_symbol(jdec *d, const jhuff *h) {
    if (d->nbits < 16) refill(d);
    const uint16_t q = h->quick[d->bits >> 23];
    if (q) {
        d->bits <<= q >> 8;
        d->nbits -= q >> 8;
        return q & 0xff;
    }
    const int32_t top = (int32_t)(d->bits >> 16);
    for (int len = 10; len <= 16; ++len)
        if (top < h->end_code[len]) {
            const int idx = h->first_index[len] + ((top - h->first_code[len]) >> (16 - len));
            d->bits <<= len;
            d->nbits -= len;
            return h->symbols[idx & 255];
        }
    return -1;
}

/* ---- inverse DCT (the arithmetic is bip_jpeg_pixels.h's) ------------------------------------------------------------- */
static void idct_block(uint8_t *out, int pitch, const int16_t c[64]) {
    int32_t mid[64], col[8];
    for (int x = 0; x < 8; ++x) { /* columns */
        if (!(c[x + 8] | c[x + 16] | c[x + 24] | c[x + 32] | c[x + 40] | c[x + 48] | c[x + 56])) {
            const int32_t dc = c[x] * 4; /* what the general pass yields for it (see bip_jpeg_idct_column); quicker */
            for (int y = 0; y < 8; ++y) mid[8 * y + x] = dc;
            continue;
        }
        bip_jpeg_idct_column(c + x, 8, col);
        for (int y = 0; y < 8; ++y) mid[8 * y + x] = col[y];
    }
    for (int y = 0; y < 8; ++y) bip_jpeg_idct_row(mid + 8 * y, out + (size_t)y * pitch);
}

/* ---- coefficient decoding --------------------------------------------------------------------------------------------- */
static int block_sequential(jdec *d, jcomp *c, int16_t blk[64]) {
    const jhuff *hd = &d->dc[c->dc_table], *ha = &d->ac[c->ac_table];
    const uint8_t *q = d->qt[c->tq];
    memset(blk, 0, 64 * sizeof(int16_t));
    const int t = huff_symbol(d, hd);
    if (t < 0 || t > 15) return 0;
    c->dc_pred += t ? take_signed(d, t) : 0;
    blk[0] = (int16_t)(c->dc_pred * q[0]);
    for (int k = 1; k < 64;) {
        const int rs = huff_symbol(d, ha);
        if (rs < 0) return 0;
        const int run = rs >> 4, size = rs & 15;
        if (size == 0) {
            if (rs != 0xf0) break; /* end of block */
            k += 16;
            continue;
        }
        k += run;
        if (k > 63) return 0;
        const int at = k_unzig[k++];
        blk[at] = (int16_t)(take_signed(d, size) * q[at]);
    }
    return 1;
}

static int block_prog_dc(jdec *d, jcomp *c, int16_t blk[64]) {
    if (d->se != 0) return 0;
    if (d->ah == 0) { /* first pass of the DC coefficient */
        memset(blk, 0, 64 * sizeof(int16_t));
        const int t = huff_symbol(d, &d->dc[c->dc_table]);
        if (t < 0 || t > 15) return 0;
        c->dc_pred += t ? take_signed(d, t) : 0;
        blk[0] = (int16_t)(c->dc_pred * (1 << d->al));
    } else if (take_bit(d)) { /* refinement: one more bit */
        blk[0] += (int16_t)(1 << d->al);
    }
    return 1;
}

/* correction bit of an already non-zero coefficient during a refinement pass */
static void refine_nonzero(jdec *d, int16_t *p, int16_t bit) {
    if (take_bit(d) && (*p & bit) == 0) *p = (int16_t)(*p > 0 ? *p + bit : *p - bit);
}

static int block_prog_ac(jdec *d, jcomp *c, int16_t blk[64]) {
    const jhuff *ha = &d->ac[c->ac_table];
    if (d->ss == 0) return 0;
    if (d->ah == 0) { /* first pass over the band ss..se */
        if (d->eob_run) { --d->eob_run; return 1; }
        for (int k = d->ss; k <= d->se;) {
            const int rs = huff_symbol(d, ha);
            if (rs < 0) return 0;
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (run < 15) { /* end of band for 2^run (+ extra bits) blocks, this one included */
                    d->eob_run = (1 << run) + (run ? take_bits(d, run) : 0) - 1;
                    break;
                }
                k += 16;
                continue;
            }
            k += run;
            if (k > 63) return 0;
            blk[k_unzig[k++]] = (int16_t)(take_signed(d, size) * (1 << d->al));
        }
        return 1;
    }
    /* refinement pass: every non-zero coefficient met gets a correction bit, new coefficients enter as +-(1 << al) */
    const int16_t bit = (int16_t)(1 << d->al);
    if (d->eob_run) {
        --d->eob_run;
        for (int k = d->ss; k <= d->se; ++k) {
            int16_t *p = &blk[k_unzig[k]];
            if (*p) refine_nonzero(d, p, bit);
        }
        return 1;
    }
    for (int k = d->ss; k <= d->se;) {
        const int rs = huff_symbol(d, ha);
        if (rs < 0) return 0;
        int run = rs >> 4, value = 0;
        const int size = rs & 15;
        if (size == 0) {
            if (run < 15) {
                d->eob_run = (1 << run) - 1 + (run ? take_bits(d, run) : 0);
                run = 64; /* the rest of the band only gets correction bits */
            }
        } else {
            if (size != 1) return 0;
            value = take_bit(d) ? bit : -bit;
        }
        while (k <= d->se) { /* skip `run` zero coefficients, correcting the non-zero ones on the way */
            int16_t *p = &blk[k_unzig[k++]];
            if (*p) {
                refine_nonzero(d, p, bit);
            } else {
                if (run == 0) { *p = (int16_t)value; break; }
                --run;
            }
        }
    }
    return 1;
}

/* ---- scans -------------------------------------------------------------------------------------------------------------- */
static void restart(jdec *d) {
    d->bits = 0; d->nbits = 0; d->marker = 0; d->eob_run = 0;
    for (int i = 0; i < 3; ++i) d->comp[i].dc_pred = 0;
    d->todo = d->restart_interval ? d->restart_interval : 0x7fffffff;
}

/* after each MCU: at the end of a restart interval the next marker must be RSTn; 0 = stop decoding this scan */
static int mcu_done(jdec *d) {
    if (--d->todo > 0) return 1;
    if (d->nbits < 24) refill(d);
    if (d->marker < 0xd0 || d->marker > 0xd7) return 0;
    restart(d);
    return 1;
}

static int one_block(jdec *d, jcomp *c, int bx, int by) {
    int16_t *blk = c->coeff + 64 * ((size_t)by * c->blocks_w + bx);
    if (d->progressive) return d->ss == 0 ? block_prog_dc(d, c, blk) : block_prog_ac(d, c, blk);
    return block_sequential(d, c, blk);
}

static int decode_scan(jdec *d) {
    restart(d);
    if (d->scan_n == 1) { /* one component: its blocks in raster order, only those that carry image content */
        jcomp *c = &d->comp[d->scan_comp[0]];
        const int bw = (c->width + 7) >> 3, bh = (c->height + 7) >> 3;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                if (!one_block(d, c, bx, by)) return 0;
                if (!mcu_done(d)) return 1;
            }
        return 1;
    }
    if (d->progressive && d->ss != 0) return 0; /* AC scans are never interleaved */
    for (int my = 0; my < d->mcus_y; ++my)
        for (int mx = 0; mx < d->mcus_x; ++mx) {
            for (int k = 0; k < d->scan_n; ++k) {
                jcomp *c = &d->comp[d->scan_comp[k]];
                for (int y = 0; y < c->v; ++y)
                    for (int x = 0; x < c->h; ++x)
                        if (!one_block(d, c, mx * c->h + x, my * c->v + y)) return 0;
            }
            if (!mcu_done(d)) return 1;
        }
    return 1;
}

/* ---- markers -------------------------------------------------------------------------------------------------------------- */
static int next_marker(jdec *d) { /* 0xff = none */
    if (d->marker) { const int m = d->marker; d->marker = 0; return m; }
    int x = get8(d);
    if (x != 0xff) return 0xff;
    while (x == 0xff && d->p < d->end) x = get8(d);
    return x;
}

static int read_tables(jdec *d, int m) {
    if (m == 0xdd) { /* DRI */
        if (get16(d) != 4) return 0;
        d->restart_interval = get16(d);
        return 1;
    }
    if (m == 0xdb) { /* DQT, 8-bit entries only */
        int left = get16(d) - 2;
        while (left > 0) {
            const int pt = get8(d);
            if ((pt >> 4) != 0 || (pt & 15) > 3) return 0;
            for (int i = 0; i < 64; ++i) d->qt[pt & 15][k_unzig[i]] = (uint8_t)get8(d);
            left -= 65;
        }
        return left == 0;
    }
    if (m == 0xc4) { /* DHT */
        int left = get16(d) - 2;
        while (left > 0) {
            const int tt = get8(d);
            int counts[16], n = 0;
            uint8_t symbols[256];
            if ((tt >> 4) > 1 || (tt & 15) > 3) return 0;
            for (int i = 0; i < 16; ++i) n += counts[i] = get8(d);
            if (n > 256) return 0;
            for (int i = 0; i < n; ++i) symbols[i] = (uint8_t)get8(d);
            if (!huff_build((tt >> 4) ? &d->ac[tt & 15] : &d->dc[tt & 15], counts, symbols, n)) return 0;
            left -= 17 + n;
        }
        return left == 0;
    }
    if ((m >= 0xe0 && m <= 0xef) || m == 0xfe) { /* APPn, COM */
        const int len = get16(d) - 2;
        if (len < 0 || d->p + len > d->end) return 0;
        d->p += len;
        return 1;
    }
    return 0;
}

static int read_frame(jdec *d) {
    const int len = get16(d);
    if (len < 11 || get8(d) != 8) return 0; /* 8-bit samples only */
    d->height = get16(d);
    d->width = get16(d);
    d->ncomp = get8(d);
    if (!d->height || !d->width || (d->ncomp != 1 && d->ncomp != 3) || len != 8 + 3 * d->ncomp) return 0;
    if ((1 << 30) / d->width / d->ncomp < d->height) return 0;
    d->hmax = d->vmax = 1;
    for (int i = 0; i < d->ncomp; ++i) {
        jcomp *c = &d->comp[i];
        c->id = get8(d);
        if (c->id != i + 1 && c->id != i) return 0;
        const int hv = get8(d);
        c->h = hv >> 4; c->v = hv & 15; c->tq = get8(d);
        if (c->h < 1 || c->h > 4 || c->v < 1 || c->v > 4 || c->tq > 3) return 0;
        if (c->h > d->hmax) d->hmax = c->h;
        if (c->v > d->vmax) d->vmax = c->v;
    }
    /* every component must divide the largest sampling factor: the upsampler replicates by the integer ratio
     * hmax / h, and with a truncated ratio (h = 3 under hmax = 4) a plane row is shorter than the image row the colour
     * conversion reads from it (heap over-read). No encoder writes such frames. */
    for (int i = 0; i < d->ncomp; ++i)
        if (d->hmax % d->comp[i].h != 0 || d->vmax % d->comp[i].v != 0) return 0;
    d->mcus_x = (d->width + 8 * d->hmax - 1) / (8 * d->hmax);
    d->mcus_y = (d->height + 8 * d->vmax - 1) / (8 * d->vmax);
    for (int i = 0; i < d->ncomp; ++i) {
        jcomp *c = &d->comp[i];
        c->width = (d->width * c->h + d->hmax - 1) / d->hmax;
        c->height = (d->height * c->v + d->vmax - 1) / d->vmax;
        c->pitch = d->mcus_x * c->h * 8;
        c->rows = d->mcus_y * c->v * 8;
        c->blocks_w = c->pitch >> 3; c->blocks_h = c->rows >> 3;
    }
    return 1;
}

static int read_scan_header(jdec *d) {
    const int len = get16(d);
    d->scan_n = get8(d);
    if (d->scan_n < 1 || d->scan_n > d->ncomp || len != 6 + 2 * d->scan_n) return 0;
    for (int i = 0; i < d->scan_n; ++i) {
        const int id = get8(d), tables = get8(d);
        int which = 0;
        while (which < d->ncomp && d->comp[which].id != id) ++which;
        if (which == d->ncomp || (tables >> 4) > 3 || (tables & 15) > 3) return 0;
        d->comp[which].dc_table = tables >> 4;
        d->comp[which].ac_table = tables & 15;
        d->scan_comp[i] = which;
    }
    d->ss = get8(d); d->se = get8(d);
    const int a = get8(d);
    d->ah = a >> 4; d->al = a & 15;
    if (d->progressive) {
        if (d->ss > 63 || d->se > 63 || d->ss > d->se || d->ah > 13 || d->al > 13) return 0;
    } else {
        if (d->ss != 0 || d->ah != 0 || d->al != 0) return 0;
        d->se = 63;
    }
    return 1;
}

static void info_from_frame(const jdec *d, bip_jpeg_info *info) {
    memset(info, 0, sizeof(*info));
    info->width = d->width; info->height = d->height; info->ncomp = d->ncomp;
    info->hmax = d->hmax; info->vmax = d->vmax; info->progressive = d->progressive;
    for (int i = 0; i < d->ncomp; ++i) {
        const jcomp *c = &d->comp[i];
        bip_jpeg_component *o = &info->comp[i];
        o->h = c->h; o->v = c->v; o->width = c->width; o->height = c->height;
        o->pitch = c->pitch; o->rows = c->rows; o->blocks_w = c->blocks_w; o->blocks_h = c->blocks_h;
        /* the one-pass baseline decoder transformed every block it decoded: all of every whole MCU; the progressive one
         * transforms, after the last scan, only the blocks that carry image content */
        o->idct_w = d->progressive ? (c->width + 7) >> 3 : c->blocks_w;
        o->idct_h = d->progressive ? (c->height + 7) >> 3 : c->blocks_h;
        info->num_coefficients += (size_t)c->blocks_w * c->blocks_h * 64;
    }
}

/* SOI, tables and application segments and the frame header; then, unless coeff is NULL (the caller only wants the
 * frame), every scan up to EOI into coeff: baseline blocks arrive dequantised, progressive ones are dequantised at the
 * end. `expect` is the frame the caller sized coeff for: a stream with another frame is refused before anything is
 * written. */
static int decode_stream(jdec *d, const bip_jpeg_info *expect, int16_t *coeff) {
    if (next_marker(d) != 0xd8) return 0; /* SOI */
    int m = next_marker(d);
    while (m != 0xc0 && m != 0xc1 && m != 0xc2) { /* tables and application segments up to the frame header */
        if (!read_tables(d, m)) return 0;
        m = next_marker(d);
        while (m == 0xff) {
            if (d->p >= d->end) return 0;
            m = next_marker(d);
        }
    }
    d->progressive = m == 0xc2;
    if (!read_frame(d)) return 0;
    if (!coeff) return 1;
    bip_jpeg_info own;
    info_from_frame(d, &own);
    if (memcmp(&own, expect, sizeof(own)) != 0) return 0; /* not this buffer's: sizes would not hold */
    /* Before the scans: a progressive stream accumulates into zeroed blocks; a baseline block that no scan reaches (a
     * scan may end early at a missing restart marker and still be accepted) holds the block that transforms to bytes 0,
     * which is what the one-pass decoder's zeroed plane kept there. */
    memset(coeff, 0, own.num_coefficients * sizeof(int16_t));
    if (!own.progressive)
        for (size_t k = 0; k < own.num_coefficients; k += 64) coeff[k] = BIP_JPEG_DC_OF_ZERO_BLOCK;
    for (int i = 0; i < d->ncomp; ++i) {
        d->comp[i].coeff = coeff;
        coeff += (size_t)d->comp[i].blocks_w * d->comp[i].blocks_h * 64;
    }
    for (m = next_marker(d); m != 0xd9; m = next_marker(d)) { /* until EOI */
        if (m == 0xda) {
            if (!read_scan_header(d) || !decode_scan(d)) return 0;
            if (!d->marker) { /* zero padding behind the entropy-coded data */
                while (d->p < d->end) {
                    const int x = get8(d);
                    if (x == 0xff) { d->marker = get8(d); break; }
                    if (x != 0) return 0;
                }
            }
        } else if (!read_tables(d, m)) {
            return 0;
        }
    }
    if (d->progressive) /* all scans seen: dequantise (16-bit arithmetic) the blocks that get transformed */
        for (int i = 0; i < d->ncomp; ++i) {
            jcomp *c = &d->comp[i];
            const int bw = (c->width + 7) >> 3, bh = (c->height + 7) >> 3;
            for (int by = 0; by < bh; ++by)
                for (int bx = 0; bx < bw; ++bx) {
                    int16_t *blk = c->coeff + 64 * ((size_t)by * c->blocks_w + bx);
                    for (int k = 0; k < 64; ++k) blk[k] = (int16_t)(blk[k] * d->qt[c->tq][k]);
                }
        }
    return 1;
}

bip_status bip_jpeg_frame_info(const uint8_t *buf, size_t len, bip_jpeg_info *info) {
    if (!buf || !info) return BIP_INVALID_PTR;
    jdec *d = (jdec *)calloc(1, sizeof(jdec));
    if (!d) return BIP_UNKNOWN_ERROR;
    d->p = buf; d->end = buf + len;
    const int ok = decode_stream(d, NULL, NULL);
    if (ok) info_from_frame(d, info);
    free(d);
    return ok ? BIP_SUCCESS : BIP_INVALID_PARAMETER;
}

bip_status bip_jpeg_read_coefficients(const uint8_t *buf, size_t len, const bip_jpeg_info *info, int16_t *coeff) {
    if (!buf || !info || !coeff) return BIP_INVALID_PTR;
    jdec *d = (jdec *)calloc(1, sizeof(jdec));
    if (!d) return BIP_UNKNOWN_ERROR;
    d->p = buf; d->end = buf + len;
    const int ok = decode_stream(d, info, coeff);
    free(d);
    return ok ? BIP_SUCCESS : BIP_INVALID_PARAMETER;
}

/* ---- chroma upsampling (one output row from the nearer and the farther source row) ---------------------------------- */
static const uint8_t *up_rows(uint8_t *out, const uint8_t *near_row, const uint8_t *far_row, int w, int hs, int vs) {
    if (hs == 1 && vs == 1) return near_row;
    const int n = w * hs;
    if (hs == 2 && (vs == 1 || vs == 2) && w > 2) {
        /* the columns at the two ends have forms of their own (bip_jpeg_up_sample); between them every pair of output
         * samples blends a column's sum with its left and its right neighbour's */
        out[0] = bip_jpeg_up_sample(near_row, far_row, w, 2, vs, 0);
        out[1] = bip_jpeg_up_sample(near_row, far_row, w, 2, vs, 1);
        out[n - 2] = bip_jpeg_up_sample(near_row, far_row, w, 2, vs, n - 2);
        out[n - 1] = bip_jpeg_up_sample(near_row, far_row, w, 2, vs, n - 1);
        if (vs == 1) {
            for (int i = 1; i < w - 1; ++i) {
                out[2 * i] = BIP_JPEG_UP_DIV4(BIP_JPEG_UP_3TO1(near_row[i], near_row[i - 1]));
                out[2 * i + 1] = BIP_JPEG_UP_DIV4(BIP_JPEG_UP_3TO1(near_row[i], near_row[i + 1]));
            }
        } else {
            int prev = BIP_JPEG_UP_3TO1(near_row[0], far_row[0]), cur = BIP_JPEG_UP_3TO1(near_row[1], far_row[1]);
            for (int i = 1; i < w - 1; ++i) {
                const int next = BIP_JPEG_UP_3TO1(near_row[i + 1], far_row[i + 1]);
                out[2 * i] = BIP_JPEG_UP_DIV16(cur, prev);
                out[2 * i + 1] = BIP_JPEG_UP_DIV16(cur, next);
                prev = cur;
                cur = next;
            }
        }
        return out;
    }
    for (int x = 0; x < n; ++x) out[x] = bip_jpeg_up_sample(near_row, far_row, w, hs, vs, x);
    return out;
}

bip_status bip_jpeg_pixels_from_coefficients(const bip_jpeg_info *info, const int16_t *coeff, uint8_t *image) {
    if (!info || !coeff || !image) return BIP_INVALID_PTR;
    const int n = info->ncomp, width = info->width, height = info->height;
    if ((n != 1 && n != 3) || width < 1 || height < 1) return BIP_INVALID_PARAMETER;
    uint8_t *plane[3] = {NULL, NULL, NULL}, *line[3] = {NULL, NULL, NULL};
    bip_status st = BIP_UNKNOWN_ERROR;
    int hs[3], vs[3], w_lores[3];
    for (int k = 0; k < n; ++k) {
        const bip_jpeg_component *c = &info->comp[k];
        if (c->h < 1 || c->v < 1 || c->idct_w > c->blocks_w || c->idct_h > c->blocks_h || c->pitch != 8 * c->blocks_w ||
            c->rows != 8 * c->blocks_h)
            { st = BIP_INVALID_PARAMETER; goto done; }
        plane[k] = (uint8_t *)calloc((size_t)c->pitch * c->rows + 16, 1);
        line[k] = (uint8_t *)malloc((size_t)width + 8);
        if (!plane[k] || !line[k]) goto done;
        for (int by = 0; by < c->idct_h; ++by)
            for (int bx = 0; bx < c->idct_w; ++bx)
                idct_block(plane[k] + (size_t)by * 8 * c->pitch + bx * 8, c->pitch, coeff + 64 * ((size_t)by * c->blocks_w + bx));
        coeff += (size_t)c->blocks_w * c->blocks_h * 64;
        hs[k] = info->hmax / c->h;
        vs[k] = info->vmax / c->v;
        w_lores[k] = (width + hs[k] - 1) / hs[k];
    }
    for (int y = 0; y < height; ++y) {
        const uint8_t *src[3] = {NULL, NULL, NULL};
        for (int k = 0; k < n; ++k) {
            int near_row, far_row;
            bip_jpeg_up_source_rows(y, vs[k], info->comp[k].height, &near_row, &far_row);
            src[k] = up_rows(line[k], plane[k] + (size_t)near_row * info->comp[k].pitch,
                             plane[k] + (size_t)far_row * info->comp[k].pitch, w_lores[k], hs[k], vs[k]);
        }
        uint8_t *out = image + (size_t)n * width * y;
        if (n == 3) for (int x = 0; x < width; ++x) bip_jpeg_ycc_to_rgb(src[0][x], src[1][x], src[2][x], out + 3 * x);
        else memcpy(out, src[0], (size_t)width);
    }
    st = BIP_SUCCESS;
done:
    for (int k = 0; k < 3; ++k) { free(plane[k]); free(line[k]); }
    return st;
}

/* NULL unless the buffer holds a JPEG stream this decoder covers; the caller frees the image */
uint8_t *bip_decode_jpeg(const uint8_t *buf, size_t len, int32_t *w, int32_t *h, int32_t *depth) {
    bip_jpeg_info info;
    if (bip_jpeg_frame_info(buf, len, &info) != BIP_SUCCESS) return NULL;
    int16_t *coeff = (int16_t *)malloc(info.num_coefficients * sizeof(int16_t));
    uint8_t *image = (uint8_t *)malloc((size_t)info.ncomp * info.width * info.height + 1);
    if (!coeff || !image || bip_jpeg_read_coefficients(buf, len, &info, coeff) != BIP_SUCCESS ||
        bip_jpeg_pixels_from_coefficients(&info, coeff, image) != BIP_SUCCESS) {
        free(image);
        image = NULL;
    } else {
        *w = info.width; *h = info.height; *depth = info.ncomp;
    }
    free(coeff);
    return image;
}
