/* label_map_rule_check.c -- the label-map rule (bcnn_amd/csrc/label_map_rule.h, the header label_map.hip compiles) walked
 * on the host over its boundary cases, for a run under the host sanitizers on the development machine (never on a GPU
 * machine: there is nothing of the device in it):
 *     cc -std=gnu99 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
 *        tools/label_map_rule_check.c -lm -o label_map_rule_check && ./label_map_rule_check
 * For every case it fits the images (both fits), plans the result block and then does what the kernel does, item by item:
 * four pixels of one row, taps from interp_rule.h, sixteen source elements per class read from a heap tensor of exactly
 * n * c * h * w floats, the argmax step, one four-byte store into a heap block of exactly the planned size, and the truth
 * byte of each real pixel classified into a heap matrix of exactly c * c counts. An index outside any of the three blocks,
 * an overflow or a misaligned store stops the run. The labels are then compared with a per-pixel evaluation that shares
 * only the tap and value functions. Prints "ok" and returns 0. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bcnn_amd/csrc/label_map_rule.h"

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            fprintf(stderr, __VA_ARGS__);     \
            fputc('\n', stderr);              \
            ++failures;                       \
        }                                     \
    } while (0)

static unsigned rng_state = 12345u;
static unsigned rng(void) { return rng_state = rng_state * 1664525u + 1013904223u; }

/* one call: n images over an [n][c][h][w] tensor of small integers (ties everywhere) */
static void run_case(int c, int h, int w, const bcnn_label_map_geom *imgs, int n, int align_corners, int ignore_label) {
    const size_t plane = (size_t)h * w, elems = (size_t)n * c * plane;
    float *x = (float *)malloc(elems * sizeof(float));
    for (size_t i = 0; i < elems; ++i) x[i] = (float)((int)(rng() >> 8) % 3 - 1);
    unsigned *strides = (unsigned *)malloc((size_t)n * sizeof(unsigned));
    unsigned long long *offsets = (unsigned long long *)malloc((size_t)n * sizeof(unsigned long long)), total = 0;
    for (int b = 0; b < n; ++b) CHECK(bcnn_label_map_geom_ok(&imgs[b], h, w), "case image %d is not runnable", b);
    CHECK(bcnn_label_map_plan(imgs, n, 1, strides, offsets, &total) == 0, "the plan refused a small batch");
    uint8_t *labels = (uint8_t *)malloc((size_t)total), *truths = (uint8_t *)malloc((size_t)total);
    long long *counts = (long long *)calloc((size_t)c * c, sizeof(long long)), other[3] = {0, 0, 0}, pixels = 0;
    memset(labels, 0xEE, (size_t)total);
    for (size_t i = 0; i < (size_t)total; ++i) truths[i] = (uint8_t)(rng() >> 8);
    for (int b = 0; b < n; ++b) {
        const bcnn_label_map_geom g = imgs[b];
        CHECK(offsets[b] % 16 == 0 && strides[b] % 4 == 0 && strides[b] >= (unsigned)g.out_w, "layout of image %d", b);
        const float step_w = bcnn_interp_step(g.roi_w, g.out_w, align_corners);
        const float step_h = bcnn_interp_step(g.roi_h, g.out_h, align_corners);
        const unsigned ipr = strides[b] / 4, items = ipr * (unsigned)g.out_h;
        for (unsigned item = 0; item < items; ++item) {
            const unsigned oy = item / ipr, q = item % ipr;
            int y0, y1, x0[4], x1[4], arg[4];
            float h1, w1[4], best[4];
            bcnn_interp_tap(g.roi_h, step_h, align_corners, (int)oy, &y0, &y1, &h1);
            for (int e = 0; e < 4; ++e) {
                const int ox = (int)q * 4 + e < g.out_w ? (int)q * 4 + e : g.out_w - 1;
                bcnn_interp_tap(g.roi_w, step_w, align_corners, ox, &x0[e], &x1[e], &w1[e]);
            }
            for (int k = 0; k < c; ++k) {
                const float *r0 = x + ((size_t)b * c + k) * plane + (size_t)(g.roi_y + y0) * w + g.roi_x;
                const float *r1 = x + ((size_t)b * c + k) * plane + (size_t)(g.roi_y + y1) * w + g.roi_x;
                for (int e = 0; e < 4; ++e) {
                    const float v = bcnn_label_map_value(r0[x0[e]], r0[x1[e]], r1[x0[e]], r1[x1[e]], 1.0f - w1[e], w1[e],
                                                         1.0f - h1, h1);
                    if (k == 0) {
                        best[e] = v;
                        arg[e] = 0;
                    } else {
                        bcnn_label_map_argmax_step(v, k, &best[e], &arg[e]);
                    }
                }
            }
            const size_t at = (size_t)offsets[b] + (size_t)oy * strides[b] + (size_t)q * 4;
            const uint32_t word = (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[2] << 16 | (uint32_t)arg[3] << 24;
            *(uint32_t *)(void *)(labels + at) = word; /* one aligned word, as the kernel stores it */
            uint32_t tw;
            memcpy(&tw, truths + at, 4);
            for (int e = 0; e < 4; ++e) {
                if ((int)q * 4 + e >= g.out_w) continue;
                int cls;
                const int kind = bcnn_label_map_truth((unsigned char)(tw >> (8 * e) & 255u), ignore_label, c, &cls);
                if (kind == BCNN_SL_VALID) counts[(size_t)cls * c + arg[e]] += 1;
                else other[kind] += 1;
                ++pixels;
            }
        }
        /* the same labels pixel by pixel, and the bytes past out_w of the last item of a row are the last pixel's */
        for (int oy = 0; oy < g.out_h; ++oy) {
            for (int ox = 0; ox < g.out_w; ++ox) {
                int y0, y1, xa, xb, arg = 0;
                float h1, wl, best = 0.0f;
                bcnn_interp_tap(g.roi_h, step_h, align_corners, oy, &y0, &y1, &h1);
                bcnn_interp_tap(g.roi_w, step_w, align_corners, ox, &xa, &xb, &wl);
                CHECK(y0 >= 0 && y1 < g.roi_h && xa >= 0 && xb < g.roi_w && y0 <= y1 && xa <= xb, "taps leave the rectangle");
                for (int k = 0; k < c; ++k) {
                    const float *pl = x + ((size_t)b * c + k) * plane;
                    const float v = bcnn_label_map_value(
                        pl[(size_t)(g.roi_y + y0) * w + g.roi_x + xa], pl[(size_t)(g.roi_y + y0) * w + g.roi_x + xb],
                        pl[(size_t)(g.roi_y + y1) * w + g.roi_x + xa], pl[(size_t)(g.roi_y + y1) * w + g.roi_x + xb],
                        1.0f - wl, wl, 1.0f - h1, h1);
                    if (k == 0 || v > best) {
                        best = v;
                        arg = k;
                    }
                }
                CHECK(labels[offsets[b] + (size_t)oy * strides[b] + ox] == (uint8_t)arg, "image %d pixel (%d, %d)", b, ox, oy);
            }
        }
    }
    long long sum = other[BCNN_SL_IGNORED] + other[BCNN_SL_OUT_OF_RANGE];
    for (size_t k = 0; k < (size_t)c * c; ++k) sum += counts[k];
    CHECK(sum == pixels && other[BCNN_SL_VALID] == 0, "counts do not add up to the pixels");
    free(x); free(strides); free(offsets); free(labels); free(truths); free(counts);
}

static void expect_fit(int fit, int W, int H, int iw, int ih, int want_status, int rx, int ry, int rw, int rh) {
    bcnn_label_map_geom g = {-7, -7, -7, -7, -7, -7};
    const int st = bcnn_label_map_fit(fit, W, H, iw, ih, &g);
    if (st != want_status || (st == 0 && (g.out_w != iw || g.out_h != ih || g.roi_x != rx || g.roi_y != ry || g.roi_w != rw ||
                                          g.roi_h != rh || !bcnn_label_map_geom_ok(&g, H, W))) ||
        (st != 0 && g.out_w != -7)) {
        fprintf(stderr, "fit %d of %d x %d into %d x %d: status %d, (%d, %d, %d, %d)\n", fit, iw, ih, W, H, st, g.roi_x, g.roi_y,
                g.roi_w, g.roi_h);
        ++failures;
    }
}

int main(void) {
    const int S = BCNN_LABEL_MAP_FIT_STRETCH, L = BCNN_LABEL_MAP_FIT_LETTERBOX;
    /* ---- fit: wide, tall, square, one-pixel, extent-equal, refusals, extents near INT_MAX (no overflow) */
    expect_fit(S, 16, 12, 40, 10, 0, 0, 0, 16, 12);
    expect_fit(L, 16, 12, 40, 10, 0, 0, 4, 16, 4);
    expect_fit(L, 16, 12, 10, 40, 0, 6, 0, 3, 12);
    expect_fit(L, 16, 12, 16, 12, 0, 0, 0, 16, 12);
    expect_fit(L, 16, 12, 1, 1, 0, 2, 0, 12, 12);
    expect_fit(L, 1, 1, 1, 1, 0, 0, 0, 1, 1);
    expect_fit(L, 416, 416, 500, 375, 0, 0, 52, 416, 312);
    expect_fit(L, 416, 416, 375, 500, 0, 52, 0, 312, 416);
    expect_fit(L, 16, 12, 1000, 3, 1, 0, 0, 0, 0);
    expect_fit(L, INT_MAX, INT_MAX, INT_MAX, 1, 0, 0, INT_MAX / 2, INT_MAX, 1);
    expect_fit(L, INT_MAX, 2, INT_MAX, INT_MAX, 0, (INT_MAX - 2) / 2, 0, 2, 2);
    expect_fit(S, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 0, 0, 0, INT_MAX, INT_MAX);
    expect_fit(2, 16, 12, 4, 4, 1, 0, 0, 0, 0);
    expect_fit(-1, 16, 12, 4, 4, 1, 0, 0, 0, 0);
    expect_fit(S, 0, 12, 4, 4, 1, 0, 0, 0, 0);
    expect_fit(S, 16, 12, 4, 0, 1, 0, 0, 0, 0);
    expect_fit(L, 16, 12, -4, 4, 1, 0, 0, 0, 0);
    /* ---- rectangles the call refuses */
    {
        const bcnn_label_map_geom bad[] = {{0, 4, 0, 0, 9, 7}, {4, 0, 0, 0, 9, 7}, {4, 4, 0, 0, 0, 7}, {4, 4, 0, 0, 9, 0},
                                           {4, 4, -1, 0, 9, 7}, {4, 4, 1, 0, 9, 7}, {4, 4, 0, 1, 9, 7}, {4, 4, 0, 0, 10, 7},
                                           {4, 4, INT_MAX, 0, 2, 2}, {4, 4, 0, INT_MAX, 2, 2}, {4, 4, 9, 0, 1, 1},
                                           {4, 4, 0, 0, INT_MAX, INT_MAX}};
        for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); ++k)
            CHECK(!bcnn_label_map_geom_ok(&bad[k], 7, 9), "rectangle %d passed", (int)k);
    }
    /* ---- plan: the limit, with and without truths, and sums that would wrap 64 bits if they were not cut short */
    {
        unsigned stride = 77;
        unsigned long long off = 77, total = 77;
        const bcnn_label_map_geom big = {65536, 32768, 0, 0, 9, 7}, one = {1, 1, 0, 0, 9, 7}, huge = {INT_MAX - 3, INT_MAX, 0, 0, 9, 7};
        bcnn_label_map_geom two[2] = {big, one}, many[8] = {huge, huge, huge, huge, huge, huge, huge, huge};
        CHECK(bcnn_label_map_plan(&big, 1, 0, &stride, &off, &total) == 0 && stride == 65536 && off == 0 && total == 1ULL << 31,
              "the limit itself");
        stride = 77; off = 77; total = 77;
        CHECK(bcnn_label_map_plan(two, 2, 0, &stride, &off, &total) == 1 && stride == 77 && off == 77 && total == 77, "past the limit");
        CHECK(bcnn_label_map_plan(&big, 1, 1, &stride, &off, &total) == 1 && total == 77, "truths double the block");
        CHECK(bcnn_label_map_plan(many, 8, 0, NULL, NULL, &total) == 1 && total == 77, "a sum past 64 bits");
        CHECK(bcnn_label_map_plan(&one, 0, 0, NULL, NULL, NULL) == 1 && bcnn_label_map_plan(NULL, 1, 0, NULL, NULL, NULL) == 1, "empty");
        CHECK(bcnn_label_map_plan(&one, 1, 1, NULL, NULL, &total) == 0 && total == 16, "one pixel");
        CHECK(bcnn_label_map_row_stride(1) == 4 && bcnn_label_map_row_stride(4) == 4 && bcnn_label_map_row_stride(5) == 8 &&
              bcnn_label_map_row_stride(INT_MAX - 3) == (unsigned)INT_MAX - 3u, "row strides");
    }
    /* ---- the item walk over heap blocks of exactly the planned size */
    {
        const int sizes[][2] = {{9, 7}, {13, 11}, {4, 3}, {1, 1}, {33, 17}, {16, 8}, {36, 28}, {5, 1}, {1, 5}, {3, 3}};
        const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
        bcnn_label_map_geom imgs[16];
        const int classes[] = {1, 2, 5, 21, 64, 65, 256};
        for (size_t k = 0; k < sizeof(classes) / sizeof(classes[0]); ++k) {
            for (int ac = 0; ac < 2; ++ac) {
                for (int b = 0; b < n; ++b) bcnn_label_map_fit(S, 9, 7, sizes[b][0], sizes[b][1], &imgs[b]);
                run_case(classes[k], 7, 9, imgs, n, ac, ac ? 255 : -1);
            }
        }
        /* letterbox rectangles of a 16 x 12 plane, a one-element rectangle in the last corner, a one-column plane */
        int m = 0;
        bcnn_label_map_fit(L, 16, 12, 40, 10, &imgs[m++]);
        bcnn_label_map_fit(L, 16, 12, 10, 40, &imgs[m++]);
        bcnn_label_map_fit(L, 16, 12, 16, 12, &imgs[m++]);
        imgs[m++] = (bcnn_label_map_geom){7, 5, 15, 11, 1, 1};
        imgs[m++] = (bcnn_label_map_geom){1, 1, 3, 2, 13, 10};
        for (int ac = 0; ac < 2; ++ac) run_case(5, 12, 16, imgs, m, ac, 3);
        imgs[0] = (bcnn_label_map_geom){6, 9, 0, 0, 1, 4};
        imgs[1] = (bcnn_label_map_geom){2, 2, 0, 3, 1, 1};
        for (int ac = 0; ac < 2; ++ac) run_case(3, 4, 1, imgs, 2, ac, 0);
    }
    /* ---- the argmax step on what is not a number: a NaN never wins, a NaN at class 0 is never replaced */
    {
        const float nan = NAN, inf = INFINITY;
        float best = 1.0f;
        int arg = 0;
        bcnn_label_map_argmax_step(nan, 1, &best, &arg);
        bcnn_label_map_argmax_step(1.0f, 2, &best, &arg);
        CHECK(arg == 0 && best == 1.0f, "a NaN or a tie replaced the first maximum");
        bcnn_label_map_argmax_step(inf, 3, &best, &arg);
        bcnn_label_map_argmax_step(inf, 4, &best, &arg);
        CHECK(arg == 3, "the first infinity");
        best = nan; arg = 0;
        bcnn_label_map_argmax_step(5.0f, 1, &best, &arg);
        CHECK(arg == 0, "a NaN at class 0 was replaced");
        int cls;
        CHECK(bcnn_label_map_truth(255, 255, 256, &cls) == BCNN_SL_IGNORED && cls == -1, "ignore wins over the range");
        CHECK(bcnn_label_map_truth(255, -1, 256, &cls) == BCNN_SL_VALID && cls == 255, "class 255");
        CHECK(bcnn_label_map_truth(21, 255, 21, &cls) == BCNN_SL_OUT_OF_RANGE && cls == -1, "t == C");
        CHECK(bcnn_label_map_truth(0, -1, 1, &cls) == BCNN_SL_VALID && cls == 0, "class 0");
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
