/* label_warp_check.c -- the host side of the label warp rule (bcnn_amd/host/bip_label_warp.h, the header libbip, the
 * segmentation-list loader and the device kernel compile) over its edge cases, for a run under the host sanitizers:
 *     cc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/label_warp_check.c -lm \
 *        -o label_warp_check && ./label_warp_check
 * Every case walks the rule over a heap map of exactly w * h bytes into a heap map of exactly w * h bytes, with tap tables
 * of exactly w and h pairs made by the loader's own tap rule (bip_resize_tap.h): a read or a write outside either stops
 * the run. Every label must be a byte of the map or the fill byte. Prints "ok" and returns 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bcnn_amd/host/bip_label_warp.h"
#include "../bcnn_amd/host/bip_resize_tap.h"

static int failures = 0, cases = 0;

/* the taps of a sample scaled by `factor` and pasted back at (x_ul, y_ul), as the loader tabulates them; 0: the scale
 * leaves nothing (the loader leaves the stage out) */
static int make_taps(int32_t *tapx, int32_t *tapy, int w, int h, float factor, int x_ul, int y_ul) {
    const int ws = (int)(w * factor), hs = (int)(h * factor);
    if (ws < 1 || hs < 1) return 0;
    const float xs = bip_resize_scale((size_t)w, (size_t)ws), ys = bip_resize_scale((size_t)h, (size_t)hs);
    for (int x = 0; x < w; ++x) {
        const long long X = (long long)x + x_ul;
        tapx[2 * x] = -1;
        tapx[2 * x + 1] = 0;
        if (X >= 0 && X < ws) bip_resize_tap((size_t)X, xs, (size_t)w, &tapx[2 * x], &tapx[2 * x + 1]);
    }
    for (int y = 0; y < h; ++y) {
        const long long Y = (long long)y + y_ul;
        tapy[2 * y] = -1;
        tapy[2 * y + 1] = 0;
        if (Y >= 0 && Y < hs) bip_resize_tap((size_t)Y, ys, (size_t)h, &tapy[2 * y], &tapy[2 * y + 1]);
    }
    return 1;
}

/* one case; want_all_fill: every label must be the fill byte; want_identity: the map must come back as it is */
static void run(int w, int h, int flags, int x_ul, int y_ul, float factor, double theta, int fill, int want_all_fill,
                int want_identity) {
    uint8_t *map = (uint8_t *)malloc((size_t)w * h), *out = (uint8_t *)malloc((size_t)w * h);
    int32_t *tapx = (int32_t *)malloc((size_t)w * 2 * sizeof(int32_t)), *tapy = (int32_t *)malloc((size_t)h * 2 * sizeof(int32_t));
    if (!map || !out || !tapx || !tapy) exit(2);
    for (int i = 0; i < w * h; ++i) map[i] = (uint8_t)(1 + (i * 7 + i / w) % 20); /* classes 1 ... 20: never a fill byte below */
    if ((flags & BIP_LABEL_SCALE) && !make_taps(tapx, tapy, w, h, factor, (flags & BIP_LABEL_SHIFT) ? x_ul : 0,
                                                (flags & BIP_LABEL_SHIFT) ? y_ul : 0))
        flags &= ~BIP_LABEL_SCALE;
    if (!bip_label_taps_ok(flags, tapx, tapy, w, h)) {
        fprintf(stderr, "%d x %d flags %d: the loader's own taps are out of range\n", w, h, flags);
        ++failures;
    } else {
        const bip_label_sample s = {map, tapx, tapy, w, h, flags, x_ul, y_ul, (int32_t)(cos(theta) * 65536),
                                    (int32_t)(sin(theta) * 65536), fill};
        memset(out, 77, (size_t)w * h);
        bip_label_warp_map(&s, out);
        for (int i = 0; i < w * h; ++i) {
            const int v = out[i];
            if ((v != fill && (v < 1 || v > 20)) || (want_all_fill && v != fill) || (want_identity && v != map[i])) {
                fprintf(stderr, "%d x %d flags %d shift (%d, %d) scale %g theta %g fill %d: label %d at %d\n", w, h, flags, x_ul,
                        y_ul, (double)factor, theta, fill, v, i);
                ++failures;
                break;
            }
        }
    }
    ++cases;
    free(map); free(out); free(tapx); free(tapy);
}

int main(void) {
    const int F = BIP_LABEL_FLIP, S = BIP_LABEL_SHIFT, C = BIP_LABEL_SCALE, R = BIP_LABEL_ROTATE;
    const int sizes[][2] = {{5, 3}, {16, 12}, {33, 17}, {1, 7}, {7, 1}, {1, 1}, {2, 2}};
    const int fills[] = {0, 21, 255};
    const double pi = 3.14159265358979323846;
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        const int w = sizes[k][0], h = sizes[k][1];
        for (size_t j = 0; j < sizeof(fills) / sizeof(fills[0]); ++j) {
            const int fill = fills[j];
            run(w, h, 0, 0, 0, 1.0f, 0.0, fill, 0, 1);
            run(w, h, F, 0, 0, 1.0f, 0.0, fill, 0, 0);
            run(w, h, S, 0, 0, 1.0f, 0.0, fill, 0, 1);
            /* shifts: inside, at the edge, beyond the sample (all fill), and where x + x_ul would wrap an int */
            const int shifts[][2] = {{1, -1}, {-3, 2}, {w - 1, 0}, {0, h - 1}, {-(w - 1), -(h - 1)}, {w, 0}, {0, -h}, {70, 70},
                                     {2147483647, 2147483647}, {-2147483647 - 1, -2147483647 - 1}};
            for (size_t i = 0; i < sizeof(shifts) / sizeof(shifts[0]); ++i) {
                const long long ax = llabs((long long)shifts[i][0]), ay = llabs((long long)shifts[i][1]);
                const int beyond = ax >= w || ay >= h;
                run(w, h, S, shifts[i][0], shifts[i][1], 1.0f, 0.0, fill, beyond, 0);
                run(w, h, F | S, shifts[i][0], shifts[i][1], 1.0f, 0.0, fill, beyond, 0);
                if (ax < 1000) {
                    run(w, h, S | C, shifts[i][0], shifts[i][1], 0.5f, 0.0, fill, 0, 0);
                    run(w, h, S | C, shifts[i][0], shifts[i][1], 1.7f, 0.0, fill, 0, 0);
                    run(w, h, F | S | C | R, shifts[i][0], shifts[i][1], 1.7f, 0.3, fill, 0, 0);
                    run(w, h, F | S | C | R, shifts[i][0], shifts[i][1], 0.5f, -0.2, fill, 0, 0);
                }
            }
            const float factors[] = {0.01f, 0.5f, 0.9f, 1.0f, 1.1f, 1.7f, 3.0f, 40.0f};
            for (size_t i = 0; i < sizeof(factors) / sizeof(factors[0]); ++i) run(w, h, C, 0, 0, factors[i], 0.0, fill, 0, 0);
            const double thetas[] = {0.0, 0.05, -0.26, pi / 6, pi / 2, -pi / 2, pi, 3.0, 7.0, -100.0};
            for (size_t i = 0; i < sizeof(thetas) / sizeof(thetas[0]); ++i) {
                /* a one-sample axis has no pixel with 0 <= m < extent - 1: rotation covers nothing */
                run(w, h, R, 0, 0, 1.0f, thetas[i], fill, w == 1 || h == 1, 0);
                run(w, h, F | S | C | R, 2, -1, 1.3f, thetas[i], fill, w == 1 || h == 1, 0);
            }
        }
    }
    /* the ties, constructed: a tap fraction of exactly 8 sixteenths picks index + 1, 7 picks index; a rotation whose
     * fixed-point fraction is exactly 0x8000 picks m + 1, 0x7fff picks m */
    {
        uint8_t map[4 * 4], out[4 * 4];
        for (int i = 0; i < 16; ++i) map[i] = (uint8_t)(i + 1);
        int32_t tapx[8] = {0, 7, 0, 8, 2, 8, 2, 16}, tapy[8] = {0, 0, 1, 8, -1, 0, 2, 7};
        bip_label_sample s = {map, tapx, tapy, 4, 4, BIP_LABEL_SCALE, 0, 0, 0, 0, 255};
        bip_label_warp_map(&s, out);
        const uint8_t want[16] = {1, 2, 4, 4, /* row tap (1, 8) -> row 2 */ 9, 10, 12, 12,
                                  /* row not covered: falls through */ 9, 10, 11, 12, /* (2, 7) -> row 2 */ 9, 10, 12, 12};
        if (memcmp(out, want, 16)) { fprintf(stderr, "the frac == 8 tie is off\n"); ++failures; }
        /* centre (2, 2), ca = 0x10000, sa = -0x8000: px = (x << 16) + 0x8000 (y - 2), py = (y << 16) - 0x8000 (x - 2) */
        bip_label_sample r = {map, NULL, NULL, 4, 4, BIP_LABEL_ROTATE, 0, 0, 0x10000, -0x8000, 255};
        bip_label_warp_map(&r, out);
        /* (x = 2, y = 1): px = 0x18000 -> mx 1, tie -> 2; py = 0x10000 -> my 1, fraction 0 -> 1: L(2, 1) = 7 */
        /* (x = 1, y = 1): px = 0x8000 -> mx 0, tie -> 1; py = 0x18000 -> my 1, tie -> 2: L(1, 2) = 10 */
        /* (x = 3, y = 1): px = 0x28000 -> mx 2, tie -> 3; py = 0x8000 -> my 0, tie -> 1: L(3, 1) = 8 */
        if (out[1 * 4 + 2] != 7 || out[1 * 4 + 1] != 10 || out[1 * 4 + 3] != 8) {
            fprintf(stderr, "the 0x8000 tie is off: %d %d %d\n", out[6], out[5], out[7]);
            ++failures;
        }
        r.sa = -0x8001; /* one past the tie at (1, 1): px = 0x7fff -> 0; py = 0x18001 -> my 1, up -> 2: L(0, 2) = 9 */
        bip_label_warp_map(&r, out);
        if (out[1 * 4 + 1] != 9) { fprintf(stderr, "one below the 0x8000 tie is off: %d\n", out[5]); ++failures; }
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
