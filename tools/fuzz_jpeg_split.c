/* fuzz_jpeg_split.c -- stand-alone driver of libbip's split JPEG decoder for a sanitizer build (tests/test_jpeg_split_fuzz.py
 * compiles it with bcnn_amd/host/bip_jpeg.c under -fsanitize=address,undefined and runs it as a process of its own).
 * Every file named on the command line goes through bip_jpeg_frame_info, bip_jpeg_read_coefficients and
 * bip_jpeg_pixels_from_coefficients as it is, truncated at every 37th byte, and with single bytes overwritten at
 * positions and with values drawn from a fixed seed. The coefficient and pixel buffers are heap blocks of exactly the size
 * the interface asks for, so a write outside them stops the run. The split must also agree with the one-call decoder:
 * both decode a stream, to the same bytes, or both refuse it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bip/bip.h"

uint8_t *bip_decode_jpeg(const uint8_t *buf, size_t len, int32_t *w, int32_t *h, int32_t *depth); /* bip_jpeg.c */

#define MAX_COEFFICIENTS ((size_t)1 << 24) /* a corrupted extent may ask for gigabytes: those streams are counted, not run */

static long n_streams, n_decoded, n_too_large;

static uint32_t rng_state = 0x2545f491u;
static uint32_t rng(void) { /* xorshift32 */
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static int one_stream(const uint8_t *data, size_t len) {
    /* a heap copy of exactly len bytes: a read past the stream's end is caught as well */
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (!buf) return 1;
    memcpy(buf, data, len);
    ++n_streams;
    bip_jpeg_info info;
    int bad = 0;
    const int have_frame = bip_jpeg_frame_info(buf, len, &info) == BIP_SUCCESS;
    if (have_frame && info.num_coefficients > MAX_COEFFICIENTS) {
        ++n_too_large;
        free(buf);
        return 0;
    }
    uint8_t *image = NULL;
    if (have_frame) {
        int16_t *coeff = (int16_t *)malloc(info.num_coefficients * sizeof(int16_t));
        if (!coeff) { free(buf); return 1; }
        if (bip_jpeg_read_coefficients(buf, len, &info, coeff) == BIP_SUCCESS) {
            image = (uint8_t *)malloc((size_t)info.width * info.height * info.ncomp);
            if (!image || bip_jpeg_pixels_from_coefficients(&info, coeff, image) != BIP_SUCCESS) {
                fprintf(stderr, "pixel stage failed behind decoded coefficients\n");
                bad = 1;
            }
        }
        free(coeff);
    }
    int32_t w = 0, h = 0, c = 0;
    uint8_t *whole = bip_decode_jpeg(buf, len, &w, &h, &c);
    if (!bad && ((whole != NULL) != (image != NULL) ||
                 (whole && (w != info.width || h != info.height || c != info.ncomp ||
                            memcmp(whole, image, (size_t)w * h * c) != 0)))) {
        fprintf(stderr, "the split and the one-call decoder disagree (%d vs %d)\n", image != NULL, whole != NULL);
        bad = 1;
    }
    if (whole) ++n_decoded;
    free(whole);
    free(image);
    free(buf);
    return bad;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc && !bad; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        uint8_t *data = (uint8_t *)malloc(1 << 20);
        const size_t len = fread(data, 1, 1 << 20, f);
        fclose(f);
        const long before = n_decoded;
        bad |= one_stream(data, len);
        if (n_decoded != before + 1) { fprintf(stderr, "%s does not decode as it is\n", argv[a]); bad = 1; }
        for (size_t cut = 0; cut < len && !bad; cut += 37) bad |= one_stream(data, cut);
        for (int k = 0; k < 400 && !bad; ++k) {
            const size_t at = rng() % len;
            const uint8_t keep = data[at];
            data[at] = (uint8_t)rng();
            bad |= one_stream(data, len);
            data[at] = keep;
        }
        free(data);
    }
    printf("%ld streams, %ld decoded, %ld not run (too large)\n", n_streams, n_decoded, n_too_large);
    return bad;
}
