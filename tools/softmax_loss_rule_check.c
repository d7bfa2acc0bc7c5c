/* softmax_loss_rule_check.c -- the host side of the softmax-loss node's label rule (bcnn_amd/csrc/softmax_loss_rule.h, the
 * header the kernels and the builder compile) over its boundary labels, for a run under the host sanitizers:
 *     cc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/softmax_loss_rule_check.c -lm \
 *        -o softmax_loss_rule_check && ./softmax_loss_rule_check
 * Every label is classified and, as the kernels do, a valid one indexes a heap row of exactly `classes` floats: a
 * conversion of a value no int holds, or an index outside the row, stops the run. Prints "ok" and returns 0. */
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../bcnn_amd/csrc/softmax_loss_rule.h"

static int failures = 0;

static void expect(float t, int ignore_label, int classes, int want_kind, int want_cls) {
    int cls = 12345;
    const int kind = bcnn_softmax_loss_classify(t, ignore_label, classes, &cls);
    float *row = (float *)calloc((size_t)classes, sizeof(float));
    if (kind == BCNN_SL_VALID) row[cls] += 1.0f; /* what a kernel does with a valid label */
    if (kind != want_kind || cls != want_cls || (kind != BCNN_SL_VALID && cls != -1)) {
        fprintf(stderr, "label %g, ignore %d, %d classes: kind %d class %d, expected %d %d\n", (double)t, ignore_label,
                classes, kind, cls, want_kind, want_cls);
        ++failures;
    }
    free(row);
}

int main(void) {
    const int V = BCNN_SL_VALID, I = BCNN_SL_IGNORED, O = BCNN_SL_OUT_OF_RANGE;
    const int class_counts[] = {1, 2, 5, 21, 150, 255, 256, 300, 1000, 1 << 20};
    for (size_t k = 0; k < sizeof(class_counts) / sizeof(class_counts[0]); ++k) {
        const int C = class_counts[k];
        const int ignores[] = {-1, -7, INT_MIN, 0, C - 1, C, 255, (1 << 24) - 1};
        for (size_t j = 0; j < sizeof(ignores) / sizeof(ignores[0]); ++j) {
            const int ig = ignores[j];
            const float labels[] = {0.0f, -0.0f, 1.0f, (float)(C - 1), (float)C, (float)(C + 1), -1.0f, -0.5f, 0.5f, 1.5f,
                                    (float)C - 0.5f, 254.0f, 255.0f, 256.0f, (float)ig - 1.0f, (float)ig, (float)ig + 1.0f,
                                    nextafterf(0.0f, -1.0f), nextafterf((float)C, 0.0f), 16777216.0f, 2147483648.0f, 3e9f,
                                    -3e9f, 1e38f, -1e38f, INFINITY, -INFINITY, NAN, -NAN};
            for (size_t i = 0; i < sizeof(labels) / sizeof(labels[0]); ++i) {
                const float t = labels[i];
                /* the rule, restated with integers where they are exact */
                int want_kind, want_cls = -1;
                if (ig >= 0 && t == (float)ig) want_kind = I;
                else if (t >= 0.0f && t < (float)C && floorf(t) == t) { want_kind = V; want_cls = (int)t; }
                else want_kind = O;
                expect(t, ig, C, want_kind, want_cls);
            }
        }
    }
    /* the cases the node's documentation names */
    expect(255.0f, 255, 21, I, -1);
    expect(255.0f, -1, 21, O, -1);
    expect(-1.0f, -1, 21, O, -1);   /* ignore_label < 0 ignores nothing: -1 in a map is out of range */
    expect(254.0f, 255, 21, O, -1);
    expect(254.0f, 255, 300, V, 254);
    expect(3.0f, 3, 5, I, -1);      /* the ignore label wins over the range */
    expect(20.0f, 255, 21, V, 20);
    expect(21.0f, 255, 21, O, -1);
    /* the denominators */
    if (bcnn_softmax_loss_denominator(BCNN_SL_NORM_NONE, 0, 8) != 1.0 || bcnn_softmax_loss_denominator(BCNN_SL_NORM_NONE, 99, 8) != 1.0 ||
        bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID, 0, 8) != 1.0 || bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID, 99, 8) != 99.0 ||
        bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID_PER_IMAGE, 0, 8) != 0.125 ||
        bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID_PER_IMAGE, 96, 8) != 12.0 ||
        bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID_PER_IMAGE, 5, 0) != 5.0 ||
        bcnn_softmax_loss_denominator(3, 5, 1) != 0.0 || bcnn_softmax_loss_denominator(-1, 5, 1) != 0.0 ||
        bcnn_softmax_loss_denominator(BCNN_SL_NORM_VALID, 2147483647LL * 4, 1) != 2147483647.0 * 4) {
        fprintf(stderr, "a denominator is off\n");
        ++failures;
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
