/* softmax_loss_rule.h -- the rules of the softmax cross-entropy loss node that host and device must agree on: how one
 * value of a class-index label map is classified, and the denominator D of a normaliser. Plain C99 / C++, no includes of
 * the project: bcnn_layers_softmax_loss.c (the builder's checks), every kernel of softmax_loss.hip and a stand-alone
 * host program under a sanitizer all compile this one definition. */
#ifndef BCNN_SOFTMAX_LOSS_RULE_H
#define BCNN_SOFTMAX_LOSS_RULE_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BCNN_SL_FN static __host__ __device__ __forceinline__
#else
#define BCNN_SL_FN static inline
#endif

/* the classes of one label value, in the order of the counts of the device record */
#define BCNN_SL_VALID 0
#define BCNN_SL_IGNORED 1
#define BCNN_SL_OUT_OF_RANGE 2

/* the values of bcnn_loss_norm (include/bcnn/bcnn.h) */
#define BCNN_SL_NORM_NONE 0
#define BCNN_SL_NORM_VALID 1
#define BCNN_SL_NORM_VALID_PER_IMAGE 2

/* An ignore label must be a float that holds an integer exactly: below 2^24. Negative: nothing is ignored on purpose. */
#define BCNN_SL_MAX_IGNORE_LABEL (1 << 24)

/* Classifies label value t of a map over `classes` classes. *cls is the class index for BCNN_SL_VALID and -1 otherwise:
 * only a value that passed 0 <= t < classes and t == (float)(int)t is ever converted, so nothing else can index memory
 * (NaN fails every comparison, +-inf and values past INT_MAX fail the range test before the conversion).
 * The ignore label wins over the range: ignore_label = 3 on a 5-class map ignores class 3. */
BCNN_SL_FN int bcnn_softmax_loss_classify(float t, int ignore_label, int classes, int *cls) {
    *cls = -1;
    if (ignore_label >= 0 && t == (float)ignore_label) return BCNN_SL_IGNORED;
    if (!(t >= 0.0f && t < (float)classes)) return BCNN_SL_OUT_OF_RANGE;
    const int k = (int)t;
    if ((float)k != t) return BCNN_SL_OUT_OF_RANGE;
    *cls = k;
    return BCNN_SL_VALID;
}

/* D of loss = (sum l) / D and dx = scale / D * (p - y); valid = V, the valid pixels of the batch of n images.
 * 0 for an unknown normaliser (the builder refuses it first). */
BCNN_SL_FN double bcnn_softmax_loss_denominator(int norm, long long valid, int n) {
    const double v = valid > 0 ? (double)valid : 1.0;
    if (norm == BCNN_SL_NORM_NONE) return 1.0;
    if (norm == BCNN_SL_NORM_VALID) return v;
    if (norm == BCNN_SL_NORM_VALID_PER_IMAGE) return v / (double)(n > 0 ? n : 1);
    return 0.0;
}

#endif /* BCNN_SOFTMAX_LOSS_RULE_H */
