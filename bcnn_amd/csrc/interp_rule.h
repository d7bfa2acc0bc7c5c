/* interp_rule.h -- the ONE definition of the bilinear interpolation node's rules: the output extent of an axis and the
 * two taps of an output index. Shared by the host runtime (../host/bcnn_layers_interp.c: builder and bcnn_resize_net), by
 * the host-side tap table (bcnn_hip_interp_axis_taps) and by every kernel of interp.hip, forward and backward. Plain C
 * that also compiles as HIP; every function is static inline, so nothing is exported.
 *
 * The tap rule is torch.nn.functional.interpolate(mode="bilinear") with the extents given as size=, for both values of
 * align_corners. Everything in it is float32 and every operation is rounded on its own: a translation unit that CALLS
 * bcnn_interp_step or bcnn_interp_tap must be compiled with contraction off (-ffp-contract=off), as csrc/ is. The extent
 * rule is integer arithmetic and carries no such condition; the host runtime includes this header for it alone. */
#ifndef BCNN_INTERP_RULE_H
#define BCNN_INTERP_RULE_H

#ifdef __HIPCC__
#define BCNN_INTERP_INLINE __host__ __device__ static inline
#else
#define BCNN_INTERP_INLINE static inline
#endif

/* Output extent of an axis of `in` elements. Exactly one form: scale >= 1 (in * scale), zoom >= 1 ((in - 1) * zoom + 1,
 * Caffe-DeepLab's Interp) or fixed > 0 (the extent itself). 0: no form or more than one, a negative value, an empty or
 * overflowing extent. */
BCNN_INTERP_INLINE int bcnn_interp_out_extent(int in, int scale, int zoom, int fixed) {
    if (in < 1 || scale < 0 || zoom < 0 || fixed < 0 || (scale > 0) + (zoom > 0) + (fixed > 0) != 1) return 0;
    const long long out = scale > 0 ? (long long)in * scale : zoom > 0 ? ((long long)in - 1) * zoom + 1 : (long long)fixed;
    return out > 0 && out < 0x7fffffffLL ? (int)out : 0;
}

/* The step of an axis: source positions per output index. */
BCNN_INTERP_INLINE float bcnn_interp_step(int in, int out, int align_corners) {
    if (align_corners) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    return (float)in / (float)out;
}

/* The taps of output index o: elements i0 and i1 (i1 == i0 at the far edge) with weights 1 - l1 and l1. */
BCNN_INTERP_INLINE void bcnn_interp_tap(int in, float step, int align_corners, int o, int *i0, int *i1, float *l1) {
    float src;
    if (align_corners) {
        src = step * (float)o;
    } else {
        src = step * ((float)o + 0.5f) - 0.5f;
        src = src < 0.0f ? 0.0f : src;
    }
    int a = (int)src;
    if (a > in - 1) a = in - 1;
    float l = src - (float)a;
    l = l < 0.0f ? 0.0f : (l > 1.0f ? 1.0f : l);
    *i0 = a;
    *i1 = a + (a < in - 1);
    *l1 = l;
}

#endif
