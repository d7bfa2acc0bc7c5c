/*
 * bcnn_unsupported.c -- entry points of the public API that lie outside the hot path (SURVEY.md
 * section 8: control plane, rarely used layers; the dataset readers are in bcnn_data.c, the detector nodes in
 * bcnn_layers_detect.c, the deconvolution node in bcnn_layers_deconv.c, LRN and dropout in bcnn_layers_lrn_dropout.c).
 * They exist so
 * that every consumer of the reference links; each returns BCNN_INVALID_PARAMETER (or does nothing)
 * and says so in the log. INTEGRATION.md lists them.
 */
#include <string.h>

#include "bcnn_internal.h"


/* uint8 HWC image -> float CHW, reference bcnn_data.c:70-100 */
void bcnn_convert_img_to_float(const uint8_t *src, int w, int h, int c, float norm_coeff, int swap_to_bgr,
                               float mean_r, float mean_g, float mean_b, float *dst) {
    const float m[3] = {mean_r, mean_g, mean_b};
    for (int k = 0; k < c; ++k) {
        const int ks = (swap_to_bgr && c == 3) ? 2 - k : k;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                dst[(size_t)k * w * h + (size_t)y * w + x] =
                    ((float)src[((size_t)y * w + x) * c + ks] - (c == 3 ? m[ks] : m[0])) * norm_coeff;
    }
}

bcnn_status bcnn_fill_tensor_with_image(bcnn_net *net, const uint8_t *src, int w, int h, int c, float norm_coeff,
                                        int swap_to_bgr, float mean_r, float mean_g, float mean_b, int tensor_index,
                                        int batch_index) {
    if (tensor_index < 0 || tensor_index >= net->num_tensors) return BCNN_INVALID_PARAMETER;
    bcnn_tensor *t = &net->tensors[tensor_index];
    if (t->w != w || t->h != h || t->c != c || batch_index < 0 || batch_index >= t->n) return BCNN_INVALID_PARAMETER;
    bcnn_convert_img_to_float(src, w, h, c, norm_coeff, swap_to_bgr, mean_r, mean_g, mean_b,
                              t->data + (size_t)batch_index * w * h * c);
    return bcnn_upload_tensor(net, tensor_index, 0);
}

void bcnn_draw_color_box(unsigned char *img, int w_img, int h_img, float cx, float cy, float w, float h,
                         unsigned char color[3]) {
    (void)img; (void)w_img; (void)h_img; (void)cx; (void)cy; (void)w; (void)h; (void)color;
}
