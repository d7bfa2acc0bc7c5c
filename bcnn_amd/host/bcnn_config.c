/* bcnn_config.c -- bcnn_load_net: build a net from an INI-style config file.
 *
 * Mirrors the reference loader (src/bcnn_net.c:504-593 net parameters, :716-966 layer parameters, :968-1112
 * section -> builder mapping, :1114-1216 driver; INI reader src/bh/inc/bh/bh_ini.h):
 *   - all blanks and tabs inside a line are removed before parsing; lines starting with '#', ';', '!' or empty
 *     are skipped; "[name]" opens a section; every other line must split into exactly "key=value";
 *   - the first section must be [net] or [network] and non-empty; unknown keys there are ignored (they belong
 *     to the command-line tool: data sources, output_model, ...);
 *   - every further section is one layer; `src` may list several tensors separated by ',';
 *   - when the model file is a Darknet *.weights file, sections may omit src/dst (implicit "lid<i-1>" ->
 *     "lid<i>" chaining; an in-place [dropout] / [activation] section stands for its source), `pad=1` means size/2 and
 *     `layers=` / `from=` name earlier sections.
 * One deliberate difference: the reference discards the status of the layer builders; here a builder that
 * fails (an out-of-scope layer of this build, a bad tensor name) aborts the load with its status instead of
 * leaving a half-built graph. */
#include <float.h>
#include <stdio.h>
#include <string.h>

#include "bcnn_internal.h"

/* ---- tiny INI reader ------------------------------------------------------------------------------ */
typedef struct { char *name, *val; } ini_key;
typedef struct { char *name; ini_key *keys; int num_keys; } ini_section;
typedef struct { ini_section *sections; int num_sections; } ini_file;

static char *dup_str(const char *s) {
    size_t n = strlen(s) + 1;
    char *d = (char *)malloc(n);
    if (d) memcpy(d, s, n);
    return d;
}

static void ini_free(ini_file *f) {
    for (int i = 0; i < f->num_sections; ++i) {
        for (int j = 0; j < f->sections[i].num_keys; ++j) {
            free(f->sections[i].keys[j].name);
            free(f->sections[i].keys[j].val);
        }
        free(f->sections[i].keys);
        free(f->sections[i].name);
    }
    free(f->sections);
    f->sections = NULL;
    f->num_sections = 0;
}

static char *read_line(FILE *fp) { /* whole line, any length; NULL at end of file */
    size_t cap = 256, len = 0;
    char *buf = (char *)malloc(cap);
    int ch;
    if (!buf) return NULL;
    while ((ch = fgetc(fp)) != EOF) {
        if (len + 2 > cap) {
            cap *= 2;
            char *nb = (char *)realloc(buf, cap);
            if (!nb) { free(buf); return NULL; }
            buf = nb;
        }
        if (ch == '\n') { buf[len] = '\0'; return buf; }
        buf[len++] = (char)ch;
    }
    if (len == 0) { free(buf); return NULL; }
    buf[len] = '\0';
    return buf;
}

static int ini_read(const char *path, ini_file *out) {
    FILE *fp = fopen(path, "r");
    out->sections = NULL;
    out->num_sections = 0;
    if (!fp) {
        fprintf(stderr, "[ERROR] Could not open file: %s\n", path);
        return -1;
    }
    char *line;
    int rc = 0;
    while (rc == 0 && (line = read_line(fp)) != NULL) {
        size_t k = 0;
        for (size_t i = 0; line[i]; ++i) /* bh_strstrip: drop blanks everywhere, not only at the ends */
            if (line[i] != ' ' && line[i] != '\t' && line[i] != '\n' && line[i] != '\r') line[k++] = line[i];
        line[k] = '\0';
        if (line[0] == '[') {
            ini_section *ns = (ini_section *)realloc(out->sections, (size_t)(out->num_sections + 1) * sizeof(ini_section));
            if (!ns) rc = -1;
            else {
                out->sections = ns;
                ini_section *s = &out->sections[out->num_sections++];
                s->name = dup_str(line); s->keys = NULL; s->num_keys = 0;
            }
        } else if (line[0] != '\0' && line[0] != '#' && line[0] != ';' && line[0] != '!') {
            char *eq = strchr(line, '=');
            if (out->num_sections == 0 || !eq || eq == line || eq[1] == '\0' || strchr(eq + 1, '=')) {
                fprintf(stderr, "[ERROR] Invalid key section %s\n", line);
                rc = -1;
            } else {
                ini_section *s = &out->sections[out->num_sections - 1];
                ini_key *nk = (ini_key *)realloc(s->keys, (size_t)(s->num_keys + 1) * sizeof(ini_key));
                if (!nk) rc = -1;
                else {
                    s->keys = nk;
                    *eq = '\0';
                    s->keys[s->num_keys].name = dup_str(line);
                    s->keys[s->num_keys].val = dup_str(eq + 1);
                    s->num_keys++;
                }
            }
        }
        free(line);
    }
    fclose(fp);
    if (rc != 0) {
        fprintf(stderr, "[ERROR] Failed to parse config file %s\n", path);
        ini_free(out);
    }
    return rc;
}

/* ---- [net] parameters (reference bcnn_net_set_param, :504-593) ------------------------------------- */
static void net_set_param(bcnn_net *net, const char *name, const char *val) {
    bcnn_learner *ln = net->learner;
    bcnn_data_augmenter *da = net->data_aug;
    if (!strcmp(name, "input_width") || !strcmp(name, "width")) net->tensors[0].w = atoi(val);
    else if (!strcmp(name, "input_height") || !strcmp(name, "height")) net->tensors[0].h = atoi(val);
    else if (!strcmp(name, "input_channels") || !strcmp(name, "channels")) net->tensors[0].c = atoi(val);
    else if (!strcmp(name, "batch_size") || !strcmp(name, "batch")) { net->batch_size = atoi(val); net->tensors[0].n = atoi(val); }
    else if (!strcmp(name, "inference_precision")) {
        if (!strcmp(val, "bf16")) bcnn_set_inference_precision(net, BCNN_PRECISION_BF16);
        else if (!strcmp(val, "fp32")) bcnn_set_inference_precision(net, BCNN_PRECISION_FP32);
        else bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown inference_precision %s (bf16 or fp32), keeping the current one\n", val);
    }
    else if (!strcmp(name, "loader_on_device")) bcnn_set_loader_on_device(net, atoi(val));
    else if (!strcmp(name, "loader_decode_on_device")) bcnn_set_loader_decode_on_device(net, atoi(val));
    else if (!strcmp(name, "loader_detection_on_device")) bcnn_set_loader_detection_on_device(net, atoi(val));
    else if (!strcmp(name, "loader_effects")) bcnn_set_loader_effects(net, atoi(val));
    else if (!strcmp(name, "train_detector")) bcnn_set_detector_training(net, atoi(val));
    else if (ln && !strcmp(name, "max_batches")) ln->max_batches = atoi(val);
    else if (ln && (!strcmp(name, "learning_policy") || !strcmp(name, "decay_type"))) {
        if (!strcmp(val, "sigmoid")) ln->decay_type = BCNN_LR_DECAY_SIGMOID;
        else if (!strcmp(val, "exp")) ln->decay_type = BCNN_LR_DECAY_EXP;
        else if (!strcmp(val, "inv")) ln->decay_type = BCNN_LR_DECAY_INV;
        else if (!strcmp(val, "step")) ln->decay_type = BCNN_LR_DECAY_STEP;
        else if (!strcmp(val, "poly")) ln->decay_type = BCNN_LR_DECAY_POLY;
        else ln->decay_type = BCNN_LR_DECAY_CONSTANT;
    } else if (ln && !strcmp(name, "optimizer")) {
        if (!strcmp(val, "sgd")) ln->optimizer = BCNN_OPTIM_SGD;
        else if (!strcmp(val, "adam")) ln->optimizer = BCNN_OPTIM_ADAM;
    } else if (ln && !strcmp(name, "step")) ln->step = atoi(val);
    else if (ln && !strcmp(name, "learning_rate")) ln->base_learning_rate = ln->learning_rate = (float)atof(val);
    else if (ln && !strcmp(name, "beta1")) ln->beta1 = (float)atof(val);
    else if (ln && !strcmp(name, "beta2")) ln->beta2 = (float)atof(val);
    else if (ln && !strcmp(name, "decay")) ln->decay = (float)atof(val);
    else if (ln && !strcmp(name, "momentum")) ln->momentum = (float)atof(val);
    else if (ln && !strcmp(name, "gamma")) ln->gamma = (float)atof(val);
    else if (da && !strcmp(name, "range_shift_x")) da->range_shift_x = atoi(val);
    else if (da && !strcmp(name, "range_shift_y")) da->range_shift_y = atoi(val);
    else if (da && !strcmp(name, "min_scale")) da->min_scale = (float)atof(val);
    else if (da && !strcmp(name, "max_scale")) da->max_scale = (float)atof(val);
    else if (da && !strcmp(name, "rotation_range")) da->rotation_range = (float)atof(val);
    else if (da && !strcmp(name, "min_contrast")) da->min_contrast = (float)atof(val);
    else if (da && !strcmp(name, "max_contrast")) da->max_contrast = (float)atof(val);
    else if (da && !strcmp(name, "min_brightness")) da->min_brightness = atoi(val);
    else if (da && !strcmp(name, "max_brightness")) da->max_brightness = atoi(val);
    else if (da && !strcmp(name, "max_distortion")) {
        const float v = (float)atof(val); /* a strength: negative, NaN and infinity are refused and the key is dropped */
        if (v >= 0.0f && v <= FLT_MAX) da->max_distortion = v;
        else bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "max_distortion=%s is negative or not finite, keeping the current one\n", val);
    }
    else if (da && !strcmp(name, "max_spots")) da->max_random_spots = (int)atof(val);
    else if (da && !strcmp(name, "flip_h")) da->random_fliph = 1;
    else if (da && !strcmp(name, "mean_r")) da->mean_r = (float)atof(val) / 255.0f;
    else if (da && !strcmp(name, "mean_g")) da->mean_g = (float)atof(val) / 255.0f;
    else if (da && !strcmp(name, "mean_b")) da->mean_b = (float)atof(val) / 255.0f;
    else if (da && !strcmp(name, "swap_to_bgr")) da->swap_to_bgr = atoi(val);
    else if (da && !strcmp(name, "no_input_norm")) da->no_input_norm = atoi(val);
}

/* ---- layer parameters (reference bcnn_layer_param, :683-966) ------------------------------------- */
#define MAX_SRCS 16
typedef struct {
    int stride, pad, n_filts, size, outputs, num_groups, batchnorm, in_w, in_h, in_c;
    float alpha, beta, k, rate;
    bcnn_padding padding_type;
    bcnn_activation a;
    bcnn_filler_type init;
    bcnn_loss_metric cost;
    bcnn_loss loss;
    int num_srcs;
    char *src_id[MAX_SRCS];
    char *dst_id;
    int boxes_per_cell, num_anchors, num_classes, num_coords, num_anchor_vals; /* [yolo] */
    int *anchors_mask;
    float *anchors;
    /* [pool] / [local_avgpool]: which of size / stride the section set (their defaults differ from the other sections'),
     * `pad` as written (a count per side in both dialects), and the three keys only these sections read */
    int has_size, has_stride, pool_pad, pool_avg, ceil_mode, count_include_pad;
    int has_from; /* Darknet `from=`: src_id[0] is the previous section, src_id[1] the named one */
    int has_groups; /* [groupnorm]: the section wrote groups= (the default of num_groups, 1, belongs to convolutions) */
    float eps;      /* [groupnorm] / [layernorm] / [instancenorm]; 0: the builder's default */
    int dilation;   /* [conv] / [convolutional], [depthwise-conv] / [dw-conv]: > 1 builds the dilated node; default 1 */
    int scale, zoom, out_w, out_h, align_corners; /* [interp] / [bilinear]; scale= may be written stride= (has_stride) */
    /* [softmax_loss] / [softmaxwithloss]: ignore_label (default -1), normalize (a bcnn_loss_norm, -1: a value the section
     * wrote that is none of the three names; default valid_per_image) and scale= read as a float (default 1) */
    int ignore_label, loss_norm;
    float loss_scale;
} layer_param;

static void lp_reset(layer_param *lp) {
    for (int i = 0; i < lp->num_srcs; ++i) free(lp->src_id[i]);
    free(lp->dst_id);
    free(lp->anchors_mask);
    free(lp->anchors);
    memset(lp, 0, sizeof(*lp));
    lp->stride = 1; lp->n_filts = 1; lp->size = 3; lp->num_groups = 1; lp->rate = 1.0f; lp->num_coords = 4;
    lp->padding_type = BCNN_PADDING_SAME; lp->a = BCNN_ACT_NONE; lp->init = BCNN_FILLER_XAVIER;
    lp->cost = BCNN_METRIC_SSE; lp->loss = BCNN_LOSS_EUCLIDEAN;
    lp->k = 1.0f; /* [lrn] without a k key: the Caffe / torch default */
    lp->count_include_pad = 1; /* [pool] type=avg: the Caffe / torch default */
    lp->dilation = 1;
    lp->ignore_label = -1; lp->loss_norm = (int)BCNN_LOSS_NORM_VALID_PER_IMAGE; lp->loss_scale = 1.0f;
}

static void lp_set_srcs(layer_param *lp, const char *list) {
    for (int i = 0; i < lp->num_srcs; ++i) free(lp->src_id[i]);
    lp->num_srcs = 0;
    const char *p = list;
    while (*p && lp->num_srcs < MAX_SRCS) {
        const char *e = strchr(p, ',');
        size_t n = e ? (size_t)(e - p) : strlen(p);
        if (n > 0) {
            char *s = (char *)malloc(n + 1);
            memcpy(s, p, n);
            s[n] = '\0';
            lp->src_id[lp->num_srcs++] = s;
        }
        if (!e) break;
        p = e + 1;
    }
}

/* comma-separated list -> number of entries; *out (calloc) gets each entry through atof (reference: bh_strsplit + atof/atoi) */
static int split_floats(const char *list, float **out) {
    int n = 1;
    for (const char *p = list; *p; ++p) n += *p == ',';
    *out = (float *)calloc((size_t)n, sizeof(float));
    const char *p = list;
    for (int i = 0; i < n; ++i) {
        (*out)[i] = (float)atof(p);
        const char *e = strchr(p, ',');
        if (!e) break;
        p = e + 1;
    }
    return n;
}

static void lp_set_lid(char **dst, int id) {
    char lid[32];
    snprintf(lid, sizeof(lid), "lid%d", id);
    free(*dst);
    *dst = dup_str(lid);
}

static void lp_set(bcnn_net *net, int section_idx, layer_param *lp, const char *name, const char *val, int format) {
    if (!strcmp(name, "dropout_rate") || !strcmp(name, "rate") || !strcmp(name, "probability")) /* Darknet: probability */
        lp->rate = (float)atof(val);
    else if (!strcmp(name, "filters")) lp->n_filts = atoi(val);
    else if (!strcmp(name, "size")) { lp->size = atoi(val); lp->has_size = 1; }
    else if (!strcmp(name, "stride")) { lp->stride = atoi(val); lp->has_stride = 1; }
    else if (!strcmp(name, "type")) { /* [pool] */
        if (!strcmp(val, "avg") || !strcmp(val, "average")) lp->pool_avg = 1;
        else if (!strcmp(val, "max")) lp->pool_avg = 0;
        else bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown pooling type %s, going with max\n", val);
    } else if (!strcmp(name, "ceil_mode")) lp->ceil_mode = atoi(val);
    else if (!strcmp(name, "count_include_pad")) lp->count_include_pad = atoi(val);
    else if (!strcmp(name, "padding")) {
        if (format == 1) { lp->pad = atoi(val); lp->padding_type = lp->pad ? BCNN_PADDING_SAME : BCNN_PADDING_VALID; }
    } else if (!strcmp(name, "pad")) {
        lp->pool_pad = atoi(val);
        if (format == 0) lp->pad = atoi(val);
        else lp->pad = atoi(val) ? lp->size / 2 : 0; /* Darknet: boolean, needs `size` to come first */
    } else if (!strcmp(name, "num_groups") || !strcmp(name, "groups")) { lp->num_groups = atoi(val); lp->has_groups = 1; }
    else if (!strcmp(name, "eps")) lp->eps = (float)atof(val);
    else if (!strcmp(name, "dilation")) lp->dilation = atoi(val);
    else if (!strcmp(name, "scale")) { lp->scale = atoi(val); lp->loss_scale = (float)atof(val); }
    else if (!strcmp(name, "ignore_label")) lp->ignore_label = atoi(val);
    else if (!strcmp(name, "normalize")) {
        if (!strcmp(val, "none")) lp->loss_norm = (int)BCNN_LOSS_NORM_NONE;
        else if (!strcmp(val, "valid")) lp->loss_norm = (int)BCNN_LOSS_NORM_VALID;
        else if (!strcmp(val, "valid_per_image")) lp->loss_norm = (int)BCNN_LOSS_NORM_VALID_PER_IMAGE;
        else lp->loss_norm = -1; /* refused by the section that reads it: no silent fallback */
    }
    else if (!strcmp(name, "zoom")) lp->zoom = atoi(val);
    else if (!strcmp(name, "out_w")) lp->out_w = atoi(val);
    else if (!strcmp(name, "out_h")) lp->out_h = atoi(val);
    else if (!strcmp(name, "align_corners")) lp->align_corners = atoi(val);
    /* only [lrn] reads these three; atof, where the reference's atoi loads a Caffe LRN (alpha=0.0001) as the identity */
    else if (!strcmp(name, "alpha")) lp->alpha = (float)atof(val);
    else if (!strcmp(name, "beta")) lp->beta = (float)atof(val);
    else if (!strcmp(name, "k")) lp->k = (float)atof(val);
    else if (!strcmp(name, "w")) lp->in_w = atoi(val);
    else if (!strcmp(name, "h")) lp->in_h = atoi(val);
    else if (!strcmp(name, "c")) lp->in_c = atoi(val);
    else if (!strcmp(name, "bn") || !strcmp(name, "batchnorm") || !strcmp(name, "batch_normalize")) lp->batchnorm = atoi(val);
    else if (!strcmp(name, "src")) lp_set_srcs(lp, val);
    else if (!strcmp(name, "dst")) { free(lp->dst_id); lp->dst_id = dup_str(val); }
    else if (!strcmp(name, "output")) lp->outputs = atoi(val);
    else if (!strcmp(name, "padding_type")) {
        if (!strcmp(val, "same")) lp->padding_type = BCNN_PADDING_SAME;
        else if (!strcmp(val, "valid")) lp->padding_type = BCNN_PADDING_VALID;
        else if (!strcmp(val, "caffe")) lp->padding_type = BCNN_PADDING_CAFFE;
    } else if (!strcmp(name, "function") || !strcmp(name, "activation")) {
        if (!strcmp(val, "relu")) lp->a = BCNN_ACT_RELU;
        else if (!strcmp(val, "tanh")) lp->a = BCNN_ACT_TANH;
        else if (!strcmp(val, "ramp")) lp->a = BCNN_ACT_RAMP;
        else if (!strcmp(val, "clamp")) lp->a = BCNN_ACT_CLAMP;
        else if (!strcmp(val, "softplus")) lp->a = BCNN_ACT_SOFTPLUS;
        else if (!strcmp(val, "leaky_relu") || !strcmp(val, "lrelu") || !strcmp(val, "leaky")) lp->a = BCNN_ACT_LRELU;
        else if (!strcmp(val, "prelu")) lp->a = BCNN_ACT_PRELU;
        else if (!strcmp(val, "abs")) lp->a = BCNN_ACT_ABS;
        else if (!strcmp(val, "none") || !strcmp(val, "linear")) lp->a = BCNN_ACT_NONE;
        else if (!strcmp(val, "logistic") || !strcmp(val, "sigmoid")) lp->a = BCNN_ACT_LOGISTIC;
        else if (!strcmp(val, "relu6")) lp->a = BCNN_ACT_RELU6;
        else if (!strcmp(val, "hard_sigmoid") || !strcmp(val, "hardsigmoid")) lp->a = BCNN_ACT_HARD_SIGMOID;
        else if (!strcmp(val, "hard_swish") || !strcmp(val, "hardswish") || !strcmp(val, "hswish")) lp->a = BCNN_ACT_HARD_SWISH;
        else if (!strcmp(val, "swish") || !strcmp(val, "silu")) lp->a = BCNN_ACT_SWISH;
        else if (!strcmp(val, "mish")) lp->a = BCNN_ACT_MISH;
        else {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown activation type %s, going with ReLU\n", val);
            lp->a = BCNN_ACT_RELU;
        }
    } else if (!strcmp(name, "init")) {
        if (!strcmp(val, "xavier")) lp->init = BCNN_FILLER_XAVIER;
        else if (!strcmp(val, "msra")) lp->init = BCNN_FILLER_MSRA;
        else {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown init type %s, going with xavier init\n", val);
            lp->init = BCNN_FILLER_XAVIER;
        }
    } else if (!strcmp(name, "metric")) {
        if (!strcmp(val, "error")) lp->cost = BCNN_METRIC_ERROR_RATE;
        else if (!strcmp(val, "logloss")) lp->cost = BCNN_METRIC_LOGLOSS;
        else if (!strcmp(val, "sse")) lp->cost = BCNN_METRIC_SSE;
        else if (!strcmp(val, "mse")) lp->cost = BCNN_METRIC_MSE;
        else if (!strcmp(val, "crps")) lp->cost = BCNN_METRIC_CRPS;
        else if (!strcmp(val, "dice")) lp->cost = BCNN_METRIC_DICE;
        else {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown cost metric %s, going with sse\n", val);
            lp->cost = BCNN_METRIC_SSE;
        }
    } else if (!strcmp(name, "loss")) {
        if (!strcmp(val, "l2") || !strcmp(val, "euclidean")) lp->loss = BCNN_LOSS_EUCLIDEAN;
        else if (!strcmp(val, "lifted_struct_similarity")) lp->loss = BCNN_LOSS_LIFTED_STRUCT;
        else {
            bcnn_log(net->log_ctx, BCNN_LOG_WARNING, "Unknown loss %s, going with euclidean loss\n", val);
            lp->loss = BCNN_LOSS_EUCLIDEAN;
        }
    } else if (!strcmp(name, "layers")) { /* Darknet [route]: absolute (0-based) or relative section numbers */
        lp_set_srcs(lp, val);
        for (int i = 0; i < lp->num_srcs; ++i) {
            const int l = atoi(lp->src_id[i]);
            lp_set_lid(&lp->src_id[i], l >= 0 ? l + 1 : section_idx + l);
        }
    } else if (!strcmp(name, "from")) { /* Darknet [shortcut] / [scale_channels] / [sam]: previous section + the named one */
        const int l = atoi(val);
        lp->has_from = 1;
        lp_set_srcs(lp, "a,b");
        lp_set_lid(&lp->src_id[0], section_idx - 1);
        lp_set_lid(&lp->src_id[1], l >= 0 ? l + 1 : section_idx + l);
    } else if (!strcmp(name, "boxes_per_cell")) lp->boxes_per_cell = atoi(val); /* the YOLO head: reference :792-818 */
    else if (!strcmp(name, "num_anchors") || !strcmp(name, "num")) lp->num_anchors = atoi(val);
    else if (!strcmp(name, "num_classes") || !strcmp(name, "classes")) lp->num_classes = atoi(val);
    else if (!strcmp(name, "num_coords")) lp->num_coords = atoi(val);
    else if (!strcmp(name, "anchors")) {
        free(lp->anchors);
        lp->num_anchor_vals = split_floats(val, &lp->anchors);
    } else if (!strcmp(name, "anchors_mask") || !strcmp(name, "mask")) {
        float *m = NULL;
        lp->boxes_per_cell = split_floats(val, &m);
        free(lp->anchors_mask);
        lp->anchors_mask = (int *)calloc((size_t)lp->boxes_per_cell, sizeof(int));
        for (int i = 0; i < lp->boxes_per_cell; ++i) lp->anchors_mask[i] = (int)m[i];
        free(m);
    }
}

static int is_any(const char *name, const char *a, const char *b, const char *c, const char *d) {
    return !strcmp(name, a) || (b && !strcmp(name, b)) || (c && !strcmp(name, c)) || (d && !strcmp(name, d));
}

/* A section with a fused activation that asks for hard-swish, swish or mish -- whose derivative needs the layer's output
 * BEFORE the activation, which a fused layer does not keep -- is built as the layer with no activation plus the in-place
 * activation node on its output. The section still stands for that output (Darknet's lid chain). */
static bcnn_activation fused_act(const layer_param *lp) { return bcnn_act_needs_input(lp->a) ? BCNN_ACT_NONE : lp->a; }
static bcnn_status add_split_act(bcnn_net *net, bcnn_status st, const layer_param *lp) {
    if (st != BCNN_SUCCESS || !bcnn_act_needs_input(lp->a)) return st;
    return bcnn_add_activation_layer(net, lp->a, lp->dst_id);
}

static bcnn_status add_layer(bcnn_net *net, const char *name, layer_param *lp) {
    if (net->num_nodes == 0) {
        BCNN_CHECK_AND_LOG(net->log_ctx, net->tensors[0].w > 0 && net->tensors[0].h > 0 && net->tensors[0].c > 0,
                           BCNN_INVALID_PARAMETER, "Input's width, height and channels must be > 0\n");
        BCNN_CHECK_AND_LOG(net->log_ctx, net->tensors[0].n > 0, BCNN_INVALID_PARAMETER, "Batch size must be > 0\n");
    }
    BCNN_CHECK_AND_LOG(net->log_ctx, lp->num_srcs > 0 && lp->src_id[0], BCNN_INVALID_PARAMETER,
                       "Invalid input node name. Hint: Are you sure that 'src' field is correctly setup?\n");
    const char *src = lp->src_id[0], *dst = lp->dst_id;
    const int needs_dst = !is_any(name, "[input]", "[activation]", "[nl]", "[dropout]");
    BCNN_CHECK_AND_LOG(net->log_ctx, !needs_dst || dst, BCNN_INVALID_PARAMETER,
                       "Invalid output node name. Hint: Are you sure that 'dst' field is correctly setup?\n");
    if (!strcmp(name, "[input]")) return bcnn_add_input(net, lp->in_w, lp->in_h, lp->in_c, src);
    if (is_any(name, "[conv]", "[convolutional]", NULL, NULL) && lp->dilation > 1) {
        if (!lp->batchnorm)
            return add_split_act(net, bcnn_add_dilated_conv_layer(net, lp->n_filts, lp->size, lp->stride, lp->pad, lp->dilation,
                                                                  lp->num_groups, lp->init, fused_act(lp), src, dst), lp);
        /* The dilated node has no fused batch-norm: the section becomes the node with no activation into "<dst>_dc", a
         * batch-norm node from there into dst, and the activation in place on dst. The section still stands for dst. */
        char inner[256];
        snprintf(inner, sizeof(inner), "%s_dc", dst);
        BCNN_CHECK_STATUS(bcnn_add_dilated_conv_layer(net, lp->n_filts, lp->size, lp->stride, lp->pad, lp->dilation,
                                                      lp->num_groups, lp->init, BCNN_ACT_NONE, src, inner));
        ((bcnn_dilated_conv_param *)net->nodes[net->num_nodes - 1].param)->section_bn = 1;
        BCNN_CHECK_STATUS(bcnn_add_batchnorm_layer(net, inner, dst));
        return lp->a == BCNN_ACT_NONE ? BCNN_SUCCESS : bcnn_add_activation_layer(net, lp->a, dst);
    }
    if (is_any(name, "[conv]", "[convolutional]", NULL, NULL))
        return add_split_act(net,bcnn_add_convolutional_layer(net, lp->n_filts, lp->size, lp->stride, lp->pad, lp->num_groups,
                                                               lp->batchnorm, lp->init, fused_act(lp), 0, src, dst), lp);
    if (is_any(name, "[deconv]", "[deconvolutional]", NULL, NULL))
        return add_split_act(net, bcnn_add_deconvolutional_layer(net, lp->n_filts, lp->size, lp->stride, lp->pad, lp->init,
                                                                 fused_act(lp), src, dst), lp);
    if (is_any(name, "[depthwise-conv]", "[dw-conv]", NULL, NULL) && lp->dilation > 1)
        return add_split_act(net, bcnn_add_dilated_depthwise_conv_layer(net, lp->size, lp->stride, lp->pad, lp->dilation,
                                                                        lp->init, fused_act(lp), src, dst), lp);
    if (is_any(name, "[depthwise-conv]", "[dw-conv]", NULL, NULL))
        return add_split_act(net, bcnn_add_depthwise_conv_layer(net, lp->size, lp->stride, lp->pad, 0, lp->init, fused_act(lp),
                                                                src, dst), lp);
    if (is_any(name, "[activation]", "[nl]", NULL, NULL)) return bcnn_add_activation_layer(net, lp->a, src);
    if (is_any(name, "[batchnorm]", "[bn]", NULL, NULL)) return bcnn_add_batchnorm_layer(net, src, dst);
    if (!strcmp(name, "[lrn]")) return bcnn_add_lrn_layer(net, lp->size, lp->alpha, lp->beta, lp->k, src, dst);
    if (is_any(name, "[connected]", "[fullconnected]", "[fc]", "[ip]"))
        return add_split_act(net, bcnn_add_fullc_layer(net, lp->outputs, lp->init, fused_act(lp), 0, src, dst), lp);
    if (!strcmp(name, "[softmax]")) return bcnn_add_softmax_layer(net, src, dst);
    if (is_any(name, "[max]", "[maxpool]", NULL, NULL))
        return bcnn_add_maxpool_layer(net, lp->size, lp->stride, lp->padding_type, src, dst);
    if (!strcmp(name, "[avgpool]")) return bcnn_add_avgpool_layer(net, src, dst);
    if (is_any(name, "[pool]", "[pool2d]", "[local_avgpool]", NULL)) {
        /* the windowed, centred pools ([maxpool] pads at the bottom / right only and [avgpool] is global, in both dialects).
         * Defaults: max, size 2, stride = size, pad 0, floor mode, padding counted; [local_avgpool] is type=avg */
        const int size = lp->has_size ? lp->size : 2, stride = lp->has_stride ? lp->stride : size;
        const int avg = lp->pool_avg || !strcmp(name, "[local_avgpool]");
        return bcnn_add_pool2d_layer(net, avg ? BCNN_POOL2D_AVG : BCNN_POOL2D_MAX, size, stride, lp->pool_pad, lp->ceil_mode,
                                     lp->count_include_pad, src, dst);
    }
    if (!strcmp(name, "[upsample]")) return bcnn_add_upsample_layer(net, lp->stride, src, dst);
    if (is_any(name, "[interp]", "[bilinear]", NULL, NULL)) {
        /* exactly one of scale= (Darknet's word: stride=), zoom= and out_w= / out_h=; the builder refuses anything else.
         * As the first section it reads the net input whatever src says, like every other first section. */
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->a == BCNN_ACT_NONE, BCNN_INVALID_PARAMETER,
                           "Interp layer %s: only activation=linear is supported; add an [activation] section\n", dst);
        BCNN_CHECK_AND_LOG(net->log_ctx, !(lp->scale && lp->has_stride), BCNN_INVALID_PARAMETER,
                           "Interp layer %s: scale= and stride= are two words for one key\n", dst);
        return bcnn_add_interp_layer(net, lp->out_w, lp->out_h, lp->has_stride ? lp->stride : lp->scale, lp->zoom,
                                     lp->align_corners, net->num_nodes == 0 ? net->tensors[0].name : src, dst);
    }
    if (!strcmp(name, "[dropout]")) return bcnn_add_dropout_layer(net, lp->rate, src);
    if (is_any(name, "[concat]", "[route]", NULL, NULL))
        return bcnn_add_concat_layer(net, lp->num_srcs, (char *const *)lp->src_id, dst);
    if (is_any(name, "[eltwise]", "[shortcut]", NULL, NULL)) {
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->num_srcs >= 2, BCNN_INVALID_PARAMETER,
                           "Eltwise layer needs two sources (src=a,b)\n");
        return add_split_act(net, bcnn_add_eltwise_layer(net, fused_act(lp), lp->src_id[0], lp->src_id[1], dst), lp);
    }
    if (is_any(name, "[scale_channels]", "[sam]", NULL, NULL)) {
        /* bcnn dialect: src=features,gate. Darknet: `from=` names the FEATURES and the previous section is the gate
         * (scale_channels_layer.c / sam_layer.c), the reverse of [shortcut]'s order in src_id. The gate's shape picks the
         * form, so the two names build the same node. */
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->num_srcs >= 2, BCNN_INVALID_PARAMETER,
                           "Scale-channels layer needs two sources (src=features,gate or from=)\n");
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->a == BCNN_ACT_NONE, BCNN_INVALID_PARAMETER,
                           "Scale-channels layer %s: only activation=linear is supported; add an [activation] section\n", dst);
        return bcnn_add_scale_channels_layer(net, lp->src_id[lp->has_from ? 1 : 0], lp->src_id[lp->has_from ? 0 : 1], dst);
    }
    if (is_any(name, "[groupnorm]", "[gn]", "[layernorm]", "[instancenorm]")) {
        /* one node: layer norm over (C,H,W) is one group, instance norm one group per channel of the source */
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->a == BCNN_ACT_NONE, BCNN_INVALID_PARAMETER,
                           "Group-norm layer %s: only activation=linear is supported; add an [activation] section\n", dst);
        int groups = lp->num_groups;
        if (!strcmp(name, "[layernorm]")) groups = 1;
        else if (!strcmp(name, "[instancenorm]")) {
            const int idx = net->num_nodes > 0 ? bcnn_net_find_tensor(net, src) : 0;
            BCNN_CHECK_AND_LOG(net->log_ctx, idx >= 0, BCNN_INVALID_PARAMETER,
                               "Instance-norm layer: invalid input node name %s\n", src);
            groups = net->tensors[idx].c;
        } else
            BCNN_CHECK_AND_LOG(net->log_ctx, lp->has_groups, BCNN_INVALID_PARAMETER,
                               "Group-norm layer %s: the section needs a groups= key\n", dst);
        return bcnn_add_groupnorm_layer(net, groups, lp->eps, src, dst);
    }
    if (!strcmp(name, "[yolo]")) {
        /* the builder copies 2 * num values (the reference reads past a shorter list); pad a short one with zeros */
        if (lp->anchors && lp->num_anchor_vals < 2 * lp->num_anchors) {
            float *a = (float *)calloc((size_t)2 * lp->num_anchors, sizeof(float));
            memcpy(a, lp->anchors, (size_t)lp->num_anchor_vals * sizeof(float));
            free(lp->anchors);
            lp->anchors = a;
            lp->num_anchor_vals = 2 * lp->num_anchors;
        }
        return bcnn_add_yolo_layer(net, lp->boxes_per_cell, lp->num_classes, lp->num_coords, lp->num_anchors,
                                   lp->anchors_mask, lp->anchors, src, dst);
    }
    if (is_any(name, "[softmax_loss]", "[softmaxwithloss]", NULL, NULL)) {
        BCNN_CHECK_AND_LOG(net->log_ctx, lp->loss_norm >= 0, BCNN_INVALID_PARAMETER,
                           "Softmax-loss layer %s: normalize must be none, valid or valid_per_image\n", dst);
        return bcnn_add_softmax_loss_layer(net, lp->ignore_label, (bcnn_loss_norm)lp->loss_norm, lp->loss_scale, src, "label",
                                           dst);
    }
    if (!strcmp(name, "[cost]")) return bcnn_add_cost_layer(net, lp->loss, lp->cost, 1.0f, src, "label", dst);
    bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Unknown Layer %s\n", name);
    return BCNN_INVALID_PARAMETER;
}

bcnn_status bcnn_load_net(bcnn_net *net, const char *config_path, const char *model_path) {
    int format = 0;
    if (model_path != NULL) { /* the model file's extension selects the dialect of the config file too */
        const char *dot = strrchr(model_path, '.');
        BCNN_CHECK_AND_LOG(net->log_ctx, dot && dot != model_path, BCNN_INVALID_DATA,
                           "File %s needs to have an extension (.bcnnmodel OR .onnx OR .weights)\n", model_path);
        if (!strcmp(dot + 1, "weights")) format = 1;
        else if (!strcmp(dot + 1, "onnx")) format = 2;
    }
    BCNN_CHECK_AND_LOG(net->log_ctx, format != 2, BCNN_INVALID_MODEL, "ONNX models are not supported by this build\n");
    BCNN_CHECK_AND_LOG(net->log_ctx, config_path, BCNN_INVALID_PARAMETER, "No config file given\n");
    ini_file cfg;
    if (ini_read(config_path, &cfg) != 0) return BCNN_INVALID_PARAMETER;
    bcnn_status st = BCNN_SUCCESS;
    if (cfg.num_sections == 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Empty config file %s\n", config_path);
        st = BCNN_INVALID_PARAMETER;
    } else if (strcmp(cfg.sections[0].name, "[net]") != 0 && strcmp(cfg.sections[0].name, "[network]") != 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid config file %s: First section must be [net] or [network]\n",
                 config_path);
        st = BCNN_INVALID_PARAMETER;
    } else if (cfg.sections[0].num_keys == 0) {
        bcnn_log(net->log_ctx, BCNN_LOG_ERROR, "Invalid config file %s: empty section [net]\n", config_path);
        st = BCNN_INVALID_PARAMETER;
    }
    if (st == BCNN_SUCCESS) {
        for (int i = 0; i < cfg.sections[0].num_keys; ++i)
            net_set_param(net, cfg.sections[0].keys[i].name, cfg.sections[0].keys[i].val);
        layer_param lp;
        memset(&lp, 0, sizeof(lp));
        lp_reset(&lp);
        /* Darknet: the tensor each section stands for. An in-place section ([dropout], [activation]) creates no tensor
         * "lid<i>": it stands for its source, so the next section and `layers=` / `from=` offsets read that tensor */
        char **stands_for = (char **)calloc((size_t)cfg.num_sections, sizeof(char *));
        for (int i = 1; st == BCNN_SUCCESS && i < cfg.num_sections; ++i) {
            for (int j = 0; j < cfg.sections[i].num_keys; ++j)
                lp_set(net, i, &lp, cfg.sections[i].keys[j].name, cfg.sections[i].keys[j].val, format);
            if (format == 1) { /* Darknet: implicit chaining of unnamed tensors */
                if (lp.num_srcs == 0) { /* "lid0" for the first layer: its builder takes the net input regardless */
                    lp_set_srcs(&lp, "x");
                    lp_set_lid(&lp.src_id[0], i - 1);
                }
                if (lp.dst_id == NULL) lp_set_lid(&lp.dst_id, i);
                for (int k = 0; k < lp.num_srcs; ++k) {
                    char *end = NULL;
                    const long j = strncmp(lp.src_id[k], "lid", 3) ? -1 : strtol(lp.src_id[k] + 3, &end, 10);
                    if (j > 0 && j < i && end && *end == '\0' && stands_for[j]) {
                        free(lp.src_id[k]);
                        lp.src_id[k] = dup_str(stands_for[j]);
                    }
                }
                const int in_place = is_any(cfg.sections[i].name, "[activation]", "[nl]", "[dropout]", NULL);
                stands_for[i] = dup_str(in_place && lp.num_srcs > 0 ? lp.src_id[0] : lp.dst_id);
            }
            st = add_layer(net, cfg.sections[i].name, &lp);
            lp_reset(&lp);
        }
        for (int i = 0; i < cfg.num_sections; ++i) free(stands_for[i]);
        free(stands_for);
        lp_reset(&lp);
    }
    ini_free(&cfg);
    if (st != BCNN_SUCCESS) return st;
    if (model_path != NULL) {
        BCNN_INFO(net->log_ctx, "Loading pre-trained model %s\n", model_path);
        BCNN_CHECK_STATUS(bcnn_load_weights(net, model_path));
    }
    return BCNN_SUCCESS;
}
