// conv.hip -- C-ABI entry points of the convolution node (include/bcnn_hip.h), composing the
// implicit-GEMM kernels (conv_fwd.hip, conv_bwd.hip) with the batch-norm / activation kernels the way
// bcnn_forward_conv_layer_cpu / bcnn_backward_conv_layer_cpu do (reference bcnn_conv_layer.c:367-587).
// Each entry point writes what it was given into a ConvNodeFwd / ConvNodeBwd by name and hands it to conv_forward_impl /
// conv_backward_impl. The calling thread's pending batch-norm fold and its side-stream mode enter there, at the ABI boundary,
// and nothing below reads them again (conv_side_stream_deferred, which the weight-gradient kernels ask, apart).
#include "batchnorm.h"
#include "conv_paths.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace bcnn_hip {
// ---- a stand-alone batch-norm node in front of a 1x1 convolution, folded into it (BnFold, conv_common.h) -------------
// The host announces the fold right before the forward / backward call it applies to (same thread): the call takes it.
static thread_local BnFold g_fold_pending = {nullptr, nullptr, nullptr, nullptr};
static BnFold take_fold() {
    const BnFold f = g_fold_pending;
    g_fold_pending = BnFold{nullptr, nullptr, nullptr, nullptr};
    return f;
}
static bool bnfold_shape_ok(const ConvShape& s) {
    return s.ksz == 1 && s.stride == 1 && s.pad == 0 && s.groups == 1 && conv_dma_fwd_wanted(s) &&
           conv_dw_dma_workspace_floats(s) > 0;
}
// rowc[f] = sum_c W[f][c] b[c], b[c] = bias - mean a[c] (a = scale / sqrt(var + 1e-6); the reference's bcnn_add_scalar adds
// nothing for a bias of exactly 0 or 1, bcnn_mat.c:366-412): what the folded-away constant adds to every output of filter f.
// One wave per filter.
__global__ __launch_bounds__(256) void bnfold_rowconst_kernel(const float* __restrict__ w, const BnFold fold, int F, int C,
                                                              float* __restrict__ rowc) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= F) return;
    double acc = 0.0;
    for (int c = lane; c < C; c += 64) {
        float bv = fold.bias[c];
        if (bv == 1.0f) bv = 0.f;
        const float b = bv - fold.mean[c] * bnfold_a(fold.var, fold.scales, c);
        acc += (double)w[(size_t)f * C + c] * (double)b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) rowc[f] = (float)acc;
}
static float* fold_rowconst(const BnFold& fold, const float* w, int C, int F) {
    float* rowc = scratch(SCRATCH_FOLD_ROWCONST, (size_t)F);
    bnfold_rowconst_kernel<<<ceil_div(F, 4), 256, 0, current_stream()>>>(w, fold, F, C, rowc);
    KERNEL_CHECK();
    return rowc;
}


// side stream for the weight-gradient GEMM of bcnn_hip_conv_backward: one per host thread and device, created on first use
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr, done = nullptr;
    bool pending = false;  // deferred mode: work queued whose completion the caller's stream has not been ordered behind yet
};
static thread_local SideStream g_side[kMaxDevices];
// 0: weight gradients on the caller's stream (default); 1: on the side stream, joined before the call returns (the round-1
// experiment); 2: on the side stream, joined when the caller says so (bcnn_hip_conv_side_join) -- bcnn_backward's mode: the
// weight gradient of a layer then runs next to the batch-norm / pooling sweeps and the data gradients of the layers in front
static thread_local int g_side_mode = 0;
bool conv_side_stream_deferred() { return g_side_mode == 2; }
static SideStream* side_stream() {
    SideStream& ss = g_side[current_device()];
    if (ss.stream == nullptr) {
        // lowest priority: when a CU frees up, the caller's stream (the pass's critical chain: data gradients, sweeps) gets it first
        int prio_lo = 0, prio_hi = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIP_CHECK(hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, BCNN_EXP_ENV("BCNN_HIP_SIDE_PRIO_SAME") ? prio_hi : prio_lo));
        HIP_CHECK(hipEventCreateWithFlags(&ss.ready, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ss.done, hipEventDisableTiming));
    }
    return &ss;
}

// ---- weight packs made ahead of their use (bcnn_hip_conv_prepack) -------------------------------------------------
struct PrepackEntry {
    const float* w;
    int kind, mode;
    float* buf;
    size_t cap, floats;
    unsigned long long epoch;
    bool fresh;
};
struct PrepackStore {
    std::vector<PrepackEntry> entries;
    unsigned long long epoch = 0;
    int dev = -1;
    void* table_dev[PREPACK_KINDS][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    size_t table_cap[PREPACK_KINDS][2] = {{0, 0}, {0, 0}};
    std::vector<char> table_host[PREPACK_KINDS][2];
};
static thread_local PrepackStore g_prepack;

float* prepack_take(const float* w, int kind, int mode, size_t floats) {
    PrepackStore& st = g_prepack;
    for (PrepackEntry& e : st.entries)
        if (e.w == w && e.kind == kind && e.mode == mode && e.fresh && e.epoch == st.epoch && e.floats == floats) {
            e.fresh = false;  // single use: a second call packs the (possibly rewritten) weights itself
            return e.buf;
        }
    return nullptr;
}

static void prepack_free_all(PrepackStore& st) {
    HIP_CHECK(hipDeviceSynchronize());
    for (PrepackEntry& e : st.entries)
        if (e.buf) HIP_CHECK(hipFree(e.buf));
    st.entries.clear();
    for (int k = 0; k < PREPACK_KINDS; ++k)
        for (int m = 0; m < 2; ++m) {
            if (st.table_dev[k][m]) HIP_CHECK(hipFree(st.table_dev[k][m]));
            st.table_dev[k][m] = nullptr;
            st.table_cap[k][m] = 0;
            st.table_host[k][m].clear();
        }
}

static PrepackEntry* prepack_entry(PrepackStore& st, const float* w, int kind, int mode, size_t floats) {
    PrepackEntry* e = nullptr;
    for (PrepackEntry& c : st.entries)
        if (c.w == w && c.kind == kind && c.mode == mode) { e = &c; break; }
    if (!e) {
        st.entries.push_back(PrepackEntry{w, kind, mode, nullptr, 0, 0, 0, false});
        e = &st.entries.back();
    }
    if (e->cap < floats) {
        if (e->buf) {
            HIP_CHECK(hipStreamSynchronize(current_stream()));
            HIP_CHECK(hipFree(e->buf));
        }
        HIP_CHECK(hipMalloc((void**)&e->buf, floats * sizeof(float)));
        e->cap = floats;
    }
    e->floats = floats;
    e->epoch = st.epoch;
    e->fresh = true;
    return e;
}

// the job table of one (kind, mode) on the device; uploaded only when it differs from the one already there
static const void* prepack_table(PrepackStore& st, int kind, int mode, const void* jobs, size_t bytes) {
    std::vector<char>& host = st.table_host[kind][mode];
    if (host.size() == bytes && memcmp(host.data(), jobs, bytes) == 0) return st.table_dev[kind][mode];
    HIP_CHECK(hipStreamSynchronize(current_stream()));  // a launch still reading the old table
    if (st.table_cap[kind][mode] < bytes) {
        if (st.table_dev[kind][mode]) HIP_CHECK(hipFree(st.table_dev[kind][mode]));
        HIP_CHECK(hipMalloc(&st.table_dev[kind][mode], bytes * 2));
        st.table_cap[kind][mode] = bytes * 2;
    }
    HIP_CHECK(hipMemcpy(st.table_dev[kind][mode], jobs, bytes, hipMemcpyHostToDevice));
    host.assign((const char*)jobs, (const char*)jobs + bytes);
    return st.table_dev[kind][mode];
}

// ---- which kernel takes a layer --------------------------------------------------------------------------------------
// The three tables below are the order: a layer runs on the first row whose gate is open, whose shape rule holds and, where
// pointers or buffers can still refuse it, whose `usable` agrees; the last row of each takes every shape. A new family is a
// row here and its declarations in conv_paths.h. (The opt-in bf16 forward, bcnn_hip_conv_forward_bf16, is one family for
// every shape: conv_forward_bf16. A folded batch-norm in front goes straight to the dma kernels: conv_forward_impl.)
// kDwFamilies in the dispatch trace, row by row: conv_dw_rows_kernel, conv_dw_stem_kernel, conv_dw_direct_kernel<1|2>, wino43_dw_kernel,
// wino_dw_fused_kernel, wino_unfused:dw, conv_dw_dma_kernel, conv_small_c:dw, conv_large_dw_kernel, conv_dw_kernel<TM,TN>.
// The forward and data-gradient launchers name their host-chosen sub-branches next to the family: conv_igemm_tile:32x128|64x128|
// 128x128, conv_fwd_window_kernel:tm1|tm2, conv_fwd_direct_kernel:tm1|tm2, wino_fused:halfblocks, conv_dx_classes:<launches>.
// A/B switches of the experiment build that take a family out: BCNN_HIP_NO_WINDOW, BCNN_HIP_NO_DMA, BCNN_HIP_NO_SMALLC_DX
enum ConvGate { GATE_NONE, GATE_WINDOW, GATE_DMA, GATE_SMALLC_DX, GATE_COUNT };
static bool gate_open(ConvGate g) {
    static const bool off[GATE_COUNT] = {false, BCNN_EXP_ENV("BCNN_HIP_NO_WINDOW") != nullptr,
                                         BCNN_EXP_ENV("BCNN_HIP_NO_DMA") != nullptr,
                                         BCNN_EXP_ENV("BCNN_HIP_NO_SMALLC_DX") != nullptr};
    return !off[g];
}
// what bcnn_hip_conv_prepack packs ahead for a layer a family wants (at most one is set): the family's plan function
struct ConvPack {
    bool (*wino)(const ConvShape& s, int dx_mode, WinoPackJob* job, size_t* floats);
    bool (*igemm)(const ConvShape& s, int dx_mode, IgemmPackJob* job, size_t* floats);
};
constexpr ConvPack kNoPack = {nullptr, nullptr};  // the kernel reads w as it is, or transforms it in a kernel of its own
template <class Call>
struct ConvFamily {
    bool (*wanted)(const ConvShape& s, int raw);  // the shape rule (raw: forward only)
    bool (*usable)(const Call& c);                // nullptr: a wanted layer is never refused
    void (*run)(const Call& c);                   // cannot refuse
    ConvPack pack;
    ConvGate gate;
};
static const ConvFamily<ConvFwdCall> kConvFwdFamilies[] = {
    {conv_window_fwd_wanted, nullptr, conv_forward_window, kNoPack, GATE_WINDOW},
    {conv_stem_fwd_wanted, nullptr, conv_forward_stem, kNoPack, GATE_WINDOW},
    {conv_direct_fwd_wanted, nullptr, conv_forward_direct, kNoPack, GATE_NONE},
    {conv_winograd43_fwd_wanted, conv_winograd43_fwd_usable, conv_forward_winograd43, {wino43_pack_plan, nullptr}, GATE_NONE},
    {conv_winograd_fused_fwd_wanted, nullptr, conv_forward_winograd_fused, {wino_fused_pack_plan, nullptr}, GATE_NONE},
    {conv_winograd_fwd_wanted, nullptr, conv_forward_winograd, kNoPack, GATE_NONE},
    {conv_large_wanted, nullptr, conv_forward_large, kNoPack, GATE_NONE},
    {conv_dma_fwd_wanted, nullptr, conv_forward_dma_timed, {nullptr, dma_pack_plan}, GATE_DMA},
    {conv_small_c_fwd_wanted, nullptr, conv_forward_small_c, kNoPack, GATE_DMA},
    {[](const ConvShape&, int) { return true; }, nullptr, conv_forward_igemm, kNoPack, GATE_NONE},
};
static const ConvFamily<ConvDxCall> kConvDxFamilies[] = {
    {conv_winograd43_dx_wanted, conv_winograd43_dx_usable, conv_backward_data_winograd43, {wino43_pack_plan, nullptr}, GATE_NONE},
    {conv_winograd_fused_dx_wanted, nullptr, conv_backward_data_winograd_fused, {wino_fused_pack_plan, nullptr}, GATE_NONE},
    {conv_winograd_dx_wanted, nullptr, conv_backward_data_winograd, kNoPack, GATE_NONE},
    {conv_large_wanted, nullptr, conv_backward_data_large, kNoPack, GATE_NONE},
    {conv_small_c_dx_wanted, nullptr, conv_backward_data_small_c, kNoPack, GATE_SMALLC_DX},
    {conv_dma_dx_wanted, nullptr, conv_backward_data_dma, {nullptr, dma_pack_plan}, GATE_DMA},
    {[](const ConvShape&, int) { return true; }, nullptr, conv_backward_data_igemm, kNoPack, GATE_NONE},
};

template <class Call, size_t R>
static void conv_run_first(const ConvFamily<Call> (&rows)[R], const Call& c, int raw) {
    for (const ConvFamily<Call>& fam : rows)
        if (gate_open(fam.gate) && fam.wanted(c.s, raw) && (!fam.usable || fam.usable(c))) {
            fam.run(c);
            return;
        }
}
// The family bcnn_hip_conv_prepack plans for: the first wanted one in the raw form. The descriptor does not say whether a
// batch-norm follows the layer; a forward layer without one then packs for itself where F(4x4,3x3) was planned, as does
// every layer whose planned family turns out not to be usable.
template <class Call, size_t R>
static ConvPack conv_planned_pack(const ConvFamily<Call> (&rows)[R], const ConvShape& s) {
    for (const ConvFamily<Call>& fam : rows)
        if (gate_open(fam.gate) && fam.wanted(s, /*raw=*/1)) return fam.pack;
    return kNoPack;
}

// bf16: the caller asked for the reduced-precision forward (bcnn_hip_conv_forward_bf16)
static void conv_fwd_any(const ConvFwdCall& c, bool bf16) {
    if (c.stats) c.stats->splits = 0;
    if (c.s.total_q <= 0 || c.s.Mg == 0) return;
    if (bf16) conv_forward_bf16(c.x, c.w, c.bias, c.slopes, c.y, c.s, c.act, c.raw, c.stats);
    else conv_run_first(kConvFwdFamilies, c, c.raw);
}

static void conv_dx_any(const float* w, const float* dy, float* dx, const ConvShape& s, DxBnSums* bs) {
    if (bs) bs->splits = 0;
    if (s.total_p == 0 || s.Cg == 0) return;
    conv_run_first(kConvDxFamilies, ConvDxCall{w, dy, dx, s, bs}, 0);
}

struct DwFamily {
    size_t (*workspace_floats)(const ConvShape& s);  // of split partials in the caller's workspace; 0: not its shape
    bool (*run)(const float* x, const float* dy, float* dw, float* dbias, const ConvShape& s, float* workspace,
                size_t workspace_floats, bool* bias_done);
    ConvGate gate;
};
static const DwFamily kDwFamilies[] = {
    {conv_dw_window_workspace_floats, conv_backward_weights_window, GATE_WINDOW},
    {conv_dw_stem_workspace_floats, conv_backward_weights_stem, GATE_WINDOW},
    {conv_dw_direct_workspace_floats, conv_backward_weights_direct, GATE_NONE},
    {conv_dw_winograd43_workspace_floats, conv_backward_weights_winograd43, GATE_NONE},
    {conv_dw_winograd_fused_workspace_floats, conv_backward_weights_winograd_fused, GATE_NONE},
    {conv_dw_winograd_workspace_floats, conv_backward_weights_winograd, GATE_NONE},
    {conv_dw_dma_workspace_floats, conv_backward_weights_dma_timed, GATE_DMA},
    {conv_dw_small_c_workspace_floats, conv_backward_weights_small_c, GATE_DMA},
    {conv_dw_large_workspace_floats, conv_backward_weights_large, GATE_NONE},
    {conv_dw_workspace_floats, conv_backward_weights, GATE_NONE},  // takes every shape
};

// ---- the convolution node: convolution [+ batch-norm] + activation, with the fusions a caller can ask for ------------------
// One description per direction. The entry points of the ABI (below) fill it by name, what is absent stays zero. The two pieces
// of per-thread state that gate a fusion are read there, once per call, and travel in it: `fold` (take_fold) and `side_mode`.
// p.bias / g.dbias are the node's: the convolution's own without batch_norm. bn_workspace: the pre-normalisation values.
// res != NULL (batch_norm, TRAIN mode, cheap activations -- bcnn_hip_conv_residual_fusable): the following eltwise node
// is folded into the batch-norm apply pass, whose result goes to res_out; y is not written
// stats_only: stop behind the batch statistics; bf16: the convolution itself on the bf16 matrix cores (conv_bf16.hip)
struct ConvNodeFwd {
    const float *x, *w, *slopes;
    float *y, *saved_mean, *saved_var, *bn_workspace, *res_out;
    ConvShape s;
    int act, batch_norm, mode;
    BnParams p;
    BnRunning run;
    const BnResidual* res;
    bool stats_only, bf16;
    BnFold fold;  // announced by bcnn_hip_conv_set_input_bnfold: x then is the batch-norm's INPUT
};
struct ConvResidualBwd {
    const float* out;   // the folded eltwise node's output
    const float* dout;  // and its gradient (read only)
    const float* res;   // the eltwise node's second operand
    float* dres;        // and its gradient (accumulated), may be NULL
    size_t res_count;
    int act;
};
// workspace: split partials of the weight gradient (bcnn_hip_conv_workspace_size floats). rb: the eltwise node folded into the
// forward pass; bs: the data-gradient kernel also emits the sums of the batch-norm node in front; own_sums: whoever wrote dy
// left this node's batch-norm sums, own_splits per channel; bn_done: dy already is the gradient of the pre-normalisation output
struct ConvNodeBwd {
    const float *x, *w, *y, *slopes, *bn_workspace, *own_sums;
    float *dy, *dx, *dw, *dslopes, *workspace;
    size_t workspace_elems;
    ConvShape s;
    int act, batch_norm, own_splits, side_mode;  // side_mode: g_side_mode's values
    BnParams p;  // p.bias lets the batch-norm backward recompute the forward output from bn_workspace (no read of y)
    BnSaved saved;
    BnGrads g;
    const ConvResidualBwd* rb;
    DxBnSums* bs;
    bool bn_done;
    BnFold fold;  // x then is the INPUT of the batch-norm in front: d/dW of W diag(a) is (dy x^T) diag(a)
};

static void conv_forward_impl(const ConvNodeFwd& nd) {
    const ConvShape& s = nd.s;
    const BnFold& fold = nd.fold;
    const int n = s.N, f = s.F, act = nd.act, mode = nd.mode;
    if (fold.mean && (!nd.batch_norm || mode != BCNN_HIP_MODE_TRAIN || !bnfold_shape_ok(s))) {
        fprintf(stderr, "[bcnn_hip] conv forward: a batch-norm fold was announced for a layer that cannot take it (ask "
                        "bcnn_hip_conv_bnfold_fusable)\n");
        exit(1);
    }
    if (!nd.batch_norm) {
        // tanh / softplus / logistic: bias in the epilogue, activation as a second in-place pass
        const int fused_act = act_is_cheap(act) ? act : BCNN_HIP_ACT_NONE;
        conv_fwd_any(ConvFwdCall{nd.x, nd.w, nd.p.bias, nd.slopes, nd.y, s, fused_act, /*raw=*/0, nullptr}, nd.bf16);
        if (fused_act != act) bcnn_hip_activation_forward(nd.y, (size_t)n * f * s.OHOW, act, nd.slopes, s.OHOW, f);
        return;
    }
    // conv -> (pre-normalisation values, kept for backward) -> statistics -> normalise+scale+bias+act
    float* raw = (nd.bn_workspace && mode != BCNN_HIP_MODE_PREDICT) ? nd.bn_workspace : nd.y;
    // TRAIN: the convolution epilogue also emits the per-channel sum / sum of squares of what it stores
    ConvStats st;
    st.partials = nullptr; st.splits = 0; st.capacity = 0;
    static const int fuse_stats = BCNN_EXP_ENV("BCNN_HIP_NO_FUSED_STATS") ? 0 : 1;  // A/B switch for profiling
    if (fuse_stats && mode == BCNN_HIP_MODE_TRAIN && s.total_q < 0x7fffffffLL) {
        // slots per channel: one per 64 output pixels on the GEMM paths; the fused Winograd kernel writes two per block
        // of 64 2x2 tiles, which is MORE than that when a tile covers fewer than two real pixels (H == 1 or W == 1)
        const long long tiles = (long long)n * ((s.OH + 1) / 2) * ((s.OW + 1) / 2);
        const long long slots_gemm = ceil_div(s.total_q, 64), slots_wino = 2 * ceil_div(tiles, 64);
        st.capacity = (size_t)f * (size_t)(slots_gemm > slots_wino ? slots_gemm : slots_wino) * 2;
        st.partials = scratch(SCRATCH_REDUCE, st.capacity);
    }
    BnFwdCall b{};
    b.x = raw; b.y = nd.res ? nd.res_out : nd.y; b.workspace = raw; b.e.n = n; b.e.c = f; b.e.hw = s.OHOW; b.mode = mode;
    b.act = (act == BCNN_HIP_ACT_PRELU) ? BCNN_HIP_ACT_NONE : act; b.pre = &st; b.res = nd.res; b.stats_only = nd.stats_only;
    b.p = nd.p; b.saved_mean = nd.saved_mean; b.saved_var = nd.saved_var; b.run = nd.run;
    ConvStats* stp = st.partials ? &st : nullptr;
    if (fold.mean) {
        // W z = (W diag(a)) y + W b: the GEMM reads y with column-scaled weights (packed here: a depends on this batch). The
        // constant W b is left out of the stored pre-normalisation values -- the batch-norm behind subtracts the batch mean,
        // so every later use (apply, backward, the consumers that normalise on the fly) sees raw - mean either way -- and
        // is added where it is visible: the running mean.
        trace_kernel("bnfold:fwd");
        b.mean_shift = fold_rowconst(fold, nd.w, s.C, f);
        KTimer kt(K_CONV_FWD, conv_gemm_flops(s), conv_gemm_bytes(s));
        if (!conv_forward_dma(nd.x, nd.w, nullptr, nullptr, raw, s, BCNN_HIP_ACT_NONE, /*raw=*/1, stp, &fold)) {
            fprintf(stderr, "[bcnn_hip] conv forward: the LDS-DMA GEMM refused a folded layer\n");
            exit(1);
        }
    } else {
        conv_fwd_any(ConvFwdCall{nd.x, nd.w, nullptr, nullptr, raw, s, BCNN_HIP_ACT_NONE, /*raw=*/1, stp}, nd.bf16);
    }
    batchnorm_forward_impl(b);
    if (nd.stats_only) return;
    if (act == BCNN_HIP_ACT_PRELU) bcnn_hip_activation_forward(nd.y, (size_t)n * f * s.OHOW, act, nd.slopes, s.OHOW, f);
}

static void conv_backward_impl(const ConvNodeBwd& nd) {
    const ConvShape& s = nd.s;
    const BnFold& fold = nd.fold;
    const int n = s.N, f = s.F, act = nd.act, batch_norm = nd.batch_norm;
    const size_t ysize = (size_t)n * f * s.OHOW;
    if (fold.mean && (!batch_norm || !bnfold_shape_ok(s))) {
        fprintf(stderr, "[bcnn_hip] conv backward: a batch-norm fold was announced for a layer that cannot take it\n");
        exit(1);
    }
    BnBwdCall b{};
    b.dy = nd.dy; b.y = nd.y; b.workspace = nd.bn_workspace; b.act = act; b.p = nd.p; b.s = nd.saved; b.g = nd.g;
    b.e.n = n; b.e.c = f; b.e.hw = s.OHOW;
    if (nd.rb) {
        // dy <- batch-norm backward of dout * act'(out): the eltwise node's backward and this node's batch-norm backward
        // in the two sweeps the latter takes alone
        b.dy = nullptr; b.dout = nd.rb->dout; b.dx = nd.dy; b.y = nd.rb->out; b.act = nd.rb->act;
        b.res = nd.rb->res; b.dres = nd.rb->dres; b.res_count = nd.rb->res_count;
        batchnorm_backward_impl(b);
    } else if (batch_norm && nd.bn_done) {
        // dy already is the gradient of the pre-normalisation output (bcnn_hip_maxpool_bn_backward wrote it)
    } else if (batch_norm) {
        if (act == BCNN_HIP_ACT_PRELU) {
            bcnn_hip_activation_backward(nd.y, nd.dy, ysize, act, nd.slopes, nd.dslopes, s.OHOW, f);
            b.act = BCNN_HIP_ACT_NONE;
        }
        if (nd.own_sums && nd.own_splits > 0 && b.act == act && act_bwd_is_cheap(act)) {  // whoever wrote dy left the sums
            b.sums = nd.own_sums; b.splits = nd.own_splits;
        }
        batchnorm_backward_impl(b);
    } else {
        bcnn_hip_activation_backward(nd.y, nd.dy, ysize, act, nd.slopes, nd.dslopes, s.OHOW, f);
    }
    // dW and dX only share their input dy, so the weight gradient CAN run on a private side stream to fill the
    // CUs the other kernel leaves idle in its last round (the side stream joins the caller's stream before
    // this function returns). Measured on ResNet-18 N=128 it is 1.7 % SLOWER than running them back to back
    // (18.15 vs 17.86 ms/step): both GEMMs are MFMA-bound and evict each other's L2 working set. Kept as an
    // opt-in experiment (BCNN_HIP_SIDE_STREAM=1), off by default.
    // deferred mode: EVERY weight gradient (the per-net workspace of split partials then belongs to the side stream alone)
    SideStream* side = (nd.side_mode == 2 || (nd.side_mode == 1 && nd.dx)) ? side_stream() : nullptr;
    hipStream_t main_stream = current_stream();
    if (side) {
        HIP_CHECK(hipEventRecord(side->ready, main_stream));
        HIP_CHECK(hipStreamWaitEvent(side->stream, side->ready, 0));
        set_current_stream(side->stream);
    }
    bool bias_done = false;
    if (fold.mean) {
        // (the term b (x) sum_q dy of the exact derivative is left out: dy here is the gradient of a batch-norm's input, whose
        // sum over the batch is zero up to rounding -- in the reference too, where it multiplies the same b)
        trace_kernel("bnfold:dw");
        KTimer kt(K_CONV_DW, conv_gemm_flops(s), conv_gemm_bytes(s));
        if (!conv_backward_weights_dma(nd.x, nd.dy, nd.dw, s, nd.workspace, nd.workspace_elems, &fold)) {
            fprintf(stderr, "[bcnn_hip] conv backward: the LDS-DMA weight-gradient kernel refused a folded layer\n");
            exit(1);
        }
    } else {
        for (const DwFamily& fam : kDwFamilies)
            if (gate_open(fam.gate) && fam.run(nd.x, nd.dy, nd.dw, batch_norm ? nullptr : nd.g.dbias, s, nd.workspace,
                                               nd.workspace_elems, &bias_done))
                break;
    }
    if (side) {
        HIP_CHECK(hipEventRecord(side->done, side->stream));
        set_current_stream(main_stream);
    }
    if (!batch_norm && !bias_done) bcnn_hip_grad_bias(nd.g.dbias, nd.dy, n, f, s.OHOW);  // uses the shared reduce scratch
    if (nd.dx) conv_dx_any(nd.w, nd.dy, nd.dx, s, nd.bs);
    else if (nd.bs) nd.bs->splits = 0;
    if (side) {
        if (nd.side_mode == 2) side->pending = true;
        else HIP_CHECK(hipStreamWaitEvent(main_stream, side->done, 0));
    }
}
// the weight gradients' stream mode of a call: the calling thread's, or the experiment build's BCNN_HIP_SIDE_STREAM=1
static int side_mode_now() {
    static const int side_env = BCNN_EXP_ENV("BCNN_HIP_SIDE_STREAM") ? 1 : 0;
    return g_side_mode ? g_side_mode : side_env;
}
}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

void bcnn_hip_conv_prepack(const bcnn_hip_conv_desc* layers, int count, int data_gradient) {
    PrepackStore& st = g_prepack;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (st.dev != dev) {  // buffers of another device are left to that device's thread / context
        if (st.dev >= 0) prepack_free_all(st);
        st.dev = dev;
    }
    ++st.epoch;  // every copy made earlier and not used is stale now
    (void)take_fold();  // a pass begins: a fold announced earlier and never consumed must not meet this pass's first convolution
    const int mode = data_gradient ? 1 : 0;
    std::vector<WinoPackJob> wj;
    std::vector<IgemmPackJob> ij;
    int wmax = 0, imax = 0;
    for (int i = 0; i < count; ++i) {
        const bcnn_hip_conv_desc& d = layers[i];
        if (!d.w_d || d.groups <= 0 || d.n <= 0) continue;
        const ConvShape s = make_conv_shape(d.n, d.c, d.h, d.w, d.f, d.k, d.stride, d.pad, d.groups);
        if (s.total_q <= 0 || s.Mg == 0 || s.Cg == 0) continue;
        const ConvPack pack = mode ? conv_planned_pack(kConvDxFamilies, s) : conv_planned_pack(kConvFwdFamilies, s);
        WinoPackJob w1;
        IgemmPackJob i1;
        memset(&w1, 0, sizeof(w1));  // padding bytes too: the tables are compared bytewise against the uploaded ones
        memset(&i1, 0, sizeof(i1));
        size_t floats = 0;
        if (pack.wino && pack.wino(s, mode, &w1, &floats)) {
            PrepackEntry* e = prepack_entry(st, d.w_d, PREPACK_WINO, mode, floats);
            w1.w = d.w_d; w1.u = e->buf;
            if (w1.blocks > wmax) wmax = w1.blocks;
            wj.push_back(w1);
        }
        if (pack.igemm && pack.igemm(s, mode, &i1, &floats)) {
            PrepackEntry* e = prepack_entry(st, d.w_d, PREPACK_IGEMM, mode, floats);
            i1.w = d.w_d; i1.at = e->buf;
            const int blocks = i1.gx * i1.gy * i1.gz;
            if (blocks > imax) imax = blocks;
            ij.push_back(i1);
        }
    }
    if (!wj.empty()) {
        const void* t = prepack_table(st, PREPACK_WINO, mode, wj.data(), wj.size() * sizeof(WinoPackJob));
        wino_fused_pack_launch((const WinoPackJob*)t, (int)wj.size(), wmax);
    }
    if (!ij.empty()) {
        const void* t = prepack_table(st, PREPACK_IGEMM, mode, ij.data(), ij.size() * sizeof(IgemmPackJob));
        dma_pack_launch((const IgemmPackJob*)t, (int)ij.size(), imax);
    }
}

void bcnn_hip_conv_prepack_discard(void) { ++g_prepack.epoch; }

void bcnn_hip_conv_prepack_reset(void) {
    PrepackStore& st = g_prepack;
    if (st.dev < 0) return;
    prepack_free_all(st);
    ++st.epoch;
}

size_t bcnn_hip_conv_workspace_size(int n, int c, int h, int w, int f, int k, int stride, int pad, int groups) {
    const ConvShape s = make_conv_shape(n, c, h, w, f, k, stride, pad, groups);
    size_t m = 0;
    for (const DwFamily& fam : kDwFamilies) m = std::max(m, fam.workspace_floats(s));
    return m;
}

int bcnn_hip_conv_bnfold_fusable(int n, int c, int h, int wd, int f) {
    if (n <= 0 || c <= 0 || h <= 0 || wd <= 0 || f <= 0) return 0;
    return bnfold_shape_ok(make_conv_shape(n, c, h, wd, f, 1, 1, 0, 1)) ? 1 : 0;
}

void bcnn_hip_conv_set_input_bnfold(const float* mean, const float* var, const float* scales, const float* bias) {
    g_fold_pending = BnFold{mean, var, scales, bias};
}

// (x_norm, here and in the backward entry points, is not materialised: the backward pass recomputes it from the raw convolution
// output kept in bn_workspace -- a full-tensor write and read less per layer and step)
void bcnn_hip_conv_forward(const float* x, const float* w, const float* bias, float* y, int n, int c, int h,
                           int wd, int f, int k, int stride, int pad, int groups, int act, const float* slopes,
                           int batch_norm, float* run_mean, float* run_var, const float* scales,
                           float* saved_mean, float* saved_var, float* x_norm, float* bn_workspace, int mode) {
    ConvNodeFwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold();
    nd.x = x; nd.w = w; nd.y = y; nd.act = act; nd.slopes = slopes; nd.batch_norm = batch_norm; nd.mode = mode;
    nd.p.scales = scales; nd.p.bias = bias; nd.saved_mean = saved_mean; nd.saved_var = saved_var;
    nd.run.run_mean = run_mean; nd.run.run_var = run_var; nd.bn_workspace = bn_workspace;
    conv_forward_impl(nd);
}

// bcnn_hip_conv_forward with the convolution itself on the bf16 matrix cores (conv_bf16.hip); everything behind the
// accumulator -- bias, fused batch-norm apply, activation passes -- is conv_forward_impl's own code. Inference only.
int bcnn_hip_conv_forward_bf16(const float* x, const float* w, const float* bias, float* y, int n, int c, int h,
                               int wd, int f, int k, int stride, int pad, int groups, int act, const float* slopes,
                               int batch_norm, float* run_mean, float* run_var, const float* scales,
                               float* saved_mean, float* saved_var, float* x_norm, float* bn_workspace, int mode) {
    if (mode != BCNN_HIP_MODE_PREDICT && mode != BCNN_HIP_MODE_VALID) return 0;
    ConvNodeFwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.bf16 = true;
    nd.x = x; nd.w = w; nd.y = y; nd.act = act; nd.slopes = slopes; nd.batch_norm = batch_norm; nd.mode = mode;
    nd.p.scales = scales; nd.p.bias = bias; nd.saved_mean = saved_mean; nd.saved_var = saved_var;
    nd.run.run_mean = run_mean; nd.run.run_var = run_var; nd.bn_workspace = bn_workspace;
    conv_forward_impl(nd);
    return 1;
}

// The convolution and the batch statistics (saved / running) of bcnn_hip_conv_forward, TRAIN mode, WITHOUT the apply sweep:
// the pre-normalisation values stay in bn_workspace and the consumer normalises them on the fly
void bcnn_hip_conv_forward_stats_only(const float* x, const float* w, const float* bias, int n, int c, int h, int wd, int f,
                                      int k, int stride, int pad, int groups, float* run_mean, float* run_var,
                                      const float* scales, float* saved_mean, float* saved_var, float* bn_workspace) {
    ConvNodeFwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.stats_only = true;
    nd.x = x; nd.w = w; nd.act = BCNN_HIP_ACT_NONE; nd.batch_norm = 1; nd.mode = BCNN_HIP_MODE_TRAIN;
    nd.p.scales = scales; nd.p.bias = bias; nd.saved_mean = saved_mean; nd.saved_var = saved_var;
    nd.run.run_mean = run_mean; nd.run.run_var = run_var; nd.bn_workspace = bn_workspace;
    conv_forward_impl(nd);
}

int bcnn_hip_conv_residual_fusable(int batch_norm, int act, int res_act, int mode, const float* bn_workspace,
                                   const float* res, const float* res_out) {
    return batch_norm && mode == BCNN_HIP_MODE_TRAIN && bn_workspace && act == BCNN_HIP_ACT_NONE && act_is_cheap(res_act) &&
           act_bwd_is_cheap(res_act) && res_act != BCNN_HIP_ACT_PRELU && al16(res) && al16(res_out) && al16(bn_workspace);
}

void bcnn_hip_conv_forward_residual(const float* x, const float* w, const float* bias, int n, int c, int h, int wd, int f,
                                    int k, int stride, int pad, int groups, float* run_mean, float* run_var,
                                    const float* scales, float* saved_mean, float* saved_var, float* bn_workspace,
                                    const float* res, size_t res_count, int res_act, float* res_out) {
    BnResidual r{res, res_count, res_act};
    ConvNodeFwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.res = &r; nd.res_out = res_out;
    nd.x = x; nd.w = w; nd.act = BCNN_HIP_ACT_NONE; nd.batch_norm = 1; nd.mode = BCNN_HIP_MODE_TRAIN;
    nd.p.scales = scales; nd.p.bias = bias; nd.saved_mean = saved_mean; nd.saved_var = saved_var;
    nd.run.run_mean = run_mean; nd.run.run_var = run_var; nd.bn_workspace = bn_workspace;
    conv_forward_impl(nd);
}

int bcnn_hip_conv_side_stream_mode(int mode) {
    const int prev = g_side_mode;
    if (mode >= 0 && mode <= 2) g_side_mode = mode;
    return prev;
}

void bcnn_hip_conv_side_join(void) {
    SideStream& ss = g_side[current_device()];  // no side stream on this device yet: nothing pending
    if (!ss.pending) return;
    ss.pending = false;
    HIP_CHECK(hipStreamWaitEvent(current_stream(), ss.done, 0));  // `done` was recorded behind the last weight-gradient launch
}

size_t bcnn_hip_conv_bnsums_size(int n, int c, int h, int wd) {
    return (size_t)c * (size_t)ceil_div((long long)n * h * wd, 64) * 2;
}

// bcnn_hip_conv_backward; own_sums: this node's batch-norm sums where whoever wrote dy left them; prev_*: the sums of the
// batch-norm node in front, emitted by the data-gradient kernel (returns the partials per channel written, 0: none)
int bcnn_hip_conv_backward_presummed(const float* x, const float* w, const float* bias, const float* y, float* dy, float* dx,
                                     float* dw, float* dbias, int n, int c, int h, int wd, int f, int k, int stride, int pad,
                                     int groups, int act, const float* slopes, float* dslopes, int batch_norm,
                                     const float* scales, float* dscales, const float* saved_mean, const float* saved_var,
                                     float* dmean, float* dvar, const float* x_norm, const float* bn_workspace,
                                     float* workspace, size_t workspace_elems, const float* own_sums, int own_splits,
                                     const float* prev_y, const float* prev_mean, float* prev_sums, size_t prev_sums_floats) {
    DxBnSums bs{prev_y, prev_mean, prev_sums, prev_sums_floats, 0};
    ConvNodeBwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.side_mode = side_mode_now();
    nd.x = x; nd.w = w; nd.y = y; nd.dy = dy; nd.dx = dx; nd.dw = dw; nd.act = act; nd.slopes = slopes; nd.dslopes = dslopes;
    nd.batch_norm = batch_norm; nd.p.scales = scales; nd.p.bias = bias; nd.saved.mean = saved_mean; nd.saved.var = saved_var;
    nd.g.dscales = dscales; nd.g.dbias = dbias; nd.g.dmean = dmean; nd.g.dvar = dvar; nd.bn_workspace = bn_workspace;
    nd.workspace = workspace; nd.workspace_elems = workspace_elems; nd.own_sums = own_sums; nd.own_splits = own_splits;
    if (prev_sums && prev_y && prev_mean) nd.bs = &bs;
    conv_backward_impl(nd);
    return bs.splits;
}

int bcnn_hip_conv_backward_bnsums(const float* x, const float* w, const float* bias, const float* y, float* dy, float* dx,
                                  float* dw, float* dbias, int n, int c, int h, int wd, int f, int k, int stride, int pad,
                                  int groups, int act, const float* slopes, float* dslopes, int batch_norm,
                                  const float* scales, float* dscales, const float* saved_mean, const float* saved_var,
                                  float* dmean, float* dvar, const float* x_norm, const float* bn_workspace,
                                  float* workspace, size_t workspace_elems, const float* prev_y, const float* prev_mean,
                                  float* sums, size_t sums_floats) {
    DxBnSums bs{prev_y, prev_mean, sums, sums_floats, 0};
    ConvNodeBwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.side_mode = side_mode_now();
    nd.x = x; nd.w = w; nd.y = y; nd.dy = dy; nd.dx = dx; nd.dw = dw; nd.act = act; nd.slopes = slopes; nd.dslopes = dslopes;
    nd.batch_norm = batch_norm; nd.p.scales = scales; nd.p.bias = bias; nd.saved.mean = saved_mean; nd.saved.var = saved_var;
    nd.g.dscales = dscales; nd.g.dbias = dbias; nd.g.dmean = dmean; nd.g.dvar = dvar; nd.bn_workspace = bn_workspace;
    nd.workspace = workspace; nd.workspace_elems = workspace_elems;
    if (sums && prev_y && prev_mean) nd.bs = &bs;
    conv_backward_impl(nd);
    return bs.splits;
}

void bcnn_hip_conv_backward(const float* x, const float* w, const float* bias, const float* y, float* dy, float* dx,
                            float* dw, float* dbias, int n, int c, int h, int wd, int f, int k, int stride, int pad,
                            int groups, int act, const float* slopes, float* dslopes, int batch_norm,
                            const float* scales, float* dscales, const float* saved_mean,
                            const float* saved_var, float* dmean, float* dvar, const float* x_norm,
                            const float* bn_workspace, float* workspace, size_t workspace_elems) {
    ConvNodeBwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.side_mode = side_mode_now();
    nd.x = x; nd.w = w; nd.y = y; nd.dy = dy; nd.dx = dx; nd.dw = dw; nd.act = act; nd.slopes = slopes; nd.dslopes = dslopes;
    nd.batch_norm = batch_norm; nd.p.scales = scales; nd.p.bias = bias; nd.saved.mean = saved_mean; nd.saved.var = saved_var;
    nd.g.dscales = dscales; nd.g.dbias = dbias; nd.g.dmean = dmean; nd.g.dvar = dvar; nd.bn_workspace = bn_workspace;
    nd.workspace = workspace; nd.workspace_elems = workspace_elems;
    conv_backward_impl(nd);
}

void bcnn_hip_conv_backward_bn_done(const float* x, const float* w, float* dy, float* dx, float* dw, int n, int c, int h, int wd,
                                    int f, int k, int stride, int pad, int groups, float* workspace, size_t workspace_elems) {
    ConvNodeBwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.side_mode = side_mode_now();
    nd.x = x; nd.w = w; nd.dy = dy; nd.dx = dx; nd.dw = dw; nd.act = BCNN_HIP_ACT_NONE; nd.batch_norm = 1; nd.bn_done = true;
    nd.workspace = workspace; nd.workspace_elems = workspace_elems;
    conv_backward_impl(nd);
}

void bcnn_hip_conv_backward_residual(const float* x, const float* w, const float* bias, float* dy, float* dx, float* dw,
                                     float* dbias, int n, int c, int h, int wd, int f, int k, int stride, int pad,
                                     int groups, const float* scales, float* dscales, const float* saved_mean,
                                     const float* saved_var, float* dmean, float* dvar, const float* bn_workspace,
                                     float* workspace, size_t workspace_elems, const float* res_out,
                                     const float* dres_out, int res_act, const float* res, float* dres, size_t res_count) {
    ConvResidualBwd rb{res_out, dres_out, res, dres, res_count, res_act};
    ConvNodeBwd nd{};
    nd.s = make_conv_shape(n, c, h, wd, f, k, stride, pad, groups); nd.fold = take_fold(); nd.side_mode = side_mode_now();
    nd.x = x; nd.w = w; nd.dy = dy; nd.dx = dx; nd.dw = dw; nd.act = BCNN_HIP_ACT_NONE; nd.batch_norm = 1; nd.rb = &rb;
    nd.p.scales = scales; nd.p.bias = bias; nd.saved.mean = saved_mean; nd.saved.var = saved_var;
    nd.g.dscales = dscales; nd.g.dbias = dbias; nd.g.dmean = dmean; nd.g.dvar = dvar; nd.bn_workspace = bn_workspace;
    nd.workspace = workspace; nd.workspace_elems = workspace_elems;
    conv_backward_impl(nd);
}

}  // extern "C"
