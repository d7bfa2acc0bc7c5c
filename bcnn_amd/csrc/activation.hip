// activation.hip -- the activation map, stand-alone entry points (HBM-bound streaming kernels).
// Reference semantics: bcnn_forward_activation_cpu / bcnn_backward_activation_cpu,
// src/layers/bcnn_activation_layer.c:90-146, 165-226. Inside conv / depthwise / batch-norm nodes the
// same act_fwd / act_bwd_factor functions run fused in the producing kernel's epilogue instead.
#include "chan_reduce.h"

namespace bcnn_hip {

struct ActFwdBody {
    float* x;
    const float* slopes;
    int act;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float sl = (act == BCNN_HIP_ACT_PRELU) ? slopes[c] : 0.f;
        if (cnt == 4 && al && (off & 3u) == 0) {
            float4 v = *reinterpret_cast<float4*>(x + off);
            v.x = act_fwd(v.x, act, sl); v.y = act_fwd(v.y, act, sl);
            v.z = act_fwd(v.z, act, sl); v.w = act_fwd(v.w, act, sl);
            *reinterpret_cast<float4*>(x + off) = v;
        } else {
            for (int k = 0; k < cnt; ++k) x[off + k] = act_fwd(x[off + k], act, sl);
        }
    }
};

struct ActBwdBody {
    const float* x;
    float* dx;
    const float* slopes;
    int act;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float sl = (act == BCNN_HIP_ACT_PRELU) ? slopes[c] : 0.f;
        if (cnt == 4 && al && (off & 3u) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(x + off);
            float4 g = *reinterpret_cast<float4*>(dx + off);
            g.x *= act_bwd_factor(v.x, act, sl); g.y *= act_bwd_factor(v.y, act, sl);
            g.z *= act_bwd_factor(v.z, act, sl); g.w *= act_bwd_factor(v.w, act, sl);
            *reinterpret_cast<float4*>(dx + off) = g;
        } else {
            for (int k = 0; k < cnt; ++k) dx[off + k] *= act_bwd_factor(x[off + k], act, sl);
        }
    }
};

// PReLU slope gradient: dslope[c] += sum dx*x*(x<0), taken BEFORE dx is rescaled (:213-216)
struct PreluGradF {
    static constexpr int kInFlight = 4;  // chan_reduce_partial's unroll
    const float* x;
    const float* dx;
    __device__ void operator()(long long off, int, float (&acc)[1]) const {
        const float v = x[off];
        acc[0] += dx[off] * v * (float)(v < 0);
    }
    __device__ void vec4(long long off, int c, float (&acc)[1]) const {
        for (int k = 0; k < 4; ++k) (*this)(off + k, c, acc);
    }
};

__global__ void accumulate_kernel(const float* __restrict__ partials, int C, int splits, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int i = 0; i < splits; ++i) s += (double)partials[(long long)c * splits + i];
    out[c] += (float)s;
}

// ---- the self-gated activations: hard-swish, swish, mish (no reference counterpart) --------------------------------------------
// Their derivative is a function of the INPUT, which an in-place node no longer has after its forward: the forward keeps a
// copy (12 bytes per element instead of 8), the backward reads it (12 bytes). hard-swish is float arithmetic written as
// torch writes it; swish and mish evaluate exp in double like LOGISTIC above and round once at the end.
__device__ __forceinline__ float gated_fwd(float x, int act) {
    if (act == BCNN_HIP_ACT_HARD_SWISH) return (x * fminf(fmaxf(x + 3.f, 0.f), 6.f)) / 6.0f;
    const double xd = (double)x;
    if (act == BCNN_HIP_ACT_SWISH) return (float)(xd / (1.0 + exp(-xd)));
    // mish: tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2), n = e (e + 2); 1 past where e^2 overflows
    const double e = exp(xd), n = e * (e + 2.0);
    return (float)(xd > 300.0 ? xd : xd * (n / (n + 2.0)));
}
// g * f'(x). hard-swish: a float factor and one float multiply, as torch writes it; swish and mish: the product is formed
// in double too, so the result carries one rounding
__device__ __forceinline__ float gated_bwd(float g, float x, int act) {
    if (act == BCNN_HIP_ACT_HARD_SWISH) return g * (x < -3.f ? 0.f : (x <= 3.f ? x / 3.0f + 0.5f : 1.f));  // torch's kinks
    const double xd = (double)x, gd = (double)g;
    if (act == BCNN_HIP_ACT_SWISH) {
        const double s = 1.0 / (1.0 + exp(-xd));
        return (float)(gd * (s * (1.0 + xd * (1.0 - s))));
    }
    // mish' = t + x s (1 - t^2), t = n / (n + 2), s = e / (1 + e); 1 - t = 2 / (n + 2) without cancellation
    if (xd > 300.0) return g;
    const double e = exp(xd), n = e * (e + 2.0), t = n / (n + 2.0), s = e / (1.0 + e);
    return (float)(gd * (t + xd * s * ((2.0 / (n + 2.0)) * (1.0 + t))));
}
// class-A and reference activations through the same sweep (forward_keep accepts every id but PRELU)
__device__ __forceinline__ float keep_fwd(float x, int act) { return act_needs_input(act) ? gated_fwd(x, act) : act_fwd(x, act, 0.f); }

// One float4 per thread and step over the first size / 4 groups (16-byte accesses when every base is 16-byte aligned,
// four scalar accesses otherwise), then the size % 4 tail, one element per thread of the first workgroup.
__global__ __launch_bounds__(256) void gated_fwd_kernel(float* __restrict__ x, float* __restrict__ saved, size_t size, int act,
                                                        int al) {
    const size_t groups = size / 4, stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += stride) {
        if (al) {
            float4 v = *reinterpret_cast<const float4*>(x + 4 * q);
            if (saved) *reinterpret_cast<float4*>(saved + 4 * q) = v;
            v.x = keep_fwd(v.x, act); v.y = keep_fwd(v.y, act); v.z = keep_fwd(v.z, act); v.w = keep_fwd(v.w, act);
            *reinterpret_cast<float4*>(x + 4 * q) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = x[4 * q + k];
                if (saved) saved[4 * q + k] = v;
                x[4 * q + k] = keep_fwd(v, act);
            }
        }
    }
    const size_t t = groups * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < size) {
        const float v = x[t];
        if (saved) saved[t] = v;
        x[t] = keep_fwd(v, act);
    }
}
__global__ __launch_bounds__(256) void gated_bwd_kernel(const float* __restrict__ saved, float* __restrict__ dx, size_t size,
                                                        int act, int al) {
    const size_t groups = size / 4, stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += stride) {
        if (al) {
            const float4 v = *reinterpret_cast<const float4*>(saved + 4 * q);
            float4 g = *reinterpret_cast<const float4*>(dx + 4 * q);
            g.x = gated_bwd(g.x, v.x, act); g.y = gated_bwd(g.y, v.y, act);
            g.z = gated_bwd(g.z, v.z, act); g.w = gated_bwd(g.w, v.w, act);
            *reinterpret_cast<float4*>(dx + 4 * q) = g;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) dx[4 * q + k] = gated_bwd(dx[4 * q + k], saved[4 * q + k], act);
        }
    }
    const size_t t = groups * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < size) dx[t] = gated_bwd(dx[t], saved[t], act);
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

void bcnn_hip_activation_forward(float* x, size_t size, int act, const float* slopes, int spatial,
                                 int channels) {
    if (!size || act == BCNN_HIP_ACT_NONE) return;
    if (act_needs_input(act)) {  // the forward needs no saved input
        bcnn_hip_activation_forward_keep(x, nullptr, size, act);
        return;
    }
    const bool al = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    if (act != BCNN_HIP_ACT_PRELU) {  // no channel dependence: treat as one long plane
        launch_chan_map(ActFwdBody{x, nullptr, act, al}, 1, 1, (int)size);
        return;
    }
    const int n = (int)(size / ((size_t)spatial * channels));
    launch_chan_map(ActFwdBody{x, slopes, act, al}, n, channels, spatial);
}

void bcnn_hip_activation_backward(const float* x, float* dx, size_t size, int act, const float* slopes,
                                  float* dslopes, int spatial, int channels) {
    if (!size || act == BCNN_HIP_ACT_NONE) return;
    if (act_needs_input(act)) {  // x here is the OUTPUT: not enough for these three, and never a silent wrong gradient
        fprintf(stderr, "[bcnn_hip] bcnn_hip_activation_backward: activation %d takes its derivative from the input "
                        "(bcnn_hip_activation_backward_from_input; the stand-alone activation node)\n", act);
        exit(1);
    }
    const bool al = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    if (act != BCNN_HIP_ACT_PRELU) {
        launch_chan_map(ActBwdBody{x, dx, nullptr, act, al}, 1, 1, (int)size);
        return;
    }
    const int n = (int)(size / ((size_t)spatial * channels));
    if (dslopes) {
        const long long M = (long long)n * spatial;
        const int splits = chan_splits(channels, M);
        float* part = scratch(SCRATCH_REDUCE, (size_t)channels * splits);
        launch_chan_reduce<1>(PreluGradF{x, dx}, channels, spatial, M, splits, part);
        accumulate_kernel<<<ceil_div(channels, 256), 256, 0, current_stream()>>>(part, channels, splits, dslopes);
        KERNEL_CHECK();
    }
    launch_chan_map(ActBwdBody{x, dx, slopes, act, al}, n, channels, spatial);
}

void bcnn_hip_activation_forward_keep(float* x, float* x_saved, size_t size, int act) {
    if (!size) return;
    if (act == BCNN_HIP_ACT_PRELU) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_activation_forward_keep: PReLU needs its slopes (bcnn_hip_activation_forward)\n");
        exit(1);
    }
    if (act == BCNN_HIP_ACT_NONE && !x_saved) return;
    gated_fwd_kernel<<<stream_grid(size / 4 + 1, 256), 256, 0, current_stream()>>>(x, x_saved, size, act,
                                                                                   al16(x) && al16(x_saved));
    KERNEL_CHECK();
}

void bcnn_hip_activation_backward_from_input(const float* x_saved, float* dx, size_t size, int act) {
    if (!size) return;
    if (!act_needs_input(act) || !x_saved) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_activation_backward_from_input: activation %d is not hard-swish, swish or "
                        "mish, or no saved input was given\n", act);
        exit(1);
    }
    gated_bwd_kernel<<<stream_grid(size / 4 + 1, 256), 256, 0, current_stream()>>>(x_saved, dx, size, act,
                                                                                   al16(x_saved) && al16(dx));
    KERNEL_CHECK();
}

}  // extern "C"
