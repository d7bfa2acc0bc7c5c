// scale_channels.hip -- the scale-channels node: y = x * gate with one factor per (image, channel) plane (the last step of
// a squeeze-and-excitation block, Darknet's [scale_channels]) or a gate of x's shape (Darknet's [sam]). No reference
// counterpart. HBM-bound streaming kernels.
//   forward : one multiply per element; x read, y written (+ the gate read once for the same-shape form).
//   backward: ONE sweep. dx += dy * gate and the plane sums of dy * x share the reads of dy (and x): x, dy and dx are read
//             once, dx is written once. The sums use no atomics and no order that depends on scheduling:
//               planes of up to kWaveMaxHW elements: a group of 2^k lanes (1..64, the smallest that covers the plane) owns a
//                 plane, so a 7 x 7 plane occupies one wave and a 2 x 2 plane four lanes; a butterfly adds the lanes;
//               larger planes: chan_reduce.h's scheme with the N * C planes as its channels -- a plane is cut into slices
//                 of at least 1024 elements until the chip is covered, one workgroup per slice, the slice sums are added
//                 in ascending order in double.
//             The number of slices follows from the shape alone, so two runs give the same bits.
// Products and sums are separate roundings (the build has -ffp-contract=off): y and dx are the bits of numpy's x * g and
// dx + dy * g.
#include "chan_reduce.h"

namespace bcnn_hip {

constexpr int kWaveMaxHW = 1024;   // up to here a plane is one lane group's; past it, workgroups take slices
constexpr int kSliceMinElems = 1024;  // one float4 per thread of a 256-thread workgroup

struct ScaleFwdBody {  // c is the plane: launch_chan_map runs with N = 1, C = planes
    const float* x;
    const float* gate;
    float* y;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float g = gate[c];
        if (cnt == 4 && al && (off & 3u) == 0) {
            float4 v = *reinterpret_cast<const float4*>(x + off);
            v.x *= g; v.y *= g; v.z *= g; v.w *= g;
            *reinterpret_cast<float4*>(y + off) = v;
        } else {
            for (int k = 0; k < cnt; ++k) y[off + k] = x[off + k] * g;
        }
    }
};

struct ScaleFwdSameBody {  // the plain product, one long plane
    const float* x;
    const float* gate;
    float* y;
    bool al;
    __device__ void operator()(unsigned off, int, int cnt) const {
        if (cnt == 4 && al && (off & 3u) == 0) {
            float4 v = *reinterpret_cast<const float4*>(x + off);
            const float4 g = *reinterpret_cast<const float4*>(gate + off);
            v.x *= g.x; v.y *= g.y; v.z *= g.z; v.w *= g.w;
            *reinterpret_cast<float4*>(y + off) = v;
        } else {
            for (int k = 0; k < cnt; ++k) y[off + k] = x[off + k] * gate[off + k];
        }
    }
};

// dx += dy * gate alone (no gate gradient asked for)
struct ScaleDxBody {
    const float* gate;
    const float* dy;
    float* dx;
    bool al;
    __device__ void operator()(unsigned off, int c, int cnt) const {
        const float g = gate[c];
        if (cnt == 4 && al && (off & 3u) == 0) {
            const float4 d = *reinterpret_cast<const float4*>(dy + off);
            float4 v = *reinterpret_cast<float4*>(dx + off);
            v.x += d.x * g; v.y += d.y * g; v.z += d.z * g; v.w += d.w * g;
            *reinterpret_cast<float4*>(dx + off) = v;
        } else {
            for (int k = 0; k < cnt; ++k) dx[off + k] += dy[off + k] * g;
        }
    }
};

// same-shape gate: dx += dy * gate, dgate += dy * x; either gradient may be absent
struct ScaleBwdSameBody {
    const float* x;
    const float* gate;
    const float* dy;
    float* dx;
    float* dgate;
    bool al;
    __device__ void operator()(unsigned off, int, int cnt) const {
        if (cnt == 4 && al && (off & 3u) == 0) {
            const float4 d = *reinterpret_cast<const float4*>(dy + off);
            if (dx) {
                const float4 g = *reinterpret_cast<const float4*>(gate + off);
                float4 v = *reinterpret_cast<float4*>(dx + off);
                v.x += d.x * g.x; v.y += d.y * g.y; v.z += d.z * g.z; v.w += d.w * g.w;
                *reinterpret_cast<float4*>(dx + off) = v;
            }
            if (dgate) {
                const float4 s = *reinterpret_cast<const float4*>(x + off);
                float4 v = *reinterpret_cast<float4*>(dgate + off);
                v.x += d.x * s.x; v.y += d.y * s.y; v.z += d.z * s.z; v.w += d.w * s.w;
                *reinterpret_cast<float4*>(dgate + off) = v;
            }
        } else {
            for (int k = 0; k < cnt; ++k) {
                const float d = dy[off + k];
                if (dx) dx[off + k] += d * gate[off + k];
                if (dgate) dgate[off + k] += d * x[off + k];
            }
        }
    }
};

// Small planes. A group of `lanes` (a power of two, 1..64) consecutive threads owns plane (global thread / lanes): lane j of
// the group takes elements j, j + lanes, ... in ascending order, the butterfly adds the lanes' sums, lane 0 adds the total to
// dgate. Consecutive groups own consecutive planes, so a wave's accesses are one contiguous run of the tensors.
__global__ __launch_bounds__(256) void scale_bwd_small_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                              const float* __restrict__ dy, float* __restrict__ dx,
                                                              float* __restrict__ dgate, int planes, int HW, int lanes) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long plane = t / lanes;
    const int j = (int)(t - plane * lanes);
    float acc = 0.f;
    if (plane < planes) {  // (whole groups are in or out: a wave's shuffles below never mix planes)
        const long long base = plane * HW;
        const float g = dx ? gate[plane] : 0.f;
        for (int i = j; i < HW; i += lanes) {
            const float d = dy[base + i];
            acc += d * x[base + i];
            if (dx) dx[base + i] += d * g;
        }
    }
    for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (plane < planes && j == 0) dgate[plane] += acc;
}

// Large planes: the functor of chan_reduce_partial also writes dx while it reads dy for the sum.
struct ScaleBwdF {
    static constexpr int kInFlight = 4;
    const float* x;
    const float* gate;
    const float* dy;
    float* dx;  // may be null: sums only
    bool al;
    __device__ void operator()(long long off, int c, float (&acc)[1]) const {
        const float d = dy[off];
        acc[0] += d * x[off];
        if (dx) dx[off] += d * gate[c];
    }
    __device__ void vec4(long long off, int c, float (&acc)[1]) const {
        if (!al) {
            for (int k = 0; k < 4; ++k) (*this)(off + k, c, acc);
            return;
        }
        const float4 d = *reinterpret_cast<const float4*>(dy + off);
        const float4 s = *reinterpret_cast<const float4*>(x + off);
        acc[0] += d.x * s.x; acc[0] += d.y * s.y; acc[0] += d.z * s.z; acc[0] += d.w * s.w;
        if (dx) {
            const float g = gate[c];
            float4 v = *reinterpret_cast<float4*>(dx + off);
            v.x += d.x * g; v.y += d.y * g; v.z += d.z * g; v.w += d.w * g;
            *reinterpret_cast<float4*>(dx + off) = v;
        }
    }
};

__global__ void scale_gate_accumulate_kernel(const float* __restrict__ partials, int planes, int splits,
                                             float* __restrict__ dgate) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    double s = 0.0;
    for (int i = 0; i < splits; ++i) s += (double)partials[(long long)p * splits + i];
    dgate[p] += (float)s;
}

// slices per plane: cover the chip (CHAN_WG_PER_CU workgroups per CU over all planes), at least kSliceMinElems each
static int scale_splits(long long planes, int hw) {
    long long want = ((long long)CHAN_WG_PER_CU * kCUs + planes - 1) / planes;
    const long long maxs = hw / kSliceMinElems;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    return (int)want;
}

static long long scale_total(const char* who, int n, int c, int hw) {
    const long long total = (long long)n * c * hw;
    if (n < 0 || c < 0 || hw < 0 || total >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] %s: a negative extent, or a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    return total;
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

void bcnn_hip_scale_channels_forward(const float* x, const float* gate, float* y, int n, int c, int hw, int same_shape) {
    const long long total = scale_total("bcnn_hip_scale_channels_forward", n, c, hw);
    if (!total) return;
    if (same_shape) {
        trace_kernel("scale_channels_fwd:same");
        launch_chan_map(ScaleFwdSameBody{x, gate, y, al16(x) && al16(gate) && al16(y)}, 1, 1, (int)total);
        return;
    }
    trace_kernel("scale_channels_fwd");
    launch_chan_map(ScaleFwdBody{x, gate, y, al16(x) && al16(y)}, 1, n * c, hw);
}

void bcnn_hip_scale_channels_backward(const float* x, const float* gate, const float* dy, float* dx, float* dgate, int n,
                                      int c, int hw, int same_shape) {
    const long long total = scale_total("bcnn_hip_scale_channels_backward", n, c, hw);
    if (!total || (!dx && !dgate)) return;
    const int planes = n * c;
    if (same_shape) {
        trace_kernel("scale_channels_bwd:same");
        launch_chan_map(ScaleBwdSameBody{x, gate, dy, dx, dgate, al16(x) && al16(gate) && al16(dy) && al16(dx) && al16(dgate)},
                        1, 1, (int)total);
        return;
    }
    if (!dgate) {
        trace_kernel("scale_channels_bwd:dx");
        launch_chan_map(ScaleDxBody{gate, dy, dx, al16(dy) && al16(dx)}, 1, planes, hw);
        return;
    }
    if (hw <= kWaveMaxHW) {
        int lanes = 1;
        while (lanes < hw && lanes < kWave) lanes <<= 1;
        trace_kernel("scale_channels_bwd:small");
        const long long threads = (long long)planes * lanes;
        scale_bwd_small_kernel<<<(unsigned)ceil_div(threads, 256), 256, 0, current_stream()>>>(x, gate, dy, dx, dgate, planes,
                                                                                                hw, lanes);
        KERNEL_CHECK();
        return;
    }
    trace_kernel("scale_channels_bwd:split");
    const int splits = scale_splits(planes, hw);
    float* part = scratch(SCRATCH_REDUCE, (size_t)planes * splits);
    launch_chan_reduce<1>(ScaleBwdF{x, gate, dy, dx, al16(x) && al16(dy) && al16(dx)}, planes, hw, hw, splits, part);
    scale_gate_accumulate_kernel<<<ceil_div(planes, 256), 256, 0, current_stream()>>>(part, planes, splits, dgate);
    KERNEL_CHECK();
}

}  // extern "C"
