// softmax_loss.hip -- softmax over the channels and cross-entropy against a class-index label map (the softmax-loss node):
// forward (probabilities, loss, counts), backward (dx = scale / D * (p - y)) and the on-demand confusion matrix.
//
// Semantics: include/bcnn_hip.h. How a label value is classified (valid / ignored / out of range) and the denominator D of
// a normaliser are softmax_loss_rule.h and nothing else; a label value indexes memory only after that rule called it valid.
//
// Forward dispatch, a function of (C, HW, alignment) alone:
//   HW == 1                 softmax_loss_fwd_rows             one wave per row, lanes along the contiguous C axis
//   HW > 1, C <= kCReg      softmax_loss_fwd_pixels_reg[:v4]  lanes along the pixel axis, the C logits of a pixel in registers:
//                                                             x is read from memory once
//   HW > 1, C >  kCReg      softmax_loss_fwd_pixels_stream[:v4]  same lanes; running maximum and rescaled sum in one sweep
//                                                             over C, a second sweep writes p
//   :v4 -- HW % 4 == 0 and x, p and the label on 16 bytes: a lane owns four consecutive pixels, every access is 16 bytes and
//   a wave's load of one channel plane is one run of 1 KiB. Otherwise one pixel per lane, 4-byte accesses, 256-byte runs.
// With a label, every workgroup leaves one partial {double sum of l, valid, ignored, out_of_range, correct} in the
// SCRATCH_SOFTMAX_LOSS block and softmax_loss_finalize (one wave) adds them in a fixed order -- lane k adds the partials k,
// k + 64, ... ascending, then the 64 lane sums go through one xor tree -- and writes the record: no floating-point atomics,
// the same bits on every run. Without a label (a PREDICT forward) only p is written.
//
// Arithmetic: float. p = e_c / sum with e_c = expf(x_c - max) and one correctly rounded reciprocal per pixel -- one
// exponential per element (two on the streaming and rows paths, which do not keep e_c), no logarithm on the way to p.
// Against float64 that is (C + 3) * 2^-24 relative at worst on the register path (expf within 1 ulp, C - 1 additions, the
// reciprocal, the product) and (3 C + 4) * 2^-24 on the streaming path (each step of the rescaled sum: an exponential, a
// product, an addition), inside the project's softmax bound of (C + 1) * 2^-22 plus the spacing terms
// (tests/_next_ref.softmax_bound), which was derived for the double-precision log-sum-exp form of softmax_kernel.
// l = log(sum) - (x_t - max): logf, and the two subtractions in double (exact on float operands).
#include <cfloat>
#include <cstdint>

#include "common.h"
#include "softmax_loss_rule.h"

namespace bcnn_hip {

// The most classes the register path holds. Its :v4 form keeps 4 * kCReg logits per lane: by the compiler's resource
// report the 32-class instance takes 179 vector registers and no scratch memory, two waves per
// SIMD; 21 classes (VOC) run in the 24-class instance with 146, three waves. 48 classes would pass 256 registers.
constexpr int kCReg = 32;

struct SlAcc {
    double loss;
    int valid, ignored, oor, correct;
};

__device__ __forceinline__ void sl_account(SlAcc& a, int kind, int cls, int arg, double l) {
    if (kind == BCNN_SL_VALID) {
        a.loss += l;
        a.valid += 1;
        a.correct += (arg == cls);
    } else if (kind == BCNN_SL_IGNORED) {
        a.ignored += 1;
    } else {
        a.oor += 1;
    }
}

// the workgroup's partial: every wave through one xor tree, then the four wave sums in wave order. 256 threads.
__device__ __forceinline__ void sl_store_partial(const SlAcc& a, double* __restrict__ ploss, int4* __restrict__ pcnt) {
    __shared__ double wl[4];
    __shared__ int4 wc[4];
    double l = a.loss;
    int4 c = make_int4(a.valid, a.ignored, a.oor, a.correct);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l += __shfl_xor(l, o);
        c.x += __shfl_xor(c.x, o);
        c.y += __shfl_xor(c.y, o);
        c.z += __shfl_xor(c.z, o);
        c.w += __shfl_xor(c.w, o);
    }
    if ((threadIdx.x & 63) == 0) { wl[threadIdx.x >> 6] = l; wc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        int4 k = make_int4(0, 0, 0, 0);
        for (int w = 0; w < 4; ++w) {
            t += wl[w];
            k.x += wc[w].x; k.y += wc[w].y; k.z += wc[w].z; k.w += wc[w].w;
        }
        ploss[blockIdx.x] = t;
        pcnt[blockIdx.x] = k;
    }
}

// ---- rows: HW == 1. One wave per row ------------------------------------------------------------------------------------
// Three sweeps over the row (maximum and first argmax, sum, p); the second and third hit the cache: a row is 4 C bytes.
__global__ __launch_bounds__(256) void sl_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                          float* __restrict__ p, double* __restrict__ ploss,
                                                          int4* __restrict__ pcnt, int C, unsigned rows, int ignore_label) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    SlAcc acc = {0.0, 0, 0, 0, 0};
    for (unsigned r = wave; r < rows; r += nwaves) {
        const float* __restrict__ px = x + (size_t)r * C;
        float* __restrict__ pp = p + (size_t)r * C;
        float m = -FLT_MAX;
        int arg = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float v = px[c];
            if (v > m || arg == 0x7fffffff) { m = v; arg = c; }  // ascending c: the first maximum of the lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o);
            const int oa = __shfl_xor(arg, o);
            if (oa != 0x7fffffff && (arg == 0x7fffffff || om > m || (om == m && oa < arg))) { m = om; arg = oa; }
        }
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(px[c] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float inv = 1.0f / s;
        for (int c = lane; c < C; c += 64) pp[c] = expf(px[c] - m) * inv;
        if (label != nullptr && lane == 0) {
            int cls;
            const int kind = bcnn_softmax_loss_classify(label[r], ignore_label, C, &cls);
            double l = 0.0;
            if (kind == BCNN_SL_VALID) l = (double)logf(s) - ((double)px[cls] - (double)m);
            sl_account(acc, kind, cls, arg, l);
        }
    }
    if (label != nullptr) sl_store_partial(acc, ploss, pcnt);
}

// ---- pixels, logits in registers: HW > 1, C <= CMAX <= kCReg ---------------------------------------------------------------
// An item is PX consecutive pixels of one image (PX = 4: VEC). v[c][e] is indexed by unrolled constants only; the
// channels past C are skipped by a wave-uniform test.
template <int CMAX, bool VEC>
__global__ __launch_bounds__(256) void sl_fwd_pixels_reg_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                                float* __restrict__ p, double* __restrict__ ploss,
                                                                int4* __restrict__ pcnt, int C, unsigned HW, const FastDiv dq,
                                                                unsigned total_items, int ignore_label) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned gstride = gridDim.x * blockDim.x;
    SlAcc acc = {0.0, 0, 0, 0, 0};
    for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < total_items; item += gstride) {
        const unsigned b = fdiv(item, dq), q = item - b * dq.d;
        const size_t pix = (size_t)q * PX;
        const float* __restrict__ px = x + (size_t)b * C * HW + pix;
        float* __restrict__ pp = p + (size_t)b * C * HW + pix;
        float v[CMAX][PX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
                if (VEC) {
                    const float4 t = *reinterpret_cast<const float4*>(px + (size_t)c * HW);
                    v[c][0] = t.x; v[c][1 % PX] = t.y; v[c][2 % PX] = t.z; v[c][3 % PX] = t.w;
                } else {
                    v[c][0] = px[(size_t)c * HW];
                }
            }
        }
        int kind[PX], cls[PX];
        if (label != nullptr) {
            float t[PX];
            if (VEC) {
                const float4 l4 = *reinterpret_cast<const float4*>(label + (size_t)b * HW + pix);
                t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
            } else {
                t[0] = label[(size_t)b * HW + pix];
            }
#pragma unroll
            for (int e = 0; e < PX; ++e) kind[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]);
        } else {
#pragma unroll
            for (int e = 0; e < PX; ++e) { kind[e] = BCNN_SL_IGNORED; cls[e] = -1; }
        }
        float m[PX], s[PX], dt[PX];
        int arg[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) { m[e] = v[0][e]; arg[e] = 0; s[e] = 0.f; dt[e] = 0.f; }
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
            if (c < C) {
#pragma unroll
                for (int e = 0; e < PX; ++e)
                    if (v[c][e] > m[e]) { m[e] = v[c][e]; arg[e] = c; }  // strict: the first maximum wins
            }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
#pragma unroll
                for (int e = 0; e < PX; ++e) {
                    const float d = v[c][e] - m[e];
                    if (c == cls[e]) dt[e] = d;
                    v[c][e] = expf(d);
                    s[e] += v[c][e];
                }
            }
        float inv[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) inv[e] = 1.0f / s[e];
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                if (VEC) {
                    *reinterpret_cast<float4*>(pp + (size_t)c * HW) =
                        make_float4(v[c][0] * inv[0], v[c][1 % PX] * inv[1 % PX], v[c][2 % PX] * inv[2 % PX],
                                    v[c][3 % PX] * inv[3 % PX]);
                } else {
                    pp[(size_t)c * HW] = v[c][0] * inv[0];
                }
            }
        if (label != nullptr) {
#pragma unroll
            for (int e = 0; e < PX; ++e)
                sl_account(acc, kind[e], cls[e], arg[e], kind[e] == BCNN_SL_VALID ? (double)logf(s[e]) - (double)dt[e] : 0.0);
        }
    }
    if (label != nullptr) sl_store_partial(acc, ploss, pcnt);
}

// ---- pixels, streaming: HW > 1, C > kCReg -----------------------------------------------------------------------------------
// Sweep 1: running maximum m and sum s of exp(x - m), rescaled by exp(m_old - m_new) when the maximum moves -- one
// exponential per element, exp(-|x - m|), either way. Sweep 2 reads x again and writes p = exp(x - m) / s.
template <bool VEC>
__global__ __launch_bounds__(256) void sl_fwd_pixels_stream_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                                   float* __restrict__ p, double* __restrict__ ploss,
                                                                   int4* __restrict__ pcnt, int C, unsigned HW, const FastDiv dq,
                                                                   unsigned total_items, int ignore_label) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned gstride = gridDim.x * blockDim.x;
    SlAcc acc = {0.0, 0, 0, 0, 0};
    for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < total_items; item += gstride) {
        const unsigned b = fdiv(item, dq), q = item - b * dq.d;
        const size_t pix = (size_t)q * PX;
        const float* __restrict__ px = x + (size_t)b * C * HW + pix;
        float* __restrict__ pp = p + (size_t)b * C * HW + pix;
        int kind[PX], cls[PX];
        if (label != nullptr) {
            float t[PX];
            if (VEC) {
                const float4 l4 = *reinterpret_cast<const float4*>(label + (size_t)b * HW + pix);
                t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
            } else {
                t[0] = label[(size_t)b * HW + pix];
            }
#pragma unroll
            for (int e = 0; e < PX; ++e) kind[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]);
        } else {
#pragma unroll
            for (int e = 0; e < PX; ++e) { kind[e] = BCNN_SL_IGNORED; cls[e] = -1; }
        }
        float m[PX], s[PX], xt[PX];
        int arg[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) { m[e] = -FLT_MAX; s[e] = 0.f; xt[e] = 0.f; arg[e] = 0; }
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            float v[PX];
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(px + (size_t)c * HW);
                v[0] = t.x; v[1 % PX] = t.y; v[2 % PX] = t.z; v[3 % PX] = t.w;
            } else {
                v[0] = px[(size_t)c * HW];
            }
#pragma unroll
            for (int e = 0; e < PX; ++e) {
                const bool up = v[e] > m[e] || c == 0;  // strict: the first maximum wins
                const float ex = expf(up ? m[e] - v[e] : v[e] - m[e]);
                s[e] = up ? s[e] * ex + 1.0f : s[e] + ex;
                if (up) { m[e] = v[e]; arg[e] = c; }
                if (c == cls[e]) xt[e] = v[e];
            }
        }
        float inv[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) inv[e] = 1.0f / s[e];
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(px + (size_t)c * HW);
                *reinterpret_cast<float4*>(pp + (size_t)c * HW) =
                    make_float4(expf(t.x - m[0]) * inv[0], expf(t.y - m[1 % PX]) * inv[1 % PX],
                                expf(t.z - m[2 % PX]) * inv[2 % PX], expf(t.w - m[3 % PX]) * inv[3 % PX]);
            } else {
                pp[(size_t)c * HW] = expf(px[(size_t)c * HW] - m[0]) * inv[0];
            }
        }
        if (label != nullptr) {
#pragma unroll
            for (int e = 0; e < PX; ++e)
                sl_account(acc, kind[e], cls[e], arg[e],
                           kind[e] == BCNN_SL_VALID ? (double)logf(s[e]) - ((double)xt[e] - (double)m[e]) : 0.0);
        }
    }
    if (label != nullptr) sl_store_partial(acc, ploss, pcnt);
}

// ---- finalize: one wave adds the partials in a fixed order and writes the record ---------------------------------------------
__global__ __launch_bounds__(64) void sl_finalize_kernel(const double* __restrict__ ploss, const int4* __restrict__ pcnt,
                                                         int nblk, int n, int norm, float scale,
                                                         bcnn_hip_softmax_loss_record* __restrict__ rec) {
    double l = 0.0;
    int4 c = make_int4(0, 0, 0, 0);
    for (int i = threadIdx.x; i < nblk; i += 64) {
        l += ploss[i];
        const int4 k = pcnt[i];
        c.x += k.x; c.y += k.y; c.z += k.z; c.w += k.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l += __shfl_xor(l, o);
        c.x += __shfl_xor(c.x, o);
        c.y += __shfl_xor(c.y, o);
        c.z += __shfl_xor(c.z, o);
        c.w += __shfl_xor(c.w, o);
    }
    if (threadIdx.x == 0) {
        const double D = bcnn_softmax_loss_denominator(norm, c.x, n);
        rec->loss = (float)(l / D);
        rec->grad_factor = (float)((double)scale / D);
        rec->valid = c.x;
        rec->ignored = c.y;
        rec->out_of_range = c.z;
        rec->correct = c.w;
    }
}

// ---- backward: dx (+)= grad_factor * (p - [c == t]) on valid pixels ---------------------------------------------------------
// One item is PX consecutive elements of one channel plane. OVERWRITE: every element is written, +0.0 where the pixel is
// not valid. Add form: an element of such a pixel keeps its bits (its own value is stored back inside a 16-byte store).
template <bool VEC, bool OVERWRITE>
__global__ __launch_bounds__(256) void sl_bwd_kernel(const float* __restrict__ p, const float* __restrict__ label,
                                                     const bcnn_hip_softmax_loss_record* __restrict__ rec, float* __restrict__ dx,
                                                     int C, unsigned HW, const FastDiv dq, const FastDiv dc, unsigned total_items,
                                                     int ignore_label) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned gstride = gridDim.x * blockDim.x;
    const float g = rec->grad_factor;
    for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < total_items; item += gstride) {
        const unsigned plane = fdiv(item, dq), q = item - plane * dq.d;
        const unsigned b = fdiv(plane, dc);
        const int c = (int)(plane - b * dc.d);
        const size_t off = (size_t)plane * HW + (size_t)q * PX, loff = (size_t)b * HW + (size_t)q * PX;
        float pv[PX], t[PX], out[PX];
        if (VEC) {
            const float4 p4 = *reinterpret_cast<const float4*>(p + off);
            const float4 l4 = *reinterpret_cast<const float4*>(label + loff);
            pv[0] = p4.x; pv[1 % PX] = p4.y; pv[2 % PX] = p4.z; pv[3 % PX] = p4.w;
            t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
            if (!OVERWRITE) {
                const float4 o4 = *reinterpret_cast<const float4*>(dx + off);
                out[0] = o4.x; out[1 % PX] = o4.y; out[2 % PX] = o4.z; out[3 % PX] = o4.w;
            }
        } else {
            pv[0] = p[off];
            t[0] = label[loff];
            if (!OVERWRITE) out[0] = dx[off];
        }
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            int cls;
            const bool valid = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls) == BCNN_SL_VALID;
            const float d = g * (pv[e] - (c == cls ? 1.0f : 0.0f));
            if (OVERWRITE) out[e] = valid ? d : 0.0f;
            else if (valid) out[e] += d;
        }
        if (VEC) *reinterpret_cast<float4*>(dx + off) = make_float4(out[0], out[1 % PX], out[2 % PX], out[3 % PX]);
        else dx[off] = out[0];
    }
}

// ---- confusion matrix: counts[label][argmax p] over valid pixels, on demand --------------------------------------------------
// One thread per pixel, lanes along the pixel axis. Integer atomics: the result does not depend on their order. LDS: the
// workgroup counts into a C x C tile (C <= 64: 16 KiB) and adds its non-zero entries to memory once.
template <bool LDS>
__global__ __launch_bounds__(256) void sl_confusion_kernel(const float* __restrict__ p, const float* __restrict__ label,
                                                           unsigned* __restrict__ counts, int C, unsigned HW, const FastDiv dq,
                                                           unsigned total, int ignore_label) {
    __shared__ unsigned tile[LDS ? 64 * 64 : 1];
    if (LDS) {
        for (int k = threadIdx.x; k < C * C; k += 256) tile[k] = 0u;
        __syncthreads();
    }
    const unsigned gstride = gridDim.x * blockDim.x;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gstride) {
        int cls;
        if (bcnn_softmax_loss_classify(label[t], ignore_label, C, &cls) != BCNN_SL_VALID) continue;
        const unsigned b = fdiv(t, dq), i = t - b * dq.d;
        const float* __restrict__ pp = p + (size_t)b * C * HW + i;
        float m = pp[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = pp[(size_t)c * HW];
            if (v > m) { m = v; arg = c; }
        }
        if (LDS) atomicAdd(&tile[cls * C + arg], 1u);
        else atomicAdd(&counts[(size_t)cls * C + arg], 1u);
    }
    if (LDS) {
        __syncthreads();
        for (int k = threadIdx.x; k < C * C; k += 256)
            if (tile[k]) atomicAdd(&counts[k], tile[k]);
    }
}

// exits like every other entry point handed a shape it cannot run; the element count, 0 for an empty tensor
static long long sl_total(const char* who, const bcnn_hip_softmax_loss_desc* d, int n, int c, int hw) {
    const bool ok = d && n >= 0 && c >= 1 && hw >= 1 && d->ignore_label < BCNN_SL_MAX_IGNORE_LABEL &&
                    bcnn_softmax_loss_denominator(d->norm, 1, 1) != 0.0;
    const long long total = ok ? (long long)n * c * hw : 0;
    if (!ok || total >= 0x7fffffffLL - 3) {
        fprintf(stderr, "[bcnn_hip] %s: invalid extents, ignore label or normaliser, or a tensor of 2^31 elements or more\n", who);
        exit(1);
    }
    return total;
}

template <bool VEC>
static void launch_pixels_reg(int grid, const float* x, const float* label, float* p, double* ploss, int4* pcnt, int C,
                              unsigned HW, const FastDiv dq, unsigned items, int ignore_label) {
#define SL_REG(CMAX)                                                                                                      \
    sl_fwd_pixels_reg_kernel<CMAX, VEC><<<grid, 256, 0, current_stream()>>>(x, label, p, ploss, pcnt, C, HW, dq, items, \
                                                                            ignore_label)
    if (C <= 4) SL_REG(4);
    else if (C <= 8) SL_REG(8);
    else if (C <= 16) SL_REG(16);
    else if (C <= 24) SL_REG(24);
    else SL_REG(kCReg);
#undef SL_REG
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_softmax_loss_c_reg(void) { return kCReg; }

void bcnn_hip_softmax_loss_forward(const bcnn_hip_softmax_loss_desc* desc, const float* x, const float* label, float* p,
                                   bcnn_hip_softmax_loss_record* rec, int n, int c, int hw) {
    if (!sl_total("bcnn_hip_softmax_loss_forward", desc, n, c, hw)) return;
    if (rec == nullptr) label = nullptr;  // statistics need both
    const long long pixels = (long long)n * hw;
    double* ploss = nullptr;
    int4* pcnt = nullptr;
    const bool vec = hw > 1 && (hw & 3) == 0 && al16(x) && al16(p) && al16(label);
    const long long items = vec ? pixels / 4 : pixels;
    const int grid = hw == 1 ? stream_grid((size_t)pixels * 64, 256) : stream_grid((size_t)items, 256);
    if (label) {  // one partial per workgroup: doubles first, then the int4 counts (16-byte aligned: grid rounded up to even)
        const size_t slots = ((size_t)grid + 1) & ~(size_t)1;
        float* block = scratch(SCRATCH_SOFTMAX_LOSS, slots * 6);
        ploss = reinterpret_cast<double*>(block);
        pcnt = reinterpret_cast<int4*>(block + slots * 2);
    }
    const FastDiv dq = make_fdiv((unsigned)(vec ? hw / 4 : hw), (unsigned long long)items);
    if (hw == 1) {
        trace_kernel("softmax_loss_fwd_rows");
        sl_fwd_rows_kernel<<<grid, 256, 0, current_stream()>>>(x, label, p, ploss, pcnt, c, (unsigned)n, desc->ignore_label);
    } else if (c <= kCReg) {
        trace_kernel(vec ? "softmax_loss_fwd_pixels_reg:v4" : "softmax_loss_fwd_pixels_reg");
        if (vec) launch_pixels_reg<true>(grid, x, label, p, ploss, pcnt, c, (unsigned)hw, dq, (unsigned)items, desc->ignore_label);
        else launch_pixels_reg<false>(grid, x, label, p, ploss, pcnt, c, (unsigned)hw, dq, (unsigned)items, desc->ignore_label);
    } else {
        trace_kernel(vec ? "softmax_loss_fwd_pixels_stream:v4" : "softmax_loss_fwd_pixels_stream");
        if (vec) sl_fwd_pixels_stream_kernel<true><<<grid, 256, 0, current_stream()>>>(x, label, p, ploss, pcnt, c, (unsigned)hw, dq, (unsigned)items, desc->ignore_label);
        else sl_fwd_pixels_stream_kernel<false><<<grid, 256, 0, current_stream()>>>(x, label, p, ploss, pcnt, c, (unsigned)hw, dq, (unsigned)items, desc->ignore_label);
    }
    KERNEL_CHECK();
    if (label) {
        trace_kernel("softmax_loss_finalize");
        sl_finalize_kernel<<<1, 64, 0, current_stream()>>>(ploss, pcnt, grid, n, desc->norm, desc->scale, rec);
        KERNEL_CHECK();
    }
}

void bcnn_hip_softmax_loss_backward(const bcnn_hip_softmax_loss_desc* desc, const float* p, const float* label,
                                    const bcnn_hip_softmax_loss_record* rec, float* dx, int n, int c, int hw, int overwrite) {
    const long long total = sl_total("bcnn_hip_softmax_loss_backward", desc, n, c, hw);
    if (!total) return;
    const bool vec = (hw & 3) == 0 && al16(p) && al16(dx) && al16(label);
    const long long items = vec ? total / 4 : total;
    const FastDiv dq = make_fdiv((unsigned)(vec ? hw / 4 : hw), (unsigned long long)items);
    const FastDiv dc = make_fdiv((unsigned)c, (unsigned long long)n * c);
    const int grid = stream_grid((size_t)items, 256);
    static const char* const names[4] = {"softmax_loss_bwd", "softmax_loss_bwd:overwrite", "softmax_loss_bwd:v4",
                                         "softmax_loss_bwd:v4:overwrite"};
    trace_kernel(names[(vec ? 2 : 0) + (overwrite ? 1 : 0)]);
#define SL_BWD(V, O)                                                                                                        \
    sl_bwd_kernel<V, O><<<grid, 256, 0, current_stream()>>>(p, label, rec, dx, c, (unsigned)hw, dq, dc, (unsigned)items, \
                                                            desc->ignore_label)
    if (vec) { if (overwrite) SL_BWD(true, true); else SL_BWD(true, false); }
    else { if (overwrite) SL_BWD(false, true); else SL_BWD(false, false); }
#undef SL_BWD
    KERNEL_CHECK();
}

void bcnn_hip_softmax_loss_confusion(const bcnn_hip_softmax_loss_desc* desc, const float* p, const float* label,
                                     unsigned* counts, int n, int c, int hw) {
    const long long total = sl_total("bcnn_hip_softmax_loss_confusion", desc, n, c, hw);
    if ((long long)c * c >= 0x7fffffffLL) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_softmax_loss_confusion: a matrix of 2^31 counts or more\n");
        exit(1);
    }
    HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)c * c * sizeof(unsigned), current_stream()));
    if (!total) return;
    const long long pixels = (long long)n * hw;
    const FastDiv dq = make_fdiv((unsigned)hw, (unsigned long long)pixels);
    const int grid = stream_grid((size_t)pixels, 256);
    trace_kernel(c <= 64 ? "softmax_loss_confusion:lds" : "softmax_loss_confusion");
    if (c <= 64) sl_confusion_kernel<true><<<grid, 256, 0, current_stream()>>>(p, label, counts, c, (unsigned)hw, dq, (unsigned)pixels, desc->ignore_label);
    else sl_confusion_kernel<false><<<grid, 256, 0, current_stream()>>>(p, label, counts, c, (unsigned)hw, dq, (unsigned)pixels, desc->ignore_label);
    KERNEL_CHECK();
}

}  // extern "C"
