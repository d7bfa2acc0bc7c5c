// dice_loss.hip -- softmax over the channels, cross-entropy and soft Dice against a class-index label map in one node (the
// dice-loss node): forward (probabilities, per-class sums, loss, counts), finalize (coefficients) and backward.
//
// Semantics and mathematics: include/bcnn_hip.h. How a label value is classified is softmax_loss_rule.h and nothing else;
// a label value indexes nothing before that rule called it valid. Design, register budget and bounds: DESIGN.md section 35.
//
// Work split. Lanes run along the pixels; a lane owns four consecutive pixels (16-byte accesses) when hw % 4 == 0 and the
// tensors of the call are 16-byte aligned, one pixel otherwise. Every workgroup is confined to ONE image: block ->
// (image, part), and part strides over the image's 256-lane tiles. So a workgroup's sums belong to one group under either
// `reduce`, and the backward reads one coefficient row through uniform loads.
//
// Forward dispatch, a function of (C, hw, alignment) alone:
//   hw > 1, C <= 32   dl_fwd_reg     a pixel's logits in registers (x read once, p written once), per-class I and Z in
//                                    registers across all tiles of the workgroup, Y and the pixel counts by ballot + popcount
//                                    (Y in one vector register, lane c for class c); folded once: xor steps across
//                                    the wave, the four waves through LDS, one partial row {I[C], Z[C], Y[C]} per workgroup.
//   hw > 1, C >  32   dl_fwd_stream  the running-maximum softmax of the softmax-loss node's streaming kernel writes p and the
//   hw == 1           dl_fwd_rows    cross-entropy partials (hw == 1: one wave per row, as that node's rows kernel); then
//                     dl_sums        forms I, Z, Y from p, class-major: a workgroup owns (image, 8 classes, part), reads the
//                                    label once per tile and eight contiguous plane segments of p. One extra read of p.
//   dl_finalize (one workgroup, 16 waves): a wave per (group, class) adds the partial rows in double, lane k the rows k,
//   k + 64, ... ascending, then one xor tree; forms Den, the Dice term, A and B; wave 0 then adds the G C terms and the
//   cross-entropy partials the same way and writes the record. No atomics anywhere: two runs give the same bits.
// Backward: one launch. C <= 32: a pixel's p in registers, the dot product and the write from there; above: two sweeps.
//
// Arithmetic of p: exactly the softmax-loss node's on the same dispatch branch (same operations in the same order), so p
// has that node's bits; alignment changes the loads only.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "softmax_loss_rule.h"

namespace bcnn_hip {

// The most classes the register kernels hold; the dispatch itself follows bcnn_hip_softmax_loss_c_reg() (p must take the
// softmax-loss node's branch to have its bits), which may not exceed this.
constexpr int kDlReg = 32;
constexpr int kDlChunk = 8;              // classes per workgroup of dl_sums
constexpr int kDlGridCap = kCUs * 8;     // persistent workgroups of one launch, as stream_grid
constexpr int kDlFinalWaves = 16;

typedef bcnn_hip_dice_loss_record DlRecord;

__device__ __forceinline__ int dl_popc(bool pred) { return (int)__popcll(__ballot(pred)); }

// the workgroup's cross-entropy partial: the loss of every lane through one xor tree, then the four wave sums in wave
// order. The counts are wave-uniform already (ballots) unless `lane_counts`. 256 threads.
__device__ __forceinline__ void dl_store_ce(double l, int4 c, bool lane_counts, double* __restrict__ ploss,
                                            int4* __restrict__ pcnt) {
    __shared__ double wl[4];
    __shared__ int4 wc[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l += __shfl_xor(l, o);
        if (lane_counts) {
            c.x += __shfl_xor(c.x, o);
            c.y += __shfl_xor(c.y, o);
            c.z += __shfl_xor(c.z, o);
            c.w += __shfl_xor(c.w, o);
        }
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

// ---- forward, logits in registers: hw > 1, C <= CMAX <= kDlReg -----------------------------------------------------------------
// v[c][e], I[c], Z[c] are indexed by unrolled constants only; the classes past C are skipped by a uniform test. The tile
// loop is wave-uniform (a lane past the image's end is inactive inside it), so the ballots see every lane. A class's
// popcount is wave-uniform; lane c adds it to its Y, so all the class counts take one vector register: CMAX scalar
// counters beside the CMAX plane offsets did not fit the scalar file and spilled on every update.
template <int CMAX, bool VEC>
__global__ __launch_bounds__(256) void dl_fwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                         float* __restrict__ p, double* __restrict__ ploss,
                                                         int4* __restrict__ pcnt, float* __restrict__ rows, int C, unsigned HW,
                                                         unsigned qn, unsigned parts, const FastDiv dp, int ignore_label,
                                                         int squared) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned b = fdiv(blockIdx.x, dp), part = blockIdx.x - b * parts;
    const float* __restrict__ xb = x + (size_t)b * C * HW;
    float* __restrict__ pb = p + (size_t)b * C * HW;
    const float* __restrict__ lb = label ? label + (size_t)b * HW : nullptr;
    float I[CMAX], Z[CMAX];
    int Y = 0;  // lane c holds class c's count (CMAX <= 64): one vector register for all classes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) { I[c] = 0.f; Z[c] = 0.f; }
    double loss = 0.0;
    int4 cnt = make_int4(0, 0, 0, 0);
    for (unsigned base = part * 256u; base < qn; base += parts * 256u) {
        const unsigned q = base + threadIdx.x;
        int kind[PX], cls[PX];
        bool hit[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) { kind[e] = -1; cls[e] = -1; hit[e] = false; }
        if (q < qn) {
            const size_t pix = (size_t)q * PX;
            float v[CMAX][PX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < C) {
                    if (VEC) {
                        const float4 t = *reinterpret_cast<const float4*>(xb + (size_t)c * HW + pix);
                        v[c][0] = t.x; v[c][1 % PX] = t.y; v[c][2 % PX] = t.z; v[c][3 % PX] = t.w;
                    } else {
                        v[c][0] = xb[(size_t)c * HW + pix];
                    }
                }
            }
            if (lb != nullptr) {
                float t[PX];
                if (VEC) {
                    const float4 l4 = *reinterpret_cast<const float4*>(lb + pix);
                    t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
                } else {
                    t[0] = lb[pix];
                }
#pragma unroll
                for (int e = 0; e < PX; ++e) kind[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]);
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
#pragma unroll
                    for (int e = 0; e < PX; ++e) {
                        v[c][e] = v[c][e] * inv[e];  // p, the bits that are stored
                        if (kind[e] == BCNN_SL_VALID) Z[c] += squared ? v[c][e] * v[c][e] : v[c][e];
                        if (c == cls[e]) I[c] += v[c][e];
                    }
                    if (VEC) {
                        *reinterpret_cast<float4*>(pb + (size_t)c * HW + pix) =
                            make_float4(v[c][0], v[c][1 % PX], v[c][2 % PX], v[c][3 % PX]);
                    } else {
                        pb[(size_t)c * HW + pix] = v[c][0];
                    }
                }
#pragma unroll
            for (int e = 0; e < PX; ++e)
                if (kind[e] == BCNN_SL_VALID) {
                    loss += (double)logf(s[e]) - (double)dt[e];
                    hit[e] = arg[e] == cls[e];
                }
        }
        if (lb != nullptr) {  // every lane of the wave is here
#pragma unroll
            for (int e = 0; e < PX; ++e) {
                cnt.x += dl_popc(kind[e] == BCNN_SL_VALID);
                cnt.y += dl_popc(kind[e] == BCNN_SL_IGNORED);
                cnt.z += dl_popc(kind[e] == BCNN_SL_OUT_OF_RANGE);
                cnt.w += dl_popc(hit[e]);
            }
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    int k = 0;
#pragma unroll
                    for (int e = 0; e < PX; ++e) k += dl_popc(cls[e] == c);
                    Y += lane == c ? k : 0;
                }
        }
    }
    if (lb == nullptr) return;
    __shared__ float sI[4][CMAX], sZ[4][CMAX];
    __shared__ int sY[4][CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) {
            float a = I[c], z = Z[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); z += __shfl_xor(z, o); }
            if (lane == 0) { sI[wave][c] = a; sZ[wave][c] = z; }
        }
    if (lane < C) sY[wave][lane] = Y;
    dl_store_ce(loss, cnt, false, ploss, pcnt);  // its barrier also publishes sI, sZ, sY
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        float* __restrict__ row = rows + (size_t)blockIdx.x * 3 * C;
        row[c] = ((sI[0][c] + sI[1][c]) + sI[2][c]) + sI[3][c];
        row[C + c] = ((sZ[0][c] + sZ[1][c]) + sZ[2][c]) + sZ[3][c];
        row[2 * C + c] = __int_as_float(sY[0][c] + sY[1][c] + sY[2][c] + sY[3][c]);
    }
}

// ---- forward, streaming softmax: hw > 1, C > kDlReg. p and the cross-entropy partials; the sums come from dl_sums -----------------
// Sweep 1: running maximum m and sum s of exp(x - m), rescaled when the maximum moves; sweep 2 reads x again and writes p.
template <bool VEC>
__global__ __launch_bounds__(256) void dl_fwd_stream_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                            float* __restrict__ p, double* __restrict__ ploss,
                                                            int4* __restrict__ pcnt, int C, unsigned HW, unsigned qn,
                                                            unsigned parts, const FastDiv dp, int ignore_label) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned b = fdiv(blockIdx.x, dp), part = blockIdx.x - b * parts;
    const float* __restrict__ xb = x + (size_t)b * C * HW;
    float* __restrict__ pb = p + (size_t)b * C * HW;
    const float* __restrict__ lb = label ? label + (size_t)b * HW : nullptr;
    double loss = 0.0;
    int4 cnt = make_int4(0, 0, 0, 0);
    for (unsigned q = part * 256u + threadIdx.x; q < qn; q += parts * 256u) {
        const size_t pix = (size_t)q * PX;
        const float* __restrict__ px = xb + pix;
        float* __restrict__ pp = pb + pix;
        int kind[PX], cls[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) { kind[e] = -1; cls[e] = -1; }
        if (lb != nullptr) {
            float t[PX];
            if (VEC) {
                const float4 l4 = *reinterpret_cast<const float4*>(lb + pix);
                t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
            } else {
                t[0] = lb[pix];
            }
#pragma unroll
            for (int e = 0; e < PX; ++e) kind[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]);
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
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            if (kind[e] == BCNN_SL_VALID) {
                loss += (double)logf(s[e]) - ((double)xt[e] - (double)m[e]);
                cnt.x += 1;
                cnt.w += (arg[e] == cls[e]);
            } else if (kind[e] == BCNN_SL_IGNORED) {
                cnt.y += 1;
            } else if (kind[e] == BCNN_SL_OUT_OF_RANGE) {
                cnt.z += 1;
            }
        }
    }
    if (lb != nullptr) dl_store_ce(loss, cnt, true, ploss, pcnt);
}

// ---- forward, rows: hw == 1. One wave per row, lanes along the contiguous class axis ------------------------------------------
__global__ __launch_bounds__(256) void dl_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                          float* __restrict__ p, double* __restrict__ ploss,
                                                          int4* __restrict__ pcnt, int C, unsigned rows, int ignore_label) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    double loss = 0.0;
    int4 cnt = make_int4(0, 0, 0, 0);
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
            if (kind == BCNN_SL_VALID) {
                loss += (double)logf(s) - ((double)px[cls] - (double)m);
                cnt.x += 1;
                cnt.w += (arg == cls);
            } else if (kind == BCNN_SL_IGNORED) {
                cnt.y += 1;
            } else {
                cnt.z += 1;
            }
        }
    }
    if (label != nullptr) dl_store_ce(loss, cnt, true, ploss, pcnt);
}

// ---- sums from p, class-major (the wide path's second launch) ---------------------------------------------------------------------
// block -> (image, chunk of kDlChunk classes, part). A tile's label is classified once and serves the chunk's planes; every
// plane segment a wave reads is one contiguous run. Row (image * parts + part) of `rows` receives the chunk's entries.
template <bool VEC>
__global__ __launch_bounds__(256) void dl_sums_kernel(const float* __restrict__ p, const float* __restrict__ label,
                                                      float* __restrict__ rows, int C, unsigned HW, unsigned qn, unsigned parts,
                                                      unsigned chunks, int ignore_label, int squared) {
    constexpr int PX = VEC ? 4 : 1;
    const unsigned part = blockIdx.x % parts, bc = blockIdx.x / parts;
    const unsigned chunk = bc % chunks, b = bc / chunks;
    const int c0 = (int)chunk * kDlChunk;
    const int kc = C - c0 < kDlChunk ? C - c0 : kDlChunk;
    const float* __restrict__ pb = p + ((size_t)b * C + c0) * HW;
    const float* __restrict__ lb = label + (size_t)b * HW;
    float I[kDlChunk], Z[kDlChunk];
    int Y[kDlChunk];
#pragma unroll
    for (int k = 0; k < kDlChunk; ++k) { I[k] = 0.f; Z[k] = 0.f; Y[k] = 0; }
    for (unsigned base = part * 256u; base < qn; base += parts * 256u) {
        const unsigned q = base + threadIdx.x;
        const bool active = q < qn;
        const size_t pix = (size_t)q * PX;
        int cls[PX];
        bool valid[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) { cls[e] = -1; valid[e] = false; }
        if (active) {
            float t[PX];
            if (VEC) {
                const float4 l4 = *reinterpret_cast<const float4*>(lb + pix);
                t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
            } else {
                t[0] = lb[pix];
            }
#pragma unroll
            for (int e = 0; e < PX; ++e) valid[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]) == BCNN_SL_VALID;
        }
#pragma unroll
        for (int k = 0; k < kDlChunk; ++k)
            if (k < kc) {
                if (active) {
                    float v[PX];
                    if (VEC) {
                        const float4 t = *reinterpret_cast<const float4*>(pb + (size_t)k * HW + pix);
                        v[0] = t.x; v[1 % PX] = t.y; v[2 % PX] = t.z; v[3 % PX] = t.w;
                    } else {
                        v[0] = pb[(size_t)k * HW + pix];
                    }
#pragma unroll
                    for (int e = 0; e < PX; ++e) {
                        if (valid[e]) Z[k] += squared ? v[e] * v[e] : v[e];
                        if (cls[e] == c0 + k) I[k] += v[e];
                    }
                }
#pragma unroll
                for (int e = 0; e < PX; ++e) Y[k] += dl_popc(cls[e] == c0 + k);
            }
    }
    __shared__ float sI[4][kDlChunk], sZ[4][kDlChunk];
    __shared__ int sY[4][kDlChunk];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kDlChunk; ++k)
        if (k < kc) {
            float a = I[k], z = Z[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); z += __shfl_xor(z, o); }
            if (lane == 0) { sI[wave][k] = a; sZ[wave][k] = z; sY[wave][k] = Y[k]; }
        }
    __syncthreads();
    if ((int)threadIdx.x < kc) {
        const int k = threadIdx.x;
        float* __restrict__ row = rows + ((size_t)b * parts + part) * 3 * C;
        row[c0 + k] = ((sI[0][k] + sI[1][k]) + sI[2][k]) + sI[3][k];
        row[C + c0 + k] = ((sZ[0][k] + sZ[1][k]) + sZ[2][k]) + sZ[3][k];
        row[2 * C + c0 + k] = __int_as_float(sY[0][k] + sY[1][k] + sY[2][k] + sY[3][k]);
    }
}

// ---- finalize: one workgroup of 16 waves ----------------------------------------------------------------------------------------
// the Dice term of one (group, class) from its sums; 0 where Den == 0 (smooth == 0 and nothing to sum: the limit of the term)
__device__ __forceinline__ double dl_term(double I, double Z, double Y, double s) {
    const double den = Z + Y + s;
    return den > 0.0 ? 1.0 - (2.0 * I + s) / den : 0.0;
}

__global__ __launch_bounds__(64 * kDlFinalWaves) void dl_finalize_kernel(const float* __restrict__ rows, unsigned rows_per_image,
                                                                        unsigned nrows, const double* __restrict__ ploss,
                                                                        const int4* __restrict__ pcnt, int nce, int C, int G,
                                                                        float ce_weight, float dice_weight, float smooth,
                                                                        DlRecord* __restrict__ rec, double* sums,
                                                                        float2* __restrict__ coef) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int GC = G * C;
    const double s = (double)smooth, k = 1.0 / (double)GC;
    for (int gc = wave; gc < GC; gc += kDlFinalWaves) {
        const int g = gc / C, c = gc - g * C;
        const unsigned first = G == 1 ? 0u : (unsigned)g * rows_per_image, count = G == 1 ? nrows : rows_per_image;
        double I = 0.0, Z = 0.0;
        int Y = 0;
        for (unsigned r = lane; r < count; r += 64) {
            const float* __restrict__ row = rows + (size_t)(first + r) * 3 * C;
            I += (double)row[c];
            Z += (double)row[C + c];
            Y += __float_as_int(row[2 * C + c]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            I += __shfl_xor(I, o);
            Z += __shfl_xor(Z, o);
            Y += __shfl_xor(Y, o);
        }
        if (lane == 0) {
            const double den = Z + (double)Y + s;
            sums[3 * (size_t)gc] = I;
            sums[3 * (size_t)gc + 1] = Z;
            sums[3 * (size_t)gc + 2] = (double)Y;
            coef[gc] = den > 0.0 ? make_float2((float)(-2.0 * k / den), (float)((2.0 * I + s) * k / (den * den)))
                                 : make_float2(0.f, 0.f);
        }
    }
    __threadfence_block();
    __syncthreads();
    if (wave != 0) return;
    double d = 0.0, l = 0.0;
    int4 c = make_int4(0, 0, 0, 0);
    for (int gc = lane; gc < GC; gc += 64) d += dl_term(sums[3 * (size_t)gc], sums[3 * (size_t)gc + 1], sums[3 * (size_t)gc + 2], s);
    for (int i = lane; i < nce; i += 64) {
        l += ploss[i];
        const int4 t = pcnt[i];
        c.x += t.x; c.y += t.y; c.z += t.z; c.w += t.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        d += __shfl_xor(d, o);
        l += __shfl_xor(l, o);
        c.x += __shfl_xor(c.x, o);
        c.y += __shfl_xor(c.y, o);
        c.z += __shfl_xor(c.z, o);
        c.w += __shfl_xor(c.w, o);
    }
    if (lane == 0) {
        const double V = c.x > 0 ? (double)c.x : 1.0;
        const double ce = l / V, dice = d * k;
        rec->loss = (float)((double)ce_weight * ce + (double)dice_weight * dice);
        rec->ce = (float)ce;
        rec->dice = (float)dice;
        rec->grad_ce = (float)((double)ce_weight / V);
        rec->valid = c.x;
        rec->ignored = c.y;
        rec->out_of_range = c.z;
        rec->correct = c.w;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// gamma_c = A_c [t = c] + B_c z'(p_c); dx_c (+)= dice_weight * (p_c * (gamma_c - sum_k gamma_k p_k)) + grad_ce * (p_c - [t = c])
// on valid pixels. The workgroup's image fixes the group, so `ab` is one row read through uniform loads. OVERWRITE: every
// element is written, +0.0 where the pixel is not valid; add form: such an element keeps its bits.
__device__ __forceinline__ float dl_gamma(float2 ab, bool target, float pv, int squared) {
    return (target ? ab.x : 0.0f) + ab.y * (squared ? 2.0f * pv : 1.0f);
}

__device__ __forceinline__ float dl_dx(float2 ab, bool target, float pv, float dot, int squared, float dw, float gce) {
    return dw * (pv * (dl_gamma(ab, target, pv, squared) - dot)) + gce * (pv - (target ? 1.0f : 0.0f));
}

// CMAX > 0: the pixel's p in registers (C <= CMAX); CMAX == 0: two sweeps over the classes
template <int CMAX, bool VEC, bool OVERWRITE>
__global__ __launch_bounds__(256) void dl_bwd_kernel(const float* __restrict__ p, const float* __restrict__ label,
                                                     const DlRecord* __restrict__ rec, const float2* __restrict__ coef,
                                                     float* __restrict__ dx, int C, unsigned HW, unsigned qn, unsigned parts,
                                                     const FastDiv dp, int G, int ignore_label, int squared, float dw) {
    constexpr int PX = VEC ? 4 : 1;
    constexpr int CR = CMAX > 0 ? CMAX : 1;
    const unsigned b = fdiv(blockIdx.x, dp), part = blockIdx.x - b * parts;
    const float* __restrict__ pb = p + (size_t)b * C * HW;
    float* __restrict__ db = dx + (size_t)b * C * HW;
    const float* __restrict__ lb = label + (size_t)b * HW;
    const float2* __restrict__ ab = coef + (G == 1 ? (size_t)0 : (size_t)b * C);
    const float gce = rec->grad_ce;
    for (unsigned q = part * 256u + threadIdx.x; q < qn; q += parts * 256u) {
        const size_t pix = (size_t)q * PX;
        float t[PX];
        if (VEC) {
            const float4 l4 = *reinterpret_cast<const float4*>(lb + pix);
            t[0] = l4.x; t[1 % PX] = l4.y; t[2 % PX] = l4.z; t[3 % PX] = l4.w;
        } else {
            t[0] = lb[pix];
        }
        int cls[PX];
        bool valid[PX], any = false;
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            valid[e] = bcnn_softmax_loss_classify(t[e], ignore_label, C, &cls[e]) == BCNN_SL_VALID;
            any = any || valid[e];
        }
        if (!any) {  // nothing to read: the overwrite form clears, the add form leaves the bits
            if (OVERWRITE) {
                for (int c = 0; c < C; ++c) {
                    if (VEC) *reinterpret_cast<float4*>(db + (size_t)c * HW + pix) = make_float4(0.f, 0.f, 0.f, 0.f);
                    else db[(size_t)c * HW + pix] = 0.f;
                }
            }
            continue;
        }
        float v[CR][PX], dot[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) dot[e] = 0.f;
        if (CMAX > 0) {
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) {
                    if (VEC) {
                        const float4 t4 = *reinterpret_cast<const float4*>(pb + (size_t)c * HW + pix);
                        v[c][0] = t4.x; v[c][1 % PX] = t4.y; v[c][2 % PX] = t4.z; v[c][3 % PX] = t4.w;
                    } else {
                        v[c][0] = pb[(size_t)c * HW + pix];
                    }
                }
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) {
                    const float2 k = ab[c];
#pragma unroll
                    for (int e = 0; e < PX; ++e) dot[e] += dl_gamma(k, c == cls[e], v[c][e], squared) * v[c][e];
                }
        } else {
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float2 k = ab[c];
                float w[PX];
                if (VEC) {
                    const float4 t4 = *reinterpret_cast<const float4*>(pb + (size_t)c * HW + pix);
                    w[0] = t4.x; w[1 % PX] = t4.y; w[2 % PX] = t4.z; w[3 % PX] = t4.w;
                } else {
                    w[0] = pb[(size_t)c * HW + pix];
                }
#pragma unroll
                for (int e = 0; e < PX; ++e) dot[e] += dl_gamma(k, c == cls[e], w[e], squared) * w[e];
            }
        }
        // the write sweep: from registers, or p read again (from cache: the lane read these lines a moment ago)
#define DL_BWD_WRITE(PV)                                                                                               \
    {                                                                                                                  \
        const float2 k = ab[c];                                                                                        \
        float out[PX];                                                                                                 \
        if (!OVERWRITE) {                                                                                              \
            if (VEC) {                                                                                                 \
                const float4 o4 = *reinterpret_cast<const float4*>(db + (size_t)c * HW + pix);                         \
                out[0] = o4.x; out[1 % PX] = o4.y; out[2 % PX] = o4.z; out[3 % PX] = o4.w;                             \
            } else {                                                                                                   \
                out[0] = db[(size_t)c * HW + pix];                                                                     \
            }                                                                                                          \
        }                                                                                                              \
        _Pragma("unroll") for (int e = 0; e < PX; ++e) {                                                               \
            const float d = dl_dx(k, c == cls[e], PV[e], dot[e], squared, dw, gce);                                    \
            if (OVERWRITE) out[e] = valid[e] ? d : 0.0f;                                                               \
            else if (valid[e]) out[e] += d;                                                                            \
        }                                                                                                              \
        if (VEC) *reinterpret_cast<float4*>(db + (size_t)c * HW + pix) = make_float4(out[0], out[1 % PX], out[2 % PX], out[3 % PX]); \
        else db[(size_t)c * HW + pix] = out[0];                                                                        \
    }
        if (CMAX > 0) {
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) DL_BWD_WRITE(v[c])
        } else {
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                float w[PX];
                if (VEC) {
                    const float4 t4 = *reinterpret_cast<const float4*>(pb + (size_t)c * HW + pix);
                    w[0] = t4.x; w[1 % PX] = t4.y; w[2 % PX] = t4.z; w[3 % PX] = t4.w;
                } else {
                    w[0] = pb[(size_t)c * HW + pix];
                }
                DL_BWD_WRITE(w)
            }
        }
#undef DL_BWD_WRITE
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int dl_c_reg() {
    const int r = bcnn_hip_softmax_loss_c_reg();
    if (r > kDlReg) {
        fprintf(stderr, "[bcnn_hip] dice_loss: the softmax-loss register limit %d exceeds this file's %d\n", r, kDlReg);
        exit(1);
    }
    return r;
}

static bool dl_shape_ok(int n, int c, int hw) {
    return n >= 1 && c >= 1 && hw >= 1 && (long long)n * c * hw < 0x80000000LL;
}

static int dl_groups(int reduce, int n) {
    return reduce == BCNN_HIP_DICE_REDUCE_BATCH ? 1 : reduce == BCNN_HIP_DICE_REDUCE_IMAGE ? n : 0;
}

// exits like every other entry point handed arguments it cannot run
static void dl_check(const char* who, bool have_args, int n, int c, int hw, int ignore_label, int reduce, float smooth) {
    if (have_args && dl_shape_ok(n, c, hw) && ignore_label < BCNN_SL_MAX_IGNORE_LABEL && dl_groups(reduce, n) > 0 &&
        smooth >= 0.0f && smooth <= FLT_MAX)
        return;
    fprintf(stderr, "[bcnn_hip] %s: an extent below 1, a tensor of 2^31 elements or more, an ignore label of 2^24 or more, an "
                    "unknown reduce or a negative or non-finite smooth\n", who);
    exit(1);
}

// block -> (image, part): parts workgroups per image, as many as the image has 256-lane tiles, capped so that the launch
// stays near kDlGridCap persistent workgroups
struct DlSplit {
    bool vec;
    unsigned qn, parts;
    int grid;
    FastDiv dp;
};
static DlSplit dl_split(int n, int hw, bool vec, int per_image_cap_div) {
    DlSplit s;
    s.vec = vec;
    s.qn = (unsigned)(vec ? hw / 4 : hw);
    const unsigned need = (s.qn + 255u) / 256u;
    const long long per = (long long)n * per_image_cap_div;
    const unsigned cap = per >= kDlGridCap ? 1u : (unsigned)(kDlGridCap / per);
    s.parts = need < cap ? need : cap;
    s.grid = (int)((unsigned)n * s.parts);
    s.dp = make_fdiv(s.parts, (unsigned long long)s.grid);
    return s;
}

struct DlScratch {
    double* ploss;
    int4* pcnt;
    float* rows;
};
// nce cross-entropy partials (doubles first, then the int4 counts, 16-byte aligned: the count rounded up to even), then
// nrows partial rows {I[C], Z[C], Y[C]}
static DlScratch dl_scratch(size_t nce, size_t nrows, int C) {
    const size_t slots = (nce + 1) & ~(size_t)1;
    float* block = scratch(SCRATCH_REDUCE, slots * 6 + nrows * 3 * (size_t)C);
    DlScratch s;
    s.ploss = reinterpret_cast<double*>(block);
    s.pcnt = reinterpret_cast<int4*>(block + slots * 2);
    s.rows = block + slots * 6;
    return s;
}

template <bool VEC>
static void dl_launch_fwd_reg(const DlSplit& sp, const BcnnDiceLossFwdArgs* a, const float* label, const DlScratch& sc) {
#define DL_REG(CMAX)                                                                                                    \
    dl_fwd_reg_kernel<CMAX, VEC><<<sp.grid, 256, 0, current_stream()>>>(a->x, label, a->p, sc.ploss, sc.pcnt, sc.rows, a->c, \
                                                                        (unsigned)a->hw, sp.qn, sp.parts, sp.dp,        \
                                                                        a->ignore_label, a->squared)
    if (a->c <= 4) DL_REG(4);
    else if (a->c <= 8) DL_REG(8);
    else if (a->c <= 16) DL_REG(16);
    else if (a->c <= 24) DL_REG(24);
    else DL_REG(kDlReg);
#undef DL_REG
}

template <bool VEC, bool OVERWRITE>
static void dl_launch_bwd(const DlSplit& sp, const BcnnDiceLossBwdArgs* a, int G, bool reg) {
    const DlRecord* rec = reinterpret_cast<const DlRecord*>(a->workspace);
    const float2* coef = reinterpret_cast<const float2*>(a->workspace + 8 + 6 * (size_t)G * a->c);
#define DL_BWD(CMAX)                                                                                                   \
    dl_bwd_kernel<CMAX, VEC, OVERWRITE><<<sp.grid, 256, 0, current_stream()>>>(a->p, a->label, rec, coef, a->dx, a->c,  \
                                                                               (unsigned)a->hw, sp.qn, sp.parts, sp.dp, G, \
                                                                               a->ignore_label, a->squared, a->dice_weight)
    if (!reg) DL_BWD(0);
    else if (a->c <= 4) DL_BWD(4);
    else if (a->c <= 8) DL_BWD(8);
    else if (a->c <= 16) DL_BWD(16);
    else if (a->c <= 24) DL_BWD(24);
    else DL_BWD(kDlReg);
#undef DL_BWD
}

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_dice_loss_path(int n, int c, int hw, int aligned) {
    (void)aligned;  // alignment selects the 16-byte form of a path, never the path
    if (!dl_shape_ok(n, c, hw)) return -1;
    return (hw > 1 && c <= dl_c_reg()) ? 0 : 1;
}

size_t bcnn_hip_dice_loss_workspace_size(int n, int c, int hw, int reduce) {
    const int G = dl_groups(reduce, n);
    if (!dl_shape_ok(n, c, hw) || G < 1) return 0;
    return 8 + 8 * (size_t)G * c;  // the record, [G][C]{I, Z, Y} doubles, [G][C]{A, B} floats
}

void bcnn_hip_dice_loss_forward(const BcnnDiceLossFwdArgs* a) {
    dl_check("bcnn_hip_dice_loss_forward", a != nullptr, a ? a->n : 0, a ? a->c : 0, a ? a->hw : 0, a ? a->ignore_label : 0,
             a ? a->reduce : 0, a ? a->smooth : 0.f);
    const int n = a->n, C = a->c, hw = a->hw;
    const float* label = a->workspace ? a->label : nullptr;  // statistics need both
    if (label && (reinterpret_cast<uintptr_t>(a->workspace) & 7)) {
        fprintf(stderr, "[bcnn_hip] bcnn_hip_dice_loss_forward: the workspace is not 8-byte aligned\n");
        exit(1);
    }
    const int path = bcnn_hip_dice_loss_path(n, C, hw, 0);
    const bool vec = hw > 1 && (hw & 3) == 0 && al16(a->x) && al16(a->p) && al16(label);
    const DlSplit sp = dl_split(n, hw, vec, 1);
    DlSplit ss = sp;  // the sums launch of the wide path: (image, chunk, part)
    const unsigned chunks = (unsigned)((C + kDlChunk - 1) / kDlChunk);
    const int rows_grid = stream_grid((size_t)n * 64, 256);
    size_t nce = (size_t)sp.grid, nrows = (size_t)sp.grid;
    if (path == 1) {
        ss = dl_split(n, hw, vec, (int)chunks);
        nrows = (size_t)n * ss.parts;
        if (hw == 1) nce = (size_t)rows_grid;
    }
    DlScratch sc = {nullptr, nullptr, nullptr};
    if (label) sc = dl_scratch(nce, nrows, C);
    trace_kernel("dice_loss_fwd");
    if (path == 0) {
        if (vec) dl_launch_fwd_reg<true>(sp, a, label, sc);
        else dl_launch_fwd_reg<false>(sp, a, label, sc);
    } else if (hw == 1) {
        dl_fwd_rows_kernel<<<rows_grid, 256, 0, current_stream()>>>(a->x, label, a->p, sc.ploss, sc.pcnt, C, (unsigned)n,
                                                                    a->ignore_label);
    } else if (vec) {
        dl_fwd_stream_kernel<true><<<sp.grid, 256, 0, current_stream()>>>(a->x, label, a->p, sc.ploss, sc.pcnt, C, (unsigned)hw,
                                                                          sp.qn, sp.parts, sp.dp, a->ignore_label);
    } else {
        dl_fwd_stream_kernel<false><<<sp.grid, 256, 0, current_stream()>>>(a->x, label, a->p, sc.ploss, sc.pcnt, C, (unsigned)hw,
                                                                           sp.qn, sp.parts, sp.dp, a->ignore_label);
    }
    KERNEL_CHECK();
    if (!label) return;
    if (path == 1) {
        trace_kernel("dice_loss_sums");
        const int grid = (int)((unsigned)n * chunks * ss.parts);
        if (vec) dl_sums_kernel<true><<<grid, 256, 0, current_stream()>>>(a->p, label, sc.rows, C, (unsigned)hw, ss.qn, ss.parts, chunks, a->ignore_label, a->squared);
        else dl_sums_kernel<false><<<grid, 256, 0, current_stream()>>>(a->p, label, sc.rows, C, (unsigned)hw, ss.qn, ss.parts, chunks, a->ignore_label, a->squared);
        KERNEL_CHECK();
    }
    const int G = dl_groups(a->reduce, n);
    trace_kernel("dice_loss_finalize");
    dl_finalize_kernel<<<1, 64 * kDlFinalWaves, 0, current_stream()>>>(
        sc.rows, (unsigned)(nrows / (size_t)n), (unsigned)nrows, sc.ploss, sc.pcnt, (int)nce, C, G, a->ce_weight, a->dice_weight,
        a->smooth, reinterpret_cast<DlRecord*>(a->workspace), reinterpret_cast<double*>(a->workspace + 8),
        reinterpret_cast<float2*>(a->workspace + 8 + 6 * (size_t)G * C));
    KERNEL_CHECK();
}

void bcnn_hip_dice_loss_backward(const BcnnDiceLossBwdArgs* a) {
    dl_check("bcnn_hip_dice_loss_backward", a != nullptr && a->workspace && a->label, a ? a->n : 0, a ? a->c : 0, a ? a->hw : 0,
             a ? a->ignore_label : 0, a ? a->reduce : 0, 0.f);
    const int n = a->n, hw = a->hw;
    const bool reg = a->c <= dl_c_reg();  // hw == 1 included: a lane holds its pixel's classes either way
    const bool vec = (hw & 3) == 0 && al16(a->p) && al16(a->dx) && al16(a->label);
    const DlSplit sp = dl_split(n, hw, vec, 1);
    const int G = dl_groups(a->reduce, n);
    trace_kernel("dice_loss_bwd");
    if (vec) { if (a->overwrite) dl_launch_bwd<true, true>(sp, a, G, reg); else dl_launch_bwd<true, false>(sp, a, G, reg); }
    else { if (a->overwrite) dl_launch_bwd<false, true>(sp, a, G, reg); else dl_launch_bwd<false, false>(sp, a, G, reg); }
    KERNEL_CHECK();
}

}  // extern "C"
