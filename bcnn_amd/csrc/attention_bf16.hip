// attention_bf16.hip -- the attention node's forward under bcnn_set_inference_precision(BCNN_PRECISION_BF16), PREDICT / VALID
// mode only. The problem is attention.hip's: per image and head Q [d][Lq], K [d][Lk], V [c][Lk],
// O [c][Lq], S = scale Q^T K, P = softmax_j S, O = V P^T, flash style. The tensors stay fp32 in memory; q, k and v are rounded
// to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) on their way into registers and LDS, the exponentiated tile is rounded to
// bf16 as the operand of the second product, and both products accumulate in fp32 on v_mfma_f32_32x32x16_bf16. The scale, the
// running maximum, the running sum, the rescale of O and the final normalisation are fp32. The running sum l adds the
// UNROUNDED exponentials: the rounding of P then moves o by at most 2^-9 max|v|, and lse = m + log l is an fp32 quantity.
//
// A lane of the bf16 instruction carries 8 consecutive reduction indices of row / column l & 31: k = 8 (l >> 5) .. + 7. The
// result layout is the fp32 instruction's: lane l holds column l & 31 and rows mfma_row(r, l) in register r.
//   Q   : the B operand of S^T = K^T Q, in registers for the whole kernel: d / 16 operands of four dwords, lane l holding
//         Q[16 s + 8 (l >> 5) + e][query l & 31] -- half of what the fp32 kernel keeps
//   K   : LDS, bf16 [key][d + 8]: the A operand of step s is ONE 16-byte read at [key l & 31][16 s + 8 (l >> 5)]
//   S^T : lane l holds query l & 31 and keys 8 b + 4 (l >> 5) + i: maximum and sum are register work plus one exchange with
//         lane l ^ 32. No LDS, no barrier
//   P   : registers 8 s .. 8 s + 7 of the exponentiated tile, packed in pairs, ARE the B operand of step s of O += V P^T; its
//         eight reduction indices are the keys 16 s + 4 (l >> 5) + {0..3} and 16 s + 8 + 4 (l >> 5) + {0..3}
//   V   : LDS, bf16 [channel][keys + 8] with the keys of every 16 stored in that order (bits 2 and 3 of the key index
//         swapped), so the A operand of step s is again one 16-byte read. P never leaves registers
// A workgroup is 4 waves of 32 queries each; a stage of NS * 32 keys goes through LDS double-buffered (the next stage's
// global loads fly over the products), one barrier per stage, one softmax update and one rescale of O per stage. The rescale
// is skipped when no query of the wave moved its maximum (a multiplication by 1.0f: the same bits). LDS rows are padded by
// 16 bytes: the 16 lanes a ds_read_b128 serves per cycle fall on distinct 4-bank slots. d is zero-filled to the K step of
// 16, c to the row tile of 32; keys past Lk are zero in LDS and -inf in S; queries past Lq are not stored.
// No atomics, a fixed summation order: two runs give the same bits; 16-byte or element loads give the same bits.
#include "attention_common.h"

namespace bcnn_hip {

// row[j .. j + 3] of a row of L floats; `ok` false (a row past the matrix) and columns from L on read as zero. vec: L is a
// multiple of 4 and the row 16-byte aligned, and j is a multiple of 4: j < L then holds for all four
__device__ __forceinline__ float4 attn_bf16_load4(const float* base, size_t row_off, int j, int L, bool ok, bool vec) {
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok && j < L) {
        const float* at = base + row_off + j;
        if (vec) {
            val = *reinterpret_cast<const float4*>(at);
        } else {
            val.x = at[0];
            if (j + 1 < L) val.y = at[1];
            if (j + 2 < L) val.z = at[2];
            if (j + 3 < L) val.w = at[3];
        }
    }
    return val;
}

constexpr int attn_bf16_lds_bytes(int dmax, int ct, int ns) {
    return 2 * 2 * (ns * 32 * (dmax + 8) + ct * 32 * (ns * 32 + 8));
}
// keys per stage in units of 32: two where both buffers fit the 64 KiB a workgroup may declare, else one
constexpr int attn_bf16_ns(int dmax, int ct) { return attn_bf16_lds_bytes(dmax, ct, 2) <= 65536 ? 2 : 1; }

// grid: nh * ceil(Lq / 128) workgroups, the query blocks of one (image, head) next to each other.
template <int DMAX, int CT, int NS>
__global__ __launch_bounds__(256, 2) void attn_bf16_fwd_kernel(const float* q, const float* k, const float* v, float* o,
                                                               float* lse, int d, int c, int lq, int lk, int qblocks,
                                                               float scale, int kvec) {
    constexpr int KT = NS * 32;                  // keys per stage
    constexpr int KLD = DMAX + 8, VLD = KT + 8;  // bf16 per LDS row: the data + 16 bytes of padding
    constexpr int QUADS = KT / 4;                // groups of 4 consecutive keys per row of a stage
    constexpr int KU = DMAX * KT / 2048;         // K units of a thread: 2 rows x 4 keys each
    constexpr int VU = CT * KT / 32;             // V units of a thread: 1 row x 4 keys each
    static_assert(KU >= 1 && VU >= 1 && DMAX % 16 == 0, "stage");
    __shared__ __attribute__((aligned(16))) unsigned short ks[2][KT * KLD];       // [key][t]
    __shared__ __attribute__((aligned(16))) unsigned short vs[2][CT * 32 * VLD];  // [channel][permuted key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int nh = blockIdx.x / qblocks;
    const int qi = (blockIdx.x - nh * qblocks) * kAttnBlock + wave * 32 + col;  // this lane's query
    const bool live = qi - col < lq;                                            // (the whole wave)
    const float* kh = k + (size_t)nh * d * lk;
    const float* vh = v + (size_t)nh * c * lk;
    const int nct = (c + 31) >> 5, nk = (lk + KT - 1) / KT;
    const int dpad = (d + 15) & ~15, cpad = nct * 32;

    // Q as the B operand: Q[16 s + 8 half + e][qi], e = 0 .. 7
    bf16x8 qr[DMAX / 16];
    {
        const float* qh = q + (size_t)nh * d * lq;
#pragma unroll
        for (int s = 0; s < DMAX / 16; ++s) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int t = 16 * s + 8 * half + e;
                x[e] = (t < d && qi < lq) ? qh[(size_t)t * lq + qi] : 0.f;
            }
            qr[s] = attn_pack8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
        }
    }
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    // staging: K unit u = (row pair u / QUADS, key quad u % QUADS), V unit u = (row u / QUADS, key quad u % QUADS)
    float4 kreg[KU][2], vreg[VU];
    auto load_stage = [&](int j0) {
#pragma unroll
        for (int p = 0; p < KU; ++p) {
            const int u = tid + 256 * p, j = j0 + (u % QUADS) * 4, t = (u / QUADS) * 2;
            kreg[p][0] = attn_bf16_load4(kh, (size_t)t * lk, j, lk, t < d, kvec);
            kreg[p][1] = attn_bf16_load4(kh, (size_t)(t + 1) * lk, j, lk, t + 1 < d, kvec);
        }
#pragma unroll
        for (int p = 0; p < VU; ++p) {
            const int u = tid + 256 * p, j = j0 + (u % QUADS) * 4, r = u / QUADS;
            vreg[p] = attn_bf16_load4(vh, (size_t)r * lk, j, lk, r < c, kvec);
        }
    };
    auto store_stage = [&](int buf) {
        unsigned* kd = reinterpret_cast<unsigned*>(ks[buf]);  // dword (key, t / 2) at key * (KLD / 2) + t / 2
#pragma unroll
        for (int p = 0; p < KU; ++p) {
            const int u = tid + 256 * p, key = (u % QUADS) * 4, tp = u / QUADS;
            if (2 * tp >= dpad) continue;  // (rows d .. dpad - 1 are zero-filled: the K step)
            unsigned* at = kd + key * (KLD / 2) + tp;
            at[0] = attn_pack_bf16(kreg[p][0].x, kreg[p][1].x);
            at[KLD / 2] = attn_pack_bf16(kreg[p][0].y, kreg[p][1].y);
            at[2 * (KLD / 2)] = attn_pack_bf16(kreg[p][0].z, kreg[p][1].z);
            at[3 * (KLD / 2)] = attn_pack_bf16(kreg[p][0].w, kreg[p][1].w);
        }
#pragma unroll
        for (int p = 0; p < VU; ++p) {
            const int u = tid + 256 * p, quad = u % QUADS, r = u / QUADS;
            if (r >= cpad) continue;  // (rows c .. cpad - 1 are zero-filled: the 32-row A tiles)
            // key 16 a + 8 hi + 4 h + i lies at 16 a + 8 h + 4 hi + i: bits 0 and 1 of the quad index change places
            const int pq = (quad & ~3) | ((quad & 1) << 1) | ((quad >> 1) & 1);
            uint2 w;
            w.x = attn_pack_bf16(vreg[p].x, vreg[p].y);
            w.y = attn_pack_bf16(vreg[p].z, vreg[p].w);
            *reinterpret_cast<uint2*>(&vs[buf][r * VLD + pq * 4]) = w;
        }
    };

    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const unsigned short* kb = ks[kt & 1];
        const unsigned short* vb = vs[kt & 1];
        const int j0 = kt * KT;
        if (kt + 1 < nk) load_stage(j0 + KT);  // the next stage's loads fly over this stage's products
        if (live) {
            f32x16 s[NS];
#pragma unroll
            for (int sub = 0; sub < NS; ++sub) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
#pragma unroll
                for (int t = 0; t < DMAX / 16; ++t) {  // S^T[j][i]: A = K^T, B = Q
                    if (16 * t >= d) break;
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(&kb[(sub * 32 + col) * KLD + 16 * t + 8 * half]);
                    s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qr[t], s[sub], 0, 0, 0);
                }
            }
            const bool ragged = j0 + KT > lk;
            float mx = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < NS; ++sub) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float sv = s[sub][r] * scale;
                    if (ragged && j0 + sub * 32 + mfma_row(r, lane) >= lk) sv = -INFINITY;  // a key past Lk takes no weight
                    s[sub][r] = sv;
                    mx = fmaxf(mx, sv);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mnew = fmaxf(m, mx);          // finite: key j0 is a key of the matrix
            const float alpha = attn_exp(m - mnew);   // 0 on the first stage
            float sum = 0.f;
            bf16x8 pb[NS][2];
#pragma unroll
            for (int sub = 0; sub < NS; ++sub) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[sub][r] = attn_exp(s[sub][r] - mnew);
                    sum += s[sub][r];
                }
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    pb[sub][t] = attn_pack8(s[sub][8 * t], s[sub][8 * t + 1], s[sub][8 * t + 2], s[sub][8 * t + 3],
                                            s[sub][8 * t + 4], s[sub][8 * t + 5], s[sub][8 * t + 6], s[sub][8 * t + 7]);
            }
            sum += __shfl_xor(sum, 32, 64);
            l = l * alpha + sum;
            m = mnew;
            const bool rescale = __any(alpha != 1.0f);  // (per wave)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {  // O[r][i] += V[r][key] P[i][key]
                if (ct >= nct) break;
                if (rescale) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ct][r] *= alpha;
                }
#pragma unroll
                for (int sub = 0; sub < NS; ++sub) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const bf16x8 a =
                            *reinterpret_cast<const bf16x8*>(&vb[(ct * 32 + col) * VLD + sub * 32 + 16 * t + 8 * half]);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb[sub][t], acc[ct], 0, 0, 0);
                    }
                }
            }
        }
        if (kt + 1 < nk) store_stage((kt + 1) & 1);
        __syncthreads();
    }
    if (!live || qi >= lq) return;
    attn_store_acc<CT>(o + (size_t)nh * c * lq, acc, c, lq, qi, lane, 1.0f / l, 1);
    if (lse && half == 0) lse[(size_t)nh * lq + qi] = m + logf(l);
}

struct AttnBf16Fwd {
    const float *q, *k, *v;
    float *o, *lse;
    int nh, d, c, lq, lk, kvec;
    float scale;
    template <int DMAX, int CT>
    void operator()() const {
        const int qblocks = ceil_div(lq, kAttnBlock);
        attn_bf16_fwd_kernel<DMAX, CT, attn_bf16_ns(DMAX, CT)><<<(unsigned)(nh * qblocks), 256, 0, current_stream()>>>(
            q, k, v, o, lse, d, c, lq, lk, qblocks, scale, kvec);
    }
};

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" void bcnn_hip_attention_forward_bf16(const float* q, const float* k, const float* v, float* o, float* lse, int n,
                                                int heads, int d, int c, int lq, int lk, float scale) {
    if (!attn_check("bcnn_hip_attention_forward_bf16", n, heads, d, c, lq, lk)) return;
    const int kvec = (lk & 3) == 0 && al16(k) && al16(v);
    trace_kernel("attention_fwd_bf16");
    attn_dispatch(d, c, AttnBf16Fwd{q, k, v, o, lse, n * heads, d, c, lq, lk, kvec, attn_scale(scale, d)});
    KERNEL_CHECK();
}
