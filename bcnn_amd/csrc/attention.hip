// attention.hip -- the multi-head attention node, forward and backward, on the fp32 matrix cores. No reference counterpart.
// Per image n and head h (nh = n * heads + h), with the positions contiguous (NCHW): Q [d][Lq], K [d][Lk], V [c][Lk], O [c][Lq],
//   S[i][j] = scale * sum_t Q[t][i] K[t][j],  P = softmax_j S,  O[r][i] = sum_j V[r][j] P[i][j].
// Flash style: S and P never reach memory. Every product is v_mfma_f32_32x32x2_f32 (conv_common.h: mfma32), whose result lane l
// holds column l & 31 and rows mfma_row(r, l) in register r, and whose B operand is B[k = l >> 5][n = l & 31]: register r of a
// result tile IS the B operand of step r of the next product, its two k being the tile rows mfma_row(r, 0) and mfma_row(r, 32).
// So the chained operand (P, dS) stays in registers and only the A side of the next product is read from LDS, at the row
// mfma_row(r, l) -- a permutation of the reduction index that costs nothing.
//   forward : a wave owns 32 queries (Q in registers as the B operand), a workgroup of 4 waves 128; key tiles of 32 go through
//             LDS, double-buffered. S^T = K^T Q leaves 16 keys of ONE query in each lane: the online maximum and sum are 16
//             registers and one exchange with lane l ^ 32, no LDS, no barrier. O += V P^T takes P straight from S^T's registers.
//   backward: Dl[i] = sum_r dO[r][i] O[r][i] by a small kernel; then a pass whose workgroups own 128 keys and loop over the
//             query tiles (S = Q^T K and dP = dO^T V have the key in the lane; P feeds dV += dO P, dS feeds dK += Q dS), and a
//             pass whose workgroups own 128 queries and loop over the key tiles (S^T, dP^T; dS^T feeds dQ += K dS^T).
// No atomics; every sum has a fixed order: two runs give the same bits. Tiles are loaded with 16-byte accesses when the row
// length is a multiple of 4 and the pointer is aligned, element by element otherwise: the same values, so the same bits.
#include "attention_common.h"

namespace bcnn_hip {

// This thread's share of the [ROWS][32] tile at column j0 of a [rows][L] matrix: float4 p covers row 32 p + tid / 8, columns
// 4 (tid % 8) .. + 3. Rows from `rows` on and columns from L on read as zero (the MFMA's K step and the ragged last tile).
template <int ROWS>
__device__ __forceinline__ void attn_load(const float* src, int rows, int L, int j0, bool vec, float4 (&reg)[ROWS / 32]) {
    const int j = j0 + (threadIdx.x & 7) * 4;
#pragma unroll
    for (int p = 0; p < ROWS / 32; ++p) {
        const int row = p * 32 + (threadIdx.x >> 3);
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < rows) {
            const float* at = src + (size_t)row * L + j;
            if (vec && j + 3 < L) {
                val = *reinterpret_cast<const float4*>(at);
            } else {
                if (j < L) val.x = at[0];
                if (j + 1 < L) val.y = at[1];
                if (j + 2 < L) val.z = at[2];
                if (j + 3 < L) val.w = at[3];
            }
        }
        reg[p] = val;
    }
}
// into LDS as [row][32]: lane l of a wave then reads 32 consecutive floats of one row
template <int ROWS>
__device__ __forceinline__ void attn_store_rows(float* lds, const float4 (&reg)[ROWS / 32], int rows) {
#pragma unroll
    for (int p = 0; p < ROWS / 32; ++p) {
        if (p * 32 >= rows) break;  // (rows of a pass that is begun are zero-filled: the K step and the 32-row A tiles)
        *reinterpret_cast<float4*>(lds + (p * 32 + (threadIdx.x >> 3)) * 32 + (threadIdx.x & 7) * 4) = reg[p];
    }
}
// into LDS transposed, [column][STRIDE] with STRIDE odd: both a walk along the rows (consecutive addresses) and a walk along
// the columns (stride STRIDE) are free of bank conflicts
template <int ROWS, int STRIDE>
__device__ __forceinline__ void attn_store_cols(float* lds, const float4 (&reg)[ROWS / 32], int rows) {
#pragma unroll
    for (int p = 0; p < ROWS / 32; ++p) {
        if (p * 32 >= rows) break;
        float* at = lds + (threadIdx.x & 7) * 4 * STRIDE + p * 32 + (threadIdx.x >> 3);
        at[0] = reg[p].x;
        at[STRIDE] = reg[p].y;
        at[2 * STRIDE] = reg[p].z;
        at[3 * STRIDE] = reg[p].w;
    }
}

// X[2 s + (l >> 5)][x0 + (l & 31)] for s = 0 .. ceil(rows / 2) - 1: a [rows][32] block as the B operand of `rows / 2` MFMA steps
template <int DIM>
__device__ __forceinline__ void attn_b_operand(const float* src, int rows, int L, int x, int lane, float (&reg)[DIM / 2]) {
#pragma unroll
    for (int s = 0; s < DIM / 2; ++s) {
        const int t = 2 * s + (lane >> 5);
        reg[s] = (t < rows && x < L) ? src[(size_t)t * L + x] : 0.f;
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// grid: nh * ceil(Lq / 128) workgroups, the query blocks of one (image, head) next to each other.
template <int DMAX, int CT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* q, const float* k, const float* v, float* o, float* lse,
                                                       int d, int c, int lq, int lk, int qblocks, float scale, int kvec) {
    constexpr int CS = CT * 32 + 1;
    __shared__ float4 ks4[2][DMAX * 32 / 4];
    __shared__ float vt[2][32 * CS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
    const int nh = blockIdx.x / qblocks;
    const int qi = (blockIdx.x - nh * qblocks) * kAttnBlock + wave * 32 + col;  // this lane's query
    const bool live = qi - col < lq;                                            // (the whole wave)
    const float* kh = k + (size_t)nh * d * lk;
    const float* vh = v + (size_t)nh * c * lk;
    const int nct = (c + 31) >> 5, nk = (lk + 31) >> 5;

    float qr[DMAX / 2];
    attn_b_operand<DMAX>(q + (size_t)nh * d * lq, d, lq, qi, lane, qr);
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    float4 kreg[DMAX / 32], vreg[CT];
    attn_load<DMAX>(kh, d, lk, 0, kvec, kreg);
    attn_load<CT * 32>(vh, c, lk, 0, kvec, vreg);
    attn_store_rows<DMAX>(reinterpret_cast<float*>(ks4[0]), kreg, d);
    attn_store_cols<CT * 32, CS>(vt[0], vreg, c);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const float* ks = reinterpret_cast<const float*>(ks4[kt & 1]);
        const float* vs = vt[kt & 1];
        const int j0 = kt * 32;
        if (kt + 1 < nk) {  // the next tile's loads fly over this tile's products
            attn_load<DMAX>(kh, d, lk, j0 + 32, kvec, kreg);
            attn_load<CT * 32>(vh, c, lk, j0 + 32, kvec, vreg);
        }
        if (live) {
            f32x16 s;
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int t = 0; t < DMAX / 2; ++t)  // S^T[j][i]: A = K[2 t + half][j0 + col], B = Q
                if (2 * t < d) s = mfma32(ks[(2 * t + half) * 32 + col], qr[t], s);
            const bool ragged = j0 + 32 > lk;
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float sv = s[r] * scale;
                if (ragged && j0 + mfma_row(r, lane) >= lk) sv = -INFINITY;  // a key past Lk takes no weight (0 would)
                s[r] = sv;
                mx = fmaxf(mx, sv);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mnew = fmaxf(m, mx);
            const float alpha = attn_exp(m - mnew);  // 0 on the first tile
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = attn_exp(s[r] - mnew);
                sum += s[r];
            }
            sum += __shfl_xor(sum, 32, 64);
            l = l * alpha + sum;
            m = mnew;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {  // O[r][i] += V[r][key] P[i][key], key = mfma_row(step, lane): P is s as it lies
                if (ct >= nct) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct] = mfma32(vs[mfma_row(r, lane) * CS + ct * 32 + col], s[r], acc[ct]);
            }
        }
        if (kt + 1 < nk) {
            attn_store_rows<DMAX>(reinterpret_cast<float*>(ks4[(kt + 1) & 1]), kreg, d);
            attn_store_cols<CT * 32, CS>(vt[(kt + 1) & 1], vreg, c);
        }
        __syncthreads();
    }
    if (!live || qi >= lq) return;
    attn_store_acc<CT>(o + (size_t)nh * c * lq, acc, c, lq, qi, lane, 1.0f / l, 1);
    if (lse && half == 0) lse[(size_t)nh * lq + qi] = m + logf(l);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_dl_kernel(const float* dout, const float* o, float* dl, int c, int lq,
                                                      long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long nh = idx / lq;
    const size_t base = (size_t)nh * c * lq + (size_t)(idx - nh * lq);
    float sum = 0.f;
    // the MFMA's own chain (fused, ascending r): with one key, where o == v, Dl has the bits of dP and dS is exactly zero
    for (int r = 0; r < c; ++r) sum = fmaf(dout[base + (size_t)r * lq], o[base + (size_t)r * lq], sum);
    dl[idx] = sum;
}

// dK and dV: a wave owns 32 keys (K and V in registers as B operands), the workgroup's 4 waves share the query tiles.
// grid: nh * ceil(Lk / 128).
template <int DMAX, int CT>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* q, const float* k, const float* v, const float* lse,
                                                          const float* dl, const float* dout, float* dk, float* dv, int d,
                                                          int c, int lq, int lk, int kblocks, float scale, int qvec,
                                                          int overwrite_k, int overwrite_v) {
    constexpr int DS = DMAX + 1, CS = CT * 32 + 1;
    __shared__ float qt[32 * DS];    // Q tile, [query][t]
    __shared__ float dot[32 * CS];   // dO tile, [query][r]
    __shared__ float lse_s[32], dl_s[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
    const int nh = blockIdx.x / kblocks;
    const int kj = (blockIdx.x - nh * kblocks) * kAttnBlock + wave * 32 + col;  // this lane's key
    const bool live = kj - col < lk;
    const float* qh = q + (size_t)nh * d * lq;
    const float* doh = dout + (size_t)nh * c * lq;
    const int nct = (c + 31) >> 5, ndt = (d + 31) >> 5, nq = (lq + 31) >> 5;

    float kr[DMAX / 2], vr[CT * 16];
    attn_b_operand<DMAX>(k + (size_t)nh * d * lk, d, lk, kj, lane, kr);
    attn_b_operand<CT * 32>(v + (size_t)nh * c * lk, c, lk, kj, lane, vr);
    f32x16 acck[DMAX / 32], accv[CT];
#pragma unroll
    for (int t = 0; t < DMAX / 32; ++t)
        for (int r = 0; r < 16; ++r) acck[t][r] = 0.f;
#pragma unroll
    for (int t = 0; t < CT; ++t)
        for (int r = 0; r < 16; ++r) accv[t][r] = 0.f;

    for (int it = 0; it < nq; ++it) {
        const int i0 = it * 32;
        float4 qreg[DMAX / 32], dreg[CT];
        attn_load<DMAX>(qh, d, lq, i0, qvec, qreg);
        attn_load<CT * 32>(doh, c, lq, i0, qvec, dreg);
        __syncthreads();  // the previous tile's readers are done
        attn_store_cols<DMAX, DS>(qt, qreg, d);
        attn_store_cols<CT * 32, CS>(dot, dreg, c);
        if (threadIdx.x < 32) {  // a query past Lq: lse = +inf makes its P, and with it its dS, zero
            const bool in = i0 + (int)threadIdx.x < lq;
            lse_s[threadIdx.x] = in ? lse[(size_t)nh * lq + i0 + threadIdx.x] : INFINITY;
            dl_s[threadIdx.x] = in ? dl[(size_t)nh * lq + i0 + threadIdx.x] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        f32x16 s, dp;
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int t = 0; t < DMAX / 2; ++t) {  // S[i][j]: A = Q[2 t + half][i0 + col], B = K
            if (2 * t >= d) break;
            s = mfma32(qt[col * DS + 2 * t + half], kr[t], s);
        }
#pragma unroll
        for (int t = 0; t < CT * 16; ++t) {  // dP[i][j]: A = dO[2 t + half][i0 + col], B = V
            if (2 * t >= c) break;
            dp = mfma32(dot[col * CS + 2 * t + half], vr[t], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = mfma_row(r, lane);
            s[r] = attn_exp(s[r] * scale - lse_s[i]);  // P
            dp[r] = s[r] * (dp[r] - dl_s[i]);          // dS
        }
        if (dv) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {  // dV[r][j] += dO[r][query] P[query][j]
                if (ct >= nct) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) accv[ct] = mfma32(dot[mfma_row(r, lane) * CS + ct * 32 + col], s[r], accv[ct]);
            }
        }
        if (dk) {
#pragma unroll
            for (int dt = 0; dt < DMAX / 32; ++dt) {  // dK[t][j] += Q[t][query] dS[query][j]
                if (dt >= ndt) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) acck[dt] = mfma32(qt[mfma_row(r, lane) * DS + dt * 32 + col], dp[r], acck[dt]);
            }
        }
    }
    if (!live) return;
    if (dk) attn_store_acc<DMAX / 32>(dk + (size_t)nh * d * lk, acck, d, lk, kj, lane, scale, overwrite_k);
    if (dv) attn_store_acc<CT>(dv + (size_t)nh * c * lk, accv, c, lk, kj, lane, 1.0f, overwrite_v);
}

// dQ: a wave owns 32 queries (Q and dO in registers as B operands), the workgroup's 4 waves share the key tiles.
// grid: nh * ceil(Lq / 128).
template <int DMAX, int CT>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* q, const float* k, const float* v, const float* lse,
                                                         const float* dl, const float* dout, float* dq, int d, int c, int lq,
                                                         int lk, int qblocks, float scale, int kvec, int overwrite_q) {
    constexpr int DS = DMAX + 1;
    __shared__ float kt_s[32 * DS];             // K tile, [key][t]
    __shared__ float4 vs4[CT * 32 * 32 / 4];    // V tile, [r][key]
    float* vs = reinterpret_cast<float*>(vs4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
    const int nh = blockIdx.x / qblocks;
    const int qi = (blockIdx.x - nh * qblocks) * kAttnBlock + wave * 32 + col;
    const bool live = qi - col < lq;
    const float* kh = k + (size_t)nh * d * lk;
    const float* vh = v + (size_t)nh * c * lk;
    const int ndt = (d + 31) >> 5, nk = (lk + 31) >> 5;

    float qr[DMAX / 2], dor[CT * 16];
    attn_b_operand<DMAX>(q + (size_t)nh * d * lq, d, lq, qi, lane, qr);
    attn_b_operand<CT * 32>(dout + (size_t)nh * c * lq, c, lq, qi, lane, dor);
    const float lse_i = qi < lq ? lse[(size_t)nh * lq + qi] : 0.f;
    const float dl_i = qi < lq ? dl[(size_t)nh * lq + qi] : 0.f;
    f32x16 acc[DMAX / 32];
#pragma unroll
    for (int t = 0; t < DMAX / 32; ++t)
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int kt = 0; kt < nk; ++kt) {
        const int j0 = kt * 32;
        float4 kreg[DMAX / 32], vreg[CT];
        attn_load<DMAX>(kh, d, lk, j0, kvec, kreg);
        attn_load<CT * 32>(vh, c, lk, j0, kvec, vreg);
        __syncthreads();
        attn_store_cols<DMAX, DS>(kt_s, kreg, d);
        attn_store_rows<CT * 32>(vs, vreg, c);
        __syncthreads();
        if (!live) continue;
        f32x16 s, dp;
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int t = 0; t < DMAX / 2; ++t) {  // S^T[j][i]: A = K[2 t + half][j0 + col], B = Q
            if (2 * t >= d) break;
            s = mfma32(kt_s[col * DS + 2 * t + half], qr[t], s);
        }
#pragma unroll
        for (int t = 0; t < CT * 16; ++t) {  // dP^T[j][i]: A = V[2 t + half][j0 + col], B = dO
            if (2 * t >= c) break;
            dp = mfma32(vs[(2 * t + half) * 32 + col], dor[t], dp);
        }
        const bool ragged = j0 + 32 > lk;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p = attn_exp(s[r] * scale - lse_i);
            if (ragged && j0 + mfma_row(r, lane) >= lk) p = 0.f;
            dp[r] = p * (dp[r] - dl_i);  // dS^T
        }
#pragma unroll
        for (int dt = 0; dt < DMAX / 32; ++dt) {  // dQ[t][i] += K[t][key] dS[i][key]
            if (dt >= ndt) break;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[dt] = mfma32(kt_s[mfma_row(r, lane) * DS + dt * 32 + col], dp[r], acc[dt]);
        }
    }
    if (!live) return;
    attn_store_acc<DMAX / 32>(dq + (size_t)nh * d * lq, acc, d, lq, qi, lane, scale, overwrite_q);
}

struct AttnArgs {
    const float *q, *k, *v, *lse, *dl, *dout;
    float *out, *lse_out, *dq, *dk, *dv;
    int nh, d, c, lq, lk, qvec, kvec, ow_q, ow_k, ow_v;
    float scale;
};
struct AttnFwd {
    AttnArgs a;
    template <int DMAX, int CT>
    void operator()() const {
        const int qblocks = ceil_div(a.lq, kAttnBlock);
        attn_fwd_kernel<DMAX, CT><<<(unsigned)(a.nh * qblocks), 256, 0, current_stream()>>>(
            a.q, a.k, a.v, a.out, a.lse_out, a.d, a.c, a.lq, a.lk, qblocks, a.scale, a.kvec);
    }
};
struct AttnBwdKV {
    AttnArgs a;
    template <int DMAX, int CT>
    void operator()() const {
        const int kblocks = ceil_div(a.lk, kAttnBlock);
        attn_bwd_kv_kernel<DMAX, CT><<<(unsigned)(a.nh * kblocks), 256, 0, current_stream()>>>(
            a.q, a.k, a.v, a.lse, a.dl, a.dout, a.dk, a.dv, a.d, a.c, a.lq, a.lk, kblocks, a.scale, a.qvec, a.ow_k, a.ow_v);
    }
};
struct AttnBwdQ {
    AttnArgs a;
    template <int DMAX, int CT>
    void operator()() const {
        const int qblocks = ceil_div(a.lq, kAttnBlock);
        attn_bwd_q_kernel<DMAX, CT><<<(unsigned)(a.nh * qblocks), 256, 0, current_stream()>>>(
            a.q, a.k, a.v, a.lse, a.dl, a.dout, a.dq, a.d, a.c, a.lq, a.lk, qblocks, a.scale, a.kvec, a.ow_q);
    }
};

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

size_t bcnn_hip_attention_lse_size(int n, int heads, int lq) {
    return (n <= 0 || heads <= 0 || lq <= 0) ? 0 : (size_t)n * (size_t)heads * (size_t)lq;
}

void bcnn_hip_attention_forward(const float* q, const float* k, const float* v, float* o, float* lse, int n, int heads,
                                int d, int c, int lq, int lk, float scale) {
    if (!attn_check("bcnn_hip_attention_forward", n, heads, d, c, lq, lk)) return;
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.out = o; a.lse_out = lse;
    a.nh = n * heads; a.d = d; a.c = c; a.lq = lq; a.lk = lk;
    a.kvec = (lk & 3) == 0 && al16(k) && al16(v);
    a.scale = attn_scale(scale, d);
    trace_kernel("attention_fwd");
    attn_dispatch(d, c, AttnFwd{a});
    KERNEL_CHECK();
}

void bcnn_hip_attention_backward(const float* q, const float* k, const float* v, const float* o, const float* lse,
                                 const float* dout, float* dq, float* dk, float* dv, int n, int heads, int d, int c, int lq,
                                 int lk, float scale, int overwrite_q, int overwrite_k, int overwrite_v) {
    if (!attn_check("bcnn_hip_attention_backward", n, heads, d, c, lq, lk) || (!dq && !dk && !dv)) return;
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.lse = lse; a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv;
    a.nh = n * heads; a.d = d; a.c = c; a.lq = lq; a.lk = lk;
    a.qvec = (lq & 3) == 0 && al16(q) && al16(dout);
    a.kvec = (lk & 3) == 0 && al16(k) && al16(v);
    a.ow_q = overwrite_q; a.ow_k = overwrite_k; a.ow_v = overwrite_v;
    a.scale = attn_scale(scale, d);
    const long long rows = (long long)a.nh * lq;
    float* dl = scratch(SCRATCH_REDUCE, (size_t)rows);
    a.dl = dl;
    trace_kernel("attention_bwd:dl");
    attn_dl_kernel<<<(unsigned)ceil_div(rows, 256), 256, 0, current_stream()>>>(dout, o, dl, c, lq, rows);
    KERNEL_CHECK();
    if (dk || dv) {  // first: with q, k and v one tensor, the three gradients add up in one buffer, one launch after the other
        trace_kernel("attention_bwd:kv");
        attn_dispatch(d, c, AttnBwdKV{a});
        KERNEL_CHECK();
    }
    if (dq) {
        trace_kernel("attention_bwd:q");
        attn_dispatch(d, c, AttnBwdQ{a});
        KERNEL_CHECK();
    }
}

}  // extern "C"
