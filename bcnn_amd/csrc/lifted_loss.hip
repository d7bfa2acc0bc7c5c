// lifted_loss.hip -- the lifted-structure loss of the cost node (Song et al., "Deep Metric Learning via Lifted Structured
// Feature Embedding") on the device. The reference computes it on the host, in its CUDA build too
// (bcnn_lifted_structure_loss.c:16-298): for every positive pair it walks every negative of both anchors with a K-wide
// axpy each, O(P B K) for P pairs. The soft maximum of a pair depends on its anchors only through the row sums
//   S_i = sum_{k: cls_k != cls_i} exp(margin - D_ik),
// so the triple loop collapses to O(B^2) element work plus two GEMM-shaped products (formulas in include/bcnn_hip.h):
//
//   lifted_prep_kernel      cls_i = first label entry > 0 of row i (-1: none), |x_i|^2                       B blocks
//   lifted_gram_kernel      x x^T on v_mfma_f32_32x32x2_f32; the epilogue turns a 64 x 64 tile into D and adds the masked
//                           exp(margin - D) down the tile's columns (the Gram matrix is symmetric: a column sum over all
//                           row tiles is S). Only D reaches memory, plus one partial sum per (row tile, column).
//                           32x32x2 because its result layout puts 16 rows of ONE column into a lane: the column sum
//                           is a chain of in-lane adds and one 4-way exchange through LDS.
//   lifted_dist_kernel      K < 32 instead of the Gram product: D_ij^2 = sum_k (x_ik - x_jk)^2. |x_i|^2 + |x_j|^2 - 2 x_i.x_j
//                           loses every digit of a small distance to cancellation, and in few dimensions a batch holds
//                           close pairs (K = 1: |x_i - x_j| ~ 1e-5 among 1024 samples) whose gradient 2 L (x_i - x_j) / D
//                           is not small.
//   lifted_colsum_kernel    S_j = the partial sums of the row tiles, added in tile order
//   lifted_pair_kernel      one block per row i: L_ij, T_i, the row's share of the loss and of P, and D_ij replaced IN PLACE by
//                           W_ij = 2 L_ij / (D_ij + 1e-10) (positive pair), -exp(margin - D_ij) / D_ij (negative pair), 0 (i == j).
//                           It needs complete S, hence its own launch.
//   lifted_grad_kernel      g = diag(rowsum(A)) x - A x on the same MFMA, A_ij = W_ij (positive) or W_ij (T_i + T_j) (negative)
//                           generated while the A tile is staged; the row sums are added up by the staging threads.
//   lifted_grad_small_kernel K < 32: g_i = sum_j A_ij (x_i - x_j), the same cancellation argument.
//   lifted_final_kernel     loss = sum L^2 / P and P into the 8-byte device record.
//   lifted_scale_kernel     the node's backward: g *= scale / P with P read on the device.
// No atomics; every sum has an order fixed by (B, K) alone, so two runs give the same bits, and nothing is read from
// the workspace before this call wrote it.
#include "conv_common.h"

namespace bcnn_hip {

namespace {

constexpr int kLsTile = 64;    // tile edge of both MFMA products: 2 x 2 waves, one 32 x 32 accumulator each
constexpr int kLsBK = 16;      // reduction rows per LDS stage
constexpr int kLsSmallK = 32;  // below: the difference-form kernels

inline size_t ls_pad(size_t n) { return (n + 3) & ~(size_t)3; }
inline int ls_tiles(int B) { return (B + kLsTile - 1) / kLsTile; }

// workspace: cls | |x|^2 | S | T | row loss | row pairs | column partials [tiles][Bp] | D, then W  [B][B]
struct LsWs {
    int* cls;
    float *sq, *S, *T, *lrow, *prow, *spart, *W;
    size_t Bp;
};
inline LsWs ls_carve(float* ws, int B) {
    LsWs r;
    r.Bp = ls_pad((size_t)B);
    r.cls = reinterpret_cast<int*>(ws);
    r.sq = ws + r.Bp;
    r.S = ws + 2 * r.Bp;
    r.T = ws + 3 * r.Bp;
    r.lrow = ws + 4 * r.Bp;
    r.prow = ws + 5 * r.Bp;
    r.spart = ws + 6 * r.Bp;
    r.W = r.spart + (size_t)ls_tiles(B) * r.Bp;
    return r;
}

__global__ __launch_bounds__(256) void lifted_prep_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                          int K, int* __restrict__ cls, float* __restrict__ sq) {
    __shared__ int first[256];
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (size_t)i * K;
    const float* lr = label + (size_t)i * K;
    float s = 0.f;
    int f = 0x7fffffff;
    for (int k = tid; k < K; k += 256) {
        s += xr[k] * xr[k];
        if (lr[k] > 0.0f && k < f) f = k;
    }
    first[tid] = f;
    const float tot = block_sum(s, red);  // synchronises after the store above
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) first[tid] = min(first[tid], first[tid + w]);
        __syncthreads();
    }
    if (tid == 0) {
        sq[i] = tot;
        cls[i] = first[0] == 0x7fffffff ? -1 : first[0];
    }
}

// A 64 x 64 tile of distances in the MFMA result layout -> D to memory, masked exp column sums to spart[row tile][column].
// `d` holds the 16 rows mfma_row(q, lane) of column l31 of the wave's 32 x 32 quadrant (wm, wn).
__device__ __forceinline__ void ls_tile_epilogue(const float (&d)[16], int i0, int j0, int wm, int wn, int lane, int B,
                                                 float margin, const int* __restrict__ cls, float* __restrict__ D,
                                                 float* __restrict__ spart_row, float (*red)[kLsTile]) {
    const int l31 = lane & 31, lhi = lane >> 5;
    const int col = j0 + wn * 32 + l31;
    const bool cv = col < B;
    const int ccol = cv ? cls[col] : 0;
    float colsum = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = i0 + wm * 32 + mfma_row(q, lane);
        if (cv && row < B) {
            D[(size_t)row * B + col] = d[q];
            if (cls[row] != ccol) colsum += expf(margin - d[q]);
        }
    }
    red[wm * 2 + lhi][wn * 32 + l31] = colsum;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kLsTile && j0 + t < B) spart_row[j0 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void lifted_gram_kernel(const float* __restrict__ x, int B, int K, float margin,
                                                          const int* __restrict__ cls, const float* __restrict__ sq,
                                                          float* __restrict__ D, float* __restrict__ spart, int Bp) {
    constexpr int BK = kLsBK, T = kLsTile, R = T * BK / 256;
    __shared__ float As[2][BK][T + 1];
    __shared__ float Bs[2][BK][T + 1];
    __shared__ float red[4][T];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, l31 = lane & 31, lhi = lane >> 5;
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const int s_k = tid % BK, s_r = tid / BK;  // staging: 16 consecutive k of one row per 16 threads
    const int nsteps = (K + BK - 1) / BK;

    float ra[R], rb[R];
    auto load = [&](int st) {
        const int k = st * BK + s_k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ia = i0 + s_r + 16 * r, ib = j0 + s_r + 16 * r;
            ra[r] = (k < K && ia < B) ? x[(size_t)ia * K + k] : 0.f;
            rb[r] = (k < K && ib < B) ? x[(size_t)ib * K + k] : 0.f;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            As[buf][s_k][s_r + 16 * r] = ra[r];
            Bs[buf][s_k][s_r + 16 * r] = rb[r];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    load(0);
    store(0);
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if (st + 1 < nsteps) load(st + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks)
            acc = mfma32(As[cur][2 * ks + lhi][wm * 32 + l31], Bs[cur][2 * ks + lhi][wn * 32 + l31], acc);
        if (st + 1 < nsteps) store(cur ^ 1);
        __syncthreads();
    }
    const int col = j0 + wn * 32 + l31;
    const float sqc = col < B ? sq[col] : 0.f;
    float d[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = i0 + wm * 32 + mfma_row(q, lane);
        const float sqr = row < B ? sq[row] : 0.f;
        const float d2 = (sqr + sqc) - 2.0f * acc[q];
        d[q] = row == col ? 0.f : sqrtf(fmaxf(d2, 0.f));
    }
    ls_tile_epilogue(d, i0, j0, wm, wn, lane, B, margin, cls, D, spart + (size_t)blockIdx.y * Bp, red);
}

// K < kLsSmallK: the same tile and the same result layout from differences.
__global__ __launch_bounds__(256) void lifted_dist_kernel(const float* __restrict__ x, int B, int K, float margin,
                                                          const int* __restrict__ cls, float* __restrict__ D,
                                                          float* __restrict__ spart, int Bp) {
    constexpr int T = kLsTile;
    __shared__ float xi[T][kLsSmallK + 1];
    __shared__ float xj[T][kLsSmallK + 1];
    __shared__ float red[4][T];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, l31 = lane & 31;
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    for (int e = tid; e < T * K; e += 256) {
        const int r = e / K, k = e - r * K;
        xi[r][k] = i0 + r < B ? x[(size_t)(i0 + r) * K + k] : 0.f;
        xj[r][k] = j0 + r < B ? x[(size_t)(j0 + r) * K + k] : 0.f;
    }
    __syncthreads();
    float d[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = wm * 32 + mfma_row(q, lane), c = wn * 32 + l31;
        float d2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float t = xi[r][k] - xj[c][k];
            d2 += t * t;
        }
        d[q] = sqrtf(d2);
    }
    ls_tile_epilogue(d, i0, j0, wm, wn, lane, B, margin, cls, D, spart + (size_t)blockIdx.y * Bp, red);
}

__global__ __launch_bounds__(256) void lifted_colsum_kernel(const float* __restrict__ spart, int B, int Bp, int tiles,
                                                            float* __restrict__ S) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= B) return;
    float s = 0.f;
    for (int t = 0; t < tiles; ++t) s += spart[(size_t)t * Bp + j];
    S[j] = s;
}

__global__ __launch_bounds__(256) void lifted_pair_kernel(int B, float margin, const int* __restrict__ cls,
                                                          const float* __restrict__ S, float* __restrict__ W,
                                                          float* __restrict__ T, float* __restrict__ lrow,
                                                          float* __restrict__ prow) {
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int ci = cls[i];
    const float si = S[i];
    float* wr = W + (size_t)i * B;
    float t = 0.f, l2 = 0.f, np = 0.f;
    for (int j = tid; j < B; j += 256) {
        const float d = wr[j];
        float w = 0.f;
        if (j != i) {
            if (cls[j] == ci) {
                const float s = si + S[j];
                const float L = s > 0.f ? fmaxf(0.f, logf(s) + d) : 0.f;
                w = 2.0f * L / (d + 1e-10f);
                if (s > 0.f) t += 2.0f * L / s;
                if (j > i) {
                    l2 += L * L;
                    np += 1.0f;
                }
            } else {
                w = -expf(margin - d) / d;
            }
        }
        wr[j] = w;
    }
    t = block_sum(t, red);
    l2 = block_sum(l2, red);
    np = block_sum(np, red);
    if (tid == 0) {
        T[i] = t;
        lrow[i] = l2;
        prow[i] = np;
    }
}

template <bool ACC>
__global__ __launch_bounds__(256) void lifted_grad_kernel(const float* __restrict__ x, int B, int K,
                                                          const int* __restrict__ cls, const float* __restrict__ Tn,
                                                          const float* __restrict__ W, float* __restrict__ g) {
    constexpr int BK = kLsBK, T = kLsTile, R = T * BK / 256;
    __shared__ float As[2][BK][T + 1];
    __shared__ float Bs[2][BK][T + 1];
    __shared__ float rsum[4][T];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, l31 = lane & 31, lhi = lane >> 5;
    const int i0 = blockIdx.y * T, c0 = blockIdx.x * T;
    // staging: thread -> (row i or column c = tid % 64, reduction index j = wid + 4 r); W is symmetric, so A_ij is read
    // as W[j][i], consecutive along the threads
    const int s_e = tid & 63;
    const int i = i0 + s_e, c = c0 + s_e;
    const bool iv = i < B, cv = c < K;
    const int ci = iv ? cls[i] : 0;
    const float ti = iv ? Tn[i] : 0.f;
    const int nsteps = (B + BK - 1) / BK;

    float ra[R], rb[R], rs = 0.f;
    auto load = [&](int st) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = st * BK + wid + 4 * r;
            float a = 0.f;
            if (iv && j < B) {
                a = W[(size_t)j * B + i];
                if (cls[j] != ci) a *= ti + Tn[j];
            }
            ra[r] = a;
            rs += a;
            rb[r] = (cv && j < B) ? x[(size_t)j * K + c] : 0.f;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            As[buf][wid + 4 * r][s_e] = ra[r];
            Bs[buf][wid + 4 * r][s_e] = rb[r];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    load(0);
    store(0);
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if (st + 1 < nsteps) load(st + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks)
            acc = mfma32(As[cur][2 * ks + lhi][wm * 32 + l31], Bs[cur][2 * ks + lhi][wn * 32 + l31], acc);
        if (st + 1 < nsteps) store(cur ^ 1);
        __syncthreads();
    }
    rsum[wid][s_e] = rs;
    __syncthreads();
    const int col = c0 + wn * 32 + l31;
    if (col >= K) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rl = wm * 32 + mfma_row(q, lane), row = i0 + rl;
        if (row >= B) continue;
        const float rsm = ((rsum[0][rl] + rsum[1][rl]) + rsum[2][rl]) + rsum[3][rl];
        const size_t e = (size_t)row * K + col;
        const float v = rsm * x[e] - acc[q];
        g[e] = ACC ? g[e] + v : v;
    }
}

// K < kLsSmallK: one block per row i, thread j-strided, g_ik = sum_j A_ij (x_ik - x_jk) in registers.
template <bool ACC>
__global__ __launch_bounds__(256) void lifted_grad_small_kernel(const float* __restrict__ x, int B, int K,
                                                                const int* __restrict__ cls, const float* __restrict__ Tn,
                                                                const float* __restrict__ W, float* __restrict__ g) {
    constexpr int KM = kLsSmallK;
    __shared__ float part[4][KM];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ci = cls[i];
    const float ti = Tn[i];
    float xi[KM], acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        xi[k] = k < K ? x[(size_t)i * K + k] : 0.f;
        acc[k] = 0.f;
    }
    for (int j = tid; j < B; j += 256) {
        float a = W[(size_t)i * B + j];
        if (cls[j] != ci) a *= ti + Tn[j];
        const float* xj = x + (size_t)j * K;
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) acc[k] += a * (xi[k] - xj[k]);
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) part[wid][k] = s;
    }
    __syncthreads();
    if (tid < K) {
        const float v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        const size_t e = (size_t)i * K + tid;
        g[e] = ACC ? g[e] + v : v;
    }
}

__global__ __launch_bounds__(256) void lifted_final_kernel(const float* __restrict__ lrow, const float* __restrict__ prow,
                                                           int B, bcnn_hip_lifted_struct_record* __restrict__ rec) {
    __shared__ double sl[256], sp[256];
    const int tid = threadIdx.x;
    double l = 0.0, p = 0.0;
    for (int i = tid; i < B; i += 256) {
        l += (double)lrow[i];
        p += (double)prow[i];
    }
    sl[tid] = l;
    sp[tid] = p;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sl[tid] += sl[tid + w];
            sp[tid] += sp[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        rec->loss = sp[0] > 0.0 ? (float)(sl[0] / sp[0]) : 0.f;
        rec->num_constraints = (int)sp[0];
    }
}

__global__ __launch_bounds__(256) void lifted_scale_kernel(float* __restrict__ g, size_t n, float scale,
                                                           const bcnn_hip_lifted_struct_record* __restrict__ rec) {
    const int P = rec->num_constraints;
    const float alpha = P > 0 ? scale / (float)P : 0.f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) g[e] *= alpha;
}

}  // namespace

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" size_t bcnn_hip_lifted_struct_workspace_size(int batch, int k) {
    (void)k;
    if (batch < 1) return 0;
    const size_t Bp = ls_pad((size_t)batch);
    return (6 + (size_t)ls_tiles(batch)) * Bp + (size_t)batch * batch;
}

extern "C" void bcnn_hip_lifted_struct_forward(const float* x_d, const float* label_d, float* g_d, int batch, int k,
                                               float margin, int accumulate, bcnn_hip_lifted_struct_record* record_d,
                                               float* workspace_d) {
    if (batch < 1 || k < 1) return;
    const int B = batch, K = k, tiles = ls_tiles(B);
    const LsWs w = ls_carve(workspace_d, B);
    hipStream_t st = current_stream();
    trace_kernel("lifted_struct_forward");
    lifted_prep_kernel<<<B, 256, 0, st>>>(x_d, label_d, K, w.cls, w.sq);
    const dim3 tgrid(tiles, tiles);
    if (K < kLsSmallK)
        lifted_dist_kernel<<<tgrid, 256, 0, st>>>(x_d, B, K, margin, w.cls, w.W, w.spart, (int)w.Bp);
    else
        lifted_gram_kernel<<<tgrid, 256, 0, st>>>(x_d, B, K, margin, w.cls, w.sq, w.W, w.spart, (int)w.Bp);
    lifted_colsum_kernel<<<ceil_div(B, 256), 256, 0, st>>>(w.spart, B, (int)w.Bp, tiles, w.S);
    lifted_pair_kernel<<<B, 256, 0, st>>>(B, margin, w.cls, w.S, w.W, w.T, w.lrow, w.prow);
    if (K < kLsSmallK) {
        if (accumulate) lifted_grad_small_kernel<true><<<B, 256, 0, st>>>(x_d, B, K, w.cls, w.T, w.W, g_d);
        else lifted_grad_small_kernel<false><<<B, 256, 0, st>>>(x_d, B, K, w.cls, w.T, w.W, g_d);
    } else {
        const dim3 ggrid(ceil_div(K, kLsTile), tiles);
        if (accumulate) lifted_grad_kernel<true><<<ggrid, 256, 0, st>>>(x_d, B, K, w.cls, w.T, w.W, g_d);
        else lifted_grad_kernel<false><<<ggrid, 256, 0, st>>>(x_d, B, K, w.cls, w.T, w.W, g_d);
    }
    lifted_final_kernel<<<1, 256, 0, st>>>(w.lrow, w.prow, B, record_d);
    KERNEL_CHECK();
}

extern "C" void bcnn_hip_lifted_struct_backward(float* g_d, int batch, int k, float scale,
                                                const bcnn_hip_lifted_struct_record* record_d) {
    const size_t n = (size_t)batch * k;
    if (n == 0) return;
    lifted_scale_kernel<<<stream_grid(n, 256), 256, 0, current_stream()>>>(g_d, n, scale, record_d);
    KERNEL_CHECK();
}
