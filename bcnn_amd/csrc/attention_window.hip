// attention_window.hip -- the window-attention node (Swin blocks), forward and backward, on the fp32 matrix cores. No reference
// counterpart. Per image n, head h and ws x ws window of the map rolled by `shift` (L = ws * ws <= 64 positions, row-major):
//   S[i][j] = scale * sum_t Q[t][i] K[t][j] + B_h[i][j],  pairs of different shift regions excluded,  P = softmax_j S,
//   O[r][i] = sum_j V[r][j] P[i][j],  everything read from and written to the positions of the unrolled NCHW map.
// The unit of work is one (image, window) of one head, and its owner is ONE wave: a workgroup is 64 threads, blockIdx.y the
// head, and the workgroup walks the units blockIdx.x, blockIdx.x + G, ... of its head. Lane p of the wave
// owns position p of the window: its offset inside a channel plane (window, roll and wrap are this one integer) and its shift
// region. K and V of the window are staged in LDS once, [channel][65]; every product is v_mfma_f32_32x32x2_f32 (conv_common.h)
// in the layout of attention.hip: S^T = K^T Q leaves ALL (<= 64) keys of one query in the 32 registers of lanes l and l ^ 32, so
// the softmax is one maximum, one sum and one exchange -- no online rescale, no log-sum-exp, nothing kept for the backward.
//   forward : per query tile of 32: Q from global as the B operand, S^T, + the dense bias tile, mask, softmax, O = V P^T with P
//             taken from S^T's registers, stored at the source positions.
//   backward: one kernel. Per query tile: S^T and dP^T = V^T dO, the softmax again, Dl = sum_j P dP from the row the lane pair
//             holds, dS^T = P (dP^T - Dl); dQ = K dS^T straight from the registers. dV += dO P and dK += Q dS want the other
//             orientation: the 32 x 64 tile goes through LDS once ([query][65], P then dS in the same block) and comes back as
//             the B operand; their accumulators live in registers over the two query tiles. dS^T has the same register layout
//             for every window of a head: the running bias gradient is 64 registers per lane over all the wave's windows,
//             written once as a dense [L][L] partial; a finalize kernel adds the partials in double and folds the pairs of
//             equal relative position into the table.
// No atomics: every gradient element has one writer and one summation order, so two runs give the same bits. Every global
// access is an element access (a window row is ws floats at a stride of W), whatever the pointers' alignment.
#include "attention_window_common.h"

namespace bcnn_hip {

constexpr int kWaStride = 65;     // LDS row of a whole window: odd, so a walk along the rows is free of bank conflicts
constexpr int kWaTileStride = 33; // LDS row of one query tile
constexpr float kWaLog2e = 1.4426950408889634f;

// exp(x) for x <= 0 (and -inf); the maximum is subtracted before the scaling to base 2 (attention.hip)
__device__ __forceinline__ float wa_exp(float x) { return __builtin_amdgcn_exp2f(x * kWaLog2e); }

// A whole window of a [rows][hw] head into LDS as [row][65]: lane p loads position p of every row. Rows up to the next
// multiple of 32 and positions from len on are zero (the MFMA's K step, the 32-row A tiles, the ragged second key tile).
template <int ROWS>
__device__ __forceinline__ void wa_stage(float* lds, const float* src, int rows, size_t hw, int off, bool in, int lane) {
#pragma unroll 8
    for (int row = 0; row < ROWS; ++row) {
        if ((row & ~31) >= rows) break;
        lds[row * kWaStride + lane] = (in && row < rows) ? src[(size_t)row * hw + off] : 0.f;
    }
}
// One query tile of a [rows][hw] head into LDS as [row][33]: lane l loads position col of rows 2 s + half.
template <int ROWS>
__device__ __forceinline__ void wa_stage_tile(float* lds, const float* src, int rows, size_t hw, int off, bool in, int lane) {
    const int col = lane & 31, half = lane >> 5;
#pragma unroll 8
    for (int s = 0; s < ROWS / 2; ++s) {
        if (((2 * s) & ~31) >= rows) break;
        const int row = 2 * s + half;
        lds[row * kWaTileStride + col] = (in && row < rows) ? src[(size_t)row * hw + off] : 0.f;
    }
}

// The score registers of one query (s[kt][r] = S^T[key kt * 32 + mfma_row(r, lane)][query i]) become its softmax row:
// scale, bias, exclusion, maximum, exponential, sum -- the same operations in the same order in forward and backward.
template <bool SHIFT>
__device__ __forceinline__ void wa_softmax(f32x16 (&s)[2], int nkt, const float* bias_h, const int* code_s, int i, int code_i,
                                           bool qin, bool masked, const WaGeom& g, int lane) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        if (kt >= nkt) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = kt * 32 + mfma_row(r, lane);
            float sv = s[kt][r] * g.scale;
            if (bias_h) sv += bias_h[j * kWaMaxLen + i];
            bool drop = j >= g.len;  // a key past L takes no weight (0 would)
            if (SHIFT) drop = drop || (masked && qin && code_s[j] != code_i);
            sv = drop ? -INFINITY : sv;
            s[kt][r] = sv;
            mx = fmaxf(mx, sv);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        if (kt >= nkt) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[kt][r] = wa_exp(s[kt][r] - mx);
            sum += s[kt][r];
        }
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        if (kt >= nkt) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kt][r] *= inv;
    }
}

// acc[tile][r] (channel tile * 32 + mfma_row(r, lane) of the position at `off`) times f, assigned or added
template <int TILES>
__device__ __forceinline__ void wa_store(float* dst, const f32x16 (&acc)[TILES], int rows, size_t hw, int off, int lane, float f,
                                         int overwrite) {
#pragma unroll
    for (int tile = 0; tile < TILES; ++tile) {
        if (tile * 32 >= rows) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile * 32 + mfma_row(r, lane);
            if (row >= rows) continue;
            float* at = dst + (size_t)row * hw + off;
            const float val = acc[tile][r] * f;
            *at = overwrite ? val : *at + val;
        }
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int DMAX, int CT, bool SHIFT>
__global__ __launch_bounds__(64) void wa_fwd_kernel(const float* q, const float* k, const float* v, const float* bias, float* o,
                                                    WaGeom g) {
    __shared__ float ks[DMAX * kWaStride];     // K, [t][key]
    __shared__ float vs[CT * 32 * kWaStride];  // V, [r][key]
    __shared__ int code_s[kWaMaxLen];
    const int lane = threadIdx.x, col = lane & 31, half = lane >> 5, head = blockIdx.y;
    const size_t hw = (size_t)g.h * g.w;
    const int nkt = g.len > 32 ? 2 : 1, nct = (g.c + 31) >> 5, nwin = g.nwx * g.nwy;
    const float* bias_h = bias ? bias + (size_t)head * kWaMaxLen * kWaMaxLen : nullptr;

    for (int u = blockIdx.x; u < g.units; u += gridDim.x) {
        const int img = u / nwin, win = u - img * nwin, wy = win / g.nwx, wx = win - wy * g.nwx;
        const bool masked = SHIFT && (wy == g.nwy - 1 || wx == g.nwx - 1);  // else the window lies in one region
        int off, code;
        wa_position(g, wy, wx, lane, off, code);
        const size_t nh = (size_t)img * g.heads + head;
        const float* qh = q + nh * g.d * hw;
        float* oh = o + nh * g.c * hw;
        __syncthreads();  // the previous window's readers are done
        wa_stage<DMAX>(ks, k + nh * g.d * hw, g.d, hw, off, lane < g.len, lane);
        wa_stage<CT * 32>(vs, v + nh * g.c * hw, g.c, hw, off, lane < g.len, lane);
        if (SHIFT) code_s[lane] = code;
        __syncthreads();
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            if (qt * 32 >= g.len) break;
            const int i = qt * 32 + col;  // this lane's query
            const int off_i = __shfl(off, i, 64), code_i = __shfl(code, i, 64);
            const bool qin = i < g.len;
            float qr[DMAX / 2];
#pragma unroll
            for (int t = 0; t < DMAX / 2; ++t) {
                const int row = 2 * t + half;
                qr[t] = (qin && row < g.d) ? qh[(size_t)row * hw + off_i] : 0.f;
            }
            f32x16 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt >= nkt) break;
                for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
                for (int t = 0; t < DMAX / 2; ++t)  // S^T[j][i]: A = K[2 t + half][key col], B = Q
                    if (2 * t < g.d) s[kt] = mfma32(ks[(2 * t + half) * kWaStride + kt * 32 + col], qr[t], s[kt]);
            }
            wa_softmax<SHIFT>(s, nkt, bias_h, code_s, i, code_i, qin, masked, g, lane);
            f32x16 acc[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {  // O[r][i] = V[r][key] P[i][key], key = mfma_row(step, lane): P is s as it lies
                for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
                if (ct >= nct) continue;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[ct] = mfma32(vs[(ct * 32 + col) * kWaStride + kt * 32 + mfma_row(r, lane)], s[kt][r], acc[ct]);
                }
            }
            if (qin) wa_store<CT>(oh, acc, g.c, hw, off_i, lane, 1.0f, 1);
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// partial: [gridDim.x][heads][L][L] sums of dS over this workgroup's windows, or NULL (no bias gradient is wanted)
template <int DMAX, int CT, bool SHIFT, bool BIAS>
__global__ __launch_bounds__(64) void wa_bwd_kernel(const float* q, const float* k, const float* v, const float* bias,
                                                    const float* dout, float* dq, float* dk, float* dv, float* partial, WaGeom g,
                                                    int ow_q, int ow_k, int ow_v) {
    constexpr int DT = DMAX / 32;
    // WIDE (a head above 32 channels on either side): dK and dV accumulators of two key tiles beside the tile in flight and
    // the running dB do not fit the register file. There P and dS of BOTH query tiles stay in LDS and dK, dV are formed one
    // output tile at a time after the query loop, when K and V are dead: their block then holds Q and dO of the whole window.
    constexpr bool WIDE = DMAX + CT * 32 > 64;
    constexpr int kKV = (DMAX + CT * 32) * kWaStride;           // K [t][key], V [r][key]; WIDE, afterwards: Q, dO [ch][query]
    constexpr int kTile = (DMAX + CT * 32) * kWaTileStride;     // Q, dO of the query tile, [ch][query]
    constexpr int kPD = 2 * 32 * kWaStride;                     // WIDE: P and dS of a query tile, [query][key] each
    constexpr int kSecond = WIDE ? (kTile > kPD ? kTile : kPD) : kTile;  // WIDE: tile 1's P and dS follow its Q and dO here
    __shared__ float lds[kKV + kSecond + (WIDE ? kPD : 32 * kWaStride)];
    float* ks = lds;
    float* vs = lds + DMAX * kWaStride;
    float* qs = lds + kKV;
    float* dos = qs + DMAX * kWaTileStride;
    float* ts = lds + kKV + kSecond;  // P, then dS, of the query tile: [query][key]; WIDE: P and dS of tile 0
    __shared__ int code_s[kWaMaxLen];
    const int lane = threadIdx.x, col = lane & 31, half = lane >> 5, head = blockIdx.y;
    const size_t hw = (size_t)g.h * g.w;
    const int nkt = g.len > 32 ? 2 : 1, nct = (g.c + 31) >> 5, ndt = (g.d + 31) >> 5, nwin = g.nwx * g.nwy;
    const float* bias_h = bias ? bias + (size_t)head * kWaMaxLen * kWaMaxLen : nullptr;

    f32x16 db[2][2];  // the running dS^T[key tile][query tile] of this workgroup's windows
    if (BIAS) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
            for (int r = 0; r < 16; ++r) db[a >> 1][a & 1][r] = 0.f;
    }

    for (int u = blockIdx.x; u < g.units; u += gridDim.x) {
        const int img = u / nwin, win = u - img * nwin, wy = win / g.nwx, wx = win - wy * g.nwx;
        const bool masked = SHIFT && (wy == g.nwy - 1 || wx == g.nwx - 1);
        int off, code;
        wa_position(g, wy, wx, lane, off, code);
        const size_t nh = (size_t)img * g.heads + head;
        __syncthreads();  // the previous window's readers are done
        wa_stage<DMAX>(ks, k + nh * g.d * hw, g.d, hw, off, lane < g.len, lane);
        wa_stage<CT * 32>(vs, v + nh * g.c * hw, g.c, hw, off, lane < g.len, lane);
        if (SHIFT) code_s[lane] = code;

        f32x16 acck[WIDE ? 1 : 2][DT], accv[WIDE ? 1 : 2][CT];  // (WIDE: unused)
#pragma unroll
        for (int kt = 0; kt < (WIDE ? 1 : 2); ++kt) {
#pragma unroll
            for (int t = 0; t < DT; ++t)
                for (int r = 0; r < 16; ++r) acck[kt][t][r] = 0.f;
#pragma unroll
            for (int t = 0; t < CT; ++t)
                for (int r = 0; r < 16; ++r) accv[kt][t][r] = 0.f;
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            if (qt * 32 >= g.len) break;
            const int i = qt * 32 + col;  // this lane's query
            const int off_i = __shfl(off, i, 64), code_i = __shfl(code, i, 64);
            const bool qin = i < g.len;
            __syncthreads();  // the previous tile's readers of qs, dos and ts are done
            wa_stage_tile<DMAX>(qs, q + nh * g.d * hw, g.d, hw, off_i, qin, lane);
            wa_stage_tile<CT * 32>(dos, dout + nh * g.c * hw, g.c, hw, off_i, qin, lane);
            __syncthreads();
            f32x16 s[2], dp[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt >= nkt) break;
                for (int r = 0; r < 16; ++r) s[kt][r] = dp[kt][r] = 0.f;
#pragma unroll
                for (int t = 0; t < DMAX / 2; ++t)  // S^T[j][i]: A = K[2 t + half][key col], B = Q[2 t + half][query col]
                    if (2 * t < g.d)
                        s[kt] = mfma32(ks[(2 * t + half) * kWaStride + kt * 32 + col], qs[(2 * t + half) * kWaTileStride + col],
                                       s[kt]);
#pragma unroll
                for (int t = 0; t < CT * 16; ++t)  // dP^T[j][i]: A = V[2 t + half][key col], B = dO[2 t + half][query col]
                    if (2 * t < g.c)
                        dp[kt] = mfma32(vs[(2 * t + half) * kWaStride + kt * 32 + col], dos[(2 * t + half) * kWaTileStride + col],
                                        dp[kt]);
            }
            wa_softmax<SHIFT>(s, nkt, bias_h, code_s, i, code_i, qin, masked, g, lane);
            float dl = 0.f;  // Dl[i] = sum_j P dP: the lane pair holds the whole row
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt >= nkt) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) dl = fmaf(s[kt][r], dp[kt][r], dl);
            }
            dl += __shfl_xor(dl, 32, 64);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt >= nkt) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dp[kt][r] = s[kt][r] * (dp[kt][r] - dl);  // dS^T
                    if (BIAS) db[kt][qt][r] += dp[kt][r];
                }
            }
            if (dq) {  // dQ[t][i] = K[t][key] dS[i][key], key = mfma_row(step, lane): dS^T is dp as it lies
                f32x16 accq[DT];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    for (int r = 0; r < 16; ++r) accq[dt][r] = 0.f;
                    if (dt >= ndt) continue;
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        if (kt >= nkt) break;
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            accq[dt] = mfma32(ks[(dt * 32 + col) * kWaStride + kt * 32 + mfma_row(r, lane)], dp[kt][r], accq[dt]);
                    }
                }
                if (qin) wa_store<DT>(dq + nh * g.d * hw, accq, g.d, hw, off_i, lane, g.scale, ow_q);
            }
            if (WIDE) {  // P and dS of this tile stay in LDS for the pass below; tile 1's replace its Q and dO
                float* pd = qt == 0 ? ts : qs;
                if (qt == 1) __syncthreads();  // (S^T and dP^T of every lane have read qs and dos)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        pd[col * kWaStride + kt * 32 + mfma_row(r, lane)] = s[kt][r];
                        pd[(32 + col) * kWaStride + kt * 32 + mfma_row(r, lane)] = dp[kt][r];
                    }
                }
            }
            if (!WIDE && dv) {  // dV[r][j] += dO[r][query] P[query][j]: P through LDS into the other orientation
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) ts[col * kWaStride + kt * 32 + mfma_row(r, lane)] = s[kt][r];
                }
                __syncthreads();
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        if (ct >= nct) break;
#pragma unroll
                        for (int st = 0; st < 16; ++st)
                            accv[kt][ct] = mfma32(dos[(ct * 32 + col) * kWaTileStride + 2 * st + half],
                                                  ts[(2 * st + half) * kWaStride + kt * 32 + col], accv[kt][ct]);
                    }
                }
                __syncthreads();
            }
            if (!WIDE && dk) {  // dK[t][j] += Q[t][query] dS[query][j]
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) ts[col * kWaStride + kt * 32 + mfma_row(r, lane)] = dp[kt][r];
                }
                __syncthreads();
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        if (dt >= ndt) break;
#pragma unroll
                        for (int st = 0; st < 16; ++st)
                            acck[kt][dt] = mfma32(qs[(dt * 32 + col) * kWaTileStride + 2 * st + half],
                                                  ts[(2 * st + half) * kWaStride + kt * 32 + col], acck[kt][dt]);
                    }
                }
            }
        }
        if (WIDE && (dk || dv)) {
            // K and V are dead: Q and dO of the whole window take their place, [channel][65], and every 32 x 32 tile of dK and
            // dV is one accumulator over the queries of both tiles (the same summation order as the register form above)
            __syncthreads();
            float* qf = lds;
            float* dof = lds + DMAX * kWaStride;
            if (dk) wa_stage<DMAX>(qf, q + nh * g.d * hw, g.d, hw, off, lane < g.len, lane);
            if (dv) wa_stage<CT * 32>(dof, dout + nh * g.c * hw, g.c, hw, off, lane < g.len, lane);
            __syncthreads();
            for (int kt = 0; kt < nkt; ++kt) {
                const int j = kt * 32 + col;
                const int off_j = __shfl(off, j, 64);
                for (int tile = 0; tile < ndt + nct; ++tile) {
                    const bool isk = tile < ndt;  // a dK tile, else a dV tile
                    if (isk ? !dk : !dv) continue;
                    const int ch0 = (isk ? tile : tile - ndt) * 32;
                    const float* a = (isk ? qf : dof) + (ch0 + col) * kWaStride;
                    f32x16 acc[1];
                    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
                    for (int qt = 0; qt < nkt; ++qt) {
                        const float* b = (qt == 0 ? ts : qs) + (isk ? 32 * kWaStride : 0) + kt * 32 + col;
#pragma unroll
                        for (int st = 0; st < 16; ++st)
                            acc[0] = mfma32(a[qt * 32 + 2 * st + half], b[(2 * st + half) * kWaStride], acc[0]);
                    }
                    if (j < g.len && isk) wa_store<1>(dk + (nh * g.d + ch0) * hw, acc, g.d - ch0, hw, off_j, lane, g.scale, ow_k);
                    if (j < g.len && !isk) wa_store<1>(dv + (nh * g.c + ch0) * hw, acc, g.c - ch0, hw, off_j, lane, 1.0f, ow_v);
                }
            }
        }
        // after dQ: with q, k and v one tensor the three gradients add up in one buffer, and the lane that wrote dQ of a
        // position is the lane that adds dK and dV to it
        if (!WIDE) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt >= nkt) break;
                const int j = kt * 32 + col;
                const int off_j = __shfl(off, j, 64);
                if (j >= g.len) continue;
                if (dk) wa_store<DT>(dk + nh * g.d * hw, acck[kt], g.d, hw, off_j, lane, g.scale, ow_k);
                if (dv) wa_store<CT>(dv + nh * g.c * hw, accv[kt], g.c, hw, off_j, lane, 1.0f, ow_v);
            }
        }
    }
    if (BIAS) {
        float* mine = partial + ((size_t)blockIdx.x * g.heads + head) * g.len * g.len;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int i = qt * 32 + col;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = kt * 32 + mfma_row(r, lane);
                    if (i < g.len && j < g.len) mine[i * g.len + j] = db[kt][qt][r];
                }
            }
        }
    }
}

// dtable[h][rel] += the sum over the pairs (i, j) of that relative position and the G partials: one workgroup per table entry,
// thread t adds the elements e = pair * G + g with e % 256 == t in ascending order in double, the 256 sums are folded in a
// fixed tree, and the start value enters as one float32 addition.
__global__ __launch_bounds__(256) void wa_bias_grad_kernel(const float* partial, float* dtable, int heads, int ws, int groups) {
    __shared__ double sums[256];
    const int span = 2 * ws - 1, len = ws * ws;
    const int head = blockIdx.x / (span * span), rel = blockIdx.x - head * span * span;
    const int dy = rel / span - (ws - 1), dx = rel - (rel / span) * span - (ws - 1);  // yi - yj, xi - xj
    const int ny = ws - abs(dy), nx = ws - abs(dx), y0 = dy > 0 ? dy : 0, x0 = dx > 0 ? dx : 0;
    double sum = 0.0;
    for (int e = threadIdx.x; e < ny * nx * groups; e += 256) {
        const int pair = e / groups, grp = e - pair * groups;
        const int yi = y0 + pair / nx, xi = x0 + pair % nx;
        const int i = yi * ws + xi, j = (yi - dy) * ws + (xi - dx);
        sum += (double)partial[((size_t)grp * heads + head) * len * len + i * len + j];
    }
    sums[threadIdx.x] = sum;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) sums[threadIdx.x] += sums[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) dtable[blockIdx.x] = dtable[blockIdx.x] + (float)sums[0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct WaFwd {
    const BcnnWindowAttnFwdArgs* a;
    const float* bias;
    WaGeom g;
    template <int DMAX, int CT>
    void operator()() const {
        const dim3 grid((unsigned)wa_groups(g), (unsigned)g.heads);
        if (g.shift) wa_fwd_kernel<DMAX, CT, true><<<grid, 64, 0, current_stream()>>>(a->q, a->k, a->v, bias, a->o, g);
        else wa_fwd_kernel<DMAX, CT, false><<<grid, 64, 0, current_stream()>>>(a->q, a->k, a->v, bias, a->o, g);
    }
};
struct WaBwd {
    const BcnnWindowAttnBwdArgs* a;
    const float* bias;
    float* partial;
    WaGeom g;
    template <int DMAX, int CT, bool SHIFT, bool BIAS>
    void wa_bwd_launch() const {
        const dim3 grid((unsigned)wa_groups(g), (unsigned)g.heads);
        wa_bwd_kernel<DMAX, CT, SHIFT, BIAS><<<grid, 64, 0, current_stream()>>>(a->q, a->k, a->v, bias, a->dout, a->dq, a->dk, a->dv,
                                                                               partial, g, a->overwrite_q, a->overwrite_k,
                                                                               a->overwrite_v);
    }
    template <int DMAX, int CT>
    void operator()() const {
        if (g.shift && partial) wa_bwd_launch<DMAX, CT, true, true>();
        else if (g.shift) wa_bwd_launch<DMAX, CT, true, false>();
        else if (partial) wa_bwd_launch<DMAX, CT, false, true>();
        else wa_bwd_launch<DMAX, CT, false, false>();
    }
};

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" {

int bcnn_hip_window_attention_check(int n, int heads, int d, int c, int h, int w, int window, int shift) {
    return wa_check(n, heads, d, c, h, w, window, shift);
}

void bcnn_hip_window_attention_forward(const BcnnWindowAttnFwdArgs* a) {
    if (a->n == 0) return;
    const WaGeom g = wa_geom("bcnn_hip_window_attention_forward", a->n, a->heads, a->d, a->c, a->h, a->w, a->window, a->shift,
                             a->scale);
    const float* bias = a->table ? wa_dense_bias(a->table, g, 0) : nullptr;
    trace_kernel("window_attention_fwd");
    wa_dispatch(a->d, a->c, WaFwd{a, bias, g});
    KERNEL_CHECK();
}

void bcnn_hip_window_attention_backward(const BcnnWindowAttnBwdArgs* a) {
    if (a->n == 0) return;
    const WaGeom g = wa_geom("bcnn_hip_window_attention_backward", a->n, a->heads, a->d, a->c, a->h, a->w, a->window, a->shift,
                             a->scale);
    const bool want_bias = a->table && a->dtable;
    if (!a->dq && !a->dk && !a->dv && !want_bias) return;
    const int groups = wa_groups(g);
    const size_t partials = want_bias ? (size_t)groups * g.heads * g.len * g.len : 0;
    float* block = (a->table || partials) ? wa_dense_bias(a->table, g, partials) : nullptr;
    const float* bias = a->table ? block : nullptr;
    float* partial = want_bias ? block + (size_t)g.heads * kWaMaxLen * kWaMaxLen : nullptr;
    trace_kernel("window_attention_bwd");
    wa_dispatch(a->d, a->c, WaBwd{a, bias, partial, g});
    KERNEL_CHECK();
    if (want_bias) {
        const int span = 2 * g.ws - 1;
        trace_kernel("window_attention_bwd:bias");
        wa_bias_grad_kernel<<<(unsigned)(g.heads * span * span), 256, 0, current_stream()>>>(partial, a->dtable, g.heads, g.ws,
                                                                                           groups);
        KERNEL_CHECK();
    }
}

}  // extern "C"
