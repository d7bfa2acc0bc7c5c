// attention_window_bf16.hip -- the window-attention node's forward under bcnn_set_inference_precision(BCNN_PRECISION_BF16),
// PREDICT / VALID mode only. The problem is attention_window.hip's: per image, head and ws x ws window of
// the map rolled by `shift`, S = scale Q^T K + B_h with the pairs of different shift regions excluded, P = softmax S,
// O = V P^T, read from and written to the positions of the unrolled NCHW map. The tensors stay fp32 in memory; q, k and v are
// rounded to bf16 (round-to-nearest-even) on their way into LDS, the exponentiated scores are rounded to bf16 as the operand
// of the second product, both products accumulate in fp32 on v_mfma_f32_32x32x16_bf16 (the operand layouts are those of
// attention_bf16.hip). Scale, bias, exclusion, maximum, sum (of the UNROUNDED exponentials) and normalisation are fp32.
//
// The unit of work is a BAND: up to G horizontally adjacent windows of one (image, head, window row). A workgroup is G waves;
// it stages the band cooperatively and wave w then owns window w of it. Persistent workgroups walk the units of their head
// (blockIdx.y), blockIdx.x, blockIdx.x + gridDim.x, ...
//   staging : lanes run along x. A thread owns one QUAD of a band row -- 4 consecutive source columns, the same quad in every
//             channel it serves -- and the channels 4 p + tid / (16 G) (K, Q: pairs of channels). Where W % 4 == 0 and q, k, v
//             are 16-byte aligned the quads lie on the SOURCE's 16-byte grid, whatever shift and band start are (the roll's wrap
//             at W then falls between two quads), and a quad is one 16-byte load, its columns outside the band dropped; else
//             the quads start at the band's first column and every column is an element load with its own wrap. The same
//             values, the same bits. (ws = 8 with shift % 4 != 0 would need one quad more per row than there are threads: it
//             takes the element route.)
//   pipeline: the next unit's K, V and Q are requested into registers (fp32, d + d + 32 CT floats per thread) before the
//             current unit's products start, and converted and written to LDS after them: two barriers per unit, one buffer.
//   LDS     : per window K [key][DMAX + 8], Q [query][DMAX + 8] (a thread's two channels of a position are one dword) and
//             V [channel][64 + 8] with every 16 keys in attention_bf16.hip's permuted order (bits 2 and 3 of the key swapped),
//             all bf16. Every MFMA operand read from LDS is one 16-byte read; the 16 bytes of row padding keep the 16 lanes of
//             a ds_read_b128 on distinct 4-bank slots. The block is zeroed once per workgroup and the padding (channels from d
//             on, keys from L on) is never written again: d is zero-filled to the K step of 16, c to 32, keys past L are zero.
//   products: per query tile of 32, S^T = K^T Q: the lane pair l, l ^ 32 holds all (<= 64) keys of query l & 31, so the softmax
//             is one maximum, one sum, one exchange. The exponentials, packed in pairs, are the B operand of O += V P^T as they
//             lie; the accumulator is multiplied by 1 / l at the store.
//   mask    : a wave's lane p knows the shift region of position p (wa_position); nine ballots give every lane the 64-bit set
//             of the keys of its query's region. Keys past L are outside every set: -inf in S.
//   stores  : element stores in runs of ws at the source positions, as the fp32 kernel's (nothing waits for a store).
// No atomics, a fixed summation order: two calls give the same bits.
#include "attention_common.h"
#include "attention_window_common.h"

namespace bcnn_hip {

constexpr int kWabMaxBand = 4;  // windows of a band at most: a workgroup of 256 threads
constexpr int kWabVld = kWaMaxLen + 8;
// bf16 K, Q and V of one window
constexpr int wab_window_bytes(int dmax, int ct) { return 2 * (2 * kWaMaxLen * (dmax + 8) + ct * 32 * kWabVld); }
// G: the windows of a band, so that the workgroup stays within the 64 KiB it may declare
constexpr int wab_band(int dmax, int ct) {
    return 65536 / wab_window_bytes(dmax, ct) < kWabMaxBand ? 65536 / wab_window_bytes(dmax, ct) : kWabMaxBand;
}

// workgroups per CU the registers are held to: the staging registers are 2 dmax + 32 ct per thread; at 96 (the 32 / 32
// instance) everything fits the 256 registers of two waves per SIMD, the wider instances take one wave's 512
constexpr int wab_blocks(int dmax, int ct) { return 2 * dmax + 32 * ct <= 96 ? 2 : 1; }

// A thread's quad of the unit it stages: where it reads and where its four columns land
struct WabQuad {
    int off[4];     // column e's offset inside a channel plane, the wrap at W taken (the 16-byte route reads at off[0])
    unsigned dest;  // byte e: (window of the band) << 6 | position in the window, of column e
    int valid;      // bit e: column e lies inside the band; bit 4: the 16-byte route
};

struct WabUnit {
    int img, wy, wx0, gw;
};

__device__ __forceinline__ WabUnit wab_unit(int u, int ngx, int band, const WaGeom& g) {
    WabUnit t;
    const int per = g.nwy * ngx, rem = u - (u / per) * per;
    t.img = u / per;
    t.wy = rem / ngx;
    t.wx0 = (rem - t.wy * ngx) * band;
    t.gw = min(band, g.nwx - t.wx0);
    return t;
}

template <int G>
__device__ __forceinline__ WabQuad wab_quad(const WabUnit& t, const WaGeom& g, int slot, bool wvec) {
    WabQuad qd;
    int xs = t.wx0 * g.ws + g.shift;  // the band's first source column
    if (xs >= g.w) xs -= g.w;
    const bool vec = wvec && g.ws * ((G * g.ws + (xs & 3) + 3) >> 2) <= 16 * G;
    const int delta = vec ? (xs & 3) : 0;
    const int bwq = (G * g.ws + delta + 3) >> 2;  // quads of a band row
    const int yi = slot / bwq, xq = slot - yi * bwq;
    int sy = t.wy * g.ws + yi + g.shift;
    if (sy >= g.h) sy -= g.h;
    const int x0 = xs - delta + 4 * xq;  // the quad's first source column before the wrap
#pragma unroll
    for (int e = 0; e < 4; ++e) qd.off[e] = sy * g.w + (x0 + e >= g.w ? x0 + e - g.w : x0 + e);
    const int xb0 = 4 * xq - delta, shifted = xb0 + 4 * g.ws;  // (xb0 >= -3)
    int wi = shifted / g.ws - 4, xi = shifted - (wi + 4) * g.ws;
    qd.dest = 0;
    qd.valid = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int xb = xb0 + e;
        if (yi < g.ws && xb >= 0 && xb < t.gw * g.ws) {
            qd.valid |= 1 << e;
            qd.dest |= (unsigned)((wi << 6) | (yi * g.ws + xi)) << (8 * e);
        }
        if (++xi == g.ws) {
            xi = 0;
            ++wi;
        }
    }
    if (vec && qd.valid) qd.valid |= 16;
    return qd;
}

// the quad's four columns of one channel row: `planes` (the same for the whole workgroup) + `chan` floats (this thread's
// channel) is the channel plane; columns outside the band and `ok` false read 0
__device__ __forceinline__ float4 wab_load(const float* planes, unsigned chan, const WabQuad& qd, bool ok) {
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok || !qd.valid) return val;
    if (qd.valid & 16) {
        const float4 got = *reinterpret_cast<const float4*>(&planes[chan + (unsigned)qd.off[0]]);
        if (qd.valid & 1) val.x = got.x;
        if (qd.valid & 2) val.y = got.y;
        if (qd.valid & 4) val.z = got.z;
        if (qd.valid & 8) val.w = got.w;
    } else {
        if (qd.valid & 1) val.x = planes[chan + (unsigned)qd.off[0]];
        if (qd.valid & 2) val.y = planes[chan + (unsigned)qd.off[1]];
        if (qd.valid & 4) val.z = planes[chan + (unsigned)qd.off[2]];
        if (qd.valid & 8) val.w = planes[chan + (unsigned)qd.off[3]];
    }
    return val;
}

__device__ __forceinline__ float wab_at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// grid: (persistent workgroups of a head, heads); ngx: bands of a window row; units: n * nwy * ngx
template <int DMAX, int CT, bool SHIFT>
__global__ __launch_bounds__(64 * wab_band(DMAX, CT), wab_blocks(DMAX, CT)) void wab_fwd_kernel(const float* q, const float* k, const float* v,
                                                                           const float* bias, float* o, WaGeom g, int ngx,
                                                                           int units, int wvec) {
    constexpr int G = wab_band(DMAX, CT), NT = 64 * G, QS = 16 * G;  // QS: quad slots of a channel row = NT / 4
    constexpr int KLD = DMAX + 8, VLD = kWabVld;                     // bf16 per LDS row
    constexpr int WIN = wab_window_bytes(DMAX, CT) / 2;              // bf16 per window: K, Q, V
    constexpr int QOFF = kWaMaxLen * KLD, VOFF = 2 * kWaMaxLen * KLD;
    constexpr int KU = DMAX / 8, VU = CT * 8;  // a thread's K (Q) units of 2 channels x 4 columns, V units of 1 x 4
    static_assert(G >= 2 && G * WIN * 2 <= 65536 && WIN % 8 == 0 && KLD % 8 == 0 && VLD % 8 == 0, "band");
    __shared__ __attribute__((aligned(16))) unsigned short lds[G * WIN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5, head = blockIdx.y;
    const int slot = tid % QS, chan = tid / QS;  // this thread's quad slot and the first of its channels (pairs)
    const size_t hw = (size_t)g.h * g.w;
    const int nkt = g.len > 32 ? 2 : 1, nct = (g.c + 31) >> 5;
    const float* bias_h = bias ? bias + (size_t)head * kWaMaxLen * kWaMaxLen : nullptr;
    const unsigned long long lenmask = g.len >= 64 ? ~0ull : (1ull << g.len) - 1;

    float4 kreg[KU][2], qreg[KU][2], vreg[VU];
    WabQuad qd;
    auto load_unit = [&](const WabUnit& t) {
        qd = wab_quad<G>(t, g, slot, wvec != 0);
        const size_t nh = (size_t)t.img * g.heads + head;
        const float *kh = k + nh * g.d * hw, *qh = q + nh * g.d * hw, *vh = v + nh * g.c * hw;
        const unsigned mine = (unsigned)chan * (unsigned)hw;  // (every tensor is below 2^31 elements: wa_check)
#pragma unroll
        for (int p = 0; p < KU; ++p) {
            const int t0 = 2 * (4 * p + chan);
            kreg[p][0] = wab_load(kh + (size_t)(8 * p) * hw, 2 * mine, qd, t0 < g.d);
            kreg[p][1] = wab_load(kh + (size_t)(8 * p + 1) * hw, 2 * mine, qd, t0 + 1 < g.d);
        }
#pragma unroll
        for (int p = 0; p < VU; ++p) vreg[p] = wab_load(vh + (size_t)(4 * p) * hw, mine, qd, 4 * p + chan < g.c);
#pragma unroll
        for (int p = 0; p < KU; ++p) {
            const int t0 = 2 * (4 * p + chan);
            qreg[p][0] = wab_load(qh + (size_t)(8 * p) * hw, 2 * mine, qd, t0 < g.d);
            qreg[p][1] = wab_load(qh + (size_t)(8 * p + 1) * hw, 2 * mine, qd, t0 + 1 < g.d);
        }
    };
    auto store_unit = [&]() {
        unsigned* kd = reinterpret_cast<unsigned*>(lds);  // dword (position, channel pair) at position * (KLD / 2) + pair
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!(qd.valid & (1 << e))) continue;
            const int dst = (qd.dest >> (8 * e)) & 255, wi = dst >> 6, pos = dst & 63;
            // key 16 a + 8 hi + 4 h + i lies at 16 a + 8 h + 4 hi + i
            const int perm = (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1);
#pragma unroll
            for (int p = 0; p < KU; ++p) {
                const int tp = 4 * p + chan;
                if (2 * tp >= g.d) continue;  // (channels from d on stay zero: the K step)
                unsigned* at = kd + wi * (WIN / 2) + pos * (KLD / 2) + tp;
                at[0] = attn_pack_bf16(wab_at(kreg[p][0], e), wab_at(kreg[p][1], e));
                at[QOFF / 2] = attn_pack_bf16(wab_at(qreg[p][0], e), wab_at(qreg[p][1], e));
            }
#pragma unroll
            for (int p = 0; p < VU; ++p) {
                const int r = 4 * p + chan;
                if (r >= g.c) continue;  // (rows from c on stay zero: the 32-row A tiles)
                lds[wi * WIN + VOFF + r * VLD + perm] = (unsigned short)attn_pack_bf16(wab_at(vreg[p], e), 0.f);
            }
        }
    };

    {  // the windows a band can hold are zero once; staging writes only channels below d (c) and positions below L
        uint4* z = reinterpret_cast<uint4*>(lds);
        for (int idx = tid; idx < min(G, g.nwx) * (WIN / 8); idx += NT) z[idx] = make_uint4(0, 0, 0, 0);
    }
    int u = blockIdx.x;
    WabUnit cur = wab_unit(u < units ? u : 0, ngx, G, g);
    if (u < units) load_unit(cur);
    __syncthreads();
    if (u < units) store_unit();
    __syncthreads();
    for (; u < units; u += gridDim.x) {
        const int un = u + gridDim.x;
        const WabUnit next = wab_unit(un < units ? un : 0, ngx, G, g);
        if (un < units) load_unit(next);  // in flight over this unit's products
        if (wave < cur.gw) {
            const unsigned short* kw = lds + wave * WIN;
            const unsigned short* qw = kw + QOFF;
            const unsigned short* vw = kw + VOFF;
            const int wx = cur.wx0 + wave;
            const bool masked = SHIFT && (cur.wy == g.nwy - 1 || wx == g.nwx - 1);  // else the window lies in one region
            int off, code;
            wa_position(g, cur.wy, wx, lane, off, code);
            float* oh = o + ((size_t)cur.img * g.heads + head) * g.c * hw;
#pragma unroll 1  // (unrolled, the two tiles' bias loads and scores cost the 32 / 32 instance its second wave per SIMD)
            for (int qt = 0; qt < 2; ++qt) {
                if (qt * 32 >= g.len) break;
                const int i = qt * 32 + col;  // this lane's query
                const int off_i = __shfl(off, i, 64), code_i = __shfl(code, i, 64);
                const bool qin = i < g.len;
                unsigned long long allow = lenmask;  // the keys of this lane's query
                if (SHIFT && masked) {
#pragma unroll
                    for (int cv = 0; cv < 9; ++cv) {
                        const unsigned long long same = __ballot(code == cv) & lenmask;
                        if (qin && code_i == cv) allow = same;
                    }
                }
                allow >>= 4 * half;  // bit (r & 3) + 8 (r >> 2) + 32 kt is now key kt * 32 + mfma_row(r, lane)
                f32x16 s[2];
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
                for (int t = 0; t < DMAX / 16; ++t) {  // S^T[j][i]: A = K^T, B = Q
                    if (16 * t >= g.d) break;
                    const bf16x8 b = *reinterpret_cast<const bf16x8*>(&qw[i * KLD + 16 * t + 8 * half]);
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        if (kt >= nkt) break;
                        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&kw[(kt * 32 + col) * KLD + 16 * t + 8 * half]);
                        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, s[kt], 0, 0, 0);
                    }
                }
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float sv = s[kt][r] * g.scale;
                        if (bias_h) sv += bias_h[(kt * 32 + mfma_row(r, lane)) * kWaMaxLen + i];
                        sv = ((allow >> (32 * kt + (r & 3) + 8 * (r >> 2))) & 1) ? sv : -INFINITY;
                        s[kt][r] = sv;
                        mx = fmaxf(mx, sv);
                    }
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // finite: a query is a key of its own region
                float sum = 0.f;
                bf16x8 pb[2][2];
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    if (kt >= nkt) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        s[kt][r] = attn_exp(s[kt][r] - mx);
                        sum += s[kt][r];
                    }
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        pb[kt][t] = attn_pack8(s[kt][8 * t], s[kt][8 * t + 1], s[kt][8 * t + 2], s[kt][8 * t + 3],
                                               s[kt][8 * t + 4], s[kt][8 * t + 5], s[kt][8 * t + 6], s[kt][8 * t + 7]);
                }
                sum += __shfl_xor(sum, 32, 64);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {  // O[r][i] = V[r][key] P[i][key]
                    if (ct >= nct) break;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        if (kt >= nkt) break;
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            const bf16x8 a =
                                *reinterpret_cast<const bf16x8*>(&vw[(ct * 32 + col) * VLD + kt * 32 + 16 * t + 8 * half]);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb[kt][t], acc, 0, 0, 0);
                        }
                    }
                    if (!qin) continue;  // a query past L is not stored
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = ct * 32 + mfma_row(r, lane);
                        if (row < g.c) oh[(size_t)row * hw + off_i] = acc[r] * inv;
                    }
                }
            }
        }
        __syncthreads();  // every wave is done with this unit's K, Q and V
        if (un < units) store_unit();
        __syncthreads();
        cur = next;
    }
}

struct WabFwd {
    const BcnnWindowAttnFwdArgs* a;
    const float* bias;
    WaGeom g;
    template <int DMAX, int CT>
    void operator()() const {
        constexpr int G = wab_band(DMAX, CT);
        const int ngx = ceil_div(g.nwx, G), units = g.n * g.nwy * ngx;
        // two workgroups per CU over all heads: half of wa_groups' aim, each workgroup being a band of waves
        const dim3 grid((unsigned)std::min(units, ceil_div(kWaWaves / 2, g.heads)), (unsigned)g.heads);
        const int wvec = (g.w & 3) == 0 && al16(a->q) && al16(a->k) && al16(a->v);
        if (g.shift)
            wab_fwd_kernel<DMAX, CT, true><<<grid, 64 * G, 0, current_stream()>>>(a->q, a->k, a->v, bias, a->o, g, ngx, units, wvec);
        else
            wab_fwd_kernel<DMAX, CT, false><<<grid, 64 * G, 0, current_stream()>>>(a->q, a->k, a->v, bias, a->o, g, ngx, units, wvec);
    }
};

}  // namespace bcnn_hip

using namespace bcnn_hip;

extern "C" void bcnn_hip_window_attention_forward_bf16(const BcnnWindowAttnFwdArgs* a) {
    if (a->n == 0) return;
    const WaGeom g = wa_geom("bcnn_hip_window_attention_forward_bf16", a->n, a->heads, a->d, a->c, a->h, a->w, a->window,
                             a->shift, a->scale);
    const float* bias = a->table ? wa_dense_bias(a->table, g, 0) : nullptr;
    trace_kernel("window_attention_fwd_bf16");
    wa_dispatch(a->d, a->c, WabFwd{a, bias, g});
    KERNEL_CHECK();
}
