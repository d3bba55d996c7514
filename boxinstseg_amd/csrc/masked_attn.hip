// masked_attn.hip -- the masked cross-attention of Box2Mask's transformer decoder on gfx950 (include/boxinst/boxinst_hip_attn.h): the mask
// of box2mask_head.py:346-355 / :397 as bits, the attention core of torch.nn.MultiheadAttention forward and backward.
//
// All products run on v_mfma_f32_32x32x2_f32: lane l holds A[row l&31][k l>>5] and B[k l>>5][column l&31], the result has its column on the
// lane and rows (reg&3) + 8 (reg>>2) + 4 (l>>5) in its 16 registers, and every element is one fmaf chain in ascending k.  A result tile is
// the B operand of the next product without any lane movement when that product sums over the tile's ROW index: register `reg` is one k
// step, whose two k values are the rows of the two lane halves.  So that those steps walk the rows in ascending order the first product's A
// operand is fed permuted: lane i supplies item sigma(i), and then register `reg` of lane half `half` holds item 2 reg + half.
//
// attn_bits_kernel     one workgroup per mask row: 64 positions per wave and step, a ballot is two words; the workgroup counts its set
//   bits and, for the resized logits, rewrites an all-set row as all clear.
// attn_fwd_kernel<D>   one workgroup = 4 waves per (span of 256 keys, (b, m), 128 queries).  K and V of the span go through LDS in chunks;
//   a wave owns 32 queries (their scaled q values are its B operand, in registers): S^T [key][query] = K Q^T has the query on the lane, so
//   the online max and sum are per lane, and P^T is the B operand of O^T [d][query] += V^T P^T.  Writes the span's (max, sum, acc [Q][D]).
// attn_combine_kernel  out and lse from the spans' partials, in span order.
// attn_delta_kernel    delta [b, m, q] = sum_d dout * out, one fmaf chain in ascending d (the chain dP runs for a row with one key).
// attn_bwd_kernel<D>   one workgroup = 8 waves per (span, (b, m)); a wave owns 32 keys, K and V in registers, and walks all queries in
//   blocks of 32 staged in LDS: S [query][key] = Q K^T has the key on the lane, so P and dS are the B operands of dV^T += dO^T P and
//   dK^T += Q^T dS, which stay in the wave's accumulators for the whole walk.  Only dS crosses LDS, once, for dQ^T = K^T dS^T; the waves'
//   dQ tiles are added in wave order and written as the span's share.
// attn_dq_kernel       dq = scale * the shares in span order.
#include "common.hpp"

#include "../../include/boxinst/boxinst_hip_attn.h"

namespace bxi {

constexpr int kAtSpan = BXI_ATTN_SPAN, kAtTiles = kAtSpan / 32;
static_assert(kAtTiles == 8, "a wave of the backward per tile of 32 keys, eight mask words per span");

typedef float at16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ at16v at_mfma(float a, float b, at16v c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
    return c;
#endif
}
__device__ __forceinline__ int at_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }
// the item lane i supplies to the first product: sigma(at_row(reg, half)) = 2 reg + half
__device__ __forceinline__ int at_sigma(int i) { return (i & ~7) | ((i & 3) << 1) | ((i >> 2) & 1); }
__device__ __forceinline__ at16v at_zero() { return at16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
// the wave's own LDS stores have landed and the compiler moves no access across
__device__ __forceinline__ void at_wave_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ float at_ninf() { return -__builtin_huge_valf(); }

// ---- mask bits -----------------------------------------------------------------------------------------------------------------------
struct BitsResized {                                                 // bit = the bilinear value at position s of the (h, w) grid is negative
    const float* pred; int H, W, w; float sy, sx;
    __device__ __forceinline__ bool operator()(size_t row, int s) const {
        const float* img = pred + row * (size_t)H * W;
        const int y = s / w, x = s - y * w;
        const float fy = fmaxf(sy * (y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * (x + 0.5f) - 0.5f, 0.f);
        const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly = fminf(fmaxf(fy - y0, 0.f), 1.f), lx = fminf(fmaxf(fx - x0, 0.f), 1.f);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float v = hy * (hx * img[(size_t)y0 * W + x0] + lx * img[(size_t)y0 * W + x1]) +
                        ly * (hx * img[(size_t)y1 * W + x0] + lx * img[(size_t)y1 * W + x1]);
        return v < 0.f;
    }
};
struct BitsBytes {
    const uint8_t* mask; int S;
    __device__ __forceinline__ bool operator()(size_t row, int s) const { return mask[row * (size_t)S + s] != 0; }
};

template <typename Src>
__global__ void __launch_bounds__(256) attn_bits_kernel(const Src src, uint32_t* __restrict__ bits, int S, int words, int repair) {
    __shared__ int s4[4];
    const size_t row = blockIdx.x;
    uint32_t* out = bits + row * (size_t)words;
    const int lane = threadIdx.x & 63;
    int count = 0;
    for (int base = 0; base < words * 32; base += 256) {             // the same trip count for every thread: the ballot is of whole waves
        const int s = base + (int)threadIdx.x;
        const bool set = s < S && src(row, s);
        const unsigned long long bal = __ballot(set);
        const int word = s >> 5;
        if ((lane & 31) == 0 && word < words) {                      // lanes 0 and 32 each store one word
            const uint32_t wv = (uint32_t)(bal >> lane);
            out[word] = wv;
            count += __popc(wv);
        }
    }
    if (!repair) return;
    const int total = block_sum_4w_i32(count, s4);
    if (total != S) return;
    for (int base = 0; base < words * 32; base += 256) {             // the lanes that stored a word store it again
        const int word = (base + (int)threadIdx.x) >> 5;
        if ((lane & 31) == 0 && word < words) out[word] = 0u;
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                       const uint32_t* __restrict__ bits, float* __restrict__ pm, float* __restrict__ pl,
                                                       float* __restrict__ pacc, int Q, int S, int B, int M, float scale, int words,
                                                       int per_head, int vec) {
    constexpr int KC = D == 64 ? 64 : 128, DS = D + 1, DB = (D + 31) / 32, KSTEPS = D / 2, PER = KC * D / 256;
    __shared__ float kv_lds[2 * KC * DS];                            // K and V of a chunk; at the end the waves' O tiles, 32 x DS each
    static_assert(2 * KC * DS >= 4 * 32 * DS, "the four waves' O tiles fit where K and V were");
    float* Ks = kv_lds;
    float* Vs = kv_lds + KC * DS;
    const int span = blockIdx.x, nspans = gridDim.x, bm = blockIdx.y, b = bm / M, m = bm - b * M;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int s0 = span * kAtSpan;
    const size_t rs = (size_t)B * M * D, head = ((size_t)b * M + m) * D;
    const int qblock = ((int)blockIdx.z * 4 + wave) * 32, qi = qblock + r;
    const bool wave_on = qblock < Q, q_on = qi < Q;
    float qreg[KSTEPS];
#pragma unroll
    for (int st = 0; st < KSTEPS; ++st) {
        const float x = q[(size_t)min(qi, Q - 1) * rs + head + 2 * st + half];
        qreg[st] = q_on ? x * scale : 0.f;
    }
    // the mask words of this lane's query: one per tile of 32 keys, asked for in front of the tile's score product
    const uint32_t* mrow = (bits && q_on) ? bits + ((size_t)(per_head ? bm : b) * Q + qi) * words : nullptr;
    at16v o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o[db] = at_zero();
    float mrun = at_ninf(), lrun = 0.f;
    for (int c = 0; c < kAtSpan / KC; ++c) {
        const int c0 = s0 + c * KC;
        if (c0 >= S) break;                                          // the same for the whole workgroup
        __syncthreads();
        if (vec) {                                                   // 16-byte aligned k and v: four channels per load
            float4 kv[PER / 4], vv[PER / 4];
#pragma unroll
            for (int u = 0; u < PER / 4; ++u) {
                const int idx = u * 256 + (int)threadIdx.x, key = idx / (D / 4), d = 4 * (idx - key * (D / 4));
                const size_t at = (size_t)min(c0 + key, S - 1) * rs + head + d;
                kv[u] = *reinterpret_cast<const float4*>(k + at);
                vv[u] = *reinterpret_cast<const float4*>(v + at);
            }
#pragma unroll
            for (int u = 0; u < PER / 4; ++u) {
                const int idx = u * 256 + (int)threadIdx.x, key = idx / (D / 4), d = 4 * (idx - key * (D / 4));
                const bool in = c0 + key < S;
                float* kd = Ks + key * DS + d;
                float* vd = Vs + key * DS + d;
                kd[0] = in ? kv[u].x : 0.f; kd[1] = in ? kv[u].y : 0.f; kd[2] = in ? kv[u].z : 0.f; kd[3] = in ? kv[u].w : 0.f;
                vd[0] = in ? vv[u].x : 0.f; vd[1] = in ? vv[u].y : 0.f; vd[2] = in ? vv[u].z : 0.f; vd[3] = in ? vv[u].w : 0.f;
            }
        } else {
            float kv[PER], vv[PER];
#pragma unroll
            for (int u = 0; u < PER; ++u) {                          // loads only, unconditional on a clamped address
                const int idx = u * 256 + (int)threadIdx.x, key = idx / D, d = idx - key * D;
                const size_t at = (size_t)min(c0 + key, S - 1) * rs + head + d;
                kv[u] = k[at];
                vv[u] = v[at];
            }
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int idx = u * 256 + (int)threadIdx.x, key = idx / D, d = idx - key * D;
                const bool in = c0 + key < S;
                Ks[key * DS + d] = in ? kv[u] : 0.f;
                Vs[key * DS + d] = in ? vv[u] : 0.f;
            }
        }
        __syncthreads();
        if (!wave_on) continue;
        for (int t = 0; t < KC / 32; ++t) {
            const int st0 = c0 + t * 32;
            if (st0 >= S) break;
            const int wi = st0 >> 5;                                  // < words: st0 < S
            const uint32_t word = mrow ? mrow[wi] : 0u;
            at16v sacc = at_zero();
            const float* krow = Ks + (t * 32 + at_sigma(r)) * DS + half;
#pragma unroll
            for (int st = 0; st < KSTEPS; ++st) sacc = at_mfma(krow[2 * st], qreg[st], sacc);
            float sv[16], tmax = at_ninf();
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int off = 2 * reg + half;
                const bool masked = ((word >> off) & 1u) || st0 + off >= S;
                sv[reg] = masked ? at_ninf() : sacc[reg];
                tmax = fmaxf(tmax, sv[reg]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mnew = fmaxf(mrun, tmax);
            const float msafe = mnew == at_ninf() ? 0.f : mnew;      // nothing unmasked so far: every p is exp(-inf) = 0
            const float alpha = expf(mrun - msafe);
            float psum = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                sv[reg] = expf(sv[reg] - msafe);
                psum += sv[reg];
            }
            lrun = lrun * alpha + psum;
            mrun = mnew;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) o[db][reg] *= alpha;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float* vrow = Vs + (t * 32 + 2 * reg + half) * DS;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int d = db * 32 + r;
                    const float a = vrow[min(d, D - 1)];
                    o[db] = at_mfma(d < D ? a : 0.f, sv[reg], o[db]);
                }
            }
        }
    }
    const float lsum = lrun + __shfl_xor(lrun, 32);
    __syncthreads();                                                 // K and V are done with: the O tiles go through their place
    if (!wave_on) return;
    const size_t slot = (size_t)bm * nspans + span;
    if (q_on && half == 0) {
        pm[slot * Q + qi] = mrun;
        pl[slot * Q + qi] = lsum;
    }
    float* tile = kv_lds + wave * 32 * DS;                           // [query][d]: a query's D values leave as one piece
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int d = db * 32 + at_row(reg, half);
            if (d < D) tile[r * DS + d] = o[db][reg];
        }
    at_wave_lds();
#pragma unroll
    for (int i = 0; i < 32; i += 2)
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const int row = i + half, d = db * 32 + r;
            const float x = tile[row * DS + min(d, D - 1)];
            if (qblock + row < Q && d < D) pacc[(slot * Q + qblock + row) * D + d] = x;
        }
}

__global__ void __launch_bounds__(256) attn_combine_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                           const float* __restrict__ pacc, float* __restrict__ out, float* __restrict__ lse,
                                                           int Q, int B, int M, int D, int nspans, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx % D), qi = (int)((idx / D) % Q), bm = (int)(idx / D / Q), b = bm / M, m = bm - b * M;
    const size_t slot0 = (size_t)bm * nspans;
    // eight spans' loads are asked for together (unconditional, on a clamped span), then used in span order: a load is a trip to L2
    float mx = at_ninf();
    for (int i0 = 0; i0 < nspans; i0 += 8) {
        float mi[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) mi[u] = pm[(slot0 + min(i0 + u, nspans - 1)) * Q + qi];
#pragma unroll
        for (int u = 0; u < 8; ++u) mx = fmaxf(mx, mi[u]);
    }
    float num = 0.f, den = 0.f;
    for (int i0 = 0; i0 < nspans; i0 += 8) {
        float mi[8], li[8], ai[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t at = (slot0 + min(i0 + u, nspans - 1)) * Q + qi;
            mi[u] = pm[at];
            li[u] = pl[at];
            ai[u] = pacc[at * D + d];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u >= nspans || mi[u] == at_ninf()) continue;    // (-inf, 0, 0): nothing of this span
            const float wgt = expf(mi[u] - mx);
            num += wgt * ai[u];
            den += wgt * li[u];
        }
    }
    const bool none = mx == at_ninf();                               // no unmasked key at all: NaN, as torch's softmax of a row of -inf
    const float nan = __builtin_nanf("");
    out[((size_t)qi * B + b) * M * D + (size_t)m * D + d] = none ? nan : num / den;
    if (d == 0) lse[(size_t)bm * Q + qi] = none ? nan : mx + logf(den);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ delta,
                                                         int Q, int B, int M, int D, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int qi = idx % Q, bm = idx / Q, b = bm / M, m = bm - b * M;
    const size_t at = ((size_t)qi * B + b) * M * D + (size_t)m * D;
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(dout[at + d], out[at + d], s);
    delta[idx] = s;
}

template <int D>
__global__ void __launch_bounds__(512) attn_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, const uint32_t* __restrict__ bits,
                                                       const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dk,
                                                       float* __restrict__ dv, float* __restrict__ dqpart, int Q, int S, int B, int M,
                                                       float scale, int words, int per_head) {
    constexpr int DS = D + 1, DB = (D + 31) / 32, KSTEPS = D / 2, AS = 33, AREA = 32 * AS;
    __shared__ float Qs[32 * DS];
    __shared__ float dOs[32 * DS];
    __shared__ float lse_s[32];
    __shared__ float delta_s[32];
    __shared__ uint32_t mw_s[32 * kAtTiles];
    __shared__ float area[8 * AREA];
    const int span = blockIdx.x, nspans = gridDim.x, bm = blockIdx.y, b = bm / M, m = bm - b * M;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, half = lane >> 5;
    const int kt0 = span * kAtSpan + wave * 32, key = kt0 + r;
    const bool key_on = key < S;
    const size_t rs = (size_t)B * M * D, head = ((size_t)b * M + m) * D;
    float* area_w = area + wave * AREA;
    // K and V of the wave's 32 keys: the key on the lane (B operands of S and dP), and K with d on the lane (the A operand of dQ^T)
    float kB[KSTEPS], vB[KSTEPS], kA[DB][16];
#pragma unroll
    for (int st = 0; st < KSTEPS; ++st) {
        const size_t at = (size_t)min(key, S - 1) * rs + head + 2 * st + half;
        const float kx = k[at], vx = v[at];
        kB[st] = key_on ? kx : 0.f;
        vB[st] = key_on ? vx : 0.f;
    }
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int kk = kt0 + 2 * st + half, d = db * 32 + r;
            const float kx = k[(size_t)min(kk, S - 1) * rs + head + min(d, D - 1)];
            kA[db][st] = (kk < S && d < D) ? kx : 0.f;
        }
    at16v dkacc[DB], dvacc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) { dkacc[db] = at_zero(); dvacc[db] = at_zero(); }
    const size_t slot = (size_t)bm * nspans + span;
    // a block's scaled q, dout, lse, delta and mask words: loaded into registers one block ahead, so that the loads fly during the products
    constexpr int NQ = 32 * D / 512;
    float nq[NQ], ng[NQ], nl = 0.f, nd = 0.f;
    uint32_t nw = 0u;
    auto fetch = [&](int q0) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int idx = u * 512 + tid, i = idx / D, d = idx - i * D;
            const size_t at = (size_t)min(q0 + i, Q - 1) * rs + head + d;
            const float qx = q[at], gx = dout[at];
            const bool in = q0 + i < Q;
            nq[u] = in ? qx * scale : 0.f;
            ng[u] = in ? gx : 0.f;
        }
        if (tid < 32) {
            const bool in = q0 + tid < Q;
            const size_t at = (size_t)bm * Q + min(q0 + tid, Q - 1);
            const float lx = lse[at], dx = delta[at];
            nl = in ? lx : 0.f;
            nd = in ? dx : 0.f;
        }
        if (tid < 32 * kAtTiles) {
            const int i = tid >> 3, wi = span * kAtTiles + (tid & 7);
            nw = 0u;
            if (bits && q0 + i < Q && wi < words) nw = bits[((size_t)(per_head ? bm : b) * Q + q0 + i) * words + wi];
        }
    };
    fetch(0);
    for (int q0 = 0; q0 < Q; q0 += 32) {
        // (the areas and these arrays are free: the barrier behind the last sum)
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int idx = u * 512 + tid, i = idx / D, d = idx - i * D;
            Qs[i * DS + d] = nq[u];
            dOs[i * DS + d] = ng[u];
        }
        if (tid < 32) {
            lse_s[tid] = nl;
            delta_s[tid] = nd;
        }
        if (tid < 32 * kAtTiles) mw_s[tid] = nw;
        __syncthreads();
        if (q0 + 32 < Q) fetch(q0 + 32);
        at16v sacc = at_zero(), dpacc = at_zero();
        const float* qrow = Qs + at_sigma(r) * DS + half;
        const float* grow = dOs + at_sigma(r) * DS + half;
#pragma unroll
        for (int st = 0; st < KSTEPS; ++st) sacc = at_mfma(qrow[2 * st], kB[st], sacc);
#pragma unroll
        for (int st = 0; st < KSTEPS; ++st) dpacc = at_mfma(grow[2 * st], vB[st], dpacc);
        float p[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = 2 * reg + half;
            const bool masked = ((mw_s[i * kAtTiles + wave] >> r) & 1u) || !key_on || q0 + i >= Q;
            const float e = expf(sacc[reg] - lse_s[i]);
            p[reg] = masked ? 0.f : e;
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {                         // dV^T += dO^T P
            const float* row = dOs + (2 * reg + half) * DS;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const int d = db * 32 + r;
                const float a = row[min(d, D - 1)];
                dvacc[db] = at_mfma(d < D ? a : 0.f, p[reg], dvacc[db]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) p[reg] = p[reg] * (dpacc[reg] - delta_s[2 * reg + half]);       // dS
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {                         // dK^T += Q^T dS
            const float* row = Qs + (2 * reg + half) * DS;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const int d = db * 32 + r;
                const float a = row[min(d, D - 1)];
                dkacc[db] = at_mfma(d < D ? a : 0.f, p[reg], dkacc[db]);
            }
        }
        // dQ^T [d][query] of the wave's keys = K^T dS^T: dS to the wave's area as [query][key], read back with the query on the lane
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) area_w[(2 * reg + half) * AS + r] = p[reg];
        at_wave_lds();
        float bv[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) bv[st] = area_w[r * AS + 2 * st + half];
        at_wave_lds();
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            at16v dq = at_zero();
#pragma unroll
            for (int st = 0; st < 16; ++st) dq = at_mfma(kA[db][st], bv[st], dq);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) area_w[r * AS + at_row(reg, half)] = dq[reg];            // [query][d of the block]
            __syncthreads();
            for (int e = tid; e < 32 * 32; e += 512) {               // the eight waves' tiles in wave order
                const int qq = e >> 5, dl = e & 31, d = db * 32 + dl;
                float s = area[qq * AS + dl];
#pragma unroll
                for (int w = 1; w < 8; ++w) s += area[w * AREA + qq * AS + dl];
                if (d < D && q0 + qq < Q) dqpart[(slot * Q + q0 + qq) * D + d] = s;
            }
            __syncthreads();
        }
    }
    // dk and dv of the wave's keys: through the wave's area, so that a row of D floats is stored as one piece
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        float* dst = which ? dv : dk;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const at16v acc = which ? dvacc[db] : dkacc[db];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) area_w[at_row(reg, half) * AS + r] = acc[reg];           // [d of the block][key]
            at_wave_lds();
#pragma unroll
            for (int st = 0; st < 16; ++st) {
                const int kk = kt0 + 2 * st + half, d = db * 32 + r;
                const float x = area_w[r * AS + 2 * st + half];
                if (kk < S && d < D) dst[(size_t)kk * rs + head + d] = x;
            }
            at_wave_lds();
        }
    }
}

__global__ void __launch_bounds__(256) attn_dq_kernel(const float* __restrict__ dqpart, float* __restrict__ dq, int Q, int B, int M, int D,
                                                      int nspans, float scale, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx % D), qi = (int)((idx / D) % Q), bm = (int)(idx / D / Q), b = bm / M, m = bm - b * M;
    const size_t slot0 = (size_t)bm * nspans;
    float s = 0.f;
    for (int i0 = 0; i0 < nspans; i0 += 8) {                         // eight loads together, added in span order
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = dqpart[((slot0 + min(i0 + u, nspans - 1)) * Q + qi) * D + d];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < nspans) s += x[u];
    }
    dq[((size_t)qi * B + b) * M * D + (size_t)m * D + d] = s * scale;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int attn_shape(int B, int M, int Q, int S, int D) {
    if (B < 1 || M < 1 || Q < 1 || S < 1 || D < 1) return BXI_ERR_BAD_SHAPE;
    if (D != 16 && D != 32 && D != 64) return BXI_ERR_UNSUPPORTED;
    if (Q > BXI_ATTN_MAX_Q || S > BXI_ATTN_MAX_S || (int64_t)B * M > BXI_ATTN_MAX_HEADS) return BXI_ERR_BAD_SHAPE;
    if (!fits_i32((int64_t)Q * B * M * D) || !fits_i32((int64_t)S * B * M * D)) return BXI_ERR_BAD_SHAPE;
    return BXI_OK;
}
static int attn_spans(int S) { return (S + kAtSpan - 1) / kAtSpan; }

template <typename Src>
static int attn_bits_launch(const Src& src, const char* label, uint32_t* bits, int64_t rows, int S, int repair, hipStream_t s) {
    const int words = (S + 31) / 32;
    BXI_LAUNCH(label, s, attn_bits_kernel<Src>, dim3((unsigned)rows), dim3(256), 0, s, src, bits, S, words, repair);
    return check_launch();
}

}  // namespace bxi

extern "C" int bxi_attn_mask_bits_f32(const float* mask_pred, int B, int Q, int H, int W, int h, int w, uint32_t* bits, void* stream) {
    using namespace bxi;
    if (B < 1 || Q < 1 || H < 1 || W < 1 || h < 1 || w < 1) return BXI_ERR_BAD_SHAPE;
    if ((int64_t)h * w > BXI_ATTN_MAX_S || !fits_i32((int64_t)B * Q * H * W) || !fits_i32((int64_t)B * Q)) return BXI_ERR_BAD_SHAPE;
    if (!mask_pred || !bits) return BXI_ERR_NULL_POINTER;
    const BitsResized src = {mask_pred, H, W, w, (float)H / (float)h, (float)W / (float)w};
    return attn_bits_launch(src, "attn_mask_bits", bits, (int64_t)B * Q, h * w, 1, as_stream(stream));
}

extern "C" int bxi_attn_pack_mask_u8(const uint8_t* mask, int rows, int S, uint32_t* bits, void* stream) {
    using namespace bxi;
    if (rows < 1 || S < 1 || S > BXI_ATTN_MAX_S) return BXI_ERR_BAD_SHAPE;
    if (!mask || !bits) return BXI_ERR_NULL_POINTER;
    const BitsBytes src = {mask, S};
    return attn_bits_launch(src, "attn_pack_mask", bits, rows, S, 0, as_stream(stream));
}

extern "C" size_t bxi_masked_attn_forward_workspace_bytes(int B, int M, int Q, int S, int D) {
    using namespace bxi;
    if (attn_shape(B, M, Q, S, D) != BXI_OK) return 0;
    return sizeof(float) * (size_t)attn_spans(S) * B * M * Q * (D + 2);
}

extern "C" int bxi_masked_attn_forward_f32(const float* q, const float* k, const float* v, const uint32_t* bits, int bits_per_head, int B, int M,
                                           int Q, int S, int D, float scale, float* out, float* lse, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    using namespace bxi;
    const int rc = attn_shape(B, M, Q, S, D);
    if (rc != BXI_OK) return rc;
    if (bits_per_head != 0 && bits_per_head != 1) return BXI_ERR_BAD_ARGUMENT;
    if (!q || !k || !v || !out || !lse) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_masked_attn_forward_workspace_bytes(B, M, Q, S, D), 16)) return BXI_ERR_WORKSPACE;
    const int nspans = attn_spans(S), words = (S + 31) / 32;
    const size_t slots = (size_t)nspans * B * M;
    float* pm = static_cast<float*>(workspace);
    float* pl = pm + slots * Q;
    float* pacc = pl + slots * Q;
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)nspans, (unsigned)(B * M), (unsigned)((Q + 127) / 128));
    const int vec = aligned(k, 16) && aligned(v, 16);                // rows of M * D floats, D a multiple of 16: every head's piece is aligned too
    if (D == 16) BXI_LAUNCH("masked_attn_fwd", s, attn_fwd_kernel<16>, grid, dim3(256), 0, s, q, k, v, bits, pm, pl, pacc, Q, S, B, M, scale, words, bits_per_head, vec);
    else if (D == 32) BXI_LAUNCH("masked_attn_fwd", s, attn_fwd_kernel<32>, grid, dim3(256), 0, s, q, k, v, bits, pm, pl, pacc, Q, S, B, M, scale, words, bits_per_head, vec);
    else BXI_LAUNCH("masked_attn_fwd", s, attn_fwd_kernel<64>, grid, dim3(256), 0, s, q, k, v, bits, pm, pl, pacc, Q, S, B, M, scale, words, bits_per_head, vec);
    int st = check_launch();
    if (st != BXI_OK) return st;
    const size_t total = (size_t)B * M * Q * D;
    BXI_LAUNCH("masked_attn_combine", s, attn_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pm, pl, pacc, out, lse, Q, B, M, D,
               nspans, total);
    return check_launch();
}

extern "C" size_t bxi_masked_attn_backward_workspace_bytes(int B, int M, int Q, int S, int D) {
    using namespace bxi;
    if (attn_shape(B, M, Q, S, D) != BXI_OK) return 0;
    return sizeof(float) * ((size_t)B * M * Q + (size_t)attn_spans(S) * B * M * Q * D);
}

extern "C" int bxi_masked_attn_backward_f32(const float* dout, const float* q, const float* k, const float* v, const uint32_t* bits,
                                            int bits_per_head, const float* out, const float* lse, int B, int M, int Q, int S, int D, float scale,
                                            float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    const int rc = attn_shape(B, M, Q, S, D);
    if (rc != BXI_OK) return rc;
    if (bits_per_head != 0 && bits_per_head != 1) return BXI_ERR_BAD_ARGUMENT;
    if (!dout || !q || !k || !v || !out || !lse || !dq || !dk || !dv) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_masked_attn_backward_workspace_bytes(B, M, Q, S, D), 16)) return BXI_ERR_WORKSPACE;
    const int nspans = attn_spans(S), words = (S + 31) / 32, rows = B * M * Q;
    float* delta = static_cast<float*>(workspace);
    float* dqpart = delta + rows;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("masked_attn_delta", s, attn_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, dout, out, delta, Q, B, M, D, rows);
    int st = check_launch();
    if (st != BXI_OK) return st;
    const dim3 grid((unsigned)nspans, (unsigned)(B * M));
    if (D == 16) BXI_LAUNCH("masked_attn_bwd", s, attn_bwd_kernel<16>, grid, dim3(512), 0, s, dout, q, k, v, bits, lse, delta, dk, dv, dqpart, Q, S, B, M, scale, words, bits_per_head);
    else if (D == 32) BXI_LAUNCH("masked_attn_bwd", s, attn_bwd_kernel<32>, grid, dim3(512), 0, s, dout, q, k, v, bits, lse, delta, dk, dv, dqpart, Q, S, B, M, scale, words, bits_per_head);
    else BXI_LAUNCH("masked_attn_bwd", s, attn_bwd_kernel<64>, grid, dim3(512), 0, s, dout, q, k, v, bits, lse, delta, dk, dv, dqpart, Q, S, B, M, scale, words, bits_per_head);
    st = check_launch();
    if (st != BXI_OK) return st;
    const size_t total = (size_t)rows * D;
    BXI_LAUNCH("masked_attn_dq", s, attn_dq_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dqpart, dq, Q, B, M, D, nspans, scale, total);
    return check_launch();
}
