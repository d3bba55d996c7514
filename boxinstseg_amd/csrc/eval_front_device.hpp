// eval_front_device.hpp -- the roles of the evaluation's first launch, which wait for nobody: table waves (table_wave, tab_entry), stream
// blocks (stream_block), pool blocks (pool_block), the head-fused first launch (head_prep_kernel) and pack_lab4_kernel for the generic
// image side.  Assumes eval_protocol_device.hpp (Ws, the tag, the loads past the caches) and dynamic_head_device.hpp.
#pragma once
#include "eval_protocol_device.hpp"

namespace bxi {

// ================================================================================================
// launch 1
// ================================================================================================
// ---- role 1: table waves (one wave per 64 table entries) --------------------------------------------------------------
struct LaneBox { int r0, r1, c0, c1, img, cnt; };
__device__ __forceinline__ int valid_cells(int limit_px, int stride, int n) {     // cells r with r*stride + stride/2 < limit_px
    const int half = stride / 2;
    const int v = limit_px - half <= 0 ? 0 : (limit_px - half + stride - 1) / stride;
    return min(v, n);
}
__device__ __forceinline__ LaneBox lane_box(const InstArgs& a, const ImageMeta& meta, int dil, int R, int m) {
    LaneBox lb = {0, 0, 0, 0, 0, 0};
    const int64_t g = a.gt_inds[m];
    const float* bp = nullptr;
    for (int b = 0; b < a.gt.B; ++b)      // uniform loop: the by-value kernel arguments are never indexed per lane
        if (g >= a.gt.first[b] && g < a.gt.first[b + 1]) {
            bp = a.gt.boxes[b] + 4 * (g - a.gt.first[b]); lb.img = b;
        }
    if (!bp) return lb;
    const Rect rc = box_rect(bp, a.Hc, a.Wc, a.stride, a.stride / 2, a.h, a.w);
    if (rc.r1 <= rc.r0 || rc.c1 <= rc.c0) return lb;
    lb.r0 = rc.r0; lb.r1 = rc.r1; lb.c0 = rc.c0; lb.c1 = rc.c1;
    const int r0 = max(rc.r0 - dil, 0), r1 = min(rc.r1 + dil, a.h);
    const int hc0 = max(rc.c0 - dil, 0), hc1 = min(rc.c1 + dil, a.w);
    const int tw = 64 - 2 * dil;
    lb.cnt = ((r1 - 1) / R - r0 / R + 1) * ((hc1 - hc0 + tw - 1) / tw);
    return lb;
}

__device__ __forceinline__ void publish_gathered_sumw(const InstArgs& a, const Ws& ws, int G, unsigned int key);
// `ready` != 0 (BXI_EVAL_TARGETS_READY; the value is the number of GT boxes + 1): the image side was evaluated by an earlier call (bxi_boxinst_targets_f32); sum W is then a GATHER --
// sum over the instances of their GT box's pair count (:1324-1328: the weights of instance n are its box's bitmask times the image's
// affinity mask, a function of the box and the image only) -- that the first table wave does behind its entries, instead of the
// predicate -> count -> reducer chain.  `key`: the digest of what the targets were computed for; a mismatch is a fault (loud).
__device__ __forceinline__ void table_wave(const InstArgs& a, const ImageMeta& meta, int dil, int R, const Ws& ws, const LossState& st, int k,
                                           bool write_status, int ready = 0, unsigned int key = 0u) {
    const int lane = threadIdx.x & 63;
    int base = 0, prefix = 0;
    LaneBox mine = {0, 0, 0, 0, 0, 0};
    for (int m0 = 0; m0 <= 64 * k; m0 += 64) {       // exclusive scan of the tile counts: deterministic offsets, no atomics
        const int m = m0 + lane;
        LaneBox lb = {0, 0, 0, 0, 0, 0};
        if (m < a.N) lb = lane_box(a, meta, dil, R, m);
        const int incl = wave_scan_incl_i32(lb.cnt);
        if (m0 == 64 * k) { prefix = base + incl - lb.cnt; mine = lb; }
        base += __shfl(incl, 63, 64);
    }
    const int m = 64 * k + lane;
    // the words that are polled later: zeroed here, written through, and DRAINED before the table entries that announce them go
    // out -- whoever holds a tagged entry m (entry 0) may use instance m's accumulators (the global ones).  No hipMemsetAsync, no
    // initialisation contract: in the two-launch form a kernel boundary follows anyway, in the single-launch form the tag orders it.
    if (m < a.N) {
        if (st.inst) { InstRec rc; rc.r0 = mine.r0; rc.r1 = mine.r1; rc.c0 = mine.c0; rc.c1 = mine.c1; rc.img = mine.img; rc.pad0 = rc.pad1 = rc.pad2 = 0; st.inst[m] = rc; }
#pragma unroll
        for (int sub = 0; sub < kAcc2Split; ++sub) __hip_atomic_store(acc2_word(ws.acc2, m, sub), 0ull, BXI_RLX, BXI_AGENT);
        __hip_atomic_store(&ws.dice[m], 0ull, BXI_RLX, BXI_AGENT);
    }
    if (k == 0) {
        __hip_atomic_store(&ws.acc1[(size_t)lane * kAcc2Stride], 0ull, BXI_RLX, BXI_AGENT);
        if (lane == 0) __hip_atomic_store(ws.sumw, 0ull, BXI_RLX, BXI_AGENT);
        if (lane == 0) __hip_atomic_store(ws.fault, 0u, BXI_RLX, BXI_AGENT);
        if (lane == 0 && st.status && write_status) { st.status[0] = 0; st.status[1] = R; }
    }
    drain_vmem();
    if (m < a.N)
        store_u64x2_through(reinterpret_cast<unsigned long long*>(ws.tab + m),
                            (unsigned long long)(unsigned int)(prefix | (mine.img << 24)) | ((unsigned long long)(unsigned int)(mine.r0 | (mine.r1 << 16)) << 32),
                            (unsigned long long)(unsigned int)(mine.c0 | (mine.c1 << 16)) | ((unsigned long long)ws.ep << 32));
    else if (m == a.N)
        store_u64x2_through(reinterpret_cast<unsigned long long*>(ws.tab + m), (unsigned long long)(unsigned int)prefix, (unsigned long long)ws.ep << 32);
    if (k != 0 || ready < 0) return;                // (ready < 0: targets ready, sum W is gathered by the reducer workgroup -- the single-launch form)
    if (!ready) {       // an evaluation that computes the image side itself overwrites lab4 / pred: targets an earlier call left are gone
        if (lane == 0) *ws.tkey() = 0u;
        return;
    }
    publish_gathered_sumw(a, ws, ready - 1, key);
}

// sum W = sum over the instances of their GT box's pair count (bxi_boxinst_targets_f32 left the counts): one wave.
// The targets must be THIS call's: the digest `key` covers the geometry and the box COUNTS (host data); the box COORDINATES are device data, so
// every instance's box is mapped to its cells again here -- from the evaluation's own boxes -- and compared with the rectangle the targets call
// recorded for that box (the counts were taken inside it).  A mismatch is a fault: NaN losses and a status word, never the old boxes' normaliser
// under the new boxes' rectangles.  (The IMAGE's pixels are not compared -- the evaluation does not read them with the targets ready: that the
// targets were made from this batch's images is the caller's side of the contract, include/boxinst_hip.h.)
__device__ __forceinline__ void publish_gathered_sumw(const InstArgs& a, const Ws& ws, int G, unsigned int key) {
    const int lane = threadIdx.x & 63;
    const unsigned int have = __hip_atomic_load(ws.tkey(), BXI_RLX, BXI_AGENT);
    double tot = 0.0;
    bool other_boxes = false;
    for (int m0 = 0; m0 < a.N; m0 += 64) {
        const int mm = m0 + lane;
        const int64_t g = mm < a.N ? a.gt_inds[mm] : -1;
        if (g >= 0 && g < G && g < kBoxCap) {
            unsigned long long c[kBoxSplit];
#pragma unroll
            for (int j = 0; j < kBoxSplit; ++j) c[j] = __hip_atomic_load(ws.boxcnt() + ((size_t)g * kBoxSplit + j) * kAcc2Stride, BXI_RLX, BXI_AGENT);
            const int4 rec = ws.boxtab()[g];                        // (img << 24, r0 | r1 << 16, c0 | c1 << 16, 0): written by an earlier launch
            const float* bp = nullptr;
            int img = 0;
            for (int b = 0; b < a.gt.B; ++b)                         // uniform loop: the by-value kernel arguments are never indexed per lane
                if (g >= a.gt.first[b] && g < a.gt.first[b + 1]) { bp = a.gt.boxes[b] + 4 * (g - a.gt.first[b]); img = b; }
            Rect rc = {0, 0, 0, 0};
            if (bp) rc = box_rect(bp, a.Hc, a.Wc, a.stride, a.stride / 2, a.h, a.w);
            other_boxes |= !bp || rec.x != (img << 24) || rec.y != (rc.r0 | (rc.r1 << 16)) || rec.z != (rc.c0 | (rc.c1 << 16));
#pragma unroll
            for (int j = 0; j < kBoxSplit; ++j) tot += (double)c[j];
        }
    }
    tot = wave_total_f64(tot);                                             // exact: integers far below 2^53
    const bool bad = __any(other_boxes) || have != key || key == 0u;
    if (lane == 0)
        __hip_atomic_store(ws.sumw, (1ull << 63) | (bad ? kSumwFault : 0ull) | (unsigned long long)tot, BXI_RLX, BXI_AGENT);
}

// This lane's table entry m (m <= N; `want` false: nothing).  Two-launch form: a plain load behind the kernel boundary.  Single-launch
// form (ONE): read past the caches until every wanted entry carries this evaluation's tag -- the table workgroup is the first of
// the grid and waits for nobody, so this is a wait for a workgroup that precedes the asker.  false = the bounded wait ran out.
template <bool ONE>
__device__ __forceinline__ bool tab_entry(const Ws& ws, int m, bool want, int spin_limit, int4& e) {
    if (!ONE) { e = want ? ws.tab[m] : make_int4(0, 0, 0, 0); return true; }
    for (int spins = 0; spins <= spin_limit; ++spins) {
        const u4v v = load16_past(ws.tab + (want ? m : 0));
        if (__all(!want || v.w == ws.ep)) {
            e = want ? make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w) : make_int4(0, 0, 0, 0);
            BXI_WL(1, spins);
            return true;
        }
        __builtin_amdgcn_s_sleep(kSleepTab);
    }
    e = make_int4(0, 0, 0, 0);
    return false;
}
// every entry 0..N tagged = every polled word of this evaluation zeroed (finisher, reducer)
template <bool ONE>
__device__ __forceinline__ bool table_complete(const Ws& ws, int N, int spin_limit) {
    if (!ONE) return true;
    const int lane = threadIdx.x & 63;
    int4 e;
    for (int m0 = 0; m0 <= N; m0 += 64)
        if (!tab_entry<true>(ws, m0 + lane, m0 + lane <= N, spin_limit, e)) return false;
    return true;
}

// ---- role 2: stream block = 4 waves x 8 rows of one instance map ---------------------------------------------------------
struct LogitRows {
    const float* L; int w, vec, nt;
    __device__ __forceinline__ float4 operator()(int r, int c) const {
        if (vec && nt) {      // non-temporal (launch_fused_eval decides: maps that outgrow the L2)
            typedef float f4n __attribute__((ext_vector_type(4)));
            const f4n t_ = __builtin_nontemporal_load(reinterpret_cast<const f4n*>(L + (int64_t)r * w + c));
            return make_float4(t_.x, t_.y, t_.z, t_.w);
        }
        return load4(L + (int64_t)r * w, c, w, vec);
    }
};

struct NoHook { __device__ __forceinline__ void operator()(Ws&) const {} };

// `after_loads(ws)` runs once the zero-fill stores and the first loads are issued: the place for work whose latency should hide
// behind them (the evaluation's tag, read from the device: with_tag)
template <bool ONE, typename Src, typename Hook = NoHook>
__device__ __forceinline__ void stream_block(const InstArgs& a, Ws& ws, float* __restrict__ g_logits, int vec, int sb,
                                             unsigned long long* colp /* LDS [kWaves][w] */, const Src& src, int tix, const Hook& after_loads = Hook()) {
    const int h = a.h, w = a.w;
    const int Sn = (h + kSBlk - 1) / kSBlk;
    const int n = sb / Sn, s = sb % Sn;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = s * kSBlk + wv * kSRows, r1 = min(h, r0 + kSRows);     // may be empty
    const int64_t P = (int64_t)h * w;
    float* G = g_logits ? g_logits + (int64_t)n * P : nullptr;
    const float4 ninf = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);

    if (G)   // zero-fill of d loss / d logits (depends on nothing); written through: drains while the launch is still reading
        for (int cb = 0; cb < w; cb += kChunkC) {
            const int c = cb + lane * 4;
            if (c < w) {
#pragma unroll
                for (int i = 0; i < kSRows; ++i)
                    if (r0 + i < r1) {
                        if (vec) store4_through(G + (int64_t)(r0 + i) * w + c, 0.f, 0.f, 0.f, 0.f);
                        else
                            for (int j = 0; j < 4; ++j)
                                if (c + j < w) __hip_atomic_store(G + (int64_t)(r0 + i) * w + c + j, 0.f, BXI_RLX, BXI_AGENT);
                    }
            }
        }
    float4 v[kSRows];
    {
        const int c = lane * 4;
#pragma unroll
        for (int i = 0; i < kSRows; ++i) v[i] = (r0 + i < r1 && c < w) ? src(r0 + i, c) : ninf;
    }
    after_loads(ws);
    BXI_TW(0, tix, 1);
    float rmax[kSRows]; int rcol[kSRows];
#pragma unroll
    for (int i = 0; i < kSRows; ++i) { rmax[i] = -INFINITY; rcol[i] = 0; }
    for (int cb = 0;;) {
        const int c = cb + lane * 4;
        if (c < w) {
            float cmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int crow[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < kSRows; ++i) {
                if (r0 + i < r1) {
                    float m = v[i].x; int mc = c;                       // first column wins ties
                    if (v[i].y > m) { m = v[i].y; mc = c + 1; }
                    if (v[i].z > m) { m = v[i].z; mc = c + 2; }
                    if (v[i].w > m) { m = v[i].w; mc = c + 3; }
                    if (m > rmax[i]) { rmax[i] = m; rcol[i] = mc; }     // chunks ascend: strict > keeps the first
                    if (v[i].x > cmax[0]) { cmax[0] = v[i].x; crow[0] = i; }   // ascending row, strict >: first row wins
                    if (v[i].y > cmax[1]) { cmax[1] = v[i].y; crow[1] = i; }
                    if (v[i].z > cmax[2]) { cmax[2] = v[i].z; crow[2] = i; }
                    if (v[i].w > cmax[3]) { cmax[3] = v[i].w; crow[3] = i; }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < w) colp[(size_t)wv * w + c + j] = pack_max(cmax[j], (uint32_t)(r0 + crow[j]));   // absolute row
        }
        cb += kChunkC;
        if (cb >= w) break;
        const int c2 = cb + lane * 4;
#pragma unroll
        for (int i = 0; i < kSRows; ++i) v[i] = (r0 + i < r1 && c2 < w) ? src(r0 + i, c2) : ninf;
    }
    BXI_TW(0, tix, 2);
    float wmax[kSRows];
#pragma unroll
    for (int i = 0; i < kSRows; ++i) wmax[i] = rmax[i];
    // eight maxima over the wave side by side: within rows of 16 lanes by DPP, the four rows by v_readlane (no LDS crossbar)
    wave_total_steps([&](int c) {
        float o[kSRows];
#pragma unroll
        for (int i = 0; i < kSRows; ++i) o[i] = __int_as_float(dpp_i32(__float_as_int(wmax[i]), c));
#pragma unroll
        for (int i = 0; i < kSRows; ++i) wmax[i] = fmaxf(wmax[i], o[i]);
    });
#pragma unroll
    for (int i = 0; i < kSRows; ++i) {
        const int b = __float_as_int(wmax[i]);
        wmax[i] = fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 0)), __int_as_float(__builtin_amdgcn_readlane(b, 16))),
                        fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 32)), __int_as_float(__builtin_amdgcn_readlane(b, 48))));
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int i = 0; i < kSRows; ++i) {
        const int col = first_col_of_max(rmax[i], rcol[i], wmax[i], w <= kChunkC);
        if (lane == i) mine = pack_max(wmax[i], (uint32_t)col);
    }
    if (lane < kSRows && r0 + lane < r1) {
        if (ONE) __hip_atomic_store(&ws.rowkey[(int64_t)n * h + r0 + lane], mine, BXI_RLX, BXI_AGENT);     // written through: read by a leader of this launch
        else ws.rowkey[(int64_t)n * h + r0 + lane] = mine;
    }
    BXI_TW(0, tix, 3);
    lds_barrier();
    BXI_TW(0, tix, 4);
    for (int c = threadIdx.x; c < w; c += kWaves * 64) {
        unsigned long long k = colp[c];
#pragma unroll
        for (int u = 1; u < kWaves; ++u) { const unsigned long long o = colp[(size_t)u * w + c]; k = o > k ? o : k; }
        if (ONE) __hip_atomic_store(&ws.colpart[((int64_t)n * Sn + s) * w + c], k, BXI_RLX, BXI_AGENT);
        else ws.colpart[((int64_t)n * Sn + s) * w + c] = k;       // larger value, then smaller row
    }
    if (ONE) {
        // single-launch form: this band's zero-fill and partial maxima are in memory (every wave drains its own stores, the
        // workgroup meets) before the band's flag says so to the instance's leader and to the tile waves that add onto these rows
        drain_vmem();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&ws.bandflag[(int64_t)n * ws.n_cb + s], ws.ep, BXI_RLX, BXI_AGENT);
    }
}

// ---- role 3: pool block = the 4 input rows of 64 pooled pixels ---------
__device__ __forceinline__ double lab_f(const double* lut, int i, int r8, int g8, int b8) {
    const double r = lut[r8], g = lut[g8], b = lut[b8];
    const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    const double white[3] = {0.95047, 1.0, 1.08883};
    const double m0 = i == 0 ? M[0][0] : (i == 1 ? M[1][0] : M[2][0]);
    const double m1 = i == 0 ? M[0][1] : (i == 1 ? M[1][1] : M[2][1]);
    const double m2 = i == 0 ? M[0][2] : (i == 1 ? M[1][2] : M[2][2]);
    const double wt = i == 0 ? white[0] : (i == 1 ? white[1] : white[2]);
    const double acc = __dadd_rn(__dadd_rn(__dmul_rn(m0, r), __dmul_rn(m1, g)), __dmul_rn(m2, b));
    const double v = acc / wt;
    return v > 0.008856 ? cbrt(v) : __dadd_rn(__dmul_rn(7.787, v), 16.0 / 116.0);
}

__device__ __forceinline__ void pool_load(const PoolArgs& pa, int item, int segs, int h, int w, float4 (&v)[3]) {
    const int seg = item % segs, r = (item / segs) % h, b = item / (segs * h);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = seg * 64 + lane;
    const int64_t plane = (int64_t)pa.Hc * pa.Wc;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < w) {
        const float* base = pa.imgs + (int64_t)b * 3 * plane + (int64_t)(4 * r + wv) * pa.Wc + 4 * c;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // non-temporal: 19.7 MB at 2 x 800 x 1024 that nobody reads twice -- kept out of the L2's way they leave it to the logits, the Lab records
            // and the predicate words the rest of the launch asks for again: 17.39 -> 16.92 us per evaluation at 32 instances, 22.4 -> 21.9 at 64,
            // 37.4 -> 36.7 at 128 (same box, interleaved three times; profiles/NOTES.md R6-7)
            typedef float f4n __attribute__((ext_vector_type(4)));
            const f4n t_ = __builtin_nontemporal_load(reinterpret_cast<const f4n*>(base + pa.dn.src_ch[ch] * plane));
            v[ch] = make_float4(t_.x, t_.y, t_.z, t_.w);
        }
    }
}

__device__ __forceinline__ float n2_of(float L0, float A0, float B0, float L1, float A1, float B1) {
    const float dL = L0 - L1, dA = A0 - A1, dB = B0 - B1;     // un-fused: the decision must equal get_image_color_similarity's (:237)
    return __fadd_rn(__fadd_rn(__fmul_rn(dL, dL), __fmul_rn(dA, dA)), __fmul_rn(dB, dB));
}

// items first, first + step, ... < n_items
template <typename Hook = NoHook>
__device__ __forceinline__ void pool_block(const PoolArgs& pa, Ws& ws, int first, int step, int n_items, double* lut /*[256]*/,
                                           int* part /*[4][3][64]*/, double* fch /*[3][64]*/, int tix, const Hook& after_loads = Hook()) {
    const int h = pa.Hc >> 2, w = pa.Wc >> 2;
    const int segs = (w + 63) >> 6;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float4 v[3], nx[3];
    pool_load(pa, first, segs, h, w, v);
    after_loads(ws);
    lut[threadIdx.x] = kSrgbLut[threadIdx.x];            // staged while the image loads fly
    for (int item = first; item < n_items; item += step) {
        const bool more = item + step < n_items;         // workgroup-uniform
        if (more) pool_load(pa, item + step, segs, h, w, nx);
        const int seg = item % segs, r = (item / segs) % h, b = item / (segs * h);
        const int c = seg * 64 + lane;
        const int y = 4 * r + wv;
        const bool act = c < w;
        const int ih = pa.meta.img_h[b], iw = pa.meta.img_w[b];
        const int x0 = 4 * c;
        const bool yin = y < ih;
        int sum[3];
        if (__all(!act || (yin && x0 + 3 < iw))) {       // wave-uniform: the whole row segment is image, not canvas padding
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double s = pa.dn.stdv[pa.dn.src_ch[ch]], m = pa.dn.mean[pa.dn.src_ch[ch]];
                sum[ch] = denorm_u8(v[ch].x, s, m) + denorm_u8(v[ch].y, s, m) + denorm_u8(v[ch].z, s, m) + denorm_u8(v[ch].w, s, m);
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double s = pa.dn.stdv[pa.dn.src_ch[ch]], m = pa.dn.mean[pa.dn.src_ch[ch]];
                int t = 0;
                t += (yin && x0 + 0 < iw) ? denorm_u8(v[ch].x, s, m) : 0;
                t += (yin && x0 + 1 < iw) ? denorm_u8(v[ch].y, s, m) : 0;
                t += (yin && x0 + 2 < iw) ? denorm_u8(v[ch].z, s, m) : 0;
                t += (yin && x0 + 3 < iw) ? denorm_u8(v[ch].w, s, m) : 0;
                sum[ch] = t;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) part[(wv * 3 + ch) * 64 + lane] = sum[ch];
        BXI_TW(0, tix, 1);
        lds_barrier();
        BXI_TW(0, tix, 2);
        if (wv < 3) {                                     // wave-uniform: wave i takes channel i of XYZ -> f_i
            int px[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                px[ch] = (part[(0 * 3 + ch) * 64 + lane] + part[(1 * 3 + ch) * 64 + lane] + part[(2 * 3 + ch) * 64 + lane] +
                          part[(3 * 3 + ch) * 64 + lane]) >> 4;
            fch[wv * 64 + lane] = lab_f(lut, wv, px[0], px[1], px[2]);
        }
        BXI_TW(0, tix, 3);
        lds_barrier();
        BXI_TW(0, tix, 4);
        if (wv == 3 && act) {       // one 16-byte store per pooled pixel (the wave that had no channel to compute)
            const double f0 = fch[lane], f1 = fch[64 + lane], f2 = fch[128 + lane];
            // the fourth component is this evaluation's tag: a predicate wave of the SAME launch (single-launch form) re-reads a pixel
            // until it carries it; the record is one 16-byte store, written through
            store4_through(reinterpret_cast<float*>(ws.lab4 + ((int64_t)b * h + r) * w + c), (float)__dadd_rn(__dmul_rn(116.0, f1), -16.0),
                           (float)__dmul_rn(500.0, __dadd_rn(f0, -f1)), (float)__dmul_rn(200.0, __dadd_rn(f1, -f2)), __uint_as_float(ws.ep));
        }
        // the next trip's `part` writes come after this barrier; its `fch` writes after the next one, which wave 3 reaches only
        // after it has read `fch` here: no extra barrier needed
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = nx[ch];
    }
}

// (prep_kernel, the first launch of the two-launch form, follows the roles of the second launch below: its folded form runs two of them)

// ---- head-fused first launch ----------------------------------------------------------------------------
// CondInstMaskHead.forward (condinst_head.py:1139-1164) and the evaluation's first launch as ONE grid of independent roles:
//   [table blocks][pool blocks][head tiles: instance x 8 x 32 tiles of y -> 16 x 64 logits]
// A head tile does the stream role's job on the tile it just produced: zero-filled gradient tile (written through), per-row and
// per-column (value, first index) maxima as partials for the leaders.  Nothing in the launch waits for anything else in it.
template <int C, bool REL>
__global__ __launch_bounds__(256, 7) void head_prep_kernel(PoolArgs pa, int n_pool, int n_items, InstArgs a, int dil, int R, Ws ws_in, LossState st,
                                                            float* __restrict__ g_logits, DynArgs da, const float* __restrict__ params,
                                                            float* __restrict__ logits_out, int ready, unsigned int key) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Ws ws = with_tag(ws_in);
    const int n_tab = ((a.N + 64) / 64 + kWaves - 1) / kWaves;
    const int blk = (int)blockIdx.x;
    const int tix = blk * kWaves + (int)(threadIdx.x >> 6);
    (void)tix;
    if (blk < n_tab) {
        const int k = blk * kWaves + (int)(threadIdx.x >> 6);
        if (64 * k <= a.N) table_wave(a, pa.meta, dil, R, ws, st, k, true, ready, key);
    } else if (blk < n_tab + n_pool) {
        double* lut = reinterpret_cast<double*>(smem);
        double* fch = lut + 256;
        int* part = reinterpret_cast<int*>(fch + 3 * 64);
        pool_block(pa, ws, blk - n_tab, n_pool, n_items, lut, part, fch, tix);
    } else {
        const int tiles_x = (da.W + kYC - 1) / kYC, tiles_y = (da.H + kHeadR - 1) / kHeadR;
        int t = blk - n_tab - n_pool;
        const int tx = t % tiles_x; t /= tiles_x;
        const int ty = t % tiles_y;
        const int n = t / tiles_y;
        unsigned long long* ckeys = reinterpret_cast<unsigned long long*>(smem);          // [4][64]
        float* otile = reinterpret_cast<float*>(ckeys + 4 * 64);                          // [2 kHeadR][64]
        float* ytile = otile + 2 * kHeadR * 64;                                           // [(kHeadR+1)*(kYC+1)]
        const DynEpi ep = {ws.colpart, ws.rowkey, g_logits, ws.n_cb, ws.n_rp, 0};
        dyn_tile_forward<C, REL, 2, true, kHeadR, kYC>(da, params, logits_out, n, ty, tx, ytile, otile, ckeys, ep);
    }
}

// ---- the image side for strides other than 4 / unaligned canvases: launches of their own (pool_rgb_generic of
// color_affinity.hip -> Lab planes, then this repacking) -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_lab4_kernel(const float* __restrict__ lab, float4* __restrict__ lab4, const unsigned int* __restrict__ epoch, int B,
                                                         int64_t P) {
    const unsigned int ep = next_tag(*epoch);          // as with_tag: the evaluation's tag is device state, never a kernel argument
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)B * P; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / P, p = i - b * P;
        const float* src = lab + b * 3 * P + p;
        lab4[i] = make_float4(src[0], src[P], src[2 * P], __uint_as_float(ep));
    }
}

}  // namespace bxi
