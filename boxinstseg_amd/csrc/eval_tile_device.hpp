// eval_tile_device.hpp -- the pair side of the evaluation: tile geometry (TG, Tile), the predicate wave of one pooled row segment (pred_item),
// the counts and their reducer, and the tile wave itself (math_tile: every unordered pair once, gradient added by float atomics).
// Assumes eval_protocol_device.hpp and the table of eval_front_device.hpp (tab_entry); knows nothing of leaders or finisher.
#pragma once
#include "eval_front_device.hpp"

namespace bxi {

// ================================================================================================
// launch 2
// ================================================================================================
template <int D, int R> struct TG { static constexpr int RD = R + 2 * D, TW = 64 - 2 * D; };

// The tile wave's pair terms that need the logits alone (log2 S and 1 / S of every pair) computed AHEAD of its wait for the predicate words and
// parked -- math_tile, phases A and B.  4-row tiles at dilation 2 only (the 8-row forms have twice the pairs and no room to park them; at
// dilation 1 the scalar loop, once split, is contracted differently by the compiler and no longer gives the un-split loop's bits: R12-1);
// one switch per kernel: the single launch that computes the image side (eval1_kernel<D, 4, false>), the single launch with the targets ready
// (eval1_kernel<D, 4, true>) and the second launch of the two-launch form (pair_kernel<D, 4>).  ON only where tile waves are resident before
// their words: in the other two every tile wave finds its words at once, phases A and B run back to back in every wave of a CU at the same
// time, and the parking traffic (16 KB through the LDS per wave) costs more than nothing -- targets ready, single launch: 13.6 -> 13.9 us at
// 32 instances, 16.85 -> 17.25 at 64; two launches at 64 instances: 22.2 -> 22.35, targets ready 17.4-17.8 -> 18.3 (profiles/NOTES.md R12-1).
// The terms and their order are the same either way, so every form gives the same bits with a switch on or off.
enum { kTilesPair = 0, kTilesOne = 1, kTilesOneReady = 2 };
constexpr bool kAheadOne = true, kAheadOneReady = false, kAheadTwo = false;
constexpr bool pair_ahead(int D, int R, int kern) {
    return R == 4 && D == 2 && (kern == kTilesOne ? kAheadOne : kern == kTilesOneReady ? kAheadOneReady : kAheadTwo);
}
constexpr int kParkBytes = 8192;                // LDS per tile wave for parked terms (128 bytes per lane); what does not fit stays in registers
// LDS of ONE tile wave: the log-space path's [R + 1][64] floats (slow_tile) and the parked pair terms share it -- a tile takes one path or the other
constexpr size_t tile_wave_lds(int D, int R, int kern) {
    return pair_ahead(D, R, kern) && (size_t)kParkBytes > sizeof(float) * (R + 1) * 64 ? (size_t)kParkBytes : sizeof(float) * (R + 1) * 64;
}

struct Tile {                                   // wave-uniform (SGPRs)
    int r0, r1, c0, c1;                         // cells whose sample lies in the GT box (bitmask == 1)
    int img, n, tile_r0, tile_c0;
    int vrow, vcol;                             // valid(q) <=> row(q) < vrow && col(q) < vcol
    int hc1;                                    // end column of the instance's tile hull (= dilated box)
};

__device__ __forceinline__ uint32_t row_bits(int lo, int hi, int base, int n) {   // bits j in [0,n) with lo <= base + j < hi
    const int a = max(lo - base, 0), b = min(hi - base, n);
    if (b <= a) return 0u;
    return ((1u << b) - 1u) & ~((1u << a) - 1u);              // n <= 16
}

// The four pair directions of a step i (j = i + D), every one between this lane and the lane D to its right or itself, so
// that only right-neighbour values are ever fetched:
//   0: A = (i, l)  B = (i, l + D)   |   1: A = (j, l)  B = (i, l + D)   |   2: A = (i, l)  B = (j, l)   |   3: A = (i, l)  B = (j, l + D)
// Pair weights, per step i:  W[k, A] and W[7 - k, B] -- [A in the GT box][B a valid image pixel][colour predicate of the pair] and the mirror --,
// and the same restricted to pixels this tile owns (math_tile builds them as bytes).
__device__ __forceinline__ uint32_t spread4(uint32_t x4) { return (x4 * 0x00204081u) & 0x01010101u; }   // bits 0..3 -> bytes 0..3
// the two 16-bit halves of a word times those of another (v_pk_mul_lo_u16 / v_pk_mad_u16: full rate, where a 32-bit multiply is a quarter-rate
// instruction and the 24-bit one loses the fourth byte)
typedef unsigned short us2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_mul_u16(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, (us2v)(__builtin_bit_cast(us2v, a) * __builtin_bit_cast(us2v, b))); }
__device__ __forceinline__ uint32_t pk_mad_u16(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_bit_cast(uint32_t, (us2v)(__builtin_bit_cast(us2v, a) * __builtin_bit_cast(us2v, b) + __builtin_bit_cast(us2v, c)));
}

template <int D>
__device__ __forceinline__ float lane_plus(float v) {
    int x = __float_as_int(v);
#pragma unroll
    for (int s = 0; s < D; ++s) x = __builtin_amdgcn_mov_dpp(x, 0x134 /* wave_rol:1 */, 0xf, 0xf, false);
    return __int_as_float(x);
}
template <int D>
__device__ __forceinline__ float lane_minus(float v) {
    int x = __float_as_int(v);
#pragma unroll
    for (int s = 0; s < D; ++s) x = __builtin_amdgcn_mov_dpp(x, 0x13C /* wave_ror:1 */, 0xf, 0xf, false);
    return __int_as_float(x);
}

// Generic (slow) evaluation of one tile: ordered pairs per owned pixel straight from global memory, pair value and
// gradient in log space exactly as pairwise.cu:38-61.  Taken for thresh <= 0 (zero_bit: padded / masked-out neighbours
// weigh 1) and for tiles with saturated logits (S underflows).  Gradients -> gout, the lane's sum W pw -> gout[R].
template <int D, int R, bool ONE>
__device__ __forceinline__ void slow_tile(const float* __restrict__ Lg, const float4* __restrict__ lab4, const Tile& t, float n2max, int zero_bit,
                                          int h, int w, int lane, float* gout /* LDS [R + 1][64] */) {
    const int c = t.tile_c0 - D + lane;
    const bool col_owned = lane >= D && lane < 64 - D && c < t.hc1;
    float num = 0.f;
    const float4* L0p = lab4 + (int64_t)t.img * h * w;
#pragma unroll 1
    for (int j = 0; j < R; ++j) {
        const int r = t.tile_r0 + j;
        float gacc = 0.f;
        if (col_owned && r < h) {
            const bool in_p = r >= t.r0 && r < t.r1 && c >= t.c0 && c < t.c1;
            const bool val_p = r < t.vrow && c < t.vcol;
            const int64_t pi = (int64_t)r * w + c;
            const float4 lp = ONE ? f4_of(load16_past(L0p + pi)) : L0p[pi];      // single-launch form: written by this launch, read past the caches
            const float xa = Lg[pi];
            const float ax = logsig(xa), bx = logsig(-xa);
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                const int kk = k < 4 ? k : k + 1;
                const int r2 = r + (kk / 3 - 1) * D, c2 = c + (kk % 3 - 1) * D;
                const bool inq = r2 >= 0 && r2 < h && c2 >= 0 && c2 < w;
                uint32_t pn = 0u;
                int64_t qi = 0;
                if (inq) {
                    qi = (int64_t)r2 * w + c2;
                    const float4 lq = ONE ? f4_of(load16_past(L0p + qi)) : L0p[qi];
                    pn = n2_of(lp.x, lp.y, lp.z, lq.x, lq.y, lq.z) <= n2max ? 1u : 0u;
                }
                const bool val_q = inq && r2 < t.vrow && c2 < t.vcol;
                const bool in_q = inq && r2 >= t.r0 && r2 < t.r1 && c2 >= t.c0 && c2 < t.c1;
                const uint32_t wp = in_p ? (val_q ? pn : (uint32_t)zero_bit) : 0u;
                const uint32_t wq = in_q ? (val_p ? pn : (uint32_t)zero_bit) : 0u;
                if (inq && (wp + wq)) {
                    const float xb = Lg[qi];
                    const float ay = logsig(xb), by = logsig(-xb);
                    const float e1 = ax + ay, e0 = bx + by;
                    const float nl2 = logsig(fabsf(e1 - e0)) - fmaxf(e1, e0);
                    num += (float)wp * nl2;
                    gacc += (float)(wp + wq) * (-(expf(ay) - expf(by)) * expf(ax + bx + nl2));
                }
            }
        }
        gout[j * 64 + lane] = gacc;
    }
    gout[R * 64 + lane] = num;
}

template <int D, int R>
__device__ __forceinline__ void load_plane(const float* __restrict__ plane, const Tile& t, int h, int w, int lane, float (&v)[R + 2 * D]) {
    const uint32_t cc4 = (uint32_t)min(max(t.tile_c0 - D + lane, 0), w - 1) * 4u;
    const char* pb = reinterpret_cast<const char*>(plane);                       // scalar base + 32-bit byte offset (one plane < 2^31 bytes)
#pragma unroll
    for (int j = 0; j < R + 2 * D; ++j) {
        const uint32_t rr = (uint32_t)min(max(t.tile_r0 - D + j, 0), h - 1);       // clamped: pairs with a pixel outside the map weigh 0
        v[j] = *reinterpret_cast<const float*>(pb + (rr * (uint32_t)w * 4u + cc4));
    }
}

// ---- predicate wave: one pooled row segment (64 pixels) of one image ------------------------------------------------------
// The colour pairs whose step row is pooled row r of segment `seg` of image b -- directions (get_image_color_similarity :220-246
// through unfold_wo_center's offsets :190-217, each unordered pair ONCE PER IMAGE, not once per instance and tile):
//   0: (r, c) - (r, c+D)    1: (r+D, c) - (r, c+D)    2: (r, c) - (r+D, c)    3: (r, c) - (r+D, c+D)
// -> one predicate byte per pixel (bit d: squared Lab distance <= n2max, i.e. sim >= thresh for a valid neighbour), and the
// segment's share of  sum W = sum_n sum_{p in box n} sum_k [sim_k(p) >= thresh]  (:1324-1328): a pair (p, q) weighs
// [p in box n][q valid] + [q in box n][p valid] for every instance n of the image (returned per lane; the workgroup arrives
// once with its total).  A byte carries its own "evaluated" bit: a tile wave re-reads the few bytes it needs until they have it.
__device__ __forceinline__ float lane_plus_n(float v, int d) {
    int x = __float_as_int(v);
    for (int s = 0; s < d; ++s) x = __builtin_amdgcn_mov_dpp(x, 0x134 /* wave_rol:1 */, 0xf, 0xf, false);
    return __int_as_float(x);
}
struct ValidCells { int vrow[BXI_MAX_IMAGES], vcol[BXI_MAX_IMAGES]; };   // per image: valid(q) <=> row(q) < vrow && col(q) < vcol (host: :1354-1369,:1405)
// PER_BOX (bxi_boxinst_targets_f32's second launch; never ONE): the rectangles are the GT BOXES' (ws.boxtab, n_ent of them) instead of the
// instances', and what a box containing a site adds is kept PER BOX (`boxacc`, LDS of the workgroup, one counter per box) instead of
// summed -- the evaluation that follows gathers sum W from its instances' boxes.  No tag is read or written (the consumer is a later launch).
template <bool ONE, bool PER_BOX = false>
__device__ __forceinline__ int pred_item(int h, int w, int n_ent, const ValidCells& vc, Ws& ws, int D, float n2max, int item, int segs, int spin_limit, bool& ok,
                                         int* boxacc = nullptr) {
    const int lane = threadIdx.x & 63;
    const int seg = item % segs, r = (item / segs) % h, b = item / (segs * h);
    const int c = seg * 64 + lane, cn = c + D;
    const bool rowD = r + D < h;                                  // wave-uniform
    const float4* L4 = ws.lab4 + (int64_t)b * h * w;
    const int cc = min(c, w - 1), cx = min(lane >= 64 - D ? cn : c, w - 1), rD = min(r + D, h - 1);
    // this row, the row D below, and for the last D lanes their right neighbours (they live in the next segment)
    float4 o0, oD, x0, xD;
    // lane n: instance n's table entry (box cells, image), requested with the Lab
    int4 rect, rect1 = make_int4(-1, 0, 0, 0);
    if (ONE) {
        // single-launch form: the pool workgroups of THIS launch write these pixels (16-byte records carrying the evaluation's
        // tag, written through); they precede this wave in the grid and wait for nobody
        bool got = false;
        for (int spins = 0; spins <= spin_limit; ++spins) {
            u4v q0, q1, q2, q3, qe;      // the table entry travels with the pixels: one round trip
            if (ws.ep == 0u) {           // wave-uniform: this wave's first poll -- the evaluation's tag travels with it too (with_tag)
                unsigned int e;
                load16_past_x5_epoch(L4 + (int64_t)r * w + cc, L4 + (int64_t)rD * w + cc, L4 + (int64_t)r * w + cx, L4 + (int64_t)rD * w + cx,
                                     ws.tab + (lane < n_ent ? lane : 0), ws.epoch, q0, q1, q2, q3, qe, e);
                ws.ep = next_tag((unsigned int)__builtin_amdgcn_readfirstlane((int)e));
            } else
                load16_past_x5(L4 + (int64_t)r * w + cc, L4 + (int64_t)rD * w + cc, L4 + (int64_t)r * w + cx, L4 + (int64_t)rD * w + cx,
                               ws.tab + (lane < n_ent ? lane : 0), q0, q1, q2, q3, qe);
            if (__all(q0.w == ws.ep && q1.w == ws.ep && q2.w == ws.ep && q3.w == ws.ep && qe.w == ws.ep)) {
                o0 = f4_of(q0); oD = f4_of(q1); x0 = f4_of(q2); xD = f4_of(q3);
                rect = lane < n_ent ? make_int4((int)qe.x, (int)qe.y, (int)qe.z, (int)qe.w) : make_int4(-1, 0, 0, 0);
                got = true;
                BXI_WL(2, spins);
                break;
            }
            __builtin_amdgcn_s_sleep(kSleepPred);
        }
        if (!got) { ok = false; return 0; }
    } else {
        const bool untagged = !PER_BOX && ws.ep == 0u;               // wave-uniform: this wave's first item -- the epoch word rides with its loads
        unsigned int ew = 0u;
        if (untagged) ew = *ws.epoch;                                // (a plain load: the word was written by an earlier kernel)
        o0 = L4[(int64_t)r * w + cc]; oD = L4[(int64_t)rD * w + cc]; x0 = L4[(int64_t)r * w + cx]; xD = L4[(int64_t)rD * w + cx];
        rect = lane < n_ent ? (PER_BOX ? ws.boxtab()[lane] : ws.tab[lane]) : make_int4(-1, 0, 0, 0);
        // (entries 64..127 ride with the same round trip: a load per 64-entry chunk BEHIND the first chunk's arithmetic was a second dependent trip
        // in every item of an evaluation of more than 64 instances)
        if (n_ent > 64) rect1 = 64 + lane < n_ent ? (PER_BOX ? ws.boxtab()[64 + lane] : ws.tab[64 + lane]) : make_int4(-1, 0, 0, 0);
        if (untagged) ws.ep = next_tag((unsigned int)__builtin_amdgcn_readfirstlane((int)ew));
    }
    float nL = lane_plus_n(o0.x, D), nA = lane_plus_n(o0.y, D), nB = lane_plus_n(o0.z, D);
    float mL = lane_plus_n(oD.x, D), mA = lane_plus_n(oD.y, D), mB = lane_plus_n(oD.z, D);
    if (lane >= 64 - D) { nL = x0.x; nA = x0.y; nB = x0.z; mL = xD.x; mA = xD.y; mB = xD.z; }
    const bool cin = c < w, nin = cn < w;
    const bool p0 = cin && nin && n2_of(o0.x, o0.y, o0.z, nL, nA, nB) <= n2max;
    const bool p1 = cin && nin && rowD && n2_of(oD.x, oD.y, oD.z, nL, nA, nB) <= n2max;
    const bool p2 = cin && rowD && n2_of(o0.x, o0.y, o0.z, oD.x, oD.y, oD.z) <= n2max;
    const bool p3 = cin && nin && rowD && n2_of(o0.x, o0.y, o0.z, mL, mA, mB) <= n2max;
    if (cin) __hip_atomic_store(ws.pred + ((int64_t)b * h + r) * w + c, (ws.ep << 4) | (p0 ? 1u : 0u) | (p1 ? 2u : 0u) | (p2 ? 4u : 0u) | (p3 ? 8u : 0u),
                                BXI_RLX, BXI_AGENT);     // the evaluation's tag = "evaluated"; written through (sc1), read past the caches
    const int vrow = vc.vrow[b], vcol = vc.vcol[b];
    const bool v00 = r < vrow && c < vcol, v0n = r < vrow && cn < vcol, vD0 = r + D < vrow && c < vcol, vDn = r + D < vrow && cn < vcol;
    // what a box containing the site adds:  (r, c)  (r, c+D)  (r+D, c)  (r+D, c+D)
    const int s00 = (p0 && v0n) + (p2 && vD0) + (p3 && vDn), s0n = (p0 && v00) + (p1 && vD0), sD0 = (p1 && v0n) + (p2 && v00), sDn = (p3 && v00) ? 1 : 0;
    int cnt = 0;
    // LANE = RECTANGLE: what rectangle [r0, r1) x [c0, c1) collects from this row segment is a sum of the four site values over a RANGE of lanes
    //   rows r:      s00 over lanes [c0 - base, c1 - base)  +  s0n over lanes [c0 - D - base, c1 - D - base)        (base = the segment's first column)
    //   rows r + D:  sD0 over the first range               +  sDn over the second
    // so ONE prefix sum over the lanes -- the four values packed into the bytes of a word: a segment's sums are <= 192, 128, 128, 64, no byte
    // carries -- and four crossbar reads per lane serve 64 rectangles at once.  ~60 instructions per 64 rectangles where rounds 2-6 walked the
    // rectangles that reach the row one after the other (ballot, readlane, four range tests: ~22 instructions each -- a handful at 32 instances, 20-30
    // of an image's 64 at 128 instances, where the predicate workgroups hold the slots the tile workgroups are waiting for).  The same integers,
    // added in another order.  profiles/NOTES.md R6-9
    const uint32_t incl = wave_scan_incl_u32((uint32_t)s00 | ((uint32_t)s0n << 8) | ((uint32_t)sD0 << 16) | ((uint32_t)sDn << 24));
    const int base = seg * 64;
    for (int m0 = 0; m0 < n_ent; m0 += 64) {
        if (m0 == 64 && !ONE) rect = rect1;
        else if (m0) {
            if (PER_BOX) rect = m0 + lane < n_ent ? ws.boxtab()[m0 + lane] : make_int4(-1, 0, 0, 0);
            else if (!tab_entry<ONE>(ws, m0 + lane, m0 + lane < n_ent, spin_limit, rect)) { ok = false; return 0; }
            if (m0 + lane >= n_ent) rect = make_int4(-1, 0, 0, 0);
        }
        const int r0 = rect.y & 0xffff, r1 = (int)((unsigned int)rect.y >> 16), c0 = rect.z & 0xffff, c1 = (int)((unsigned int)rect.z >> 16);
        const bool mine = m0 + lane < n_ent && (int)((unsigned int)rect.x >> 24) == b;
        const bool rr = mine && r >= r0 && r < r1, rD2 = mine && r + D >= r0 && r + D < r1;
        if (!__any(rr || rD2)) continue;                       // wave-uniform
        const int i0 = min(max(c0 - base, 0), 64), i1 = min(max(c1 - base, 0), 64);
        const int j0 = min(max(c0 - D - base, 0), 64), j1 = min(max(c1 - D - base, 0), 64);
        // sum over the lanes below i (i in [0, 64]): the inclusive sum of lane i - 1
        const uint32_t ei0 = (uint32_t)__builtin_amdgcn_ds_bpermute(((i0 - 1) & 63) << 2, (int)incl), ei1 = (uint32_t)__builtin_amdgcn_ds_bpermute(((i1 - 1) & 63) << 2, (int)incl);
        const uint32_t ej0 = (uint32_t)__builtin_amdgcn_ds_bpermute(((j0 - 1) & 63) << 2, (int)incl), ej1 = (uint32_t)__builtin_amdgcn_ds_bpermute(((j1 - 1) & 63) << 2, (int)incl);
        const uint32_t X = (i1 > 0 ? ei1 : 0u) - (i0 > 0 ? ei0 : 0u), Y = (j1 > 0 ? ej1 : 0u) - (j0 > 0 ? ej0 : 0u);      // bytewise monotone: no borrows
        const int add = (rr ? (int)((X & 255u) + ((Y >> 8) & 255u)) : 0) + (rD2 ? (int)(((X >> 16) & 255u) + (Y >> 24)) : 0);
        if (PER_BOX) { if (add) atomicAdd(&boxacc[m0 + lane], add); }       // LDS; flushed once per workgroup (targets_pred_kernel)
        else cnt += add;
    }
    return cnt;
}

// sum W, once every pooled row segment has been evaluated: ONE word for the (hundreds of) askers; the reducer -- one wave of the
// finisher workgroup -- watches the 64 count words and publishes it.
__device__ __forceinline__ bool counts_complete(const Ws& ws, int n_items, double* total, bool* fault) {
    (void)n_items;
    const unsigned long long x = __hip_atomic_load(ws.sumw, BXI_RLX, BXI_AGENT);
    *total = (double)(x & (kSumwFault - 1ull));                         // exact: an integer far below 2^53
    if ((x >> 63) != 0ull && (x & kSumwFault)) *fault = true;
    return (x >> 63) != 0ull;
}
__device__ __forceinline__ bool reduce_counts(const Ws& ws, int n_items, int spin_limit) {
    for (int spins = 0; spins <= spin_limit; ++spins) {
        const unsigned long long x = __hip_atomic_load(&ws.acc1[(size_t)(threadIdx.x & 63) * kAcc2Stride], BXI_RLX, BXI_AGENT);
        const int arrived = wave_total_i32((int)(x >> 40));
        const double tot = wave_total_f64((double)(x & (kCountFault - 1ull)));        // exact
        const bool flt = __any((x & kCountFault) != 0ull);
        if (arrived == n_items) {
            if ((threadIdx.x & 63) == 0)
                __hip_atomic_store(ws.sumw, (1ull << 63) | (flt ? kSumwFault : 0ull) | (unsigned long long)tot, BXI_RLX, BXI_AGENT);
            BXI_WL(3, spins);
            return true;
        }
    }
    return false;
}
// thresh <= 0: every pair (padded ones too) weighs 1 (:1324), sum W = 8 x the box areas; no predicate waves then
__device__ __forceinline__ double total_weight_all_pairs(const InstArgs& a, const Ws& ws) {
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int m0 = 0; m0 < a.N; m0 += 64) {
        const int m = m0 + lane;
        if (m < a.N) {
            const int4 e = ws.tab[m];
            const int r0 = e.y & 0xffff, r1 = (int)((unsigned int)e.y >> 16), c0 = e.z & 0xffff, c1 = (int)((unsigned int)e.z >> 16);
            s += 8.0 * (double)((r1 - r0) * (int64_t)(c1 - c0));
        }
    }
    return wave_total_f64(s);
}

// ---- tile wave (wave64, no barrier; LDS only as the wave's own parking space, pair_ahead) -----------------------------------
// Every UNORDERED pair is evaluated once and feeds both of its pixels: f(p,q) = f(q,p), the two weights W[k,p] + W[7-k,q]
// share the colour predicate.  Per pixel (a, b) = (sigmoid(x), sigmoid(-x)), t = a - b, u = a b.  Per pair (p, q):
//   S = a_p a_q + b_p b_q ; pw = -log S ; d pw / d x_p = -t_q u_p / S ; d pw / d x_q = -t_p u_q / S      (pairwise.cu:38-61)
// S cannot underflow while every |x| <= 34; tiles with a larger logit take the log-space path.
// Its waits: the predicate bytes of its own pixels (bit 7 set), when the logits have arrived and the per-pixel quantities -- with
// 4-row tiles at dilation 2 in the un-split single launch also S, log2 S and 1 / S of every pair (math_tile, phase A) -- are computed;
// and, before the gradient goes out, sum W (the global normaliser, :1327-1328) = every predicate wave's arrival.  The
// predicate waves precede the tile waves in the grid and never wait; by the time a tile wave asks they are normally done.
// A tile wave's own few predicate words (written through by the predicate waves, which precede it in the grid), read past the
// caches until every one carries this evaluation's tag; usually they are there at once.
// BATCH: the words in one asm statement (one round trip).  Not in the short single-launch kernels (eval1_kernel<D, 4, *>): there a tile wave is resident
// before the predicate waves start and polls anyway -- the trips hide in that wait (17.15 us per evaluation either way, R6-11) --, and the statement's
// twelve early-clobber outputs leave the kernel with a 36-byte private segment that nothing ever touches.
template <int D, int R, bool BATCH>
__device__ __forceinline__ bool pred_words(const Ws& ws, const Tile& t, int h, int w, int c, int spin_limit, uint32_t (&pbyte)[R + D]) {
    const unsigned int* pp = ws.pred + (int64_t)t.img * h * w;            // scalar base + 32-bit byte offsets (one plane < 2^31 bytes)
    const uint32_t cc = (uint32_t)min(max(c, 0), w - 1);
    const unsigned int want = ws.pred_any ? 0u : ws.ep;       // words an earlier launch left (bxi_boxinst_targets_f32) carry tag 0: no tag of this evaluation
    uint32_t off[R + D];
#pragma unroll
    for (int i = 0; i < R + D; ++i) off[i] = ((uint32_t)min(max(t.tile_r0 - D + i, 0), h - 1) * (uint32_t)w + cc) * 4u;
    bool ok = false;
    for (int spins = 0; spins <= spin_limit; ++spins) {
        bool all = true;
        if constexpr (BATCH) {
            load_words_past<R + D>(pp, off, pbyte);
#pragma unroll
            for (int i = 0; i < R + D; ++i) all = all && (pbyte[i] >> 4) == want;
        } else {
#pragma unroll
            for (int i = 0; i < R + D; ++i) {
                pbyte[i] = __hip_atomic_load(pp + off[i] / 4u, BXI_RLX, BXI_AGENT);
                all = all && (pbyte[i] >> 4) == want;
            }
        }
        if (__all(all)) { ok = true; BXI_WL(4, spins); break; }
        if (ws.pred_any) break;        // targets ready: the words are an EARLIER launch's -- what is not there now will not come (foreign or overwritten targets: loud at once, not after kSpinLimit polls)
        __builtin_amdgcn_s_sleep(kSleepWords);
    }
    return ok;        // false: the caller's arrival says so, and the finisher turns both losses into NaN
}

// A tile wave's ONE arrival, with or without tiles: its share of sum W pw (+ 1.0: keeps the packed field non-negative -- S may exceed 1 by
// a rounding) and whether one of its bounded waits ran out, as one atomic without return on one of the N x 8 arrival words (each in its
// own 128 bytes).  The finisher counts WAVES, so its last act -- advancing the workspace's epoch -- comes after every tile wave of
// the launch has read the epoch (an idle wave that started late could otherwise draw the NEXT evaluation's tag and wait for nobody).
// WHICH word: one of an instance whose table entry this wave has SEEN tagged -- the table wave of instances 64 k .. 64 k + 63 zeroes their arrival
// words and drains before it writes their entries, and a tile wave checks entries 0 .. 63 and N only (tile_role).  Rounds 3-5 spread the arrivals
// over all N x 8 words: in the single-launch forms a tile wave could then arrive on a word of instances 64 .. N - 1 that the SECOND table wave --
// draining its written-through zeroes under the logit stream's traffic -- had not zeroed yet; the zero wiped the arrival, the finisher never saw its
// count, ran out (status 2, NaN losses for that evaluation) after kSpinLimit polls = 4.1 s.  Seen five times in 4800 evaluations with the 8-row
// kernels at four workgroups per CU and 128 instances, where the tile workgroups start just as the stream workgroups' traffic lets the table's
// drains complete (profiles/NOTES.md R5-7, R6-3: the stall's length follows kSpinLimit, the wait that runs out is the finisher's).
// A wave whose bounded wait ran out (or that saw a fault word) says so on the evaluation's fault word BEFORE it arrives -- a returning atomic, waited
// for -- so that the round in which the finisher sees the last arrival sees the fault too.  (Rounds 3-5 added a flag bit to the arrival itself: with
// six arrivals per word four faults carry into the arrival count, the finisher never sees the count it waits for and the -- already loud -- error path
// takes kSpinLimit polls: 4.5 s for an evaluation whose targets are somebody else's.)
// WHEN: as soon as the share is complete -- behind the pair math of the wave's LAST tile, ahead of that tile's wait for sum W / the band flags
// and its adds (math_tile) --; a wave without tiles, or whose earlier wait ran out, after its tile loop; in the two-launch form and in the wrap
// evaluation (tag kMaxTag) after its adds -- there so that the finisher's zeroing of the workspace comes after every read of it (tile_role).
__device__ __forceinline__ void tile_wave_arrives(const Ws& ws, int N, int wid, long long fx_sum, bool bad) {
    if ((threadIdx.x & 63) == 0) {
        if (bad) {
            const unsigned int seen = __hip_atomic_fetch_or(ws.fault, kFaultCounts, BXI_RLX, BXI_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::"v"(seen) : "memory");
        }
        __hip_atomic_fetch_add(ws.acc2 + (size_t)(wid % ((N < 64 ? N : 64) * kAcc2Split)) * kAcc2Stride,
                               (1ull << 52) + (unsigned long long)(fx_sum + (1ll << 24)), BXI_RLX, BXI_AGENT);
    }
}

template <int D, int R, bool ONE, int KERN>
__device__ __forceinline__ void math_tile(const InstArgs& a, const Ws& ws, const Tile& t, float upw_warm, float n2max, int zero_bit, int n_items,
                                          int spin_limit, float& scale, bool& have_scale, float* __restrict__ g_logits, float* gbuf /* LDS of this wave: tile_wave_lds bytes */,
                                          int tix, long long& fx_sum, bool& bad_out, bool arrive, const LossState& st, float* __restrict__ losses) {
    constexpr int RD = TG<D, R>::RD;
    const int lane = threadIdx.x & 63;
    const int h = a.h, w = a.w, n = t.n;
    const int64_t P = (int64_t)h * w;
    const float* Lg = a.logits + (int64_t)n * P;
    const int c = t.tile_c0 - D + lane;
    const bool col_owned = g_logits && lane >= D && lane < 64 - D && c < t.hc1;
    float x[RD];
    load_plane<D, R>(Lg, t, h, w, lane, x);
    // targets ready: the predicate words are an earlier launch's -- asked for WITH the logits (one round trip instead of two; the per-pixel
    // arithmetic below runs while they fly), looked at once where the other forms start polling
    // (Measured and dropped, R6-13: the same early look in the two-launch form, where most tile waves get their slots behind the predicate workgroups --
    // 31.2 vs 30.6 us at 128 instances, 23.4 vs 22.8 with 4-row tiles at 64: the waves that come too early pay ten wasted loads and poll anyway.)
    uint32_t pearly[R + D];
    const bool early = ws.pred_any != 0u && zero_bit == 0;             // wave-uniform
    if (early) {
        const unsigned int* pp = ws.pred + (int64_t)t.img * h * w;
        const uint32_t cc = (uint32_t)min(max(c, 0), w - 1);
#pragma unroll
        for (int i = 0; i < R + D; ++i) pearly[i] = __hip_atomic_load(pp + (uint32_t)min(max(t.tile_r0 - D + i, 0), h - 1) * (uint32_t)w + cc, BXI_RLX, BXI_AGENT);
    }
    float g[R];
    float num = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j) g[j] = 0.f;
    // What runs BEFORE the wait for the predicate words needs the logits only: the per-pixel quantities of this lane and of the lane D to its
    // right (here) and, where pair_ahead says so, the pair terms S, log2 S, 1 / S (phase A below).  Behind the wait: the weights, then per pair
    // two multiply-adds and the gradient products (phase B), the arrival.
    // PK (even dilation): rows 2k, 2k + 1 ride in the two halves of packed FP32 instructions (v_pk_mul / v_pk_fma: two pairs per instruction;
    // the conversions and the two transcendentals per pair stay scalar).  Every row's gradient receives the same terms in the same order.
    // 122 -> 106 registers at <2, 4>, 159 -> 138 at <2, 8>; 17.43 -> 17.07 us per evaluation at 32 instances (same box).  (The 8-row role
    // fits 113 registers when t and u are made again per pair -- four workgroups per CU --: slower, and the targets-ready long form then
    // stalled for seconds at 128 instances with every slot of the device taken from the start: profiles/NOTES.md R5-7.  Not built.)
    constexpr bool PK = D % 2 == 0 && RD % 2 == 0;
    typedef float v2 __attribute__((ext_vector_type(2)));
    float pa_[PK ? 1 : RD], pb_[PK ? 1 : RD], pt_[PK ? 1 : RD], pu_[PK ? 1 : RD], aR[PK ? 1 : RD], bR[PK ? 1 : RD], tR[PK ? 1 : RD], uR[PK ? 1 : RD];
    v2 pa2[PK ? RD / 2 : 1], pb2[PK ? RD / 2 : 1], pt2[PK ? RD / 2 : 1], pu2[PK ? RD / 2 : 1], aR2[PK ? RD / 2 : 1], bR2[PK ? RD / 2 : 1],
        tR2[PK ? RD / 2 : 1], uR2[PK ? RD / 2 : 1];
    bool sat = false;
    if constexpr (PK) {
#pragma unroll
        for (int k = 0; k < RD / 2; ++k) {
            sat |= !(fabsf(x[2 * k]) <= 34.f) || !(fabsf(x[2 * k + 1]) <= 34.f);
            const float2 s0 = sig_pair(x[2 * k]), s1 = sig_pair(x[2 * k + 1]);
            pa2[k] = v2{s0.x, s1.x}; pb2[k] = v2{s0.y, s1.y};
            aR2[k] = v2{lane_plus<D>(s0.x), lane_plus<D>(s1.x)}; bR2[k] = v2{lane_plus<D>(s0.y), lane_plus<D>(s1.y)};
            pt2[k] = pa2[k] - pb2[k]; pu2[k] = pa2[k] * pb2[k]; tR2[k] = aR2[k] - bR2[k]; uR2[k] = aR2[k] * bR2[k];
        }
    } else {
#pragma unroll
    for (int j = 0; j < RD; ++j) {
        sat |= !(fabsf(x[j]) <= 34.f);
        const float2 s = sig_pair(x[j]); pa_[j] = s.x; pb_[j] = s.y; pt_[j] = s.x - s.y; pu_[j] = s.x * s.y;
        aR[j] = lane_plus<D>(pa_[j]); bR[j] = lane_plus<D>(pb_[j]); tR[j] = aR[j] - bR[j]; uR[j] = aR[j] * bR[j];
    }
    }
    const bool slow = zero_bit != 0 || __any(sat);
    // Phase A (pair_ahead): what a pair needs of the LOGITS alone -- S, log2 S, 1 / S, the two quarter-rate transcendentals per pair -- for every
    // pair the loop below visits, in its order and with its expressions, BEFORE the wait for the predicate words: a wave that is resident before
    // its words are there (the stream workgroups that stay on: most tile waves at 32 instances) does this arithmetic while it would otherwise
    // idle, and between seeing the words and the arrival only the weights and the multiply-adds remain.  Parked per lane: the first kParkBytes /
    // 64 bytes in the wave's LDS (slot s of lane l at [s][l]: nobody else reads it), the rest in registers -- the a / b planes that S needed are
    // dead from here on, which is the room.  A wave whose words are already there runs A and B back to back and pays the parking traffic only.
    constexpr bool AHEAD = pair_ahead(D, R, KERN);
    static_assert(!AHEAD || (PK && D == 2), "the packed loop only; slot numbering below: direction 0 is skipped in the first step only");
    constexpr int NSLOT = AHEAD ? 4 * ((R + D) / 2) - 1 : 0;                              // slot of (step, direction) = 4 step + direction - 1
    constexpr int NPARK = kParkBytes / (64 * 16), NLDS = AHEAD ? (NSLOT < NPARK ? NSLOT : NPARK) : 0;      // slots in LDS: 16 bytes (two pairs) each
    constexpr int NREG = AHEAD ? NSLOT - NLDS : 0;
    typedef float v4 __attribute__((ext_vector_type(4)));
    v2 klg2[NREG ? NREG : 1], krc2[NREG ? NREG : 1];
    if constexpr (AHEAD) {
        if (!slow) {
            if constexpr (PK) {
                v4* park = reinterpret_cast<v4*>(gbuf) + lane;
#define BXI_AHEAD2(ip, ka, kb, qa, qb, dir)                                                                         \
                {                                                                                                   \
                    const int s = 4 * (ip) + (dir) - 1;                                                             \
                    const v2 S = pa2[ka] * qa[kb] + pb2[ka] * qb[kb];                                               \
                    const v2 lg = {__builtin_amdgcn_logf(S.x), __builtin_amdgcn_logf(S.y)};                         \
                    const v2 rc = {__builtin_amdgcn_rcpf(S.x), __builtin_amdgcn_rcpf(S.y)};                         \
                    if (s < NLDS) park[s * 64] = v4{lg.x, lg.y, rc.x, rc.y};                                        \
                    else { klg2[s < NLDS ? 0 : s - NLDS] = lg; krc2[s < NLDS ? 0 : s - NLDS] = rc; }                \
                }
#pragma unroll
                for (int ip = 0; ip < (R + D) / 2; ++ip) {
                    const int jp = ip + D / 2;
                    if (2 * ip >= D) BXI_AHEAD2(ip, ip, ip, aR2, bR2, 0)
                    BXI_AHEAD2(ip, jp, ip, aR2, bR2, 1)
                    BXI_AHEAD2(ip, ip, jp, pa2, pb2, 2)
                    BXI_AHEAD2(ip, ip, jp, aR2, bR2, 3)
                }
#undef BXI_AHEAD2
#pragma unroll
                for (int k = 0; k < NREG; ++k) asm volatile("" : "+v"(klg2[k]), "+v"(krc2[k]));      // made HERE, not sunk behind the wait
            }
            asm volatile("" ::: "memory");        // the parked words are read back from the LDS behind the wait, not carried in registers across it
        }
    }
    bool bad = false;          // a bounded wait of this wave ran out (never expected): its arrival carries the fact to the finisher
    const int band0 = t.tile_r0 / kSBlk, band1 = (min(t.tile_r0 + R, h) - 1) / kSBlk;
    const bool look_early = !slow && (!have_scale || (ONE && g_logits));       // wave-uniform
    unsigned long long sw_early = 0ull;
    unsigned int f0e = 0u, f1e = 0u;
    BXI_TW(1, tix, 2);
    if (!slow) {
        uint32_t pbyte[R + D];
        if (early) {
            bool all = true;
#pragma unroll
            for (int i = 0; i < R + D; ++i) { pbyte[i] = pearly[i]; all = all && (pbyte[i] >> 4) == 0u; }      // (words an earlier launch left carry tag 0)
            bad |= !__all(all);
        } else bad |= !pred_words<D, R, (!ONE || R == 8)>(ws, t, h, w, c, spin_limit, pbyte);
        float gq[PK ? 1 : RD], gR[PK ? 1 : RD];      // gradient of this lane's pixels / of lane + D's
        v2 gq2[PK ? RD / 2 : 1], gR2[PK ? RD / 2 : 1];
        if constexpr (PK) {
#pragma unroll
            for (int k = 0; k < RD / 2; ++k) { gq2[k] = v2{0.f, 0.f}; gR2[k] = v2{0.f, 0.f}; }
        } else {
#pragma unroll
            for (int j = 0; j < RD; ++j) { gq[j] = 0.f; gR[j] = 0.f; }
        }
        // pair weights as bytes, four rows per word: cw = W[k,A] + W[7-k,B] (gradient), dw = the same restricted to
        // pixels this tile owns (loss sum)
        constexpr int NQ = (R + D + 3) / 4;
        uint32_t cw[4][NQ], dw[4][NQ];
        // Every mask of dir_masks is (a 0/1 of the LANE: its column in the box / valid / owned) x (a row range of the TILE: wave-uniform) x (the colour
        // predicate), so the weights are made in the byte domain at once: the predicate nibbles of four rows packed into a word (bytes = rows), one
        // shift + AND per direction, an AND with the row range's byte mask (scalar registers, made on the scalar unit) and a packed 16-bit multiply by the
        // lane's 0 / 1 / 2.  ~160 vector instructions per tile where the bit-mask form (transpose to row bits, AND the flag words, spread nibble by
        // nibble: rounds 3-6, ~300) stood next to ~500 of the pair loop itself.  The same bytes.  profiles/NOTES.md R6-11
        {
            uint32_t spb[4][NQ];
#pragma unroll
            for (int q4 = 0; q4 < NQ; ++q4) {
                uint32_t W = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * q4 + k < R + D) W |= (pbyte[4 * q4 + k] & 15u) << (8 * k);
#pragma unroll
                for (int d = 0; d < 4; ++d) spb[d][q4] = (W >> d) & 0x01010101u;
            }
            const int base = t.tile_r0 - D;
            const uint32_t rows_box = row_bits(t.r0, t.r1, base, RD), rows_val = row_bits(0, min(h, t.vrow), base, RD);
            const uint32_t rows_own = row_bits(t.tile_r0, min(t.tile_r0 + R, h), base, RD);
            const uint32_t X1 = rows_box & rows_val, X2 = (rows_box >> D) & rows_val, X3 = rows_box & (rows_val >> D);
            const uint32_t X1O = X1 & rows_own, X2OD = X2 & (rows_own >> D), X3O = X3 & rows_own;
            const int cl = t.tile_c0 - D + lane, cr = cl + D, cv = min(w, t.vcol);
            const bool inR = lane + D < 64;          // lanes without a right neighbour: every pair weight 0 (they receive some other lane's data)
            const uint32_t fa = cl >= t.c0 && cl < t.c1, fv = cl >= 0 && cl < cv, fo = lane >= D && lane < 64 - D && cl < t.hc1;
            const uint32_t faR = inR && cr >= t.c0 && cr < t.c1, fvR = inR && cr >= 0 && cr < cv, foR = inR && lane < 64 - 2 * D && cr < t.hc1;
            // the lane's multipliers, one per 16-bit half
            const uint32_t p1 = fa & fvR, q1 = faR & fv, s1 = fa & fv;
            const uint32_t kp = p1 * 0x10001u, kq = q1 * 0x10001u, ks = s1 * 0x10001u, kpq = kp + kq;
            const uint32_t kpo = (p1 & fo) * 0x10001u, kqo = (q1 & foR) * 0x10001u, kso = (s1 & fo) * 0x10001u, kpqo = kpo + kqo;
#pragma unroll
            for (int q4 = 0; q4 < NQ; ++q4) {
                const uint32_t b1 = spread4((X1 >> (4 * q4)) & 15u), b2 = spread4((X2 >> (4 * q4)) & 15u), b3 = spread4((X3 >> (4 * q4)) & 15u);
                const uint32_t b1o = spread4((X1O >> (4 * q4)) & 15u), b2o = spread4((X2OD >> (4 * q4)) & 15u), b3o = spread4((X3O >> (4 * q4)) & 15u);
                cw[0][q4] = pk_mul_u16(spb[0][q4] & b1, kpq);
                cw[1][q4] = pk_mad_u16(spb[1][q4] & b2, kp, pk_mul_u16(spb[1][q4] & b3, kq));
                cw[2][q4] = pk_mul_u16((spb[2][q4] & b3) + (spb[2][q4] & b2), ks);
                cw[3][q4] = pk_mad_u16(spb[3][q4] & b3, kp, pk_mul_u16(spb[3][q4] & b2, kq));
                dw[0][q4] = pk_mul_u16(spb[0][q4] & b1o, kpqo);
                dw[1][q4] = pk_mad_u16(spb[1][q4] & b2o, kpo, pk_mul_u16(spb[1][q4] & b3o, kqo));
                dw[2][q4] = pk_mul_u16((spb[2][q4] & b3o) + (spb[2][q4] & b2o), kso);
                dw[3][q4] = pk_mad_u16(spb[3][q4] & b3o, kpo, pk_mul_u16(spb[3][q4] & b2o, kqo));
            }
        }
        BXI_TW(1, tix, 3);
        // the first look at sum W (and, single-launch form, at the band flags of the rows this tile adds onto) goes out BEFORE the pair loop and is
        // evaluated behind it: the round trip hides under ~2 us of arithmetic; what is not there yet is polled for as before
        if (look_early) {
            if (!have_scale) sw_early = __hip_atomic_load(ws.sumw, BXI_RLX, BXI_AGENT);
            if (ONE && g_logits) {
                f0e = __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + band0], BXI_RLX, BXI_AGENT);
                f1e = __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + band1], BXI_RLX, BXI_AGENT);
            }
        }
        const v4* park2 = reinterpret_cast<const v4*>(gbuf) + lane;       // phase A's slots of this lane
        (void)park2;
        // one unordered pair: A = (row ra, this lane) ; B = (row rb of the lane `q` names) ; num collects -log2 S
#define BXI_PAIR(i, ra, rb, qa, qb, qt, qu, dir, GA, GB)                                                            \
        {                                                                                                           \
            const float gw = (float)((cw[dir][(i) >> 2] >> (8 * ((i) & 3))) & 255u);                                \
            const float nw = (float)((dw[dir][(i) >> 2] >> (8 * ((i) & 3))) & 255u);                                \
            const float S = pa_[ra] * qa[rb] + pb_[ra] * qb[rb];                    /* P(y_A == y_B) */            \
            num -= nw * __builtin_amdgcn_logf(S);                                   /* v_log_f32 = log2 */         \
            const float mm = gw * __builtin_amdgcn_rcpf(S);                                                         \
            GA -= mm * qt[rb] * pu_[ra];                                                                            \
            GB -= mm * pt_[ra] * qu[rb];                                                                            \
        }
        if constexpr (PK) {
            v2 num2 = {0.f, 0.f};
            // two unordered pairs: rows (2 ka, 2 ka + 1) of this lane against rows (2 kb, 2 kb + 1) of the lane `q` names; bytes 2 ip, 2 ip + 1 of the weights
#define BXI_PAIR2(ip, ka, kb, qa, qb, qt, qu, dir, GA, GB)                                                          \
            {                                                                                                       \
                const uint32_t cwd = cw[dir][(2 * (ip)) >> 2] >> (8 * ((2 * (ip)) & 3));                              \
                const uint32_t dwd = dw[dir][(2 * (ip)) >> 2] >> (8 * ((2 * (ip)) & 3));                              \
                const v2 gw = {(float)(cwd & 255u), (float)((cwd >> 8) & 255u)};                                      \
                const v2 nw = {(float)(dwd & 255u), (float)((dwd >> 8) & 255u)};                                      \
                v2 lg, rc;                                                                                            \
                if constexpr (AHEAD) {                                              /* phase B: parked by phase A */  \
                    const int s = 4 * (ip) + (dir) - 1;                                                               \
                    if (s < NLDS) { const v4 pk = park2[s * 64]; lg = v2{pk.x, pk.y}; rc = v2{pk.z, pk.w}; }          \
                    else { lg = klg2[s < NLDS ? 0 : s - NLDS]; rc = krc2[s < NLDS ? 0 : s - NLDS]; }                  \
                } else {                                                                                              \
                    const v2 S = pa2[ka] * qa[kb] + pb2[ka] * qb[kb];                                                 \
                    lg = v2{__builtin_amdgcn_logf(S.x), __builtin_amdgcn_logf(S.y)};                                  \
                    rc = v2{__builtin_amdgcn_rcpf(S.x), __builtin_amdgcn_rcpf(S.y)};                                  \
                }                                                                                                     \
                num2 -= nw * lg;                                                                                      \
                const v2 mm = gw * rc;                                                                                \
                GA -= mm * qt[kb] * pu2[ka];                                                                          \
                GB -= mm * pt2[ka] * qu[kb];                                                                          \
            }
#pragma unroll
            for (int ip = 0; ip < (R + D) / 2; ++ip) {
                const int jp = ip + D / 2;
                if (2 * ip >= D) BXI_PAIR2(ip, ip, ip, aR2, bR2, tR2, uR2, 0, gq2[ip], gR2[ip])
                BXI_PAIR2(ip, jp, ip, aR2, bR2, tR2, uR2, 1, gq2[jp], gR2[ip])
                BXI_PAIR2(ip, ip, jp, pa2, pb2, pt2, pu2, 2, gq2[ip], gq2[jp])
                BXI_PAIR2(ip, ip, jp, aR2, bR2, tR2, uR2, 3, gq2[ip], gR2[jp])
                if (2 * ip >= D) {
                    const float fromL0 = lane_minus<D>(gR2[ip].x), fromL1 = lane_minus<D>(gR2[ip].y);
                    g[2 * ip - D] = gq2[ip].x + (lane >= D ? fromL0 : 0.f);
                    g[2 * ip + 1 - D] = gq2[ip].y + (lane >= D ? fromL1 : 0.f);
                }
            }
#undef BXI_PAIR2
            num = num2.x + num2.y;
        } else {
#pragma unroll
        for (int i = 0; i < R + D; ++i) {
            const int j = i + D;
            if (i >= D) BXI_PAIR(i, i, i, aR, bR, tR, uR, 0, gq[i], gR[i])
            BXI_PAIR(i, j, i, aR, bR, tR, uR, 1, gq[j], gR[i])
            BXI_PAIR(i, i, j, pa_, pb_, pt_, pu_, 2, gq[i], gq[j])
            BXI_PAIR(i, i, j, aR, bR, tR, uR, 3, gq[i], gR[j])
            if (i >= D) {     // row i is complete: collect what the lane D to the left computed for it
                const float fromL = lane_minus<D>(gR[i]);
                g[i - D] = gq[i] + (lane >= D ? fromL : 0.f);
            }
        }
        }
        num *= 0.69314718055994531f;
#undef BXI_PAIR
    } else {         // wave-uniform; rare
        if (ONE) {   // single-launch form: the tile's predicate words vouch for the Lab pixels the log-space path reads
            uint32_t pbyte[R + D];
            bad |= !pred_words<D, R, (!ONE || R == 8)>(ws, t, h, w, c, spin_limit, pbyte);
        }
        slow_tile<D, R, ONE>(Lg, ws.lab4, t, n2max, zero_bit, h, w, lane, gbuf);
        num = gbuf[R * 64 + lane];
#pragma unroll
        for (int j = 0; j < R; ++j) g[j] = gbuf[j * 64 + lane];
    }
    BXI_TW(1, tix, 5);
    num = wave_total_f32(num);
    fx_sum += (long long)(num * kNumScale);                                    // this tile's share of sum W pw, fixed point: integer adds commute
    // `arrive` (the wave's last tile, outside the wrap evaluation -- tile_role): the wave's share of sum W pw is complete, and it is all the
    // finisher needs of it.  So the wave arrives HERE, ahead of its wait for sum W / the band flags and of its adds: the finisher no longer
    // waits for three hops whose results it never reads, and the launch ends at the later of the last tile wave's adds and the finisher's store.
    if (arrive) tile_wave_arrives(ws, a.N, tix, fx_sum, bad);
    // single-launch form: the rows this tile adds onto were zero-filled by stream workgroups of THIS launch; their band flags are
    // asked for in the same round as sum W
    bool bands_ok = !ONE || !g_logits;
    if (look_early) {
        if (!have_scale && (sw_early >> 63) != 0ull) {
            if (sw_early & kSumwFault) bad = true;
            have_scale = true;
            scale = upw_warm / fmaxf((float)(double)(sw_early & (kSumwFault - 1ull)), 1.f);
        }
        if (ONE && g_logits) bands_ok = f0e == ws.ep && f1e == ws.ep;
    }
    if (!have_scale || !bands_ok) {           // wave-uniform
        double total_w = 0.0;
        bool ok = false;
        for (int spins = 0; spins <= spin_limit; ++spins) {
            unsigned int f0 = ws.ep, f1 = ws.ep;
            if (!bands_ok) {
                f0 = __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + band0], BXI_RLX, BXI_AGENT);
                f1 = __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + band1], BXI_RLX, BXI_AGENT);
            }
            if (!have_scale) {
                if (zero_bit) { total_w = total_weight_all_pairs(a, ws); have_scale = true; }
                else have_scale = counts_complete(ws, n_items, &total_w, &bad);
                if (have_scale) scale = upw_warm / fmaxf((float)total_w, 1.f);
            }
            bands_ok = f0 == ws.ep && f1 == ws.ep;
            if (have_scale && bands_ok) { ok = true; BXI_WL(5, spins); break; }
            __builtin_amdgcn_s_sleep(kSleepSumw);
        }
        bad |= !ok;
        have_scale = true;
    }
    BXI_TW(1, tix, 4);
    if (arrive && bad) {      // wave-uniform; never expected
        // A wave that has arrived cannot tell the finisher any more: it is loud by itself -- NaN in its tile's gradient elements, the fault word,
        // the status word and NaN losses.  Ordering: a wait that runs out after the arrival has polled for kSpinLimit rounds (seconds), while the
        // finisher, which needs nothing of this wave beyond its arrival, has stored the losses and the status microseconds after the last arrival:
        // these stores come long after the finisher's, and rescale_kernel (a later launch) sees the status.  (A fault word or a sum W fault bit seen
        // here the finisher sees as well: it publishes NaN by itself.)  The wrap evaluation keeps the old order (tile_role): nothing of this wave
        // touches the workspace after its arrival there.
        if (g_logits) {
            float* G = g_logits + (int64_t)n * P;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int r = t.tile_r0 + j;
                if (col_owned && r < h) G[(int64_t)r * w + c] = __int_as_float(0x7fc00000);
            }
        }
        if (lane == 0) {
            atomicOr(ws.fault, kFaultCounts);
            if (st.status) atomicOr(st.status, (int)kFaultCounts);
            losses[0] = __int_as_float(0x7fc00000); losses[1] = losses[0];
        }
    } else if (g_logits) {
        char* G = reinterpret_cast<char*>(g_logits + (int64_t)n * P);      // scalar base + 32-bit byte offset
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int r = t.tile_r0 + j;
            if (col_owned && r < h) add_f32(reinterpret_cast<float*>(G + (uint32_t)(r * w + c) * 4u), g[j] * scale);
        }
    }
    BXI_TW(1, tix, 6);
    bad_out |= bad;
}

}  // namespace bxi
