// paste_device.hpp -- what the two test-time mask kernels share (mask_paste.hip: CondInst, seg_paste.hip: the SOLOv2-style heads): the
// ATen bilinear tap, the walk from a band of output rows to the source rows it reads, the band-height choice on the host, and the tile
// itself -- stage the source rows in LDS, resize them horizontally once (K), combine K's rows into 16 output bytes per lane.
//
// Both kernels compute   p(Y, X) = resize2( crop( stage1( source ) ) )(Y, X),   mask = p > threshold
// with resize2 = F.interpolate(bilinear, align_corners=False, size=out) and a stage 1 of their own (an Axis functor: crop index -> the two
// source indices and weights).  Each stage is separable, so for an output row the pixel is
//   p = H0 (h0 K[ra] + h1 K[rb]) + H1 (h0' K[ra'] + h1' K[rb'])        (H: stage-2 row weights, h/h': stage-1 of its two taps)
//   K[r][X] = W0 (w0 P[r][ca] + w1 P[r][cb]) + W1 (w0' P[r][ca'] + w1' P[r][cb'])  (the same, horizontally, on source row r)
// -- the reference's h0(w0 x00 + w1 x01) + h1(...) products of the two stages, regrouped: the same taps and weights, rounding
// differences only (p within ~1e-7 of the torch composition).
//
// paste_tile  one workgroup = one band of band_rows output rows x one chunk of <= kChunkCols output columns of one mask:
//   a. the band's source rows (a contiguous range: both maps are monotone) -> LDS, each evaluated once, loads issued in batches of 8 per
//      thread (a band is ~2700 floats: one or two round trips, not eleven); the per-row taps -> LDS;
//   b. thread = output column: its stage-2 and two stage-1 column taps once, then K of every staged row -> LDS;
//   c. thread = 16 consecutive output bytes of one row: 4 x 4 ds_read_b128 of K, 16 FMA chains, one 128-bit store (16-B aligned
//      addresses; byte stores at a misaligned row start and at the row's tail).
// No global atomics; every output byte is written exactly once.  LDS: rows_cap x (kw + w) floats, rows_cap = the most source rows a band
// of the launch needs (the host walks the same index arithmetic), kw = the chunk width rounded up to 16; with STATS, three ints per row of
// the band behind them: the count and the first / last set column of the row inside the chunk (LDS integer atomics: order-free); with
// SCORE (inst_post.hip: Box2Mask), one float per row and 16-byte segment of the chunk behind those: the segment's sum of sigmoid(p) over
// its set pixels, which one thread per row adds up in ascending order (no float atomics: the order is part of the result).
#pragma once

#include "common.hpp"

namespace bxi {

constexpr int kPasteThreads = 256;
constexpr int kBandRows = 16;                      // output rows per workgroup (fewer when the staged rows would not fit)
constexpr int kChunkCols = 1024;                   // output columns per workgroup: 64 lanes x 16 bytes
constexpr size_t kPasteLdsMax = 64 * 1024;         // bytes of dynamic LDS a workgroup may ask for (4 waves, >= 2 per CU)
constexpr int kLoadBatch = 8;                      // source loads a thread issues before it waits for the first

struct Tap { int i0, i1; float l0, l1; };

// F.interpolate(mode='bilinear', align_corners=False, size=out) as the GPU kernel of ATen indexes it
__host__ __device__ inline Tap tap_resize(int dst, int in, int out, float scale) {
    if (in == out) return Tap{dst, dst, 1.f, 0.f};
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// a plain resize as stage 1: n source samples -> `up` samples, scale = (float)n / up
struct ResizeAxis {
    int n, up; float scale;
    __host__ __device__ Tap operator()(int dst) const { return tap_resize(dst, n, up, scale); }
};

// source rows [lo, hi] that output rows [y0, y1) read
template <class Axis>
__host__ __device__ inline void band_rows_range(int y0, int y1, int crop, int out, float scale2, const Axis& s1, int& lo, int& hi) {
    const Tap first = tap_resize(y0, crop, out, scale2), last = tap_resize(y1 - 1, crop, out, scale2);
    lo = s1(first.i0).i0;
    hi = s1(last.i1).i1;
}

// the most source rows a band of `band_rows` output rows of one image reads (host: the walk the workgroups repeat)
template <class Axis>
inline int band_rows_needed(int band_rows, int crop, int out, float scale2, const Axis& s1) {
    int cap = 0;
    for (int y0 = 0; y0 < out; y0 += band_rows) {
        const int y1 = y0 + band_rows < out ? y0 + band_rows : out;
        int lo, hi;
        band_rows_range(y0, y1, crop, out, scale2, s1, lo, hi);
        cap = hi - lo + 1 > cap ? hi - lo + 1 : cap;
    }
    return cap;
}

struct RowTab { int r[4]; float H0, H1, h0a, h1a, h0b, h1b; };

inline size_t paste_lds_bytes(int rows_cap, int w, int kw, int band_rows, bool stats, bool score = false) {
    return sizeof(float) * (size_t)rows_cap * (size_t)(w + kw) +
           (sizeof(RowTab) + (stats ? 3 * sizeof(int) : 0) + (score ? sizeof(float) * (size_t)(kw >> 4) : 0)) * (size_t)band_rows;
}

// The band height: the largest (16, 8, ..., 1) whose staged rows fit -- `needed(band_rows)` is the most rows a band of the launch reads,
// plus two rows of margin.  False when even single rows do not fit (source rows wider than ~5000 columns).
template <class Needed>
inline bool choose_band(int h, int w, int kw, bool stats, Needed needed, int& band_rows, int& rows_cap, size_t& lds, bool score = false) {
    for (band_rows = kBandRows; band_rows >= 1; band_rows /= 2) {
        const int cap = needed(band_rows);
        rows_cap = cap + 2 < h ? cap + 2 : h;
        lds = paste_lds_bytes(rows_cap, w, kw, band_rows, stats, score);
        if (lds <= kPasteLdsMax) return true;
    }
    return false;
}

struct PasteTile {
    const float* plane;                             // row 0 of the mask's source plane (rows of w floats)
    uint8_t* base;                                  // byte (0, 0) of its output [out_h, out_w]
    int w, kw, rows_cap;
    int crop_h, crop_w, out_h, out_w;
    float s2h, s2w, thr;
    int Y0, Y1, X0, cw;                             // the band's rows [Y0, Y1), the chunk's columns [X0, X0 + cw)
};

// SIGMOID: the source holds logits.  STATS: rows[y * rows_stride], y < Y1 - Y0, = (set bytes, first set column, last set column, 0) of every row of the tile
// (-1 columns for an empty row) by plain stores, and `valid == false` writes an all-zero tile and reads nothing of `plane`.  SCORE (with
// STATS; the source holds logits that are thresholded as they are): the fourth word of the row's record is the bits of the fp32 sum of
// 1 / (1 + expf(-p)) over the row's set pixels inside the chunk -- every thread adds its 16 pixels in element order, one thread per row
// adds the row's segments in ascending order.
template <bool SIGMOID, bool STATS, bool SCORE = false, class Axis>
__device__ __forceinline__ void paste_tile(float* lds, const PasteTile& t, const Axis& s1h, const Axis& s1w, bool valid, int4* rows,
                                           int rows_stride) {
    const int w = t.w, kw = t.kw, Y0 = t.Y0, Y1 = t.Y1, X0 = t.X0, cw = t.cw;
    const int crop_h = t.crop_h, crop_w = t.crop_w, out_h = t.out_h, out_w = t.out_w;
    const float s2h = t.s2h, s2w = t.s2w;

    int rlo, rhi;
    band_rows_range(Y0, Y1, crop_h, out_h, s2h, s1h, rlo, rhi);
    int nr = rhi - rlo + 1;
    nr = nr < t.rows_cap ? nr : t.rows_cap;                  // never taken (the host sized rows_cap by the same walk): LDS bounds
    float* K = lds;                                          // [rows_cap][kw]   (16-B aligned rows)
    float* P = lds + (size_t)t.rows_cap * kw;                // [rows_cap][w]
    RowTab* rt = reinterpret_cast<RowTab*>(P + (size_t)t.rows_cap * w);    // [band_rows]
    int* rs = reinterpret_cast<int*>(rt + (Y1 - Y0));        // STATS: [Y1 - Y0][3]
    float* sg = reinterpret_cast<float*>(rs + 3 * (Y1 - Y0)); // SCORE: [Y1 - Y0][kw / 16]

    // a. the band's source rows (kLoadBatch loads in flight per thread before the first is used), the per-row taps
    if (valid) {
        const float* src = t.plane + (size_t)rlo * w;
        const int n_src = nr * w;
        for (int i0 = threadIdx.x; i0 < n_src; i0 += kLoadBatch * kPasteThreads) {
            float v[kLoadBatch];
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int i = i0 + k * kPasteThreads;
                v[k] = i < n_src ? src[i] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int i = i0 + k * kPasteThreads;
                if (i < n_src) P[i] = SIGMOID ? 1.f / (1.f + expf(-v[k])) : v[k];
            }
        }
    }
    for (int y = threadIdx.x; y < Y1 - Y0; y += kPasteThreads) {
        const Tap t2 = tap_resize(Y0 + y, crop_h, out_h, s2h);
        const Tap ta = s1h(t2.i0), tb = s1h(t2.i1);
        RowTab r;
        const int hi = nr - 1;
        r.r[0] = min(max(ta.i0 - rlo, 0), hi); r.r[1] = min(max(ta.i1 - rlo, 0), hi);
        r.r[2] = min(max(tb.i0 - rlo, 0), hi); r.r[3] = min(max(tb.i1 - rlo, 0), hi);
        r.H0 = t2.l0; r.H1 = t2.l1; r.h0a = ta.l0; r.h1a = ta.l1; r.h0b = tb.l0; r.h1b = tb.l1;
        rt[y] = r;
        if (STATS) { rs[3 * y] = 0; rs[3 * y + 1] = 0x7fffffff; rs[3 * y + 2] = -1; }
    }
    __syncthreads();

    // b. K[r][x] for every staged row r and column x of the chunk
    if (valid) {
        for (int x = threadIdx.x; x < cw; x += kPasteThreads) {
            const Tap t2 = tap_resize(X0 + x, crop_w, out_w, s2w);
            const Tap ta = s1w(t2.i0), tb = s1w(t2.i1);
            for (int r = 0; r < nr; ++r) {
                const float* row = P + (size_t)r * w;
                K[(size_t)r * kw + x] = t2.l0 * (ta.l0 * row[ta.i0] + ta.l1 * row[ta.i1]) +
                                        t2.l1 * (tb.l0 * row[tb.i0] + tb.l1 * row[tb.i1]);
            }
        }
    }
    __syncthreads();

    // c. 16 output bytes per item
    const int segs = (cw + 15) >> 4;
    const int items = (Y1 - Y0) * segs;
    uint8_t* base = t.base;
    const float thr = t.thr;
    for (int it = threadIdx.x; it < items; it += kPasteThreads) {
        const int y = it / segs, x = (it - y * segs) << 4;
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        float seg_sum = 0.f;                                 // SCORE only
        if (valid) {
            const RowTab r = rt[y];
            const float4* k0 = reinterpret_cast<const float4*>(K + (size_t)r.r[0] * kw + x);
            const float4* k1 = reinterpret_cast<const float4*>(K + (size_t)r.r[1] * kw + x);
            const float4* k2 = reinterpret_cast<const float4*>(K + (size_t)r.r[2] * kw + x);
            const float4* k3 = reinterpret_cast<const float4*>(K + (size_t)r.r[3] * kw + x);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v0 = k0[q], v1 = k1[q], v2 = k2[q], v3 = k3[q];
                const float e0[4] = {v0.x, v0.y, v0.z, v0.w}, e1[4] = {v1.x, v1.y, v1.z, v1.w};
                const float e2[4] = {v2.x, v2.y, v2.z, v2.w}, e3[4] = {v3.x, v3.y, v3.z, v3.w};
                uint32_t wd = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = r.H0 * (r.h0a * e0[e] + r.h1a * e1[e]) + r.H1 * (r.h0b * e2[e] + r.h1b * e3[e]);
                    wd |= (p > thr ? 1u : 0u) << (8 * e);
                    if (SCORE) {
                        if (p > thr && x + 4 * q + e < cw) seg_sum += 1.f / (1.f + expf(-p));
                    }
                }
                word[q] = wd;
            }
        }
        if (SCORE) sg[y * (kw >> 4) + (x >> 4)] = seg_sum;
        uint8_t* dst = base + (size_t)(Y0 + y) * out_w + X0 + x;
        const int n = cw - x < 16 ? cw - x : 16;
        if (n == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
            for (int e = 0; e < n; ++e) dst[e] = (uint8_t)(word[e >> 2] >> (8 * (e & 3)));
        }
        if (STATS) {
            // the bytes of K behind the chunk's last column are whatever the LDS held: they are not part of the row
            int cnt = 0, first = 16, last = -1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nb = n - 4 * q;
                const uint32_t m = nb >= 4 ? 0xffffffffu : nb <= 0 ? 0u : (1u << (8 * nb)) - 1u;
                const uint32_t wd = word[q] & m;
                if (wd) {
                    cnt += __popc(wd);
                    first = first < 16 ? first : 4 * q + ((__ffs((int)wd) - 1) >> 3);
                    last = 4 * q + ((31 - __clz((int)wd)) >> 3);
                }
            }
            if (cnt) {
                atomicAdd(&rs[3 * y], cnt);
                atomicMin(&rs[3 * y + 1], X0 + x + first);
                atomicMax(&rs[3 * y + 2], X0 + x + last);
            }
        }
    }
    if (STATS) {
        __syncthreads();
        for (int y = threadIdx.x; y < Y1 - Y0; y += kPasteThreads) {
            const int c = rs[3 * y];
            int fourth = 0;
            if (SCORE) {
                float row_sum = 0.f;
                for (int sgm = 0; sgm < segs; ++sgm) row_sum += sg[y * (kw >> 4) + sgm];
                fourth = __float_as_int(row_sum);
            }
            rows[(size_t)y * rows_stride] = make_int4(c, c ? rs[3 * y + 1] : -1, rs[3 * y + 2], fourth);
        }
    }
}

}  // namespace bxi
