// mask_paste.hip -- the test-time end of CondInstMaskHead (condinst_head.py:1259-1285) on gfx950: the mask logits of the
// detections become the uint8 masks of their images in one launch.
//
//   p(Y, X) = bilinear_{align_corners=False}( crop( aligned_bilinear( sigmoid(logits), f ) ), out )(Y, X)
//   mask    = p > threshold
//
// Both resizes are the bilinear kernels of ATen (UpSample.h: area_pixel_compute_scale, area_pixel_compute_source_index and
// the GPU kernel's index/lambda arithmetic) in fp32:
//   stage 1, aligned_bilinear (:146-167): replicate pad (h,w) -> (h+1,w+1), align_corners resize to (f h+1, f w+1), replicate
//            pad f//2 at the top/left, crop to f h x f w.  Crop row y samples row max(y - f//2, 0) of the resize, whose source
//            is scale1 * that row with scale1 = h / (f h); source rows past h-1 are the pad, i.e. row h-1.  f == 1: identity.
//   stage 2, F.interpolate(size=(out_h, out_w)) when the output differs from the crop: src = max(scale2 (Y + 0.5) - 0.5, 0),
//            scale2 = crop / out, second tap clamped at the edge; equal dims are the identity (ATen copies).
// Each stage is separable, so for an output row the pixel is
//   p = H0 (h0 K[ra] + h1 K[rb]) + H1 (h0' K[ra'] + h1' K[rb'])        (H: stage-2 row weights, h/h': stage-1 of its two taps)
//   K[r][X] = W0 (w0 P[r][ca] + w1 P[r][cb]) + W1 (w0' P[r][ca'] + w1' P[r][cb'])  (the same, horizontally, on logit row r)
// -- the reference's h0(w0 x00 + w1 x01) + h1(...) products of the two stages, regrouped: the same taps and weights, rounding
// differences only (p within ~1e-7 of the torch composition).
//
// mask_paste_kernel  one workgroup = one instance x one band of kBandRows output rows x one chunk of <= kChunkCols output columns
//   (1-D grid; instances of images with fewer bands / chunks than the largest exit at once).
//   a. the band's logit rows (a contiguous range: both maps are monotone) -> sigmoid -> LDS, each evaluated once, loads issued
//      in batches of 8 per thread (a band is ~2700 floats: one or two round trips, not eleven); the per-row taps -> LDS;
//   b. thread = output column: its stage-2 and two stage-1 column taps once, then K of every staged row -> LDS;
//   c. thread = 16 consecutive output bytes of one row: 4 x 4 ds_read_b128 of K, 16 FMA chains, one 128-bit store (16-B aligned
//      addresses; byte stores at a misaligned row start and at the row's tail).
// No atomics; every output byte is written exactly once.  LDS: rows_cap x (kw + w) floats, rows_cap = the most logit rows a band
// of the launch needs (the host walks the same index arithmetic), kw = the chunk width rounded up to 16.
#include "common.hpp"

namespace bxi {

constexpr int kPasteThreads = 256;
constexpr int kBandRows = 16;                      // output rows per workgroup (fewer when the staged rows would not fit)
constexpr int kChunkCols = 1024;                   // output columns per workgroup: 64 lanes x 16 bytes
constexpr size_t kPasteLdsMax = 64 * 1024;         // bytes of dynamic LDS a workgroup may ask for (4 waves, >= 2 per CU)
constexpr int kLoadBatch = 8;                      // logit loads a thread issues before it waits for the first

struct PasteArgs {
    const float* logits;
    const int64_t* img_inds;
    const int64_t* out_offsets;
    uint8_t* masks;
    int N, h, w, factor;
    float scale1_h, scale1_w;                       // stage 1: (float)h / (f h), (float)w / (f w)
    float threshold;
    int band_rows, rows_cap, kw;                    // rows per band, LDS rows, K row stride (floats, multiple of 16)
    int bands, chunks;                              // grid extent per instance (the largest image)
    int B;
    int dims[BXI_MAX_IMAGES][4];                    // crop_h, crop_w, out_h, out_w
    float scale2[BXI_MAX_IMAGES][2];                // stage 2: (float)crop / out per axis
};

struct Tap { int i0, i1; float l0, l1; };

// stage 2, F.interpolate(mode='bilinear', align_corners=False, size=out) as the GPU kernel of ATen indexes it
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

// stage 1, aligned_bilinear: crop index -> logit indices (the bottom/right replicate pad folded into the clamp to n-1)
__host__ __device__ inline Tap tap_aligned(int dst, int n, int factor, float scale) {
    if (factor == 1) return Tap{dst, dst, 1.f, 0.f};
    const int a = dst - factor / 2 > 0 ? dst - factor / 2 : 0;          // the top/left replicate pad
    const float src = scale * (float)a;                                  // align_corners: scale * dst
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < n ? 1 : 0);                                    // input of the resize: n + 1 (padded)
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    t.i0 = t.i0 < n - 1 ? t.i0 : n - 1;
    t.i1 = t.i1 < n - 1 ? t.i1 : n - 1;
    return t;
}

// logit rows [lo, hi] that output rows [y0, y1) of an image read
__host__ __device__ inline void band_rows_range(int y0, int y1, int crop, int out, float scale2, int n, int factor, float scale1,
                                                int& lo, int& hi) {
    const Tap first = tap_resize(y0, crop, out, scale2), last = tap_resize(y1 - 1, crop, out, scale2);
    lo = tap_aligned(first.i0, n, factor, scale1).i0;
    hi = tap_aligned(last.i1, n, factor, scale1).i1;
}

struct RowTab { int r[4]; float H0, H1, h0a, h1a, h0b, h1b; };

__global__ void __launch_bounds__(kPasteThreads) mask_paste_kernel(const PasteArgs a) {
    extern __shared__ float lds[];
    const int bands = a.bands, chunks = a.chunks;
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const int rest = (int)(blockIdx.x / (unsigned)bands);
    const int chunk = rest % chunks;
    const int j = rest / chunks;
    const int64_t b64 = a.img_inds[j];
    if (b64 < 0 || b64 >= a.B) return;
    const int b = (int)b64;
    const int crop_h = a.dims[b][0], crop_w = a.dims[b][1], out_h = a.dims[b][2], out_w = a.dims[b][3];
    const int Y0 = band * a.band_rows, X0 = chunk * kChunkCols;
    if (Y0 >= out_h || X0 >= out_w) return;
    const int Y1 = Y0 + a.band_rows < out_h ? Y0 + a.band_rows : out_h;
    const int cw = out_w - X0 < kChunkCols ? out_w - X0 : kChunkCols;
    const int h = a.h, w = a.w, kw = a.kw;
    const float s2h = a.scale2[b][0], s2w = a.scale2[b][1];

    int rlo, rhi;
    band_rows_range(Y0, Y1, crop_h, out_h, s2h, h, a.factor, a.scale1_h, rlo, rhi);
    int nr = rhi - rlo + 1;
    nr = nr < a.rows_cap ? nr : a.rows_cap;                  // never taken (the host sized rows_cap by the same walk): LDS bounds
    float* K = lds;                                          // [rows_cap][kw]   (16-B aligned rows)
    float* P = lds + (size_t)a.rows_cap * kw;                // [rows_cap][w]
    RowTab* rt = reinterpret_cast<RowTab*>(P + (size_t)a.rows_cap * w);    // [band_rows]

    // a. probabilities of the band's logit rows (kLoadBatch loads in flight per thread before the first is used), the per-row taps
    const int64_t out_offset = a.out_offsets[j];
    const float* src = a.logits + ((size_t)j * h + rlo) * w;
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
            if (i < n_src) P[i] = 1.f / (1.f + expf(-v[k]));
        }
    }
    for (int y = threadIdx.x; y < Y1 - Y0; y += kPasteThreads) {
        const Tap t2 = tap_resize(Y0 + y, crop_h, out_h, s2h);
        const Tap ta = tap_aligned(t2.i0, h, a.factor, a.scale1_h), tb = tap_aligned(t2.i1, h, a.factor, a.scale1_h);
        RowTab r;
        const int hi = nr - 1;
        r.r[0] = min(max(ta.i0 - rlo, 0), hi); r.r[1] = min(max(ta.i1 - rlo, 0), hi);
        r.r[2] = min(max(tb.i0 - rlo, 0), hi); r.r[3] = min(max(tb.i1 - rlo, 0), hi);
        r.H0 = t2.l0; r.H1 = t2.l1; r.h0a = ta.l0; r.h1a = ta.l1; r.h0b = tb.l0; r.h1b = tb.l1;
        rt[y] = r;
    }
    __syncthreads();

    // b. K[r][x] for every staged row r and column x of the chunk
    for (int x = threadIdx.x; x < cw; x += kPasteThreads) {
        const Tap t2 = tap_resize(X0 + x, crop_w, out_w, s2w);
        const Tap ta = tap_aligned(t2.i0, w, a.factor, a.scale1_w), tb = tap_aligned(t2.i1, w, a.factor, a.scale1_w);
        for (int r = 0; r < nr; ++r) {
            const float* row = P + (size_t)r * w;
            K[(size_t)r * kw + x] = t2.l0 * (ta.l0 * row[ta.i0] + ta.l1 * row[ta.i1]) +
                                    t2.l1 * (tb.l0 * row[tb.i0] + tb.l1 * row[tb.i1]);
        }
    }
    __syncthreads();

    // c. 16 output bytes per item
    const int segs = (cw + 15) >> 4;
    const int items = (Y1 - Y0) * segs;
    uint8_t* base = a.masks + out_offset;
    const float thr = a.threshold;
    for (int it = threadIdx.x; it < items; it += kPasteThreads) {
        const int y = it / segs, x = (it - y * segs) << 4;
        const RowTab r = rt[y];
        const float4* k0 = reinterpret_cast<const float4*>(K + (size_t)r.r[0] * kw + x);
        const float4* k1 = reinterpret_cast<const float4*>(K + (size_t)r.r[1] * kw + x);
        const float4* k2 = reinterpret_cast<const float4*>(K + (size_t)r.r[2] * kw + x);
        const float4* k3 = reinterpret_cast<const float4*>(K + (size_t)r.r[3] * kw + x);
        uint32_t word[4];
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
            }
            word[q] = wd;
        }
        uint8_t* dst = base + (size_t)(Y0 + y) * out_w + X0 + x;
        const int n = cw - x < 16 ? cw - x : 16;
        if (n == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
            for (int e = 0; e < n; ++e) dst[e] = (uint8_t)(word[e >> 2] >> (8 * (e & 3)));
        }
    }
}

}  // namespace bxi

extern "C" int bxi_mask_paste_u8(const float* logits, int N, int h, int w, int factor, const int64_t* img_inds,
                                 const int64_t* out_offsets, int B, const int32_t* image_dims_host, float threshold,
                                 uint8_t* masks, void* stream) {
    using namespace bxi;
    if (N < 0 || h < 1 || w < 1 || factor < 1 || B < 1 || B > BXI_MAX_IMAGES) return BXI_ERR_BAD_SHAPE;
    if (!image_dims_host) return BXI_ERR_NULL_POINTER;
    if (!(threshold == threshold)) return BXI_ERR_BAD_ARGUMENT;
    if (!fits_i32((int64_t)factor * h) || !fits_i32((int64_t)factor * w) || !fits_i32((int64_t)h * w)) return BXI_ERR_BAD_SHAPE;
    PasteArgs a;
    a.N = N; a.h = h; a.w = w; a.factor = factor; a.B = B; a.threshold = threshold;
    a.scale1_h = factor == 1 ? 1.f : (float)h / (float)(factor * h);    // area_pixel_compute_scale, align_corners: (in-1)/(out-1)
    a.scale1_w = factor == 1 ? 1.f : (float)w / (float)(factor * w);
    int max_h = 0, max_w = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* d = image_dims_host + 4 * b;
        if (d[0] < 1 || d[1] < 1 || d[2] < 1 || d[3] < 1 || d[0] > factor * h || d[1] > factor * w) return BXI_ERR_BAD_SHAPE;
        for (int k = 0; k < 4; ++k) a.dims[b][k] = d[k];
        a.scale2[b][0] = (float)d[0] / (float)d[2];                      // compute_scales_value: (float)in / out
        a.scale2[b][1] = (float)d[1] / (float)d[3];
        max_h = d[2] > max_h ? d[2] : max_h;
        max_w = d[3] > max_w ? d[3] : max_w;
    }
    if (N == 0) return BXI_OK;
    if (!logits || !img_inds || !out_offsets || !masks) return BXI_ERR_NULL_POINTER;
    const int chunk = max_w < kChunkCols ? max_w : kChunkCols;
    a.kw = (chunk + 15) / 16 * 16;
    a.chunks = (max_w + kChunkCols - 1) / kChunkCols;
    // the band height: the largest (16, 8, ..., 1) whose staged rows fit, the same index walk as the kernel's plus two rows of margin
    size_t lds = 0;
    for (a.band_rows = kBandRows; a.band_rows >= 1; a.band_rows /= 2) {
        int cap = 0;
        for (int b = 0; b < B; ++b)
            for (int y0 = 0; y0 < a.dims[b][2]; y0 += a.band_rows) {
                const int y1 = y0 + a.band_rows < a.dims[b][2] ? y0 + a.band_rows : a.dims[b][2];
                int lo, hi;
                band_rows_range(y0, y1, a.dims[b][0], a.dims[b][2], a.scale2[b][0], h, factor, a.scale1_h, lo, hi);
                cap = hi - lo + 1 > cap ? hi - lo + 1 : cap;
            }
        a.rows_cap = cap + 2 < h ? cap + 2 : h;
        lds = sizeof(float) * (size_t)a.rows_cap * (size_t)(w + a.kw) + sizeof(RowTab) * (size_t)a.band_rows;
        if (lds <= kPasteLdsMax) break;
    }
    if (a.band_rows < 1) return BXI_ERR_UNSUPPORTED;           // logit rows wider than ~5000 columns
    a.bands = (max_h + a.band_rows - 1) / a.band_rows;
    const int64_t grid = (int64_t)N * a.chunks * a.bands;
    if (grid * kPasteThreads > 0xffffffffLL) return BXI_ERR_UNSUPPORTED;        // the dispatch's 32-bit work-item count
    a.logits = logits; a.img_inds = img_inds; a.out_offsets = out_offsets; a.masks = masks;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("mask_paste", s, mask_paste_kernel, dim3((unsigned)grid), dim3(kPasteThreads), lds, s, a);
    return check_launch();
}
