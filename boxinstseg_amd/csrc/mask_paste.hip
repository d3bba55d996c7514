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
// Each stage is separable and the two are regrouped into one horizontal and one vertical pass: paste_device.hpp spells the products out
// and holds the tile (shared with seg_paste.hip); stage 1 is the AlignedAxis below and the source goes through a sigmoid.
//
// mask_paste_kernel  one workgroup = one instance x one band of kBandRows output rows x one chunk of <= kChunkCols output columns
//   (1-D grid; instances of images with fewer bands / chunks than the largest exit at once).  No atomics; every output byte is
//   written exactly once.
#include "paste_device.hpp"

namespace bxi {

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

struct AlignedAxis {
    int n, factor; float scale;
    __host__ __device__ Tap operator()(int dst) const { return tap_aligned(dst, n, factor, scale); }
};

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
    PasteTile t;
    t.plane = a.logits + (size_t)j * a.h * a.w;
    t.base = a.masks + a.out_offsets[j];
    t.w = a.w; t.kw = a.kw; t.rows_cap = a.rows_cap;
    t.crop_h = crop_h; t.crop_w = crop_w; t.out_h = out_h; t.out_w = out_w;
    t.s2h = a.scale2[b][0]; t.s2w = a.scale2[b][1]; t.thr = a.threshold;
    t.Y0 = Y0; t.Y1 = Y1; t.X0 = X0; t.cw = cw;
    paste_tile<true, false>(lds, t, AlignedAxis{a.h, a.factor, a.scale1_h}, AlignedAxis{a.w, a.factor, a.scale1_w}, true, nullptr, 0);
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
    size_t lds = 0;
    const bool fits = choose_band(h, w, a.kw, false, [&](int band_rows) {
        int cap = 0;
        for (int b = 0; b < B; ++b) {
            const int need = band_rows_needed(band_rows, a.dims[b][0], a.dims[b][2], a.scale2[b][0], AlignedAxis{h, factor, a.scale1_h});
            cap = need > cap ? need : cap;
        }
        return cap;
    }, a.band_rows, a.rows_cap, lds);
    if (!fits) return BXI_ERR_UNSUPPORTED;                     // logit rows wider than ~5000 columns
    a.bands = (max_h + a.band_rows - 1) / a.band_rows;
    const int64_t grid = (int64_t)N * a.chunks * a.bands;
    if (grid * kPasteThreads > 0xffffffffLL) return BXI_ERR_UNSUPPORTED;        // the dispatch's 32-bit work-item count
    a.logits = logits; a.img_inds = img_inds; a.out_offsets = out_offsets; a.masks = masks;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("mask_paste", s, mask_paste_kernel, dim3((unsigned)grid), dim3(kPasteThreads), lds, s, a);
    return check_launch();
}
