// seg_paste.hip -- the end of get_seg_single of the SOLOv2-style heads (box_solov2_head.py:576-588, discobox_head.py:1641-1655) on
// gfx950: the probabilities of the candidates Matrix NMS kept become the image's final uint8 masks, with the area and the tight box of
// each, in two launches.
//
//   p(Y, X) = bilinear_{align_corners=False}( crop( bilinear_{align_corners=False}( probs[keep_inds[i]], up ) ), out )(Y, X)
//   mask    = p > threshold
//
// Both resizes are F.interpolate(mode='bilinear', size=...) of ATen in fp32 (UpSample.h: area_pixel_compute_scale,
// area_pixel_compute_source_index and the GPU kernel's index/lambda arithmetic): src = max(scale (dst + 0.5) - 0.5, 0), scale =
// (float)in / out, second tap clamped at the edge -- of the SOURCE for stage 1 and of the CROP for stage 2, as the reference resizes the
// cropped tensor; equal sizes are the identity.  The two stages are regrouped into one horizontal and one vertical pass: paste_device.hpp
// spells the products out and holds the tile (shared with mask_paste.hip); stage 1 is its ResizeAxis, the source is read as it is, and the
// row of `probs` is keep_inds[i]: no copy of the kept rows exists.
//
// seg_paste_kernel   one workgroup = one kept mask x one band of <= kBandRows output rows x one chunk of <= kChunkCols output columns.
//   Every output byte is written exactly once; the tile also counts every row's set bytes and its first / last set column inside the
//   chunk and stores them in the row's own workspace slot [n][out_h][chunks] x int4 (plain stores: nobody waits for anybody, and the
//   workspace is written completely).  A keep_inds[i] outside [0, n_all) reads nothing and writes zeros and empty rows.
// seg_stats_kernel   one workgroup per mask folds its out_h x chunks slots into stats[i] = (area, x_min, y_min, x_max, y_max), or
//   (0, -1, -1, -1, -1).  Integer sums, minima and maxima: the order does not matter, runs are bit-identical.
#include "paste_device.hpp"

#include "../../include/boxinst/boxinst_hip_seg.h"

namespace bxi {

struct SegArgs {
    const float* probs;
    const int64_t* keep_inds;
    uint8_t* masks;
    int4* rows;                                     // workspace: [n][out_h][chunks]
    int n_all, h, w, up_h, up_w;
    int crop_h, crop_w, out_h, out_w;
    float scale1_h, scale1_w, scale2_h, scale2_w;
    float threshold;
    int band_rows, rows_cap, kw, bands, chunks;
};

__global__ void __launch_bounds__(kPasteThreads) seg_paste_kernel(const SegArgs a) {
    extern __shared__ float lds[];
    const int band = (int)(blockIdx.x % (unsigned)a.bands);
    const int rest = (int)(blockIdx.x / (unsigned)a.bands);
    const int chunk = rest % a.chunks;
    const int i = rest / a.chunks;
    const int64_t k = a.keep_inds[i];
    const bool valid = k >= 0 && k < a.n_all;
    const int Y0 = band * a.band_rows, X0 = chunk * kChunkCols;                 // inside the output: the grid is exact (one image)
    PasteTile t;
    t.plane = a.probs + (size_t)(valid ? k : 0) * a.h * a.w;
    t.base = a.masks + (size_t)i * a.out_h * a.out_w;
    t.w = a.w; t.kw = a.kw; t.rows_cap = a.rows_cap;
    t.crop_h = a.crop_h; t.crop_w = a.crop_w; t.out_h = a.out_h; t.out_w = a.out_w;
    t.s2h = a.scale2_h; t.s2w = a.scale2_w; t.thr = a.threshold;
    t.Y0 = Y0; t.Y1 = Y0 + a.band_rows < a.out_h ? Y0 + a.band_rows : a.out_h;
    t.X0 = X0; t.cw = a.out_w - X0 < kChunkCols ? a.out_w - X0 : kChunkCols;
    int4* rows = a.rows + ((size_t)i * a.out_h + Y0) * a.chunks + chunk;
    paste_tile<false, true>(lds, t, ResizeAxis{a.h, a.up_h, a.scale1_h}, ResizeAxis{a.w, a.up_w, a.scale1_w}, valid, rows, a.chunks);
}

__global__ void __launch_bounds__(kPasteThreads) seg_stats_kernel(const int4* __restrict__ rows, int out_h, int chunks, int32_t* __restrict__ stats) {
    __shared__ int red[5][kPasteThreads / kWave];
    const int i = blockIdx.x;
    const int4* mine = rows + (size_t)i * out_h * chunks;
    int area = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    const int slots = out_h * chunks;
    for (int s = threadIdx.x; s < slots; s += kPasteThreads) {
        const int4 r = mine[s];
        if (r.x > 0) {
            const int y = s / chunks;
            area += r.x;
            x0 = min(x0, r.y); x1 = max(x1, r.z);
            y0 = min(y0, y); y1 = max(y1, y);
        }
    }
    area = wave_total_i32(area);
    x0 = wave_min_i32(x0); y0 = wave_min_i32(y0);
    x1 = -wave_min_i32(-x1); y1 = -wave_min_i32(-y1);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        red[0][wv] = area; red[1][wv] = x0; red[2][wv] = y0; red[3][wv] = x1; red[4][wv] = y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kPasteThreads / kWave; ++wv) {
            area += red[0][wv];
            x0 = min(x0, red[1][wv]); y0 = min(y0, red[2][wv]);
            x1 = max(x1, red[3][wv]); y1 = max(y1, red[4][wv]);
        }
        int32_t* o = stats + 5 * (size_t)i;
        o[0] = area;
        o[1] = area ? x0 : -1; o[2] = area ? y0 : -1; o[3] = area ? x1 : -1; o[4] = area ? y1 : -1;
    }
}

// shapes the entry point and the size query accept
static bool seg_shape_ok(int n, int out_h, int out_w) {
    if (n < 0 || out_h < 1 || out_w < 1 || !fits_i32((int64_t)out_h * out_w)) return false;
    const int64_t bands = (out_h + kBandRows - 1) / kBandRows, chunks = (out_w + kChunkCols - 1) / kChunkCols;
    return fits_i32((int64_t)n * bands) && fits_i32((int64_t)n * bands * chunks);
}

}  // namespace bxi

extern "C" size_t bxi_seg_paste_workspace_bytes(int n, int out_h, int out_w) {
    using namespace bxi;
    if (!seg_shape_ok(n, out_h, out_w)) return 0;
    const size_t chunks = (size_t)(out_w + kChunkCols - 1) / kChunkCols;
    return sizeof(int4) * (size_t)n * (size_t)out_h * chunks;
}

extern "C" int bxi_seg_paste_u8(const float* probs, int n_all, int h, int w, const int64_t* keep_inds, int n, int up_h, int up_w,
                                int crop_h, int crop_w, int out_h, int out_w, float threshold, uint8_t* masks, int32_t* stats,
                                void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (n_all < 1 || h < 1 || w < 1 || up_h < 1 || up_w < 1 || crop_h < 1 || crop_w < 1 || crop_h > up_h || crop_w > up_w) return BXI_ERR_BAD_SHAPE;
    if (!seg_shape_ok(n, out_h, out_w) || !fits_i32((int64_t)h * w) || !fits_i32((int64_t)n_all * h * w)) return BXI_ERR_BAD_SHAPE;
    if (!(threshold == threshold)) return BXI_ERR_BAD_ARGUMENT;
    if (n == 0) return BXI_OK;
    if (!probs || !keep_inds || !masks || !stats) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_seg_paste_workspace_bytes(n, out_h, out_w), 16)) return BXI_ERR_WORKSPACE;
    SegArgs a;
    a.n_all = n_all; a.h = h; a.w = w; a.up_h = up_h; a.up_w = up_w;
    a.crop_h = crop_h; a.crop_w = crop_w; a.out_h = out_h; a.out_w = out_w; a.threshold = threshold;
    a.scale1_h = (float)h / (float)up_h;                                  // compute_scales_value: (float)in / out
    a.scale1_w = (float)w / (float)up_w;
    a.scale2_h = (float)crop_h / (float)out_h;
    a.scale2_w = (float)crop_w / (float)out_w;
    const int chunk = out_w < kChunkCols ? out_w : kChunkCols;
    a.kw = (chunk + 15) / 16 * 16;
    a.chunks = (out_w + kChunkCols - 1) / kChunkCols;
    size_t lds = 0;
    const bool fits = choose_band(h, w, a.kw, true, [&](int band_rows) {
        return band_rows_needed(band_rows, crop_h, out_h, a.scale2_h, ResizeAxis{h, up_h, a.scale1_h});
    }, a.band_rows, a.rows_cap, lds);
    if (!fits) return BXI_ERR_UNSUPPORTED;                                // source rows wider than ~5000 columns
    a.bands = (out_h + a.band_rows - 1) / a.band_rows;
    const int64_t grid = (int64_t)n * a.chunks * a.bands;
    if (grid * kPasteThreads > 0xffffffffLL) return BXI_ERR_UNSUPPORTED;   // the dispatch's 32-bit work-item count
    a.probs = probs; a.keep_inds = keep_inds; a.masks = masks; a.rows = static_cast<int4*>(workspace);
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("seg_paste", s, seg_paste_kernel, dim3((unsigned)grid), dim3(kPasteThreads), lds, s, a);
    int rc = check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("seg_stats", s, seg_stats_kernel, dim3((unsigned)n), dim3(kPasteThreads), 0, s, a.rows, out_h, a.chunks, stats);
    return check_launch();
}
