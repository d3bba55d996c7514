// solo_dconv_level.hip -- BoxLevelSet's training masks on gfx950 (box_solov2_head.py:205-216 in forward, :317-320 in loss): the dynamic
// 1x1 convolution of the ASSIGNED grid cells only, followed by the per-level bilinear resize; forward and backward
// (include/boxinst/boxinst_hip_dconvl.h).
//
// The product (over e) and the resize (over pixels) commute, so the FEATURE is resized, once per size group (a run of consecutive levels
// of one output size), and the product of solo_dconv.hip -- its gather, its MFMA walk, its per-tile partial sums, its pass over every map
// element -- runs on the resized feature for the group's levels through that family's own entry points: the rows of a group are
// contiguous (level-major), so a group is a sub-range of the maps, the counts, the cells and the output.  At ratios 2 and 4 the product
// runs over a quarter and a sixteenth of the pixels.  From solo_dconv_device.hpp this file takes only the constants; what lives here is
// the size-group plan (dconvl_plan), the two entry points and three kernels:
//
// dconvl_resize_kernel   one thread per (image, channel, output pixel) of a resampled group: torch's bilinear weights for a given size
//   (taps_of), the four taps in torch's order.  An image without rows in the group returns before it reads anything, and nothing reads
//   its part of the workspace: the product returns early for it as well.
// dconvl_adjoint_kernel  four elements of grad_feat per thread: the sum over the groups, in group order, of the adjoint resize of the
//   group's feature gradient (written once to the workspace by the product's backward, zeros for an image without rows).  For a source
//   pixel it visits the output pixels whose taps name it, rows then columns ascending, found with the forward's own taps_of over a
//   range that cannot miss one.  No atomics, every element written.
// dconvl_zero_kernel     (dconvl_zero) every element of a gradient that no row reaches: all of them when N == 0, the maps of a group
//   without rows otherwise.
#include "solo_dconv_device.hpp"

#include "../../include/boxinst/boxinst_hip_dconvl.h"

namespace bxi {

struct Taps { int i0, i1; float l0, l1; };
// torch's area_pixel_compute_scale for align_corners=False and a given size: in / out in fp32 (IEEE division, the same value on the host
// and on the device; the host computes it once per group and axis and every kernel gets that value)
static inline float scale_of(int in, int out) { return (float)in / (float)out; }
// torch's area_pixel_compute_source_index, in fp32 and without contraction
__device__ __forceinline__ Taps taps_of(int dst, int in, float scale) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    Taps t;
    t.i0 = min((int)src, in - 1);
    t.i1 = min(t.i0 + 1, in - 1);
    t.l1 = __fsub_rn(src, (float)t.i0);
    t.l0 = __fsub_rn(1.f, t.l1);
    return t;
}
// the output indices that can tap source index `at`: those with src in (at - 1, at + 1), i.e. o in ((at - 0.5) / scale - 0.5,
// (at + 1.5) / scale - 0.5), and the clamped ones at index 0.  floor of the lower end and ceil of the upper are each one index wider than
// the open interval, which covers the rounding of `inv` (about out / in) and of src; taps_of decides
__device__ __forceinline__ void tap_range(int at, int out, float inv, int& lo, int& hi) {
    lo = max((int)floorf(((float)at - 0.5f) * inv - 0.5f), 0);
    hi = min((int)ceilf(((float)at + 1.5f) * inv - 0.5f), out - 1);
}

__global__ void __launch_bounds__(kDcThreads) dconvl_resize_kernel(const float* __restrict__ feat, float* __restrict__ rf, unsigned long long live,
                                                                   int E, int H, int W, int oh, int ow, float sy, float sx) {
    const int b = blockIdx.z, e = blockIdx.y;
    if (!((live >> b) & 1ull)) return;
    const int p = blockIdx.x * kDcThreads + threadIdx.x;
    if (p >= oh * ow) return;
    const int oy = p / ow, ox = p % ow;
    const Taps ty = taps_of(oy, H, sy), tx = taps_of(ox, W, sx);
    const float* f = feat + ((size_t)b * E + e) * H * W;
    const float v00 = f[(size_t)ty.i0 * W + tx.i0], v01 = f[(size_t)ty.i0 * W + tx.i1];
    const float v10 = f[(size_t)ty.i1 * W + tx.i0], v11 = f[(size_t)ty.i1 * W + tx.i1];
    const float top = __fadd_rn(__fmul_rn(tx.l0, v00), __fmul_rn(tx.l1, v01));
    const float bot = __fadd_rn(__fmul_rn(tx.l0, v10), __fmul_rn(tx.l1, v11));
    rf[((size_t)b * E + e) * oh * ow + p] = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
}

struct AdjGroups {
    const float* g[BXI_DCONV_MAX_LEVELS];                            // [B,E,oh,ow] of the groups with rows, in group order
    int oh[BXI_DCONV_MAX_LEVELS], ow[BXI_DCONV_MAX_LEVELS], same[BXI_DCONV_MAX_LEVELS];
    float sy[BXI_DCONV_MAX_LEVELS], sx[BXI_DCONV_MAX_LEVELS];         // scale_of per axis
    float iy[BXI_DCONV_MAX_LEVELS], ix[BXI_DCONV_MAX_LEVELS];         // about 1 / scale: for the ranges only
    int n;
};

constexpr int kDclPerThread = 4;                                     // pixels of one plane per thread, a workgroup's width apart

__global__ void __launch_bounds__(kDcThreads) dconvl_adjoint_kernel(const AdjGroups a, float* __restrict__ gfeat, int E, int H, int W) {
    const int b = blockIdx.z, e = blockIdx.y;
    for (int u = 0; u < kDclPerThread; ++u) {
        const int p = (blockIdx.x * kDclPerThread + u) * kDcThreads + threadIdx.x;
        if (p >= H * W) return;
        const int y = p / W, x = p % W;
        float s = 0.f;
        for (int k = 0; k < a.n; ++k) {
            const int oh = a.oh[k], ow = a.ow[k];
            const float* gp = a.g[k] + ((size_t)b * E + e) * oh * ow;
            if (a.same[k]) { s += gp[p]; continue; }
            const float sy = a.sy[k], sx = a.sx[k];
            int ylo, yhi, xlo, xhi;
            tap_range(y, oh, a.iy[k], ylo, yhi);
            tap_range(x, ow, a.ix[k], xlo, xhi);
            for (int oy = ylo; oy <= yhi; ++oy) {
                const Taps ty = taps_of(oy, H, sy);
                const bool y0 = ty.i0 == y, y1 = ty.i1 == y;
                if (!(y0 || y1)) continue;
                for (int ox = xlo; ox <= xhi; ++ox) {
                    const Taps tx = taps_of(ox, W, sx);
                    const bool x0 = tx.i0 == x, x1 = tx.i1 == x;
                    if (!(x0 || x1)) continue;
                    const float gv = gp[(size_t)oy * ow + ox];
                    if (y0 && x0) s += gv * (ty.l0 * tx.l0);
                    if (y0 && x1) s += gv * (ty.l0 * tx.l1);
                    if (y1 && x0) s += gv * (ty.l1 * tx.l0);
                    if (y1 && x1) s += gv * (ty.l1 * tx.l1);
                }
            }
        }
        gfeat[((size_t)b * E + e) * H * W + p] = s;
    }
}

// every element of every gradient of a call without rows
__global__ void __launch_bounds__(kDcThreads) dconvl_zero_kernel(float* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (i < n) dst[i] = 0.f;
}
static int dconvl_zero(void* dst, int64_t n, hipStream_t s) {
    BXI_LAUNCH("solo_dconvl_zero", s, dconvl_zero_kernel, dim3((unsigned)((n + kDcThreads - 1) / kDcThreads)), dim3(kDcThreads), 0, s,
               static_cast<float*>(dst), n);
    return check_launch();
}

// a run of consecutive levels of one output size
struct LGroup {
    int l0, nl, oh, ow, n, row0, same;
    size_t out0, planes;                                             // first float of its rows in out; B*E*oh*ow rounded up to 4
    unsigned long long live;                                         // bit b: image b has rows in the group
};
struct LPlan {
    LGroup g[BXI_DCONV_MAX_LEVELS];
    int groups, N;
    size_t rf_max, grf_sum, sub_fwd, sub_bwd;                        // floats, floats, bytes, bytes
};

static size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

// the argument checks both entry points and both size queries share; fills the plan
static int dconvl_plan(int B, int E, int H, int W, const int* grids, const int* level_sizes, const int* seg_counts, int L, LPlan& pl) {
    if (!level_sizes || !seg_counts) return BXI_ERR_NULL_POINTER;
    if (B < 1 || B > BXI_MAX_IMAGES || L < 1 || L > BXI_DCONV_MAX_LEVELS || E < 1 || E > BXI_DCONV_MAX_E || H < 1 || W < 1) return BXI_ERR_BAD_SHAPE;
    if (!fits_i32((int64_t)H * W) || !fits_i32((int64_t)B * E * H * W)) return BXI_ERR_BAD_SHAPE;
    int64_t total = 0, rows = 0;
    for (int l = 0; l < L; ++l) {
        const int oh = level_sizes[2 * l], ow = level_sizes[2 * l + 1];
        if (oh < 1 || ow < 1 || (grids && grids[l] < 1)) return BXI_ERR_BAD_SHAPE;
        if (!fits_i32((int64_t)oh * ow) || !fits_i32((int64_t)B * E * oh * ow)) return BXI_ERR_BAD_SHAPE;
        int64_t nl = 0;
        for (int b = 0; b < B; ++b) {
            if (seg_counts[l * B + b] < 0) return BXI_ERR_BAD_SHAPE;
            nl += seg_counts[l * B + b];
        }
        rows += nl;
        total += nl * oh * ow;
        if (!fits_i32(rows) || !fits_i32(total)) return BXI_ERR_BAD_SHAPE;
    }
    for (int l = 0; l < L; ++l) {
        const int64_t oh = level_sizes[2 * l], ow = level_sizes[2 * l + 1];
        if (H > BXI_DCONVL_MAX_DOWN * oh || W > BXI_DCONVL_MAX_DOWN * ow || oh > (int64_t)BXI_DCONVL_MAX_UP * H || ow > (int64_t)BXI_DCONVL_MAX_UP * W)
            return BXI_ERR_UNSUPPORTED;
    }
    pl.groups = 0; pl.N = (int)rows; pl.rf_max = 0; pl.grf_sum = 0; pl.sub_fwd = 0; pl.sub_bwd = 0;
    int row = 0;
    size_t at = 0;
    for (int l = 0; l < L; ++l) {
        const int oh = level_sizes[2 * l], ow = level_sizes[2 * l + 1];
        if (l == 0 || oh != pl.g[pl.groups - 1].oh || ow != pl.g[pl.groups - 1].ow) {
            LGroup& g = pl.g[pl.groups++];
            g.l0 = l; g.nl = 0; g.oh = oh; g.ow = ow; g.n = 0; g.row0 = row; g.out0 = at; g.live = 0ull;
            g.same = oh == H && ow == W;
            g.planes = round4((size_t)B * E * oh * ow);
        }
        LGroup& g = pl.g[pl.groups - 1];
        ++g.nl;
        for (int b = 0; b < B; ++b) {
            const int c = seg_counts[l * B + b];
            if (c > 0) g.live |= 1ull << b;
            g.n += c; row += c;
            at += (size_t)c * oh * ow;
        }
    }
    for (int k = 0; k < pl.groups; ++k) {
        const LGroup& g = pl.g[k];
        if (g.n == 0) continue;
        if (!g.same && g.planes > pl.rf_max) pl.rf_max = g.planes;
        pl.grf_sum += g.planes;
        const size_t f = bxi_solo_dconv_forward_workspace_bytes(g.n, B, E), w = bxi_solo_dconv_backward_workspace_bytes(g.n, B, E, g.oh, g.ow);
        if (f == 0 || w == 0) return BXI_ERR_BAD_SHAPE;                 // N_g * oh * ow >= 2^31
        pl.sub_fwd = f > pl.sub_fwd ? f : pl.sub_fwd;
        pl.sub_bwd = w > pl.sub_bwd ? w : pl.sub_bwd;
    }
    return BXI_OK;
}

static int dconvl_resize(const float* feat, float* rf, const LGroup& g, int B, int E, int H, int W, hipStream_t s) {
    const dim3 grid((unsigned)((g.oh * g.ow + kDcThreads - 1) / kDcThreads), (unsigned)E, (unsigned)B);
    BXI_LAUNCH("solo_dconvl_resize", s, dconvl_resize_kernel, grid, dim3(kDcThreads), 0, s, feat, rf, g.live, E, H, W, g.oh, g.ow, scale_of(H, g.oh),
               scale_of(W, g.ow));
    return check_launch();
}

}  // namespace bxi

extern "C" size_t bxi_solo_dconvl_forward_workspace_bytes(int B, int E, int H, int W, const int* level_sizes, const int* seg_counts, int L) {
    using namespace bxi;
    LPlan pl;
    if (dconvl_plan(B, E, H, W, nullptr, level_sizes, seg_counts, L, pl) != BXI_OK || pl.N == 0) return 0;
    return sizeof(float) * pl.rf_max + pl.sub_fwd;
}

extern "C" size_t bxi_solo_dconvl_backward_workspace_bytes(int B, int E, int H, int W, const int* level_sizes, const int* seg_counts, int L) {
    using namespace bxi;
    LPlan pl;
    if (dconvl_plan(B, E, H, W, nullptr, level_sizes, seg_counts, L, pl) != BXI_OK || pl.N == 0) return 0;
    return sizeof(float) * (pl.grf_sum + pl.rf_max) + pl.sub_bwd;
}

extern "C" int bxi_solo_dconvl_forward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                           const int* level_sizes, int L, const int64_t* cells, const int* seg_counts, int N, float* out,
                                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (!kernel_maps || !grids) return BXI_ERR_NULL_POINTER;
    LPlan pl;
    int rc = dconvl_plan(B, E, H, W, grids, level_sizes, seg_counts, L, pl);
    if (rc != BXI_OK) return rc;
    if (N < 0 || pl.N != N) return BXI_ERR_BAD_SHAPE;
    if (N == 0) return BXI_OK;
    if (!feat || !out || !status || !cells) return BXI_ERR_NULL_POINTER;
    for (int l = 0; l < L; ++l)
        if (!kernel_maps[l]) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, sizeof(float) * pl.rf_max + pl.sub_fwd, 16)) return BXI_ERR_WORKSPACE;
    float* rf = static_cast<float*>(workspace);
    void* sub = rf + pl.rf_max;
    hipStream_t s = as_stream(stream);
    for (int k = 0; k < pl.groups; ++k) {
        const LGroup& g = pl.g[k];
        if (g.n == 0) continue;
        if (!g.same) {
            rc = dconvl_resize(feat, rf, g, B, E, H, W, s);
            if (rc != BXI_OK) return rc;
        }
        rc = bxi_solo_dconv_forward_f32(g.same ? feat : rf, B, E, g.oh, g.ow, kernel_maps + g.l0, grids + g.l0, g.nl, BXI_DCONV_MAPS, cells + g.row0,
                                        seg_counts + g.l0 * B, g.n, BXI_DCONV_NONE, out + g.out0, nullptr, status, sub, pl.sub_fwd, stream);
        if (rc != BXI_OK) return rc;
    }
    return BXI_OK;
}

extern "C" int bxi_solo_dconvl_backward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                            const int* level_sizes, int L, const int64_t* cells, const int* seg_counts, int N,
                                            const float* grad_out, float* grad_feat, void* const* grad_kernel_maps, int32_t* status,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (!kernel_maps || !grids) return BXI_ERR_NULL_POINTER;
    LPlan pl;
    int rc = dconvl_plan(B, E, H, W, grids, level_sizes, seg_counts, L, pl);
    if (rc != BXI_OK) return rc;
    if (N < 0 || pl.N != N) return BXI_ERR_BAD_SHAPE;
    for (int l = 0; l < L; ++l)
        if (!fits_i32((int64_t)B * E * grids[l] * grids[l])) return BXI_ERR_BAD_SHAPE;
    if (!grad_feat && !grad_kernel_maps) return BXI_OK;
    if (N > 0) {
        if (!grad_out || !status || !cells || (grad_kernel_maps && !feat)) return BXI_ERR_NULL_POINTER;
        for (int l = 0; l < L; ++l)
            if (!kernel_maps[l]) return BXI_ERR_NULL_POINTER;
    }
    if (grad_kernel_maps)
        for (int l = 0; l < L; ++l)
            if (!grad_kernel_maps[l]) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    if (N == 0) {                                                    // all-zero gradients, nothing else
        if (grad_feat) {
            rc = dconvl_zero(grad_feat, (int64_t)B * E * H * W, s);
            if (rc != BXI_OK) return rc;
        }
        for (int l = 0; grad_kernel_maps && l < L; ++l) {
            rc = dconvl_zero(grad_kernel_maps[l], (int64_t)B * E * grids[l] * grids[l], s);
            if (rc != BXI_OK) return rc;
        }
        return BXI_OK;
    }
    if (!workspace_ok(workspace, workspace_bytes, sizeof(float) * (pl.grf_sum + pl.rf_max) + pl.sub_bwd, 16)) return BXI_ERR_WORKSPACE;
    float* grf = static_cast<float*>(workspace);
    float* rf = grf + pl.grf_sum;
    void* sub = rf + pl.rf_max;
    AdjGroups adj;
    adj.n = 0;
    for (int k = 0; k < BXI_DCONV_MAX_LEVELS; ++k) {
        adj.g[k] = nullptr; adj.oh[k] = adj.ow[k] = 1; adj.same[k] = 0;
        adj.sy[k] = adj.sx[k] = adj.iy[k] = adj.ix[k] = 1.f;
    }
    for (int k = 0; k < pl.groups; ++k) {
        const LGroup& g = pl.g[k];
        void* const* gmaps = grad_kernel_maps ? grad_kernel_maps + g.l0 : nullptr;
        if (g.n == 0) {                                              // no row names a cell of these levels: their maps are zero
            for (int l = g.l0; gmaps && l < g.l0 + g.nl; ++l) {
                rc = dconvl_zero(grad_kernel_maps[l], (int64_t)B * E * grids[l] * grids[l], s);
                if (rc != BXI_OK) return rc;
            }
            continue;
        }
        if (gmaps && !g.same) {
            rc = dconvl_resize(feat, rf, g, B, E, H, W, s);
            if (rc != BXI_OK) return rc;
        }
        float* mine = nullptr;
        if (grad_feat) {
            mine = grf;
            adj.g[adj.n] = mine; adj.oh[adj.n] = g.oh; adj.ow[adj.n] = g.ow; adj.same[adj.n] = g.same;
            adj.sy[adj.n] = scale_of(H, g.oh); adj.sx[adj.n] = scale_of(W, g.ow);
            adj.iy[adj.n] = scale_of(g.oh, H); adj.ix[adj.n] = scale_of(g.ow, W);
            ++adj.n;
            grf += g.planes;
        }
        // the product's backward; without an activation its saved output is not read (grad_out stands in for the pointer check)
        rc = bxi_solo_dconv_backward_f32(g.same ? feat : rf, B, E, g.oh, g.ow, kernel_maps + g.l0, grids + g.l0, g.nl, BXI_DCONV_MAPS, cells + g.row0,
                                         seg_counts + g.l0 * B, g.n, BXI_DCONV_NONE, grad_out + g.out0, grad_out + g.out0, mine, gmaps, status, sub,
                                         pl.sub_bwd, stream);
        if (rc != BXI_OK) return rc;
    }
    if (grad_feat) {
        const int per = kDcThreads * kDclPerThread;
        const dim3 grid((unsigned)((H * W + per - 1) / per), (unsigned)E, (unsigned)B);
        BXI_LAUNCH("solo_dconvl_adjoint", s, dconvl_adjoint_kernel, grid, dim3(kDcThreads), 0, s, adj, grad_feat, E, H, W);
        rc = check_launch();
    }
    return rc;
}
