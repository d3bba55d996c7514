// focal_device.hpp -- what the two training-loss files share (fcos_loss.hip, solo_targets.hip): the (level, image, tile) grid of the
// flattened training order, the flat segment grid, the sigmoid focal loss of one logit with its
// derivative and of one workgroup's tile of a [B][C][HW] map, the flat rescale kernel of the backward step, and the per-image box
// offsets as the kernels take them.  Everything sits in an unnamed namespace: each file has its own copy.
#pragma once

#include <float.h>
#include <math.h>

#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_fcos.h"

// The rounded-operation intrinsics of the HIP headers are plain operators there, and the compiler may still contract a product and
// a sum that meet after inlining.  Nothing in these files is contracted: the single fp32 operations are what the bit-equal targets rest on.
#pragma clang fp contract(off)

namespace bxi {
namespace {

__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_div(float a, float b) { return a / b; }

constexpr int kLocTile = BXI_FCOS_LOC_TILE;
constexpr int kElemTile = BXI_FCOS_ELEM_TILE;
constexpr int kMaxL = BXI_DET_MAX_LEVELS;

// the per-location grid: workgroup -> (level, image, tile)
struct LocGrid {
    int H[kMaxL], W[kMaxL], stride[kMaxL];
    int first[kMaxL + 1];       // locations of one image in the levels before l
    int tiles[kMaxL];           // ceil(H*W / kLocTile)
    int blk_first[kMaxL + 1];   // first workgroup of level l; blk_first[n] = number of workgroups
    int n, B;
};
// flat segments: workgroup -> (segment, tile of kElemTile elements)
struct FlatGrid {
    int count[3 * kMaxL];           // elements of segment s
    int blk_first[3 * kMaxL + 1];
    int n;                          // segments
};
// first box of every image, padded with the total: v[b] = gt_offsets_host[min(b, B)]
struct GtOffsets { int v[BXI_MAX_IMAGES + 1]; };

// ---- focal loss -----------------------------------------------------------------------------------------------------------
template <bool G2>
__device__ __forceinline__ void focal_one(float x, bool t, float gamma, float alpha, float scale, float& loss, float& grad) {
    const float e = expf(-fabsf(x));
    const float inv = 1.f / (1.f + e);
    const float big = inv, small = e * inv;                 // sigmoid(|x|), sigmoid(-|x|)
    const float p = x >= 0.f ? big : small, q = x >= 0.f ? small : big;    // sigmoid(x), 1 - sigmoid(x) without cancellation
    const float bce = fmaxf(t ? -x : x, 0.f) + log1pf(e);   // max(x,0) - x t + log1p(exp(-|x|))
    const float pt = t ? q : p;
    float mod, dmod;
    if (G2) {
        mod = pt * pt;
        dmod = 2.f * pt;
    } else {
        mod = powf(pt, gamma);
        dmod = gamma == 0.f ? 0.f : gamma * powf(pt, gamma - 1.f);
    }
    const float aw = t ? alpha : 1.f - alpha;
    const float dpt = t ? -(p * q) : p * q;
    loss = aw * bce * mod;
    grad = scale * aw * ((t ? -q : p) * mod + bce * dmod * dpt);           // d bce / dx = sigmoid(x) - t
}

// One workgroup's tile of a flat [B][C][hw] map: four consecutive elements per thread from e0 (one 16-byte load and store where
// the pointers allow it, four scalar ones elsewhere and on the tail -- the same element-to-thread map either way, so the sums do not
// depend on alignment).  Writes the four gradients and returns the workgroup's loss total before `scale` (thread 0 holds it).
template <bool G2>
__device__ __forceinline__ double focal_tile(const float* __restrict__ src, float* __restrict__ dst, int count, int e0, int hw, int C,
                                             size_t row0, const int64_t* __restrict__ labels, float gamma, float alpha, float scale,
                                             double* s4d) {
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && e0 + 3 < count;
    float v[4] = {0.f, 0.f, 0.f, 0.f}, gr[4];
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(src + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < count) v[j] = src[e0 + j];
    }
    // element e of the level is (b, c, yx) = (e / (C hw), (e / hw) % C, e % hw); its label is row row0 + b hw + yx
    int plane = e0 / hw, yx = e0 - plane * hw;
    int b = plane / C, c = plane - b * C;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float lo = 0.f;
        gr[j] = 0.f;
        if (e0 + j < count) {
            const bool t = labels[row0 + (size_t)b * hw + yx] == (int64_t)c;
            focal_one<G2>(v[j], t, gamma, alpha, scale, lo, gr[j]);
        }
        sum += lo;
        if (++yx == hw) {
            yx = 0;
            if (++c == C) { c = 0; ++b; }
        }
    }
    if (vec) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(gr[0], gr[1], gr[2], gr[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < count) dst[e0 + j] = gr[j];
    }
    return block_sum_4w_f64((double)sum, s4d);
}

// ---- backward rescale -----------------------------------------------------------------------------------------------------
struct RescaleSegs { const float* src[3 * kMaxL]; float* dst[3 * kMaxL]; int which[3 * kMaxL]; };

__global__ __launch_bounds__(256) void flat_rescale_kernel(RescaleSegs sg, FlatGrid f, const float* __restrict__ upstream) {
    const int blk = blockIdx.x;
    int s = 0;
    while (s + 1 < f.n && blk >= f.blk_first[s + 1]) ++s;
    const int count = f.count[s];
    const int e0 = (blk - f.blk_first[s]) * kElemTile + threadIdx.x * 4;
    if (e0 >= count) return;
    const float* src = sg.src[s];
    float* dst = sg.dst[s];
    const float u = upstream[sg.which[s]];
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && e0 + 3 < count) {
        float4 q = *reinterpret_cast<const float4*>(src + e0);
        q.x *= u; q.y *= u; q.z *= u; q.w *= u;
        *reinterpret_cast<float4*>(dst + e0) = q;
    } else {
        for (int j = 0; j < 4 && e0 + j < count; ++j) dst[e0 + j] = src[e0 + j] * u;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int make_grid(const int* H, const int* W, const int* stride, int n_levels, int B, LocGrid& g) {
    if (n_levels < 1 || n_levels > kMaxL || B < 0 || B > BXI_MAX_IMAGES) return BXI_ERR_BAD_SHAPE;
    g.n = n_levels;
    g.B = B;
    int64_t at = 0, blk = 0;
    for (int l = 0; l < kMaxL; ++l) {
        if (l < n_levels) {
            if (H[l] < 1 || W[l] < 1 || stride[l] < 1) return BXI_ERR_BAD_SHAPE;
            const int64_t hw = (int64_t)H[l] * W[l];
            if (!fits_i32(hw)) return BXI_ERR_BAD_SHAPE;
            g.H[l] = H[l]; g.W[l] = W[l]; g.stride[l] = stride[l];
            g.first[l] = (int)at;
            g.tiles[l] = (int)((hw + kLocTile - 1) / kLocTile);
            g.blk_first[l] = (int)blk;
            at += hw;
            blk += (int64_t)B * g.tiles[l];
            if (!fits_i32(at * (B > 0 ? B : 1) * 4) || !fits_i32(blk)) return BXI_ERR_BAD_SHAPE;
        } else {
            g.H[l] = g.W[l] = g.stride[l] = 1;
            g.first[l] = (int)at;
            g.tiles[l] = 1;
            g.blk_first[l] = (int)blk;
        }
    }
    g.first[kMaxL] = (int)at;
    g.blk_first[kMaxL] = (int)blk;
    for (int l = n_levels; l <= kMaxL; ++l) { g.first[l] = (int)at; g.blk_first[l] = (int)blk; }
    return BXI_OK;
}

// segments of `per_level` maps with `chan[k]` channels each; returns the number of workgroups or -1
int64_t make_flat(const LocGrid& g, const int* chan, int per_level, FlatGrid& f) {
    f.n = g.n * per_level;
    int64_t blk = 0;
    for (int s = 0; s < 3 * kMaxL; ++s) {
        f.blk_first[s] = (int)blk;
        if (s < f.n) {
            const int l = s / per_level, k = s - l * per_level;
            const int64_t cnt = (int64_t)g.B * chan[k] * g.H[l] * g.W[l];
            if (!fits_i32(cnt)) return -1;
            f.count[s] = (int)cnt;
            blk += (cnt + kElemTile - 1) / kElemTile;
            if (!fits_i32(blk)) return -1;
        } else {
            f.count[s] = 0;
        }
    }
    f.blk_first[3 * kMaxL] = (int)blk;
    for (int s = f.n; s <= 3 * kMaxL; ++s) f.blk_first[s] = (int)blk;
    return blk;
}

int read_offsets(const int* gt_offsets_host, int B, GtOffsets& off) {
    if (B < 0 || B > BXI_MAX_IMAGES) return BXI_ERR_BAD_SHAPE;
    if (B == 0) return BXI_OK;
    if (!gt_offsets_host) return BXI_ERR_NULL_POINTER;
    if (gt_offsets_host[0] != 0) return BXI_ERR_BAD_SHAPE;
    for (int b = 0; b <= BXI_MAX_IMAGES; ++b) {
        off.v[b] = gt_offsets_host[b <= B ? b : B];
        if (b > 0 && off.v[b] < off.v[b - 1]) return BXI_ERR_BAD_SHAPE;
    }
    return BXI_OK;
}

}  // namespace
}  // namespace bxi
