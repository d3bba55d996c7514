// solo_dconv_device.hpp -- what the fp32 family (solo_dconv.hip) and the half-precision family (solo_dconv16.hip) of the dynamic mask
// convolution share: the segment table that travels in the kernel arguments, the walk from (image, j-th row) to the output row, the
// accumulator's row map and the host-side argument checks of include/boxinst/boxinst_hip_dconv.h.
#pragma once

#include "common.hpp"

#include "../../include/boxinst/boxinst_hip_dconv.h"

namespace bxi {

constexpr int kDcThreads = 256;

typedef float f16v __attribute__((ext_vector_type(16)));

struct DconvTable {
    const float* maps[BXI_DCONV_MAX_LEVELS];                         // the half family keeps its 2-byte maps here too and casts
    float* gmaps[BXI_DCONV_MAX_LEVELS];
    int cells[BXI_DCONV_MAX_LEVELS];                                 // cells of one image's map of the level (S^2), or the matrix's rows
    int start[BXI_DCONV_MAX_LEVELS * BXI_MAX_IMAGES + 1];            // start[l*B + b]: first row of segment (l, b); start[L*B] = N
    int chunk0[BXI_MAX_IMAGES + 1];                                  // first chunk of 32 rows of image b in kT; chunk0[B] = all chunks
    int L, B, layout;
};

__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ int rows_of_image(const DconvTable& t, int b) {
    int n = 0;
    for (int l = 0; l < t.L; ++l) n += t.start[l * t.B + b + 1] - t.start[l * t.B + b];
    return n;
}
// the j-th row of image b (levels in order): its output row, or -1 past the image's last; `lev` its level
__device__ __forceinline__ int locate(const DconvTable& t, int b, int j, int& lev) {
    int row = -1;
    lev = 0;
    for (int l = 0; l < t.L; ++l) {
        const int s0 = t.start[l * t.B + b], cnt = t.start[l * t.B + b + 1] - s0;
        if (j >= 0 && j < cnt) { row = s0 + j; lev = l; }
        j -= cnt;                                                    // negative from the hit on
    }
    return row;
}

// gk[row][e] = sum over the tiles of part[tile][row][e]: kDcReduceLanes interleaved sums (tile % 32), then those in order.
constexpr int kDcReduceLanes = 32;
static __global__ void __launch_bounds__(32 * kDcReduceLanes) dconv_reduce_kernel(const float* __restrict__ part, float* __restrict__ gk, int E,
                                                                                  int tiles, int N) {
    __shared__ float red[kDcReduceLanes][32];
    const int row = blockIdx.x, e = blockIdx.y * 32 + (threadIdx.x & 31), tl = threadIdx.x >> 5;
    float s = 0.f;
    if (e < E)
        for (int k = tl; k < tiles; k += kDcReduceLanes) s += part[((size_t)k * N + row) * E + e];
    red[tl][threadIdx.x & 31] = s;
    __syncthreads();
    if (tl == 0 && e < E) {
        float v = red[0][threadIdx.x];
        for (int k = 1; k < kDcReduceLanes; ++k) v += red[k][threadIdx.x];
        gk[(size_t)row * E + e] = v;
    }
}

// the checks both entry points share; fills the table
static int dconv_table(int B, int E, int H, int W, const void* const* maps, const int* grids, int L, int layout, const int* seg_counts, int N,
                       int activation, DconvTable& t) {
    if (!maps || !grids || !seg_counts) return BXI_ERR_NULL_POINTER;
    if (B < 1 || B > BXI_MAX_IMAGES || L < 1 || L > BXI_DCONV_MAX_LEVELS || E < 1 || E > BXI_DCONV_MAX_E || H < 1 || W < 1 || N < 0)
        return BXI_ERR_BAD_SHAPE;
    if (!fits_i32((int64_t)H * W) || !fits_i32((int64_t)B * E * H * W) || !fits_i32((int64_t)N * H * W)) return BXI_ERR_BAD_SHAPE;
    if (layout != BXI_DCONV_MAPS && layout != BXI_DCONV_ROWS) return BXI_ERR_BAD_ARGUMENT;
    if (activation != BXI_DCONV_NONE && activation != BXI_DCONV_SIGMOID) return BXI_ERR_BAD_ARGUMENT;
    if (layout == BXI_DCONV_ROWS && (L != 1 || B != 1)) return BXI_ERR_BAD_SHAPE;
    t.L = L; t.B = B; t.layout = layout;
    int64_t at = 0;
    for (int l = 0; l < L; ++l) {
        if (grids[l] < 1) return BXI_ERR_BAD_SHAPE;
        const int64_t ncell = layout == BXI_DCONV_ROWS ? (int64_t)grids[l] : (int64_t)grids[l] * grids[l];
        if (!fits_i32(ncell) || !fits_i32((int64_t)(layout == BXI_DCONV_ROWS ? 1 : B) * E * ncell)) return BXI_ERR_BAD_SHAPE;
        t.cells[l] = (int)ncell;
        t.maps[l] = static_cast<const float*>(maps[l]);
        t.gmaps[l] = nullptr;
        for (int b = 0; b < B; ++b) {
            const int c = seg_counts[l * B + b];
            if (c < 0 || c > N) return BXI_ERR_BAD_SHAPE;
            t.start[l * B + b] = (int)at;
            at += c;
        }
    }
    if (at != N) return BXI_ERR_BAD_SHAPE;
    t.start[L * B] = N;
    t.chunk0[0] = 0;
    for (int b = 0; b < B; ++b) {
        int nb = 0;
        for (int l = 0; l < L; ++l) nb += seg_counts[l * B + b];
        t.chunk0[b + 1] = t.chunk0[b] + (nb + 31) / 32;
    }
    return BXI_OK;
}

static bool dconv_query_ok(int N, int B, int E, int H, int W) {
    return N >= 1 && B >= 1 && B <= BXI_MAX_IMAGES && E >= 1 && E <= BXI_DCONV_MAX_E && H >= 1 && W >= 1 && fits_i32((int64_t)H * W) &&
           fits_i32((int64_t)N * H * W);
}

}  // namespace bxi
