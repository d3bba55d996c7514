// solo_dconv_device.hpp -- everything the families of the dynamic mask convolution share: fp32 (solo_dconv.hip), fp16 / bf16
// (solo_dconv16.hip) and BoxLevelSet's per-level form (solo_dconv_level.hip, which runs the fp32 family group by group).
//   device   the segment table that travels in the kernel arguments, the walk from (image, j-th row) to the output row (locate), the
//            accumulator's row map (acc_row), the cell look-up that sets BXI_DCONV_STATUS_BAD_CELL (kernel_of), and the three small kernels
//            around the product: gather (by element type and kT layout tag), reduce, scatter (by the element type of the gradient maps).
//   host     the argument checks of include/boxinst/boxinst_hip_dconv.h in their ABI order (dconv_table, dconv_forward_args,
//            dconv_backward_args), the workspace carve, and the gather / reduce / scatter launches.
// The product kernels, their kT layouts (kt_at, kt16_at, kr16_at) and the layout tags built on them stay in the family's own file.
#pragma once

#include "common.hpp"

#include "../../include/boxinst/boxinst_hip_dconv.h"

namespace bxi {

constexpr int kDcThreads = 256;

typedef float f16v __attribute__((ext_vector_type(16)));
typedef uint16_t h16;                                                // a half value's bits, fp16 or bf16

struct DconvTable {
    const void* maps[BXI_DCONV_MAX_LEVELS];                          // of the family's element type: read through kernel_of<T> only
    void* gmaps[BXI_DCONV_MAX_LEVELS];                               // written by dconv_scatter_kernel<T, BF> only
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
// where kernel(row, e = 0) lies and the stride between channels; nullptr for no row or a cell outside its map (never read)
template <typename T>
__device__ __forceinline__ const T* kernel_of(const DconvTable& t, const int64_t* cells, int b, int row, int lev, int E, int& estride,
                                              int32_t* status) {
    estride = 0;
    if (row < 0) return nullptr;
    const int64_t cell = cells ? cells[row] : (int64_t)row;
    const int ncell = t.cells[lev];
    if (cell < 0 || cell >= ncell) {
        *status = BXI_DCONV_STATUS_BAD_CELL;
        return nullptr;
    }
    if (t.layout == BXI_DCONV_ROWS) { estride = 1; return static_cast<const T*>(t.maps[0]) + (size_t)cell * E; }
    estride = ncell;
    return static_cast<const T*>(t.maps[lev]) + (size_t)b * E * ncell + cell;
}

// One workgroup per (chunk of 32 rows of an image, quarter of E): the kernel values of the chunk from the maps (or from the test-time
// matrix) through the cells, as copies of T, to the place the layout tag names.  Lay::round(E) is the E the product kernel walks and
// Lay::at(ER, chunk, e, r) the element of (channel e, row r of the chunk).  Zeros for the chunk's missing rows, for the tail of E up to
// ER, for a cell outside its map and for the slots past the last chunk: every element of kT is written.
template <typename T, class Lay>
__global__ void __launch_bounds__(kDcThreads) dconv_gather_kernel(const DconvTable t, const int64_t* __restrict__ cells, T* __restrict__ kT,
                                                                  int32_t* status, int E) {
    const int chunk = blockIdx.x, ER = Lay::round(E), r = threadIdx.x & 31;
    int b = 0;
    while (b + 1 < t.B && chunk >= t.chunk0[b + 1]) ++b;
    int lev = 0, estride;
    const int row = chunk < t.chunk0[t.B] ? locate(t, b, (chunk - t.chunk0[b]) * 32 + r, lev) : -1;      // a slot past the last chunk: zeros
    const T* kp = kernel_of<T>(t, cells, b, row, lev, E, estride, status);
    const int per = (ER + (int)gridDim.y - 1) / (int)gridDim.y, e_end = min(ER, ((int)blockIdx.y + 1) * per);
    for (int e = blockIdx.y * per + (threadIdx.x >> 5); e < e_end; e += kDcThreads / 32)
        kT[Lay::at(ER, chunk, e, r)] = (kp && e < E) ? kp[(size_t)e * estride] : T(0);
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

// fp32 -> half, to nearest even; fp16 overflows to inf, a bf16 NaN is 0x7FC0 (as torch's casts)
template <bool BF> __device__ __forceinline__ h16 f2h(float x) {
    if constexpr (BF) {
        const uint32_t u = __float_as_uint(x);
        return x != x ? (h16)0x7FC0 : (h16)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    } else {
        return __builtin_bit_cast(h16, (_Float16)x);
    }
}
// Every element of every gradient map (T = float, or h16 as fp16 / bf16 by BF): the fp32 sum of gk over the rows of its segment that
// name its cell, in row order, rounded once for a half map.
template <typename T, bool BF>
__global__ void __launch_bounds__(kDcThreads) dconv_scatter_kernel(const DconvTable t, const int64_t* __restrict__ cells,
                                                                   const float* __restrict__ gk, int E) {
    const int l = blockIdx.y, ncell = t.cells[l];
    const int64_t total = (int64_t)(t.layout == BXI_DCONV_ROWS ? 1 : t.B) * E * ncell;
    const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (idx >= total) return;
    int b, e, cell;
    if (t.layout == BXI_DCONV_ROWS) { b = 0; cell = (int)(idx / E); e = (int)(idx % E); }
    else { cell = (int)(idx % ncell); e = (int)((idx / ncell) % E); b = (int)(idx / ncell / E); }
    const int i0 = t.start[l * t.B + b], i1 = t.start[l * t.B + b + 1];
    float s = 0.f;
    for (int i = i0; i < i1; ++i)
        if ((cells ? cells[i] : (int64_t)i) == cell) s += gk[(size_t)i * E + e];
    if constexpr (sizeof(T) == sizeof(float)) static_cast<float*>(t.gmaps[l])[idx] = s;
    else static_cast<h16*>(t.gmaps[l])[idx] = f2h<BF>(s);
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
        t.maps[l] = maps[l];
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

// The pointer checks of an entry point, in the order of the ABI: after dconv_table (and the half family's dtype check), before the
// workspace check.  Forward, after its return for N == 0: the call's pointers, then the maps.
static int dconv_forward_args(const DconvTable& t, const void* feat, const void* out, const int32_t* status, const int64_t* cells) {
    if (!feat || !out || !status || (!cells && t.layout == BXI_DCONV_MAPS)) return BXI_ERR_NULL_POINTER;
    for (int l = 0; l < t.L; ++l)
        if (!t.maps[l]) return BXI_ERR_NULL_POINTER;
    return BXI_OK;
}
// Backward, after its return for a call that wants no gradient: the call's pointers and the maps when there are rows, then the gradient
// maps, which go into the table.
static int dconv_backward_args(DconvTable& t, int N, const void* feat, const void* out, const void* grad_out, const int32_t* status,
                               const int64_t* cells, void* const* grad_kernel_maps) {
    if (N > 0) {
        if (!out || !grad_out || !status || (!cells && t.layout == BXI_DCONV_MAPS)) return BXI_ERR_NULL_POINTER;
        if (grad_kernel_maps && !feat) return BXI_ERR_NULL_POINTER;
        for (int l = 0; l < t.L; ++l)
            if (!t.maps[l]) return BXI_ERR_NULL_POINTER;
    }
    if (grad_kernel_maps)
        for (int l = 0; l < t.L; ++l) {
            if (!grad_kernel_maps[l]) return BXI_ERR_NULL_POINTER;
            t.gmaps[l] = grad_kernel_maps[l];
        }
    return BXI_OK;
}

// kT [slots][ER][32] of T with slots = N / 32 + B (never fewer than the chunks: sum_b ceil(n_b / 32)) and ER = E as the family's layout
// rounds it, then for the backward part [tiles][N][E] and gk [N][E] as fp32, back to back: kT is a multiple of 128 bytes and there is
// no padding, so every byte of the workspace is written.  `tile`: the pixels of one workgroup of the family's backward kernel.
template <typename T> struct DconvSpace { T* kT; float *part, *gk; int slots; };
template <typename T>
static size_t dconv_workspace(int ER, int tile, int N, int B, int E, int H, int W, bool backward, void* base, DconvSpace<T>* sp) {
    const size_t slots = (size_t)N / 32 + B, kt = slots * ER * 32, rows = (size_t)N * E;
    const size_t tiles = backward ? ((size_t)H * W + tile - 1) / tile : 0;
    if (sp) {
        sp->kT = static_cast<T*>(base);
        sp->part = reinterpret_cast<float*>(sp->kT + kt);
        sp->gk = sp->part + tiles * rows;
        sp->slots = (int)slots;
    }
    return sizeof(T) * kt + (backward ? sizeof(float) * rows * (tiles + 1) : 0);
}

// the three launches around the product; `label` is the family's BXI_LAUNCH name
template <typename T, class Lay>
static int dconv_gather(const char* label, const DconvTable& t, const int64_t* cells, const DconvSpace<T>& sp, int32_t* status, int E, hipStream_t s) {
    BXI_LAUNCH(label, s, (dconv_gather_kernel<T, Lay>), dim3((unsigned)sp.slots, 4), dim3(kDcThreads), 0, s, t, cells, sp.kT, status, E);
    return check_launch();
}
static int dconv_reduce(const char* label, const float* part, float* gk, int E, int tiles, int N, hipStream_t s) {
    BXI_LAUNCH(label, s, dconv_reduce_kernel, dim3((unsigned)N, (unsigned)((E + 31) / 32)), dim3(32 * kDcReduceLanes), 0, s, part, gk, E, tiles, N);
    return check_launch();
}
template <typename T, bool BF>
static int dconv_scatter(const char* label, const DconvTable& t, const int64_t* cells, const float* gk, int E, hipStream_t s) {
    int64_t most = 0;                                                // one grid row per level, as wide as the largest map
    for (int l = 0; l < t.L; ++l) {
        const int64_t total = (int64_t)(t.layout == BXI_DCONV_ROWS ? 1 : t.B) * E * t.cells[l];
        most = total > most ? total : most;
    }
    BXI_LAUNCH(label, s, (dconv_scatter_kernel<T, BF>), dim3((unsigned)((most + kDcThreads - 1) / kDcThreads), (unsigned)t.L), dim3(kDcThreads), 0, s, t,
               cells, gk, E);
    return check_launch();
}

}  // namespace bxi
