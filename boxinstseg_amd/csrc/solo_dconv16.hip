// solo_dconv16.hip -- the dynamic 1x1 mask convolution of the SOLOv2-style heads on fp16 / bf16 tensors read in place
// (include/boxinst/boxinst_hip_dconv16.h): the precision the reference runs these statements in under autocast.  The row order, the
// segment table, the layouts and the argument checks are those of solo_dconv.hip (solo_dconv_device.hpp); the products run on
// v_mfma_f32_32x32x16_{f16,bf16}: lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][column r], j = 0..7, as
// ONE 16-byte fragment, the fp32 result has its column on the lane and rows acc_row(reg, h) in its 16 registers.
//
// Here: the two product kernels with their four (type, out type) dispatches, their two kT layouts (kt16_at and kr16_at, the tags Kt16 and
// Kr16) and the two entry points.  The gather, the reduction, the pass over the gradient maps, f2h, the pointer checks, the workspace
// carve and the launches of the three small kernels are solo_dconv_device.hpp's, shared with solo_dconv.hip.
//
// dconv_gather_kernel<h16, Kt16 | Kr16>  (solo_dconv_device.hpp) one workgroup per (chunk of 32 rows, quarter of E): 2-byte copies, the
//   same for both types.  Forward (Kt16): per chunk and k step of 16 channels lane l's fragment at [step][l][8]: a wave reads the A
//   operand of a step as one 1 KB piece.  Backward (Kr16): [chunk][channel][32 rows], the A operand of grad_feat's product (A row =
//   channel, k = rows).  Zeros for a chunk's missing rows, for the tail of E up to a multiple of 16 and for a cell outside its map.
// dconv16_fwd_kernel    one workgroup = one tile of 64 pixels of one image.  The tile's E16 x 64 feature values go to LDS once,
//   PIXEL-major ([pixel][E16 + 8]): the B fragment of a lane is one 16-byte read, and a row's 8 extra halves keep the 32 lanes of a
//   16-byte read on different banks.  Then every wave takes chunks of 32 of the image's rows; sigmoid in fp32, one rounding, stores
//   contiguous along the pixels.  An image without rows returns before it reads anything.
// dconv16_bwd_kernel    one workgroup = one tile of 64 pixels of one image; g of up to 64 of the image's rows sits in LDS as halves, row-
//   major AND pixel-major.  A wave owns blocks of 32 channels: grad_feat's block is A = kR, B = g pixel-major, k = the image's rows;
//   grad_kernel's per-tile partial is A = g row-major, B = the feature block [channel][pixel] in LDS, k = the tile's pixels, stored as
//   fp32 to part[tile][row][e].
// dconv_reduce_kernel, dconv_scatter_kernel<h16, BF>  (solo_dconv_device.hpp) the fp32 family's reduction; every element of every
//   gradient map, the fp32 sum of gk over the rows of its segment that name its cell, in row order, rounded once.
#include "solo_dconv_device.hpp"

#include "../../include/boxinst/boxinst_hip_dconv16.h"

namespace bxi {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // eight of them: one MFMA fragment
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kP16 = BXI_DCONV16_TILE;
constexpr int kPad16 = 8;                                            // halves added to an LDS row: rows stay 16-byte aligned
constexpr int kStride16 = kP16 + kPad16;                             // the backward's LDS rows of 64 values

__host__ __device__ __forceinline__ int e16_of(int E) { return (E + 15) & ~15; }
__device__ __forceinline__ size_t kt16_at(int E16, int chunk, int e, int r) {
    return (size_t)chunk * E16 * 32 + (size_t)(e >> 4) * 512 + (size_t)((((e >> 3) & 1) * 32 + r) * 8 + (e & 7));
}
__device__ __forceinline__ size_t kr16_at(int E16, int chunk, int e, int r) { return ((size_t)chunk * E16 + e) * 32 + r; }
struct Kt16 {                                                        // the layout tags of dconv_gather_kernel: forward, backward
    static __host__ __device__ __forceinline__ int round(int E) { return e16_of(E); }
    static __device__ __forceinline__ size_t at(int E16, int chunk, int e, int r) { return kt16_at(E16, chunk, e, r); }
};
struct Kr16 : Kt16 {
    static __device__ __forceinline__ size_t at(int E16, int chunk, int e, int r) { return kr16_at(E16, chunk, e, r); }
};

template <bool BF> __device__ __forceinline__ float h2f(h16 v) {
    if constexpr (BF) return __uint_as_float((uint32_t)v << 16);
    else return (float)__builtin_bit_cast(_Float16, v);
}
template <bool BF, bool F32> __device__ __forceinline__ float load_o(const void* p, size_t at) {
    if constexpr (F32) return static_cast<const float*>(p)[at];
    else return h2f<BF>(static_cast<const h16*>(p)[at]);
}
template <bool BF, bool F32> __device__ __forceinline__ void store_o(void* p, size_t at, float v) {
    if constexpr (F32) static_cast<float*>(p)[at] = v;
    else static_cast<h16*>(p)[at] = f2h<BF>(v);
}

template <bool BF> __device__ __forceinline__ f16v mfma16(u32x4 a, u32x4 b, f16v c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
#else
    return c;
#endif
}

template <bool BF, bool F32>
__global__ void __launch_bounds__(kDcThreads) dconv16_fwd_kernel(const DconvTable t, const h16* __restrict__ feat, const h16* __restrict__ kT,
                                                                 void* __restrict__ out, int64_t* __restrict__ img_inds, int E, int HW, int tiles,
                                                                 int act, int vec) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    h16* lds = reinterpret_cast<h16*>(lds_raw);                      // [kP16][S]
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles, p0 = tile * kP16;
    const int nb = rows_of_image(t, b);
    if (nb == 0) return;
    const int E16 = e16_of(E), S = E16 + kPad16;
    const h16* fb = feat + (size_t)b * E * HW;
    if (vec) {
        // H*W a multiple of 8 and a 16-byte aligned feature: an item is two channels x eight pixels, two 16-byte loads (unconditional on a
        // clamped address, zeros by select) and eight 4-byte LDS stores of (f(e, p), f(e + 1, p)); four items' loads go out before the stores
        const int total = (E16 / 2) * (kP16 / 8);
        uint32_t* lds32 = reinterpret_cast<uint32_t*>(lds);
        for (int base = 0; base < total; base += 4 * kDcThreads) {
            u32x4 v[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = min(base + u * kDcThreads + (int)threadIdx.x, total - 1);
                const int e = 2 * (idx >> 3), p = p0 + 8 * (idx & 7);
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    v[u][w] = *reinterpret_cast<const u32x4*>(fb + (size_t)min(e + w, E - 1) * HW + min(p, HW - 8));
                    if (e + w >= E || p >= HW) v[u][w] = u32x4{0, 0, 0, 0};
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * kDcThreads + (int)threadIdx.x;
                if (idx < total) {
                    const int e = 2 * (idx >> 3), pl = 8 * (idx & 7);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t lo = (v[u][0][i >> 1] >> (16 * (i & 1))) & 0xffffu, hi = (v[u][1][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                        lds32[((pl + i) * S + e) >> 1] = lo | (hi << 16);
                    }
                }
            }
        }
    } else {
        // any other feature: an item is one channel x one 16-byte ALIGNED piece of its row; the tile's 64 pixels of a row start `a` elements
        // past such a boundary and touch nine pieces.  A piece that lies whole inside the tile's pixels is one vector load, the pieces at
        // the row's head and tail are element loads; pixels past the image and channels past E are zeros.
        const int total = E16 * 9, pend = min(p0 + kP16, HW);
        for (int idx = threadIdx.x; idx < total; idx += kDcThreads) {
            const int e = idx / 9, j = idx % 9;
            const h16* rowp = fb + (size_t)min(e, E - 1) * HW;
            const int a = (int)((reinterpret_cast<uintptr_t>(rowp + p0) >> 1) & 7);
            const int start = p0 - a + 8 * j;
            h16 val[8];
            if (e < E && start >= p0 && start + 8 <= pend) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(rowp + start);
#pragma unroll
                for (int i = 0; i < 8; ++i) val[i] = (h16)(v[i >> 1] >> (16 * (i & 1)));
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int p = start + i;
                    val[i] = (e < E && p >= p0 && p < pend) ? rowp[p] : (h16)0;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = start + i;
                if (p >= p0 && p < p0 + kP16) lds[(p - p0) * S + e] = val[i];
            }
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int ps = wave & 1, px = p0 + ps * 32 + r;                  // two pixel slices of 32; the two waves of a slice take every other chunk
    const u32x4* col = reinterpret_cast<const u32x4*>(lds + (ps * 32 + r) * S + 8 * half);
    const int chunks = (nb + 31) / 32, steps = E16 / 16;
    for (int c = wave >> 1; c < chunks; c += 2) {
        int lev;
        const int row = locate(t, b, c * 32 + r, lev);
        const u32x4* ka = reinterpret_cast<const u32x4*>(kT + (size_t)(t.chunk0[b] + c) * E16 * 32) + lane;
        f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int s = 0;
        for (; s + 4 <= steps; s += 4) {                             // four A fragments asked for before the first product waits
            u32x4 a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = ka[(s + u) * 64];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma16<BF>(a[u], col[(s + u) * 2], acc);
        }
        for (; s < steps; ++s) acc = mfma16<BF>(ka[s * 64], col[s * 2], acc);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int orow = __shfl(row, acc_row(reg, half));
            if (orow >= 0 && px < HW) {
                float v = acc[reg];
                if (act) v = 1.f / (1.f + expf(-v));
                store_o<BF, F32>(out, (size_t)orow * HW + px, v);
            }
        }
        if (img_inds && tile == 0 && ps == 0 && half == 0 && row >= 0) img_inds[row] = b;
    }
}

template <bool BF, bool F32>
__global__ void __launch_bounds__(kDcThreads) dconv16_bwd_kernel(const DconvTable t, const h16* __restrict__ feat, const h16* __restrict__ kR,
                                                                 const void* __restrict__ out, const void* __restrict__ gout,
                                                                 h16* __restrict__ gfeat, float* __restrict__ part, int E, int HW, int tiles, int N,
                                                                 int act, int vec) {
    constexpr int P = kP16, S = kStride16;
    __shared__ __align__(16) h16 g_lds[64 * S];                      // [row of the chunk][pixel]
    __shared__ __align__(16) h16 gt_lds[P * S];                      // [pixel][row of the chunk]
    __shared__ __align__(16) h16 f_lds[4][32 * S];                   // per wave: [channel of the block][pixel]
    __shared__ int row_lds[64];
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles, p0 = tile * P;
    const int nb = rows_of_image(t, b);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int eblocks = (E + 31) / 32, chunks = (nb + 63) / 64, E16 = e16_of(E);
    const h16* fb = feat + (size_t)b * E * HW;
    for (int eb0 = 0; eb0 < eblocks; eb0 += 4) {                     // the same trip count for every wave: the barriers below are uniform
        const int eb = eb0 + wave;
        const bool active = eb < eblocks;
        const int e_mine = eb * 32 + r;                              // grad_feat: this lane's A row; grad_kernel: its B / C column
        f16v accf[2];
        for (int s = 0; s < 2; ++s) accf[s] = f16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (active && part && nb > 0) {                              // the feature block of this wave: 32 channels x 64 pixels
            if (vec) {                                               // 16-byte pieces: four loads, unconditional on a clamped address, four stores
                u32x4 fv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = eb * 32 + u * 8 + (lane >> 3), p = p0 + 8 * (lane & 7);
                    fv[u] = *reinterpret_cast<const u32x4*>(fb + (size_t)min(e, E - 1) * HW + min(p, HW - 8));
                    if (e >= E || p >= HW) fv[u] = u32x4{0, 0, 0, 0};
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<u32x4*>(&f_lds[wave][(u * 8 + (lane >> 3)) * S + 8 * (lane & 7)]) = fv[u];
            } else {
                for (int r0 = 0; r0 < 32; r0 += 8) {
                    h16 fv[8];
                    const int p = p0 + lane;
#pragma unroll
                    for (int u = 0; u < 8; ++u) fv[u] = fb[(size_t)min(eb * 32 + r0 + u, E - 1) * HW + min(p, HW - 1)];
#pragma unroll
                    for (int u = 0; u < 8; ++u) f_lds[wave][(r0 + u) * S + lane] = (eb * 32 + r0 + u < E && p < HW) ? fv[u] : (h16)0;
                }
            }
        }
        for (int ic = 0; ic < chunks; ++ic) {
            if (chunks > 1 || eb0 == 0) {                            // one chunk: g stays for every channel block
                __syncthreads();
                if (threadIdx.x < 64) {
                    int lev;
                    row_lds[threadIdx.x] = locate(t, b, ic * 64 + (int)threadIdx.x, lev);
                }
                __syncthreads();
                static_assert(64 * P == 16 * kDcThreads, "sixteen values of g per thread");
                float gl[16], pl[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {                       // loads only, unconditional on a clamped address: they overlap
                    const int idx = u * kDcThreads + (int)threadIdx.x, row = row_lds[idx / P];
                    const size_t at = (size_t)max(row, 0) * HW + min(p0 + idx % P, HW - 1);
                    gl[u] = load_o<BF, F32>(gout, at);
                    pl[u] = act ? load_o<BF, F32>(out, at) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int idx = u * kDcThreads + (int)threadIdx.x, il = idx / P, p = idx % P;
                    const float g = act ? gl[u] * pl[u] * (1.f - pl[u]) : gl[u];
                    const h16 gh = (row_lds[il] >= 0 && p0 + p < HW) ? f2h<BF>(g) : (h16)0;        // the one rounding of g: an MFMA operand
                    g_lds[il * S + p] = gh;
                    gt_lds[p * S + il] = gh;
                }
            }
            __syncthreads();
            if (!active) continue;
            const int cnt = nb - ic * 64 < 64 ? nb - ic * 64 : 64;
            if (gfeat) {
                // kR holds zeros for a missing row and for a cell outside its map; a k step of 16 rows lies inside one chunk of 32
                const int ec = e_mine < E16 ? e_mine : 0;
                for (int s = 0; 16 * s < cnt; ++s) {
                    u32x4 a = *reinterpret_cast<const u32x4*>(kR + kr16_at(E16, t.chunk0[b] + 2 * ic + (s >> 1), ec, (16 * s + 8 * half) & 31));
                    if (e_mine >= E16) a = u32x4{0, 0, 0, 0};
                    const int k0 = 16 * s + 8 * half;
                    accf[0] = mfma16<BF>(a, *reinterpret_cast<const u32x4*>(&gt_lds[r * S + k0]), accf[0]);
                    accf[1] = mfma16<BF>(a, *reinterpret_cast<const u32x4*>(&gt_lds[(32 + r) * S + k0]), accf[1]);
                }
            }
            if (part) {
                for (int sub = 0; sub * 32 < cnt; ++sub) {
                    f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < P / 16; ++s) {
                        const int k0 = 16 * s + 8 * half;
                        acc = mfma16<BF>(*reinterpret_cast<const u32x4*>(&g_lds[(sub * 32 + r) * S + k0]),
                                         *reinterpret_cast<const u32x4*>(&f_lds[wave][r * S + k0]), acc);
                    }
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = row_lds[sub * 32 + acc_row(reg, half)];
                        if (row >= 0 && e_mine < E) part[((size_t)tile * N + row) * E + e_mine] = acc[reg];
                    }
                }
            }
        }
        if (active && gfeat) {
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int e = eb * 32 + acc_row(reg, half), p = p0 + s * 32 + r;
                    if (e < E && p < HW) gfeat[((size_t)b * E + e) * HW + p] = f2h<BF>(accf[s][reg]);
                }
            }
        }
    }
}

// the workspace: kT (or kR) as halves, a multiple of 1 KB, the backward's tiles of kP16 pixels
typedef DconvSpace<h16> Dconv16Space;
static size_t dconv16_workspace(int N, int B, int E, int H, int W, bool backward, void* base, Dconv16Space* sp) {
    return dconv_workspace<h16>(e16_of(E), kP16, N, B, E, H, W, backward, base, sp);
}

static bool dconv16_types_ok(int dtype, int out_dtype) {
    return (dtype == BXI_DCONV16_F16 || dtype == BXI_DCONV16_BF16) && (out_dtype == dtype || out_dtype == BXI_DCONV16_OUT_F32);
}

template <bool BF, bool F32>
static int dconv16_forward_launch(const DconvTable& t, const h16* feat, const Dconv16Space& sp, void* out, int64_t* img_inds, int E, int HW,
                                  int activation, hipStream_t s) {
    const int tiles = (HW + kP16 - 1) / kP16;
    const size_t lds = sizeof(h16) * (size_t)kP16 * (e16_of(E) + kPad16);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dconv16_fwd_kernel<BF, F32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) { set_last_hip_error((int)e); return BXI_ERR_LAUNCH; }
    }
    const int vec = !(HW & 7) && aligned(feat, 16);
    BXI_LAUNCH("solo_dconv16_fwd", s, (dconv16_fwd_kernel<BF, F32>), dim3((unsigned)((int64_t)t.B * tiles)), dim3(kDcThreads), lds, s, t, feat, sp.kT,
               out, img_inds, E, HW, tiles, activation, vec);
    return check_launch();
}

template <bool BF, bool F32>
static int dconv16_backward_launch(const DconvTable& t, const h16* feat, const Dconv16Space& sp, const void* out, const void* gout, h16* gfeat,
                                   float* part, int E, int HW, int N, int activation, hipStream_t s) {
    const int tiles = (HW + kP16 - 1) / kP16;
    const int vec = !(HW & 7) && aligned(feat, 16);
    BXI_LAUNCH("solo_dconv16_bwd", s, (dconv16_bwd_kernel<BF, F32>), dim3((unsigned)((int64_t)t.B * tiles)), dim3(kDcThreads), 0, s, t, feat, sp.kT, out,
               gout, gfeat, part, E, HW, tiles, N, activation, vec);
    return check_launch();
}

}  // namespace bxi

extern "C" size_t bxi_solo_dconv16_forward_workspace_bytes(int N, int B, int E) {
    using namespace bxi;
    return dconv_query_ok(N, B, E, 1, 1) ? dconv16_workspace(N, B, E, 1, 1, false, nullptr, nullptr) : 0;
}

extern "C" int bxi_solo_dconv16_forward(const void* feat, int dtype, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                        int L, int layout, const int64_t* cells, const int* seg_counts, int N, int activation, void* out,
                                        int out_dtype, int64_t* img_inds, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    DconvTable t;
    int rc = dconv_table(B, E, H, W, kernel_maps, grids, L, layout, seg_counts, N, activation, t);
    if (rc != BXI_OK) return rc;
    if (!dconv16_types_ok(dtype, out_dtype)) return BXI_ERR_BAD_ARGUMENT;
    if (N == 0) return BXI_OK;
    rc = dconv_forward_args(t, feat, out, status, cells);
    if (rc != BXI_OK) return rc;
    if (!workspace_ok(workspace, workspace_bytes, bxi_solo_dconv16_forward_workspace_bytes(N, B, E), 16)) return BXI_ERR_WORKSPACE;
    Dconv16Space sp;
    dconv16_workspace(N, B, E, H, W, false, workspace, &sp);
    hipStream_t s = as_stream(stream);
    rc = dconv_gather<h16, Kt16>("solo_dconv16_gather", t, cells, sp, status, E, s);
    if (rc != BXI_OK) return rc;
    const h16* f = static_cast<const h16*>(feat);
    const bool f32 = out_dtype == BXI_DCONV16_OUT_F32;
    if (dtype == BXI_DCONV16_BF16)
        return f32 ? dconv16_forward_launch<true, true>(t, f, sp, out, img_inds, E, H * W, activation, s)
                   : dconv16_forward_launch<true, false>(t, f, sp, out, img_inds, E, H * W, activation, s);
    return f32 ? dconv16_forward_launch<false, true>(t, f, sp, out, img_inds, E, H * W, activation, s)
               : dconv16_forward_launch<false, false>(t, f, sp, out, img_inds, E, H * W, activation, s);
}

extern "C" size_t bxi_solo_dconv16_backward_workspace_bytes(int N, int B, int E, int H, int W) {
    using namespace bxi;
    return dconv_query_ok(N, B, E, H, W) ? dconv16_workspace(N, B, E, H, W, true, nullptr, nullptr) : 0;
}

extern "C" int bxi_solo_dconv16_backward(const void* feat, int dtype, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                         int L, int layout, const int64_t* cells, const int* seg_counts, int N, int activation, const void* out,
                                         const void* grad_out, int out_dtype, void* grad_feat, void* const* grad_kernel_maps, int32_t* status,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    DconvTable t;
    int rc = dconv_table(B, E, H, W, kernel_maps, grids, L, layout, seg_counts, N, activation, t);
    if (rc != BXI_OK) return rc;
    if (!dconv16_types_ok(dtype, out_dtype)) return BXI_ERR_BAD_ARGUMENT;
    if (!grad_feat && !grad_kernel_maps) return BXI_OK;
    rc = dconv_backward_args(t, N, feat, out, grad_out, status, cells, grad_kernel_maps);
    if (rc != BXI_OK) return rc;
    Dconv16Space sp = {nullptr, nullptr, nullptr, 0};
    hipStream_t s = as_stream(stream);
    if (N > 0) {
        if (!workspace_ok(workspace, workspace_bytes, bxi_solo_dconv16_backward_workspace_bytes(N, B, E, H, W), 16)) return BXI_ERR_WORKSPACE;
        dconv16_workspace(N, B, E, H, W, true, workspace, &sp);
        rc = dconv_gather<h16, Kr16>("solo_dconv16_gather", t, cells, sp, status, E, s);
        if (rc != BXI_OK) return rc;
    }
    // without gradient maps the feature is not read and the partial sums are not formed
    float* part = grad_kernel_maps ? sp.part : nullptr;
    const int HW = H * W, tiles = (HW + kP16 - 1) / kP16;
    const h16* f = static_cast<const h16*>(feat);
    h16* gf = static_cast<h16*>(grad_feat);
    const bool bf = dtype == BXI_DCONV16_BF16, f32 = out_dtype == BXI_DCONV16_OUT_F32;
    if (bf) rc = f32 ? dconv16_backward_launch<true, true>(t, f, sp, out, grad_out, gf, part, E, HW, N, activation, s)
                     : dconv16_backward_launch<true, false>(t, f, sp, out, grad_out, gf, part, E, HW, N, activation, s);
    else rc = f32 ? dconv16_backward_launch<false, true>(t, f, sp, out, grad_out, gf, part, E, HW, N, activation, s)
                  : dconv16_backward_launch<false, false>(t, f, sp, out, grad_out, gf, part, E, HW, N, activation, s);
    if (rc != BXI_OK || !grad_kernel_maps) return rc;
    if (part) {
        rc = dconv_reduce("solo_dconv16_reduce", part, sp.gk, E, tiles, N, s);
        if (rc != BXI_OK) return rc;
    }
    return bf ? dconv_scatter<h16, true>("solo_dconv16_scatter", t, cells, sp.gk, E, s)
              : dconv_scatter<h16, false>("solo_dconv16_scatter", t, cells, sp.gk, E, s);
}
