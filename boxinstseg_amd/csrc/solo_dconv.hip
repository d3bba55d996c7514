// solo_dconv.hip -- the dynamic 1x1 mask convolution of the SOLOv2-style heads on gfx950 (discobox_head.py:1180-1246 / :1275 in loss,
// :936-1022 in corr_loss, :1607-1608 in get_seg_single): out[i,p] = act(sum_e kernel(i,e) feat[image_i,e,p]), forward and backward.
//
// Rows are level-major, image by image inside a level (include/boxinst/boxinst_hip_dconv.h); the segment table travels in the kernel
// arguments and the cells are device data.  A first small launch gathers the kernel values of every chunk of 32 rows of an image into the
// workspace (kT, layout at kt_at: zeros for the chunk's missing rows, for the tail of E up to a multiple of 8 and for a cell outside its
// map): read in the map's layout a row's E values lie in E different cache lines, and every workgroup of the main kernel would fetch them
// again; from kT a wave reads the A operands of four k steps of 32 rows as one 1 KB piece.  All products run on
// v_mfma_f32_32x32x2_f32: lane l holds A[row l&31][k l>>5] and B[k l>>5][column l&31], the result has its column on the lane and rows
// (reg&3) + 8 (reg>>2) + 4 (l>>5) in its 16 registers, and every element is one fmaf chain in ascending k.
//
// Here: the two product kernels, their kT layout (kt_at, the tag Kt) and the two entry points.  The gather, the reduction, the pass over
// the gradient maps, the pointer checks, the workspace carve and the launches of the three small kernels are solo_dconv_device.hpp's,
// shared with solo_dconv16.hip.
//
// dconv_gather_kernel<float, Kt>  (solo_dconv_device.hpp) one workgroup per (chunk, quarter of E): kT from the maps (or from the test-time
//   matrix) through the cells.
// dconv_fwd_kernel<P>   one workgroup = one tile of P pixels of one image.  The tile's E x P feature values go to LDS once; then every
//   wave takes chunks of 32 of the image's rows (A rows = instances, B / C columns = pixels: a pixel stays on its lane, the stores are
//   coalesced), k = e ascending.  An image without rows returns before it reads anything.
// dconv_bwd_kernel      one workgroup = one tile of 64 pixels of one image; g = grad_out (* p (1 - p)) of up to 64 of the image's rows
//   sits in LDS.  A wave owns blocks of 32 channels: grad_feat's block is A = kernel values [e][i], B = g [i][pixel], k = the image's rows
//   ascending; grad_kernel's per-tile partial is A = g [i][pixel], B = the feature block [pixel][e] (staged through LDS, read coalesced),
//   k = the tile's pixels ascending, stored to part[tile][row][e].
// dconv_reduce_kernel   (solo_dconv_device.hpp) gk[row][e] = the partials of the row's image's tiles, 32 interleaved sums added in order.
// dconv_scatter_kernel<float, false>  (solo_dconv_device.hpp) every element of every gradient map: the sum of gk over the rows of its
//   segment that name its cell, in row order.
#include "solo_dconv_device.hpp"

namespace bxi {

constexpr int kDcStride = BXI_DCONV_TILE + 1;        // LDS row stride of the backward's tiles: column reads hit 32 banks

__device__ __forceinline__ f16v mfma32(float a, float b, f16v c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
    return c;
#endif
}
// kT: per chunk of 32 rows E8 x 32 floats (E8 = E rounded up to 8), as float4 records [e / 8][e & 1][row][(e >> 1) & 3]: the lane that holds
// A[row][k = e & 1] of four consecutive k steps reads them as ONE 16-byte load, a wave 1 KB in a piece
__host__ __device__ __forceinline__ int e8_of(int E) { return (E + 7) & ~7; }
__device__ __forceinline__ size_t kt_at(int E8, int chunk, int e, int r) {
    return (size_t)chunk * E8 * 32 + (size_t)((e >> 3) * 2 + (e & 1)) * 128 + r * 4 + ((e >> 1) & 3);
}
struct Kt {                                                          // the layout tag of dconv_gather_kernel
    static __host__ __device__ __forceinline__ int round(int E) { return e8_of(E); }
    static __device__ __forceinline__ size_t at(int E8, int chunk, int e, int r) { return kt_at(E8, chunk, e, r); }
};

template <int P>
__global__ void __launch_bounds__(kDcThreads) dconv_fwd_kernel(const DconvTable t, const float* __restrict__ feat, const float* __restrict__ kT,
                                                               float* __restrict__ out, int64_t* __restrict__ img_inds, int E, int HW,
                                                               int tiles, int act, int vec) {
    extern __shared__ float lds[];                                   // [E8][P]
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles, p0 = tile * P;
    const int nb = rows_of_image(t, b);
    if (nb == 0) return;
    const int E8 = e8_of(E);
    const float* fb = feat + (size_t)b * E * HW;
    // Batches of eight loads per thread with no exit between them, each unconditional on a clamped address, zeros by select: behind a branch
    // or a loop exit every load would wait for the one before.
    if (vec) {                                                       // HW % 4 == 0 and a 16-byte aligned feature: four pixels per load
        const int total = E8 * (P / 4);
        for (int base = 0; base < total; base += 8 * kDcThreads) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = min(base + u * kDcThreads + (int)threadIdx.x, total - 1);
                const int e = idx / (P / 4), p = p0 + 4 * (idx % (P / 4));
                v[u] = *reinterpret_cast<const float4*>(fb + (size_t)min(e, E - 1) * HW + min(p, HW - 4));
                if (e >= E || p >= HW) v[u] = float4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + u * kDcThreads + (int)threadIdx.x;
                if (idx < total) *reinterpret_cast<float4*>(lds + 4 * idx) = v[u];
            }
        }
    } else {
        const int total = E8 * P;
        for (int base = 0; base < total; base += 8 * kDcThreads) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = min(base + u * kDcThreads + (int)threadIdx.x, total - 1);
                const int e = idx / P, p = p0 + idx % P;
                v[u] = fb[(size_t)min(e, E - 1) * HW + min(p, HW - 1)];
                if (e >= E || p >= HW) v[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + u * kDcThreads + (int)threadIdx.x;
                if (idx < total) lds[idx] = v[u];
            }
        }
    }
    __syncthreads();
    constexpr int PS = P / 32, CS = 4 / PS;                          // pixel slices of 32; waves that share a slice take every CS-th chunk
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int ps = wave % PS, px = p0 + ps * 32 + r;
    const float* col = lds + ps * 32 + r;
    const int chunks = (nb + 31) / 32;
    for (int c = wave / PS; c < chunks; c += CS) {
        int lev;
        const int row = locate(t, b, c * 32 + r, lev);
        // record q of this lane: A[r][k = half] of the k steps e = 8 q + {0, 2, 4, 6} + half.  The records of the next kAhead groups of
        // eight e are loaded before the current ones are used: a load is an L2 round trip, four MFMA are 256 cycles
        const float4* ka = reinterpret_cast<const float4*>(kT + (size_t)(t.chunk0[b] + c) * E8 * 32) + half * 32 + r;
        const int nq = E8 / 8;
        f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        auto steps = [&](const float4& v, int q) {
            const float* f = col + (8 * q + half) * P;
            acc = mfma32(v.x, f[0], acc);
            acc = mfma32(v.y, f[2 * P], acc);
            acc = mfma32(v.z, f[4 * P], acc);
            acc = mfma32(v.w, f[6 * P], acc);
        };
        constexpr int kAhead = 8;
        int q0 = 0;
        if (nq >= kAhead) {
            float4 cur[kAhead], nxt[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) cur[u] = ka[u * 64];
            for (; q0 + 2 * kAhead <= nq; q0 += kAhead) {
#pragma unroll
                for (int u = 0; u < kAhead; ++u) nxt[u] = ka[(q0 + kAhead + u) * 64];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) steps(cur[u], q0 + u);
#pragma unroll
                for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) steps(cur[u], q0 + u);
            q0 += kAhead;
        }
        for (; q0 < nq; ++q0) steps(ka[q0 * 64], q0);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int orow = __shfl(row, acc_row(reg, half));
            if (orow >= 0 && px < HW) {
                float v = acc[reg];
                if (act) v = 1.f / (1.f + expf(-v));
                out[(size_t)orow * HW + px] = v;
            }
        }
        if (img_inds && tile == 0 && ps == 0 && half == 0 && row >= 0) img_inds[row] = b;
    }
}

__global__ void __launch_bounds__(kDcThreads) dconv_bwd_kernel(const DconvTable t, const float* __restrict__ feat, const float* __restrict__ kT,
                                                               const float* __restrict__ out, const float* __restrict__ gout,
                                                               float* __restrict__ gfeat, float* __restrict__ part, int E, int HW, int tiles, int N,
                                                               int act) {
    constexpr int P = BXI_DCONV_TILE;
    __shared__ float g_lds[64 * kDcStride];                          // [row of the chunk][pixel]
    __shared__ float f_lds[4][32 * kDcStride];                       // per wave: [channel of the block][pixel]
    __shared__ int row_lds[64];
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles, p0 = tile * P;
    const int nb = rows_of_image(t, b);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int eblocks = (E + 31) / 32, chunks = (nb + 63) / 64, E8 = e8_of(E);
    const float* fb = feat + (size_t)b * E * HW;
    for (int eb0 = 0; eb0 < eblocks; eb0 += 4) {                     // the same trip count for every wave: the barriers below are uniform
        const int eb = eb0 + wave;
        const bool active = eb < eblocks;
        const int e_mine = eb * 32 + r;                              // grad_feat: this lane's A row; grad_kernel: its B / C column
        f16v accf[2];
        for (int s = 0; s < 2; ++s) accf[s] = f16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (active && part && nb > 0) {                              // the feature block of this wave, rows of 64 pixels read coalesced
            for (int r0 = 0; r0 < 32; r0 += 8) {                     // eight loads, unconditional on a clamped address, then eight stores
                float fv[8];
                const int p = p0 + lane;
#pragma unroll
                for (int u = 0; u < 8; ++u) fv[u] = fb[(size_t)min(eb * 32 + r0 + u, E - 1) * HW + min(p, HW - 1)];
#pragma unroll
                for (int u = 0; u < 8; ++u) f_lds[wave][(r0 + u) * kDcStride + lane] = (eb * 32 + r0 + u < E && p < HW) ? fv[u] : 0.f;
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
                    gl[u] = gout[at];
                    pl[u] = act ? out[at] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int idx = u * kDcThreads + (int)threadIdx.x, il = idx / P, p = idx % P;
                    const float g = act ? gl[u] * pl[u] * (1.f - pl[u]) : gl[u];
                    g_lds[il * kDcStride + p] = (row_lds[il] >= 0 && p0 + p < HW) ? g : 0.f;
                }
            }
            __syncthreads();
            if (!active) continue;
            const int cnt = nb - ic * 64 < 64 ? nb - ic * 64 : 64;
            if (gfeat) {
                // kT holds zeros for a missing row and for a cell outside its map (nothing for grad_feat; that row's grad_kernel sums reach
                // no cell).  All of the chunk's values of this lane's channel are asked for before the first product waits for one.
                const int ec = e_mine < E ? e_mine : 0;
                float a[32];
#pragma unroll
                for (int st = 0; st < 32; ++st) {
                    const int i = 2 * st + half;
                    a[st] = (2 * st < cnt && e_mine < E) ? kT[kt_at(E8, t.chunk0[b] + 2 * ic + (i >> 5), ec, i & 31)] : 0.f;
                }
#pragma unroll
                for (int st = 0; st < 32; ++st) {
                    if (2 * st < cnt) {
                        const int i = 2 * st + half;
                        accf[0] = mfma32(a[st], g_lds[i * kDcStride + r], accf[0]);
                        accf[1] = mfma32(a[st], g_lds[i * kDcStride + 32 + r], accf[1]);
                    }
                }
            }
            if (part) {
                for (int sub = 0; sub * 32 < cnt; ++sub) {
                    f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    const float* ga = g_lds + (sub * 32 + r) * kDcStride;
                    const float* fbk = f_lds[wave] + r * kDcStride;
#pragma unroll 4
                    for (int q0 = 0; q0 < P; q0 += 2) acc = mfma32(ga[q0 + half], fbk[q0 + half], acc);
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
                    if (e < E && p < HW) gfeat[((size_t)b * E + e) * HW + p] = accf[s][reg];
                }
            }
        }
    }
}

// the workspace: kT as floats in the layout of kt_at, the backward's tiles of BXI_DCONV_TILE pixels
static size_t dconv32_workspace(int N, int B, int E, int H, int W, bool backward, void* base, DconvSpace<float>* sp) {
    return dconv_workspace<float>(e8_of(E), BXI_DCONV_TILE, N, B, E, H, W, backward, base, sp);
}

}  // namespace bxi

extern "C" size_t bxi_solo_dconv_forward_workspace_bytes(int N, int B, int E) {
    using namespace bxi;
    return dconv_query_ok(N, B, E, 1, 1) ? dconv32_workspace(N, B, E, 1, 1, false, nullptr, nullptr) : 0;
}

extern "C" int bxi_solo_dconv_forward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                                          int layout, const int64_t* cells, const int* seg_counts, int N, int activation, float* out,
                                          int64_t* img_inds, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    DconvTable t;
    int rc = dconv_table(B, E, H, W, kernel_maps, grids, L, layout, seg_counts, N, activation, t);
    if (rc != BXI_OK) return rc;
    if (N == 0) return BXI_OK;
    rc = dconv_forward_args(t, feat, out, status, cells);
    if (rc != BXI_OK) return rc;
    if (!workspace_ok(workspace, workspace_bytes, bxi_solo_dconv_forward_workspace_bytes(N, B, E), 16)) return BXI_ERR_WORKSPACE;
    DconvSpace<float> sp;
    dconv32_workspace(N, B, E, H, W, false, workspace, &sp);
    const int HW = H * W, E8 = e8_of(E);
    const bool wide = E <= 512;                                      // 64 pixels while the tile fits 128 KB of LDS
    const int P = wide ? 64 : 32, tiles = (HW + P - 1) / P;
    const size_t lds = sizeof(float) * (size_t)E8 * P;
    const void* fn = wide ? reinterpret_cast<const void*>(dconv_fwd_kernel<64>) : reinterpret_cast<const void*>(dconv_fwd_kernel<32>);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { set_last_hip_error((int)e); return BXI_ERR_LAUNCH; }
    }
    hipStream_t s = as_stream(stream);
    rc = dconv_gather<float, Kt>("solo_dconv_gather", t, cells, sp, status, E, s);
    if (rc != BXI_OK) return rc;
    const dim3 grid((unsigned)((int64_t)B * tiles));
    const int vec = !(HW & 3) && aligned(feat, 16);
    if (wide) BXI_LAUNCH("solo_dconv_fwd", s, dconv_fwd_kernel<64>, grid, dim3(kDcThreads), lds, s, t, feat, sp.kT, out, img_inds, E, HW, tiles, activation, vec);
    else BXI_LAUNCH("solo_dconv_fwd", s, dconv_fwd_kernel<32>, grid, dim3(kDcThreads), lds, s, t, feat, sp.kT, out, img_inds, E, HW, tiles, activation, vec);
    return check_launch();
}

extern "C" size_t bxi_solo_dconv_backward_workspace_bytes(int N, int B, int E, int H, int W) {
    using namespace bxi;
    return dconv_query_ok(N, B, E, H, W) ? dconv32_workspace(N, B, E, H, W, true, nullptr, nullptr) : 0;
}

extern "C" int bxi_solo_dconv_backward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                                           int layout, const int64_t* cells, const int* seg_counts, int N, int activation, const float* out,
                                           const float* grad_out, float* grad_feat, void* const* grad_kernel_maps, int32_t* status,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    DconvTable t;
    int rc = dconv_table(B, E, H, W, kernel_maps, grids, L, layout, seg_counts, N, activation, t);
    if (rc != BXI_OK) return rc;
    if (!grad_feat && !grad_kernel_maps) return BXI_OK;
    rc = dconv_backward_args(t, N, feat, out, grad_out, status, cells, grad_kernel_maps);
    if (rc != BXI_OK) return rc;
    DconvSpace<float> sp = {nullptr, nullptr, nullptr, 0};
    hipStream_t s = as_stream(stream);
    if (N > 0) {
        if (!workspace_ok(workspace, workspace_bytes, bxi_solo_dconv_backward_workspace_bytes(N, B, E, H, W), 16)) return BXI_ERR_WORKSPACE;
        dconv32_workspace(N, B, E, H, W, true, workspace, &sp);
        rc = dconv_gather<float, Kt>("solo_dconv_gather", t, cells, sp, status, E, s);
        if (rc != BXI_OK) return rc;
    }
    // without gradient maps the feature is not read and the partial sums are not formed
    float* part = grad_kernel_maps ? sp.part : nullptr;
    const int HW = H * W, tiles = (HW + BXI_DCONV_TILE - 1) / BXI_DCONV_TILE;
    BXI_LAUNCH("solo_dconv_bwd", s, dconv_bwd_kernel, dim3((unsigned)((int64_t)B * tiles)), dim3(kDcThreads), 0, s, t, feat, sp.kT, out, grad_out, grad_feat,
               part, E, HW, tiles, N, activation);
    rc = check_launch();
    if (rc != BXI_OK || !grad_kernel_maps) return rc;
    if (part) {
        rc = dconv_reduce("solo_dconv_reduce", part, sp.gk, E, tiles, N, s);
        if (rc != BXI_OK) return rc;
    }
    return dconv_scatter<float, false>("solo_dconv_scatter", t, cells, sp.gk, E, s);
}
