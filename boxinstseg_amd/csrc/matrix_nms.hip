// matrix_nms.hip -- the test-time block the two SOLOv2-style heads of the reference share (box_solov2_head.py:546-574,
// discobox_head.py:1610-1639 -> mask_matrix_nms, matrix_nms.py:5-121) on gfx950, wave64.
//
//   mask_pack_kernel   one workgroup = one candidate, one pass over its h*w probabilities (or mask bytes).  A lane loads four
//                      consecutive pixels (one 16-byte non-temporal load at any dword address; the last partial group by dwords),
//                      the wave's __ballot of component k is word 4g + k of pixel group g (256 pixels): pixel 256 g + 4 l + k is
//                      bit l of that word.  The last, partial group is read word by word instead (pixel 256 g + 64 k + l is bit l
//                      of word 4g + k), so a candidate fills exactly ceil(h*w / 64) words.  The position of a pixel depends on
//                      h*w alone, not on the alignment of the candidate -- so bit positions agree between candidates, which is all
//                      the popcounts below need.  Pixels past h*w never set a bit; every word is written.
//                      area = popcounts of the ballots (integers); psum = four partials per lane (one per component, groups in
//                      ascending order) -> (s0 + s1) + (s2 + s3) -> the DPP wave total -> the eight waves in a fixed tree.
//   nms_iou_kernel     one workgroup = one 32 x 32 tile of (i, j) pairs of the sorted candidates; tiles below the diagonal and
//                      tiles in which no pair i < j shares a label only write their zeros.  32-word chunks of the two row groups
//                      are staged in LDS (row stride 33 words: the 32 columns of a half wave hit 32 different bank pairs, the
//                      rows are broadcasts), a thread owns column tx and rows ty, ty + 8, ty + 16, ty + 24.  Rows are fetched
//                      through `order`.  inter / (area_j + area_i - inter) on the integers converted to fp32 is what the
//                      reference's fp32 matrix product and division give, bit for bit.  Each tile also writes the maximum of each
//                      of its columns (NaN wins, as in torch.max) to part[ti][j].
//   nms_decay_kernel   one workgroup = 64 columns x 8 slices of the rows.  Every workgroup first reduces part[0 .. i/32][i] to
//                      compensate[i] for all i into LDS (a second pass instead of a float atomic: order-independent AND written
//                      by plain stores, <= n * T / 2 L2 reads per workgroup), then min over i < j with equal labels of the ratio,
//                      slices combined in a fixed order.
// No atomics, no allocation, no synchronisation; three launches on the caller's stream.
#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_post.h"

namespace bxi {

constexpr int kPackThreads = 512;                   // 8 waves per candidate
constexpr int kPackWaves = kPackThreads / kWave;
constexpr int kNmsTile = 32;                        // pairs per tile side
constexpr int kNmsChunk = 32;                       // 64-bit words of a row staged per round
constexpr int kNmsStride = kNmsChunk + 1;           // LDS row stride in words
constexpr int kIouThreads = 256;
constexpr int kDecayThreads = 512;                  // 64 columns x 8 row slices
constexpr int kDecaySlices = kDecayThreads / kWave;
constexpr int kMaxPixels = 1 << 24;                 // h*w below this: every count is an exact fp32

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));                    // a float4 at any dword address
typedef unsigned char u8x4 __attribute__((ext_vector_type(4), aligned(1)));          // four bytes at any address

// max as torch.max reduces: a NaN operand wins
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __uint_as_float(0x7fc00000u) : fmaxf(a, b); }

template <bool F32>
__global__ void __launch_bounds__(kPackThreads) mask_pack_kernel(const void* __restrict__ src_, int hw, int nwords, float thr,
                                                                 unsigned long long* __restrict__ bits, int32_t* __restrict__ area,
                                                                 float* __restrict__ psum) {
    __shared__ float red_s[kPackWaves];
    __shared__ int red_n[kPackWaves];
    const int cand = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const size_t base = (size_t)cand * hw;
    const float* pf = reinterpret_cast<const float*>(src_) + base;
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(src_) + base;
    unsigned long long* out = bits + (size_t)cand * nwords;
    const int ngroups = (hw + 255) >> 8;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int g = wave; g < ngroups; g += kPackWaves) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        bool on[4] = {false, false, false, false};
        if ((g << 8) + 256 <= hw) {                  // a whole group: four consecutive pixels per lane
            const int p = (g << 8) + (lane << 2);
            if (F32) {
                const f4u t = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(pf + p));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                const u8x4 t = __builtin_nontemporal_load(reinterpret_cast<const u8x4*>(pb + p));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) on[k] = F32 ? v[k] > thr : v[k] != 0.f;
        } else {                                     // the last, partial group: word by word, so that it fills ceil(rest / 64) words
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = (g << 8) + (k << 6) + lane;
                if (p < hw) {
                    v[k] = F32 ? pf[p] : (float)pb[p];
                    on[k] = F32 ? v[k] > thr : v[k] != 0.f;
                }
            }
        }
        unsigned long long b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = __ballot(on[k]);
            cnt += __popcll(b[k]);
            if (F32) s[k] += on[k] ? v[k] : 0.f;
        }
        const unsigned long long mine = lane == 0 ? b[0] : lane == 1 ? b[1] : lane == 2 ? b[2] : b[3];
        if (lane < 4 && (g << 2) + lane < nwords) out[(g << 2) + lane] = mine;
    }
    float total = 0.f;
    if (F32) total = wave_total_f32((s[0] + s[1]) + (s[2] + s[3]));
    if (lane == 0) { red_s[wave] = total; red_n[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        area[cand] = ((red_n[0] + red_n[1]) + (red_n[2] + red_n[3])) + ((red_n[4] + red_n[5]) + (red_n[6] + red_n[7]));
        if (F32) psum[cand] = ((red_s[0] + red_s[1]) + (red_s[2] + red_s[3])) + ((red_s[4] + red_s[5]) + (red_s[6] + red_s[7]));
    }
}

__global__ void __launch_bounds__(kIouThreads) nms_iou_kernel(const unsigned long long* __restrict__ bits, const int32_t* __restrict__ area,
                                                              const int64_t* __restrict__ labels, const int64_t* __restrict__ order,
                                                              int n_all, int n, int nwords, float* __restrict__ decay_iou,
                                                              float* __restrict__ part) {
    __shared__ unsigned long long rows[2 * kNmsTile * kNmsStride];      // group A (rows i) | group B (columns j)
    __shared__ long long row_of[2 * kNmsTile];                           // candidate index, -1: none
    __shared__ long long lab[2 * kNmsTile];
    __shared__ float ar[2 * kNmsTile];
    __shared__ float colmax[kIouThreads / kNmsTile][kNmsTile];
    __shared__ int tile_wanted;                                          // some pair of the tile has i < j and equal labels
    const int tj = blockIdx.x, ti = blockIdx.y, tid = threadIdx.x;
    const int tx = tid & (kNmsTile - 1), ty = tid / kNmsTile;
    const int j = tj * kNmsTile + tx;
    if (ti > tj) {                                   // below the diagonal: zeros
        if (j < n)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = ti * kNmsTile + ty + 8 * k;
                if (i < n) decay_iou[(size_t)i * n + j] = 0.f;
            }
        if (ty == 0 && j < n) part[(size_t)ti * n + j] = 0.f;      // (never read: the workspace is written in full)
        return;
    }
    if (tid < 2 * kNmsTile) {
        const int pos = (tid < kNmsTile ? ti : tj) * kNmsTile + (tid & (kNmsTile - 1));
        long long r = -1, l = 0;
        float a = 0.f;
        if (pos < n) {
            const long long o = order[pos];
            if (o >= 0 && o < n_all) { r = o; a = (float)area[o]; l = labels[o]; }
            else l = -1 - (long long)pos;            // an index outside the candidates: an empty mask of a label of its own
        }
        row_of[tid] = r; lab[tid] = l; ar[tid] = a;
    }
    if (tid == 0) tile_wanted = 0;
    __syncthreads();
    bool want[4];
    int any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = ti * kNmsTile + ty + 8 * k;
        want[k] = i < j && j < n && lab[ty + 8 * k] == lab[kNmsTile + tx];
        any |= want[k] ? 1 : 0;
    }
    if (any) tile_wanted = 1;                        // (every writer stores the same value)
    __syncthreads();
    int acc[4] = {0, 0, 0, 0};
    if (tile_wanted) {
        for (int w0 = 0; w0 < nwords; w0 += kNmsChunk) {
            const int cw = nwords - w0 < kNmsChunk ? nwords - w0 : kNmsChunk;
#pragma unroll
            for (int q = 0; q < 2 * kNmsTile * kNmsChunk / kIouThreads; ++q) {
                const int idx = tid + q * kIouThreads;
                const int r = idx / kNmsChunk, wd = idx % kNmsChunk;
                const long long src = row_of[r];
                rows[r * kNmsStride + wd] = (src >= 0 && wd < cw) ? bits[(size_t)src * nwords + w0 + wd] : 0ull;
            }
            __syncthreads();
            const unsigned long long* A = rows + ty * kNmsStride;
            const unsigned long long* B = rows + (kNmsTile + tx) * kNmsStride;
            for (int wd = 0; wd < cw; ++wd) {
                const unsigned long long b = B[wd];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += __popcll(A[8 * k * kNmsStride + wd] & b);
            }
            __syncthreads();
        }
    }
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = ti * kNmsTile + ty + 8 * k;
        float v = 0.f;
        if (want[k]) {
            const float inter = (float)acc[k];
            v = inter / ((ar[kNmsTile + tx] + ar[ty + 8 * k]) - inter);
        }
        if (i < n && j < n) decay_iou[(size_t)i * n + j] = v;
        m = nan_max(m, v);
    }
    colmax[ty][tx] = m;
    __syncthreads();
    if (ty == 0 && j < n) {
#pragma unroll
        for (int q = 1; q < kIouThreads / kNmsTile; ++q) m = nan_max(m, colmax[q][tx]);
        part[(size_t)ti * n + j] = m;
    }
}

__global__ void __launch_bounds__(kDecayThreads) nms_decay_kernel(const float* __restrict__ decay_iou, const float* __restrict__ part,
                                                                  const int64_t* __restrict__ labels, const int64_t* __restrict__ order,
                                                                  const float* __restrict__ scores, int n_all, int n, int linear,
                                                                  float sigma, float* __restrict__ compensate, float* __restrict__ decayed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
    long long* lab = reinterpret_cast<long long*>(nms_lds);              // [n]
    float* den = reinterpret_cast<float*>(lab + n);                      // [n]  exp(-sigma c_i^2)  or  1 - c_i
    __shared__ float red_min[kDecaySlices][kWave];
    __shared__ int red_nan[kDecaySlices][kWave];
    __shared__ int any_nan;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), slice = tid / kWave;
    if (tid == 0) any_nan = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kDecayThreads) {
        float c = 0.f;
        for (int t = 0; t <= i / kNmsTile; ++t) c = nan_max(c, part[(size_t)t * n + i]);
        if (c != c) any_nan = 1;
        den[i] = linear ? 1.f - c : expf(-sigma * (c * c));
        const long long o = order[i];
        lab[i] = (o >= 0 && o < n_all) ? labels[o] : -1 - (long long)i;
        if (blockIdx.x == 0) compensate[i] = c;
    }
    __syncthreads();
    const int j = blockIdx.x * kWave + lane;
    const int jend = min(n, (int)(blockIdx.x + 1) * kWave);              // rows below the workgroup's last column
    float mn = 1.f;
    int bad = 0;
    if (j < n) {
        const long long lj = lab[j];
        for (int i = slice; i < jend - 1; i += kDecaySlices) {
            if (i < j && lab[i] == lj) {
                const float d = decay_iou[(size_t)i * n + j];
                const float r = linear ? (1.f - d) / den[i] : expf(-sigma * (d * d)) / den[i];
                if (r != r) bad = 1;
                else mn = fminf(mn, r);
            }
        }
    }
    red_min[slice][lane] = mn;
    red_nan[slice][lane] = bad;
    __syncthreads();
    if (slice == 0 && j < n) {
        bad |= any_nan;
#pragma unroll
        for (int q = 1; q < kDecaySlices; ++q) { mn = fminf(mn, red_min[q][lane]); bad |= red_nan[q][lane]; }
        decayed[j] = scores[j] * (bad ? __uint_as_float(0x7fc00000u) : mn);
    }
}

inline int nms_tiles(int n) { return (n + kNmsTile - 1) / kNmsTile; }

template <bool F32>
int launch_pack(const void* src, int n_all, int h, int w, float thr, uint64_t* bits, int32_t* area, float* psum, void* stream) {
    if (n_all < 0 || h < 1 || w < 1 || (int64_t)h * w >= kMaxPixels) return BXI_ERR_BAD_SHAPE;
    if (n_all == 0) return BXI_OK;
    if (!src || !bits || !area || (F32 && !psum)) return BXI_ERR_NULL_POINTER;
    const int hw = h * w, nwords = (hw + 63) / 64;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH(F32 ? "mask_pack_f32" : "mask_pack_u8", s, mask_pack_kernel<F32>, dim3((unsigned)n_all), dim3(kPackThreads), 0, s, src, hw,
               nwords, thr, reinterpret_cast<unsigned long long*>(bits), area, psum);
    return check_launch();
}

}  // namespace bxi

extern "C" int bxi_mask_pack_f32(const float* probs, int n_all, int h, int w, float mask_thr, uint64_t* bits, int32_t* area,
                                 float* psum, void* stream) {
    return bxi::launch_pack<true>(probs, n_all, h, w, mask_thr, bits, area, psum, stream);
}

extern "C" int bxi_mask_pack_u8(const uint8_t* masks, int n_all, int h, int w, uint64_t* bits, int32_t* area, void* stream) {
    return bxi::launch_pack<false>(masks, n_all, h, w, 0.f, bits, area, nullptr, stream);
}

extern "C" size_t bxi_matrix_nms_workspace_bytes(int n) {
    if (n < 1 || n > BXI_NMS_MAX_CANDIDATES) return 0;
    return sizeof(float) * (size_t)n * (size_t)(1 + bxi::nms_tiles(n));
}

extern "C" int bxi_matrix_nms_f32(const uint64_t* bits, const int32_t* area, const int64_t* labels, const int64_t* order,
                                  const float* scores_sorted, int n_all, int n, int h, int w, int kernel, float sigma, float* decayed,
                                  float* decay_iou, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (n_all < 1 || h < 1 || w < 1 || (int64_t)h * w >= kMaxPixels) return BXI_ERR_BAD_SHAPE;
    if (n < 1 || n > BXI_NMS_MAX_CANDIDATES) return BXI_ERR_UNSUPPORTED;
    if ((kernel != BXI_NMS_KERNEL_GAUSSIAN && kernel != BXI_NMS_KERNEL_LINEAR) || !(sigma == sigma)) return BXI_ERR_BAD_ARGUMENT;
    if (!bits || !area || !labels || !order || !scores_sorted || !decayed || !decay_iou) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_matrix_nms_workspace_bytes(n), 4)) return BXI_ERR_WORKSPACE;
    const int nwords = (h * w + 63) / 64, T = nms_tiles(n);
    float* compensate = reinterpret_cast<float*>(workspace);
    float* part = compensate + n;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("nms_iou", s, nms_iou_kernel, dim3((unsigned)T, (unsigned)T), dim3(kIouThreads), 0, s,
               reinterpret_cast<const unsigned long long*>(bits), area, labels, order, n_all, n, nwords, decay_iou, part);
    const size_t lds = (sizeof(long long) + sizeof(float)) * (size_t)n;
    BXI_LAUNCH("nms_decay", s, nms_decay_kernel, dim3((unsigned)((n + kWave - 1) / kWave)), dim3(kDecayThreads), lds, s, decay_iou, part,
               labels, order, scores_sorted, n_all, n, kernel == BXI_NMS_KERNEL_LINEAR ? 1 : 0, sigma, compensate, decayed);
    return check_launch();
}
