// box_nms.hip -- CondInst's test-time detections (include/boxinst/boxinst_hip_det.h): location scores, candidate decode and
// filter, greedy box NMS, and the gather of the kept detections.  gfx950 only.
//
//   det_location_score_kernel   one thread per (image, location): max over the class logits, two sigmoids, one product.
//   det_candidates_kernel<W>    64 rows of `sel` per workgroup, four threads per row (a quarter of the classes each, in class
//                               order).  W = false counts the tile's candidates into the workspace; W = true sums the counts of the
//                               tiles before it, scans its own threads and writes the candidates in (row, class) order.  Nothing
//                               waits for another workgroup: the two passes are two launches.
//   box_sort_kernel             one workgroup per segment: bitonic sort of (score key, ~index) 64-bit keys in 128 KiB of LDS.
//   box_nms_kernel              one workgroup (4 waves) per segment.  The kept list lives in LDS (BXI_DET_KEEP_TILE boxes; beyond that
//                               in the workspace).  A round takes the next 256 candidates in sorted order: every lane tests its
//                               candidate against the kept list (all lanes read the same kept box: an LDS broadcast), then the four
//                               chunks of 64 resolve in order -- against what the earlier chunks of the round added, then among
//                               themselves with one __ballot per surviving candidate.  Every loop is bounded by count / max_keep.
//   det_gather_kernel           one thread per (image, kept slot, column): params from the NCHW maps, boxes and scores from the
//                               candidates, points from the location index.
#include <math.h>

#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_det.h"

namespace bxi {
namespace {

constexpr int kSortThreads = 1024;
constexpr int kNmsThreads = BXI_DET_NMS_ROUND;
constexpr int kNmsWaves = kNmsThreads / kWave;
constexpr int kRowTile = BXI_DET_ROW_TILE;
constexpr int kCandThreads = 4 * kRowTile;
constexpr int kSpillWords = 6;

struct DetLevels {
    const float* cls[BXI_DET_MAX_LEVELS];
    const float* bbox[BXI_DET_MAX_LEVELS];
    const float* ctr[BXI_DET_MAX_LEVELS];
    const float* params[BXI_DET_MAX_LEVELS];
    int H[BXI_DET_MAX_LEVELS], W[BXI_DET_MAX_LEVELS], stride[BXI_DET_MAX_LEVELS];
    int first[BXI_DET_MAX_LEVELS + 1];   // first[l] = locations of the levels before l; first[n] = M_all
    int n;
};
struct ImgDims { float v[BXI_MAX_IMAGES][6]; };

// 1 / (1 + exp(-x)), ATen's formula; the division is correctly rounded.
__device__ __forceinline__ float sigmoidf_(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))); }

// level of a location and its offset inside the level's H*W plane
__device__ __forceinline__ int level_of(const DetLevels& lv, int loc, int& yx) {
    int l = 0;
    while (l + 1 < lv.n && loc >= lv.first[l + 1]) ++l;
    yx = loc - lv.first[l];
    return l;
}

__global__ __launch_bounds__(256) void det_location_score_kernel(DetLevels lv, int C, float* __restrict__ loc_score) {
    const int m_all = lv.first[lv.n];
    const int loc = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (loc >= m_all) return;
    int yx;
    const int l = level_of(lv, loc, yx);
    const size_t hw = (size_t)lv.H[l] * lv.W[l];
    const float* p = lv.cls[l] + (size_t)b * C * hw + yx;
    float mx = p[0];
    for (int c = 1; c < C; ++c) {
        const float v = p[(size_t)c * hw];
        mx = (v > mx || v != v) ? v : mx;
    }
    const float ctr = lv.ctr[l][(size_t)b * hw + yx];
    loc_score[(size_t)b * m_all + loc] = __fmul_rn(sigmoidf_(mx), sigmoidf_(ctr));
}

template <bool WRITE>
__global__ __launch_bounds__(kCandThreads) void det_candidates_kernel(DetLevels lv, ImgDims dims, int C, const int64_t* __restrict__ sel,
                                                                      int M, int rescale, float thr, int cap, float* __restrict__ boxes,
                                                                      float* __restrict__ scores, int64_t* __restrict__ labels,
                                                                      int32_t* __restrict__ pos, int32_t* __restrict__ count,
                                                                      int32_t* __restrict__ tile_counts) {
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int tile = blockIdx.x, tiles = gridDim.x, b = blockIdx.y;
    const int tid = threadIdx.x, r = tid >> 2, q = tid & 3;
    const int m_all = lv.first[lv.n];
    const int m = tile * kRowTile + r;
    const int cq = (C + 3) >> 2;
    const int c0 = min(C, q * cq), c1 = min(C, c0 + cq);
    bool row_ok = m < M;
    int loc = 0;
    if (row_ok) {
        const int64_t s = sel ? sel[(size_t)b * M + m] : (int64_t)m;
        row_ok = s >= 0 && s < m_all;
        loc = row_ok ? (int)s : 0;
    }
    int yx = 0, l = 0;
    size_t hw = 1;
    const float* p = nullptr;
    if (row_ok) {
        l = level_of(lv, loc, yx);
        hw = (size_t)lv.H[l] * lv.W[l];
        p = lv.cls[l] + (size_t)b * C * hw + yx;
    }
    int n = 0;
    if (row_ok)
        for (int c = c0; c < c1; ++c) n += sigmoidf_(p[(size_t)c * hw]) > thr ? 1 : 0;

    if (!WRITE) {
        n = wave_total_i32(n);
        if ((tid & 63) == 0) s_wave[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) tile_counts[(size_t)b * tiles + tile] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        return;
    }

    // candidates of the tiles before this one
    int part = 0;
    for (int t = tid; t < tile; t += kCandThreads) part += tile_counts[(size_t)b * tiles + t];
    part = wave_total_i32(part);
    if ((tid & 63) == 0) s_wave[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) s_base = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
    const int base = s_base;
    int total;
    int slot = base + block_scan_excl_i32<kCandThreads / 64>(n, s_wave, total);
    if (tile == tiles - 1 && tid == 0) count[b] = base + total;
    if (n == 0) return;
    if (slot >= cap) return;

    // the row's box (transforms.py:153-184, condinst_head.py:808-810)
    const float st = (float)lv.stride[l];
    const int y = yx / lv.W[l], x = yx - y * lv.W[l];
    const float px = __fmul_rn((float)x + 0.5f, st), py = __fmul_rn((float)y + 0.5f, st);
    const float* d = lv.bbox[l] + (size_t)b * 4 * hw + yx;
    float bx[4] = {__fsub_rn(px, d[0]), __fsub_rn(py, d[hw]), __fadd_rn(px, d[2 * hw]), __fadd_rn(py, d[3 * hw])};
    const float* dim = dims.v[b];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float mx = (k & 1) ? dim[0] : dim[1];
        float v = bx[k];
        v = v < 0.f ? 0.f : v;
        v = v > mx ? mx : v;
        if (rescale) v = __fdiv_rn(v, dim[2 + k]);
        bx[k] = v;
    }
    const float sc = sigmoidf_(lv.ctr[l][(size_t)b * hw + yx]);
    for (int c = c0; c < c1; ++c) {
        const float s = sigmoidf_(p[(size_t)c * hw]);
        if (s > thr) {
            if (slot >= cap) return;
            const size_t o = (size_t)b * cap + slot;
            boxes[4 * o + 0] = bx[0];
            boxes[4 * o + 1] = bx[1];
            boxes[4 * o + 2] = bx[2];
            boxes[4 * o + 3] = bx[3];
            scores[o] = __fmul_rn(s, sc);
            labels[o] = c;
            pos[o] = m;
            ++slot;
        }
    }
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
// larger key = earlier: NaN first, then descending score (-0 == +0), then ascending index
__device__ __forceinline__ unsigned long long sort_key(float s, uint32_t idx) {
    uint32_t hi;
    if (s != s) hi = 0xffffffffu;
    else hi = float_key(s == 0.f ? 0.f : s);
    return ((unsigned long long)hi << 32) | (unsigned long long)(0xffffffffu - idx);
}

__global__ __launch_bounds__(kSortThreads) void box_sort_kernel(const float* __restrict__ scores, const int32_t* __restrict__ count,
                                                                int cap, int32_t* __restrict__ order) {
    __shared__ unsigned long long keys[BXI_DET_SORT_MAX];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int cnt = count[p];
    if (cnt <= 0 || cnt > cap || cnt > BXI_DET_SORT_MAX) return;       // box_nms_kernel reports it
    int n2 = 2;
    while (n2 < cnt) n2 <<= 1;                                         // <= BXI_DET_SORT_MAX, a power of two
    const float* s = scores + (size_t)p * cap;
    for (int i = tid; i < n2; i += kSortThreads) keys[i] = i < cnt ? sort_key(s[i], (uint32_t)i) : 0ull;   // 0 sorts behind every real key
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += kSortThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool desc = (i & k) == 0;
                const unsigned long long a = keys[i], bb = keys[i + j];
                if ((a < bb) == desc && a != bb) {
                    keys[i] = bb;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    int32_t* o = order + (size_t)p * cap;
    for (int i = tid; i < cnt; i += kSortThreads) o[i] = (int32_t)(0xffffffffu - (uint32_t)keys[i]);
}

// ---- greedy NMS -----------------------------------------------------------------------------------------------------------
struct Box { float x1, y1, x2, y2; };

// does the kept box k suppress a?  single fp32 operations, no contraction
__device__ __forceinline__ bool suppresses(const Box& a, const Box& k, float thr, float off) {
    const float w = fmaxf(__fadd_rn(__fsub_rn(fminf(a.x2, k.x2), fmaxf(a.x1, k.x1)), off), 0.f);
    const float h = fmaxf(__fadd_rn(__fsub_rn(fminf(a.y2, k.y2), fmaxf(a.y1, k.y1)), off), 0.f);
    const float inter = __fmul_rn(w, h);
    const float sa = __fmul_rn(__fadd_rn(__fsub_rn(a.x2, a.x1), off), __fadd_rn(__fsub_rn(a.y2, a.y1), off));
    const float sb = __fmul_rn(__fadd_rn(__fsub_rn(k.x2, k.x1), off), __fadd_rn(__fsub_rn(k.y2, k.y1), off));
    return inter > __fmul_rn(thr, __fsub_rn(__fadd_rn(sa, sb), inter));
}

__global__ __launch_bounds__(kNmsThreads) void box_nms_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ labels,
                                                              const int32_t* __restrict__ count, const int32_t* __restrict__ order,
                                                              int own_sort, int cap, float thr, float off, int max_keep,
                                                              int32_t* __restrict__ keep, int32_t* __restrict__ n_keep,
                                                              int32_t* __restrict__ status, int32_t* spill, int spill_n) {
    __shared__ float kx1[BXI_DET_KEEP_TILE], ky1[BXI_DET_KEEP_TILE], kx2[BXI_DET_KEEP_TILE], ky2[BXI_DET_KEEP_TILE];
    __shared__ long long klab[BXI_DET_KEEP_TILE];
    __shared__ float cx1[kNmsThreads], cy1[kNmsThreads], cx2[kNmsThreads], cy2[kNmsThreads];
    __shared__ long long clab[kNmsThreads];
    __shared__ int s_nk, s_bad;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = count[p];
    int32_t* kp = keep + (size_t)p * max_keep;
    int st = 0;
    if (cnt < 0 || cnt > cap) st = BXI_DET_STATUS_OVER_CAP;
    else if (own_sort && cnt > BXI_DET_SORT_MAX) st = BXI_DET_STATUS_OVER_SORT;
    if (st) {
        if (tid == 0) {
            status[p] = st;
            n_keep[p] = -1;
        }
        for (int i = tid; i < max_keep; i += kNmsThreads) kp[i] = -1;
        return;
    }
    if (tid == 0) {
        s_nk = 0;
        s_bad = 0;
    }
    __syncthreads();
    const float* bp = boxes + (size_t)p * cap * 4;
    const int64_t* lp = labels ? labels + (size_t)p * cap : nullptr;
    const int32_t* op = order + (size_t)p * cap;
    int32_t* sp = spill ? spill + (size_t)p * spill_n * kSpillWords : nullptr;

    auto kept_box = [&](int k, Box& kb, long long& kl) {
        if (k < BXI_DET_KEEP_TILE) {
            kb = Box{kx1[k], ky1[k], kx2[k], ky2[k]};
            kl = klab[k];
        } else {     // written by this workgroup earlier in the launch: read past the CU's vector cache
            const int32_t* e = sp + (size_t)(k - BXI_DET_KEEP_TILE) * kSpillWords;
            int v[kSpillWords];
#pragma unroll
            for (int j = 0; j < kSpillWords; ++j) v[j] = __hip_atomic_load(e + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            kb = Box{__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3])};
            kl = (long long)(((unsigned long long)(unsigned int)v[5] << 32) | (unsigned int)v[4]);
        }
    };

    int nk = 0;
    for (int base = 0; base < cnt && nk < max_keep; base += kNmsThreads) {
        const int i = base + tid;
        int idx = -1;
        if (i < cnt) {
            idx = op[i];
            if ((unsigned)idx >= (unsigned)cnt) {
                idx = -1;
                s_bad = 1;
            }
        }
        bool alive = idx >= 0;
        Box a{0.f, 0.f, 0.f, 0.f};
        long long lab = 0;
        if (alive) {
            const float* q = bp + (size_t)idx * 4;
            a = Box{q[0], q[1], q[2], q[3]};
            lab = lp ? (long long)lp[idx] : 0;
        }
        cx1[tid] = a.x1;
        cy1[tid] = a.y1;
        cx2[tid] = a.x2;
        cy2[tid] = a.y2;
        clab[tid] = lab;
        // against everything kept in earlier rounds
        for (int k = 0; k < nk; ++k) {
            if (__ballot(alive) == 0ull) break;
            Box kb;
            long long kl;
            kept_box(k, kb, kl);
            if (alive && kl == lab && suppresses(a, kb, thr, off)) alive = false;
        }
        __syncthreads();
        // the four chunks of the round, in order
        for (int w = 0; w < kNmsWaves; ++w) {
            if (wave == w) {
                const int nkc = s_nk;
                for (int k = nk; k < nkc; ++k) {       // what the earlier chunks of this round added
                    if (__ballot(alive) == 0ull) break;
                    Box kb;
                    long long kl;
                    kept_box(k, kb, kl);
                    if (alive && kl == lab && suppresses(a, kb, thr, off)) alive = false;
                }
                unsigned long long rem = __ballot(alive), kept_mask = 0ull;
                int added = 0;
                while (rem != 0ull && nkc + added < max_keep) {
                    const int j = __ffsll((long long)rem) - 1;      // the best candidate of the chunk nobody has suppressed: kept
                    rem &= rem - 1ull;
                    kept_mask |= 1ull << j;
                    ++added;
                    const int cj = w * kWave + j;
                    const Box jb{cx1[cj], cy1[cj], cx2[cj], cy2[cj]};
                    const bool sup = lane > j && alive && clab[cj] == lab && suppresses(a, jb, thr, off);
                    rem &= ~__ballot(sup);
                }
                if ((kept_mask >> lane) & 1ull) {
                    const int slot = nkc + __popcll(kept_mask & ((1ull << lane) - 1ull));
                    if (slot < BXI_DET_KEEP_TILE) {
                        kx1[slot] = a.x1;
                        ky1[slot] = a.y1;
                        kx2[slot] = a.x2;
                        ky2[slot] = a.y2;
                        klab[slot] = lab;
                    } else {
                        int32_t* e = sp + (size_t)(slot - BXI_DET_KEEP_TILE) * kSpillWords;
                        e[0] = __float_as_int(a.x1);
                        e[1] = __float_as_int(a.y1);
                        e[2] = __float_as_int(a.x2);
                        e[3] = __float_as_int(a.y2);
                        e[4] = (int)(unsigned int)(unsigned long long)lab;
                        e[5] = (int)(unsigned int)((unsigned long long)lab >> 32);
                    }
                    kp[slot] = idx;
                }
                if (lane == 0) s_nk = nkc + added;
            }
            if (spill_n > 0) __threadfence();
            __syncthreads();
        }
        nk = s_nk;
    }
    for (int i = nk + tid; i < max_keep; i += kNmsThreads) kp[i] = -1;
    if (tid == 0) {
        n_keep[p] = nk;
        status[p] = s_bad ? BXI_DET_STATUS_BAD_ORDER : 0;
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void det_gather_kernel(DetLevels lv, int C, int n_params, const int64_t* __restrict__ sel, int M,
                                                         const float* __restrict__ cboxes, const float* __restrict__ cscores,
                                                         const int64_t* __restrict__ clabels, const int32_t* __restrict__ cpos, int cap,
                                                         const int32_t* __restrict__ keep, const int32_t* __restrict__ n_keep, int max_keep,
                                                         float* __restrict__ dets, int64_t* __restrict__ det_labels,
                                                         float* __restrict__ det_params, float* __restrict__ det_coors,
                                                         int64_t* __restrict__ det_level_inds) {
    const int cols = n_params + 1;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)max_keep * cols) return;
    const int slot = (int)(e / cols), col = (int)(e - (long long)slot * cols);
    const int m_all = lv.first[lv.n];
    const size_t o = (size_t)b * max_keep + slot;
    bool ok = slot < n_keep[b];
    int idx = 0, loc = 0, m = 0;
    if (ok) {
        idx = keep[o];
        ok = idx >= 0 && idx < cap;
    }
    if (ok) {
        m = cpos[(size_t)b * cap + idx];
        ok = sel ? (m >= 0 && m < M) : (m >= 0 && m < m_all);
    }
    if (ok) {
        const int64_t s = sel ? sel[(size_t)b * M + m] : (int64_t)m;
        ok = s >= 0 && s < m_all;
        loc = ok ? (int)s : 0;
    }
    int yx = 0, l = 0;
    if (ok) l = level_of(lv, loc, yx);
    if (col < n_params) {
        float v = 0.f;
        if (ok) {
            const size_t hw = (size_t)lv.H[l] * lv.W[l];
            v = lv.params[l][((size_t)b * n_params + col) * hw + yx];
        }
        det_params[o * n_params + col] = v;
        return;
    }
    float d[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, px = 0.f, py = 0.f;
    int64_t lab = 0, lvl = 0;
    if (ok) {
        const size_t c = (size_t)b * cap + idx;
        d[0] = cboxes[4 * c + 0];
        d[1] = cboxes[4 * c + 1];
        d[2] = cboxes[4 * c + 2];
        d[3] = cboxes[4 * c + 3];
        d[4] = cscores[c];
        lab = clabels[c];
        lvl = l;
        const float st = (float)lv.stride[l];
        const int y = yx / lv.W[l], x = yx - y * lv.W[l];
        px = __fmul_rn((float)x + 0.5f, st);
        py = __fmul_rn((float)y + 0.5f, st);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) dets[5 * o + k] = d[k];
    det_labels[o] = lab;
    det_coors[2 * o + 0] = px;
    det_coors[2 * o + 1] = py;
    det_level_inds[o] = lvl;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int make_levels(const bxi_det_level* levels, int n_levels, int B, int C, bool need_params, DetLevels& lv) {
    if (n_levels < 1 || n_levels > BXI_DET_MAX_LEVELS || B < 0 || B > BXI_MAX_IMAGES || C < 1) return BXI_ERR_BAD_SHAPE;
    if (!levels) return BXI_ERR_NULL_POINTER;
    lv.n = n_levels;
    int64_t at = 0;
    for (int l = 0; l < BXI_DET_MAX_LEVELS; ++l) {
        if (l < n_levels) {
            const bxi_det_level& s = levels[l];
            if (s.H < 1 || s.W < 1 || s.stride < 1) return BXI_ERR_BAD_SHAPE;
            if (B > 0 && (!s.cls || !s.bbox || !s.ctr || (need_params && !s.params))) return BXI_ERR_NULL_POINTER;
            lv.cls[l] = s.cls; lv.bbox[l] = s.bbox; lv.ctr[l] = s.ctr; lv.params[l] = s.params;
            lv.H[l] = s.H; lv.W[l] = s.W; lv.stride[l] = s.stride;
            lv.first[l] = (int)at;
            at += (int64_t)s.H * s.W;
            if (!fits_i32(at * C)) return BXI_ERR_BAD_SHAPE;
        } else {
            lv.cls[l] = lv.bbox[l] = lv.ctr[l] = lv.params[l] = nullptr;
            lv.H[l] = lv.W[l] = lv.stride[l] = 1;
            lv.first[l] = (int)at;
        }
    }
    lv.first[BXI_DET_MAX_LEVELS] = (int)at;
    for (int l = n_levels; l <= BXI_DET_MAX_LEVELS; ++l) lv.first[l] = (int)at;
    return BXI_OK;
}

inline int row_tiles(int M) { return M < 1 ? 1 : (M + kRowTile - 1) / kRowTile; }

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" int bxi_det_location_score_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, float* loc_score, void* stream) {
    DetLevels lv;
    if (int rc = make_levels(levels_host, n_levels, B, C, false, lv)) return rc;
    if (B == 0) return BXI_OK;
    if (!loc_score) return BXI_ERR_NULL_POINTER;
    const int m_all = lv.first[lv.n];
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("det_location_score", s, det_location_score_kernel, dim3((unsigned)((m_all + 255) / 256), (unsigned)B), dim3(256), 0, s, lv, C,
               loc_score);
    return check_launch();
}

extern "C" size_t bxi_det_candidates_workspace_bytes(int B, int M) {
    if (B < 1 || B > BXI_MAX_IMAGES || M < 0) return 0;
    return sizeof(int32_t) * (size_t)B * (size_t)row_tiles(M);
}

extern "C" int bxi_det_candidates_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, const int64_t* sel, int M,
                                      const float* img_dims_host, int rescale, float score_thr, int cap, float* cand_boxes,
                                      float* cand_scores, int64_t* cand_labels, int32_t* cand_pos, int32_t* count, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    DetLevels lv;
    if (int rc = make_levels(levels_host, n_levels, B, C, false, lv)) return rc;
    if (B == 0) return BXI_OK;
    if (!sel) M = lv.first[lv.n];
    if (M < 0 || cap < 0 || !fits_i32((int64_t)M * C) || !fits_i32((int64_t)B * cap * 4)) return BXI_ERR_BAD_SHAPE;
    if (!(score_thr == score_thr)) return BXI_ERR_BAD_ARGUMENT;
    if (!img_dims_host || !count || (cap > 0 && (!cand_boxes || !cand_scores || !cand_labels || !cand_pos))) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_det_candidates_workspace_bytes(B, M), 4))
        return BXI_ERR_WORKSPACE;
    ImgDims dims;
    for (int b = 0; b < BXI_MAX_IMAGES; ++b)
        for (int k = 0; k < 6; ++k) dims.v[b][k] = b < B ? img_dims_host[b * 6 + k] : 1.f;
    hipStream_t s = as_stream(stream);
    int32_t* tiles = static_cast<int32_t*>(workspace);
    const dim3 grid((unsigned)row_tiles(M), (unsigned)B);
    BXI_LAUNCH("det_candidates_count", s, det_candidates_kernel<false>, grid, dim3(kCandThreads), 0, s, lv, dims, C, sel, M, rescale ? 1 : 0,
               score_thr, cap, cand_boxes, cand_scores, cand_labels, cand_pos, count, tiles);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("det_candidates_write", s, det_candidates_kernel<true>, grid, dim3(kCandThreads), 0, s, lv, dims, C, sel, M, rescale ? 1 : 0,
               score_thr, cap, cand_boxes, cand_scores, cand_labels, cand_pos, count, tiles);
    return check_launch();
}

static bool nms_shape_ok(int P, int cap, int max_keep) {
    return P >= 1 && P <= 65535 && cap >= 1 && max_keep >= 1 && fits_i32((int64_t)P * cap * 4) && fits_i32((int64_t)P * max_keep);
}

// kept boxes that do not fit in LDS: a segment keeps at most min(max_keep, cap)
static int nms_spill_rows(int cap, int max_keep) {
    const int most = max_keep < cap ? max_keep : cap;
    return most > BXI_DET_KEEP_TILE ? most - BXI_DET_KEEP_TILE : 0;
}

extern "C" size_t bxi_box_nms_workspace_bytes(int P, int cap, int max_keep) {
    if (!nms_shape_ok(P, cap, max_keep)) return 0;
    return sizeof(int32_t) * ((size_t)P * cap + (size_t)P * (size_t)nms_spill_rows(cap, max_keep) * kSpillWords);
}

extern "C" int bxi_box_nms_f32(const float* boxes, const float* scores, const int64_t* labels, const int32_t* count, const int32_t* order,
                               int P, int cap, float iou_thr, int offset, int max_num, int32_t* keep, int32_t* n_keep, int32_t* status,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (P == 0) return BXI_OK;
    const int max_keep = max_num > 0 ? max_num : cap;                 // the stride of `keep`, also where max_num > cap
    if (!nms_shape_ok(P, cap, max_keep)) return BXI_ERR_BAD_SHAPE;
    if ((offset != 0 && offset != 1) || !(iou_thr == iou_thr)) return BXI_ERR_BAD_ARGUMENT;
    if (!boxes || !count || !keep || !n_keep || !status || (!order && !scores)) return BXI_ERR_NULL_POINTER;
    const int spill_n = nms_spill_rows(cap, max_keep);
    const bool need_ws = !order || spill_n > 0;
    if (need_ws && !workspace_ok(workspace, workspace_bytes, bxi_box_nms_workspace_bytes(P, cap, max_keep), 4))
        return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    int32_t* ws = static_cast<int32_t*>(workspace);
    const int32_t* ord = order;
    if (!order) {
        BXI_LAUNCH("box_nms_sort", s, box_sort_kernel, dim3((unsigned)P), dim3(kSortThreads), 0, s, scores, count, cap, ws);
        if (int rc = check_launch()) return rc;
        ord = ws;
    }
    int32_t* spill = spill_n > 0 ? ws + (size_t)P * cap : nullptr;
    BXI_LAUNCH("box_nms", s, box_nms_kernel, dim3((unsigned)P), dim3(kNmsThreads), 0, s, boxes, labels, count, ord, order ? 0 : 1, cap, iou_thr,
               (float)offset, max_keep, keep, n_keep, status, spill, spill_n);
    return check_launch();
}

extern "C" int bxi_det_gather_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, int n_params, const int64_t* sel, int M,
                                  const float* cand_boxes, const float* cand_scores, const int64_t* cand_labels, const int32_t* cand_pos,
                                  int cap, const int32_t* keep, const int32_t* n_keep, int max_keep, float* dets, int64_t* det_labels,
                                  float* det_params, float* det_coors, int64_t* det_level_inds, void* stream) {
    DetLevels lv;
    if (n_params < 0) return BXI_ERR_BAD_SHAPE;
    if (int rc = make_levels(levels_host, n_levels, B, C, n_params > 0, lv)) return rc;
    if (B == 0 || max_keep == 0) return BXI_OK;
    if (!sel) M = lv.first[lv.n];
    if (M < 0 || cap < 1 || max_keep < 0 || !fits_i32((int64_t)B * cap * 4) || !fits_i32((int64_t)B * max_keep * (n_params + 5)))
        return BXI_ERR_BAD_SHAPE;
    if (!cand_boxes || !cand_scores || !cand_labels || !cand_pos || !keep || !n_keep || !dets || !det_labels || !det_coors || !det_level_inds ||
        (n_params > 0 && !det_params))
        return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    const long long elems = (long long)max_keep * (n_params + 1);
    BXI_LAUNCH("det_gather", s, det_gather_kernel, dim3((unsigned)((elems + 255) / 256), (unsigned)B), dim3(256), 0, s, lv, C, n_params, sel, M,
               cand_boxes, cand_scores, cand_labels, cand_pos, cap, keep, n_keep, max_keep, dets, det_labels, det_params, det_coors,
               det_level_inds);
    return check_launch();
}
