// box_match.hip -- the target assignment of one Box2Mask decoder layer (box2mask_head.py:135-189 -> MaskHungarianAssigner.assign,
// mask_hungarian_assigner.py:46-132, with ClassificationCost and BoxMatchingCost, match_cost.py:153-193, 365-425) on gfx950, wave64.
//
//   project_pred_kernel   one workgroup = one plane x one tile of 128 destination rows x 1024 destination columns.  A thread owns four
//                         destination columns (x = tile + 256 k + tid): their source columns and weights stay in registers.  The
//                         horizontal lerp l0x a + l1x b of a source row is computed once and reused by every destination row that
//                         touches the row (four at ratio 4); the next source row is fetched one step ahead.  Per destination row the
//                         thread's values go into its four column maxima and, through a DPP wave maximum and LDS, into the row's.
//                         The up-sampled plane is never stored: what leaves the workgroup is 128 row maxima and 1024 column maxima.
//   project_plain_kernel  the same tiles over a plane that already has the target size (ground-truth masks as bytes or floats,
//                         predictions the caller up-sampled): a thread owns four CONSECUTIVE columns, one 4- or 16-byte load per row.
//   project_finish_kernel one workgroup = one plane: maximum over the tiles' partial maxima, the activation on the H + W maxima, and
//                         the two sums of squares in fp64 in a fixed order.
//   match_cost_kernel     one workgroup = one query of one problem; a wave per ground truth, lanes stride the H + W projection
//                         entries, fp64 partial sums, DPP wave totals.
//   lsa_kernel            one wave = one problem: shortest augmenting paths with duals in fp64 (the structure of scipy's
//                         rectangular_lsap), the column scan spread over the lanes, arg-min by wave reductions, state in LDS.
// Maxima are NaN-propagating (torch.max); no atomics, no allocation, no synchronisation.
#include <math.h>

#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_assign.h"

namespace bxi {

constexpr int kProjThreads = 256;
constexpr int kProjWaves = kProjThreads / kWave;
constexpr int kProjCpt = 4;                                     // destination columns per thread
constexpr int kTileCols = BXI_MATCH_TILE_COLS;
constexpr int kTileRows = BXI_MATCH_TILE_ROWS;
static_assert(kTileCols == kProjThreads * kProjCpt, "a thread owns four columns of its tile");
constexpr int kCostThreads = 256;
constexpr int kCostWaves = kCostThreads / kWave;
constexpr int kLsaMax = BXI_MATCH_MAX_SIDE;

typedef float mf4u __attribute__((ext_vector_type(4), aligned(4)));                    // a float4 at any dword address
typedef unsigned char mu8x4 __attribute__((ext_vector_type(4), aligned(1)));          // four bytes at any address

struct MatchProblems {                                           // offsets_host by value: no device copy, no sync
    int first[BXI_MAX_IMAGES + 1];
    int P;
};

__device__ __forceinline__ float qnan() { return __uint_as_float(0x7fc00000u); }
// max as torch.max reduces: a NaN operand wins
__device__ __forceinline__ float pmax(float a, float b) { return (a != a || b != b) ? qnan() : fmaxf(a, b); }
__device__ __forceinline__ float wave_pmax_f32(float v) {
    wave_total_steps([&](int c) { v = pmax(v, __int_as_float(dpp_i32(__float_as_int(v), c))); });
    const int b = __float_as_int(v);
    return pmax(pmax(__int_as_float(__builtin_amdgcn_readlane(b, 0)), __int_as_float(__builtin_amdgcn_readlane(b, 16))),
                pmax(__int_as_float(__builtin_amdgcn_readlane(b, 32)), __int_as_float(__builtin_amdgcn_readlane(b, 48))));
}
__device__ __forceinline__ double wave_min_f64(double v) {
    wave_total_steps([&](int c) {
        const long long b = __double_as_longlong(v);
        const int lo = dpp_i32((int)b, c), hi = dpp_i32((int)(b >> 32), c);
        v = fmin(v, __longlong_as_double(((long long)hi << 32) | (unsigned int)lo));
    });
    auto row = [&](int l) {
        const long long b = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
        return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    };
    return fmin(fmin(row(0), row(16)), fmin(row(32), row(48)));
}

// ATen's align_corners=False source index (UpSample.h: area_pixel_compute_source_index, guard_index_and_lambda) in fp32, the two
// roundings of scale * (dst + 0.5) - 0.5 kept apart as the CPU path has them
__device__ __forceinline__ void source_index(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = __fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}

// the maxima of the tile's rows: the waves' partials of every row, combined in wave order
__device__ __forceinline__ void store_row_maxima(const float (*red)[kTileRows], int rows, float* __restrict__ dst) {
    __syncthreads();
    for (int r = threadIdx.x; r < rows; r += kProjThreads) {
        float m = red[0][r];
#pragma unroll
        for (int q = 1; q < kProjWaves; ++q) m = pmax(m, red[q][r]);
        dst[r] = m;
    }
}

__global__ void __launch_bounds__(kProjThreads) project_pred_kernel(const float* __restrict__ logits, int h, int w, int H, int W, float sy,
                                                                    float sx, float* __restrict__ rowpart, float* __restrict__ colpart) {
    __shared__ float red[kProjWaves][kTileRows];
    const int ct = blockIdx.x, rb = blockIdx.y, n = blockIdx.z, CT = gridDim.x, RB = gridDim.y;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float* __restrict__ src = logits + (size_t)n * h * w;
    const float ninf = -INFINITY;
    int x0[kProjCpt], x1[kProjCpt];
    float lx0[kProjCpt], lx1[kProjCpt], cm[kProjCpt];
    bool live[kProjCpt];
#pragma unroll
    for (int k = 0; k < kProjCpt; ++k) {
        const int x = ct * kTileCols + k * kProjThreads + tid;
        live[k] = x < W;
        source_index(live[k] ? x : W - 1, sx, w, x0[k], x1[k], lx0[k], lx1[k]);
        cm[k] = ninf;
    }
    const int d0 = rb * kTileRows, d1 = min(H, d0 + kTileRows);
    // ha / hb: the horizontal lerps of source rows ra / rb_ ; pa / pb: the raw neighbours of row rp, fetched one step ahead
    int ra = -1, rb_ = -1, rp = -1;
    float ha[kProjCpt], hb[kProjCpt], pa[kProjCpt], pb[kProjCpt];
#pragma unroll
    for (int k = 0; k < kProjCpt; ++k) ha[k] = hb[k] = pa[k] = pb[k] = 0.f;
    auto fetch = [&](int y, float* a, float* b) {
        const float* __restrict__ row = src + (size_t)y * w;
#pragma unroll
        for (int k = 0; k < kProjCpt; ++k) { a[k] = row[x0[k]]; b[k] = row[x1[k]]; }
    };
    auto lerp_row = [&](int y, float* out) {                     // (y is the same in every lane)
        if (y != rp) { fetch(y, pa, pb); rp = y; }
#pragma unroll
        for (int k = 0; k < kProjCpt; ++k) out[k] = lx0[k] * pa[k] + lx1[k] * pb[k];
    };
    for (int d = d0; d < d1; ++d) {
        int y0, y1;
        float ly0, ly1;
        source_index(d, sy, h, y0, y1, ly0, ly1);
        if (y0 != ra) {
            if (y0 == rb_) {
#pragma unroll
                for (int k = 0; k < kProjCpt; ++k) ha[k] = hb[k];
            } else {
                lerp_row(y0, ha);
            }
            ra = y0;
        }
        if (y1 != rb_) {
            if (y1 == ra) {
#pragma unroll
                for (int k = 0; k < kProjCpt; ++k) hb[k] = ha[k];
            } else {
                lerp_row(y1, hb);
            }
            rb_ = y1;
        }
        const int ahead = min(rb_ + 1, h - 1);
        if (ahead != rp && ahead != rb_) { fetch(ahead, pa, pb); rp = ahead; }
        float rm = ninf;
#pragma unroll
        for (int k = 0; k < kProjCpt; ++k) {
            const float v = ly0 * ha[k] + ly1 * hb[k];
            if (live[k]) { cm[k] = pmax(cm[k], v); rm = pmax(rm, v); }
        }
        rm = wave_pmax_f32(rm);
        if (lane == 0) red[wave][d - d0] = rm;
    }
    float* __restrict__ cp = colpart + ((size_t)n * RB + rb) * W;
#pragma unroll
    for (int k = 0; k < kProjCpt; ++k) {
        const int x = ct * kTileCols + k * kProjThreads + tid;
        if (live[k]) cp[x] = cm[k];
    }
    store_row_maxima(red, d1 - d0, rowpart + ((size_t)n * CT + ct) * H + d0);
}

template <typename T>
__global__ void __launch_bounds__(kProjThreads) project_plain_kernel(const T* __restrict__ planes, int H, int W, float* __restrict__ rowpart,
                                                                     float* __restrict__ colpart) {
    __shared__ float red[kProjWaves][kTileRows];
    const int ct = blockIdx.x, rb = blockIdx.y, n = blockIdx.z, CT = gridDim.x, RB = gridDim.y;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const T* __restrict__ src = planes + (size_t)n * H * W;
    const float ninf = -INFINITY;
    const int x = ct * kTileCols + kProjCpt * tid;               // four consecutive columns
    const int nlive = min(max(W - x, 0), kProjCpt);
    float cm[kProjCpt] = {ninf, ninf, ninf, ninf};
    const int d0 = rb * kTileRows, d1 = min(H, d0 + kTileRows);
    for (int d = d0; d < d1; ++d) {
        const T* __restrict__ row = src + (size_t)d * W + x;
        float v[kProjCpt] = {ninf, ninf, ninf, ninf};
        if (nlive == kProjCpt) {
            if constexpr (sizeof(T) == 4) {
                const mf4u t = __builtin_nontemporal_load(reinterpret_cast<const mf4u*>(row));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                const mu8x4 t = __builtin_nontemporal_load(reinterpret_cast<const mu8x4*>(row));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kProjCpt; ++k)
                if (k < nlive) v[k] = (float)row[k];
        }
        float rm = ninf;
#pragma unroll
        for (int k = 0; k < kProjCpt; ++k) { cm[k] = pmax(cm[k], v[k]); rm = pmax(rm, v[k]); }
        rm = wave_pmax_f32(rm);
        if (lane == 0) red[wave][d - d0] = rm;
    }
    float* __restrict__ cp = colpart + ((size_t)n * RB + rb) * W;
#pragma unroll
    for (int k = 0; k < kProjCpt; ++k)
        if (k < nlive) cp[x + k] = cm[k];
    store_row_maxima(red, d1 - d0, rowpart + ((size_t)n * CT + ct) * H + d0);
}

__global__ void __launch_bounds__(kProjThreads) project_finish_kernel(const float* __restrict__ rowpart, const float* __restrict__ colpart,
                                                                      int H, int W, int CT, int RB, int act, float* __restrict__ proj_rows,
                                                                      float* __restrict__ proj_cols, float* __restrict__ sumsq) {
    __shared__ double red[2][kProjWaves];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int len = side ? W : H, parts = side ? RB : CT;
        const float* __restrict__ part = (side ? colpart : rowpart) + (size_t)n * parts * len;
        float* __restrict__ out = (side ? proj_cols : proj_rows) + (size_t)n * len;
        for (int j = tid; j < len; j += kProjThreads) {
            float m = part[j];
            for (int t = 1; t < parts; ++t) m = pmax(m, part[(size_t)t * len + j]);
            const float p = act ? 1.f / (1.f + expf(-m)) : m;
            out[j] = p;
            acc[side] += (double)p * (double)p;
        }
        const double total = wave_total_f64(acc[side]);
        if (lane == 0) red[side][wave] = total;
    }
    __syncthreads();
    if (tid < 2) sumsq[2 * (size_t)n + tid] = (float)((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]));
}

__global__ void __launch_bounds__(kCostThreads) match_cost_kernel(const float* __restrict__ cls, int C, const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ pr, const float* __restrict__ pc,
                                                                  const float* __restrict__ ps, const float* __restrict__ tr,
                                                                  const float* __restrict__ tc, const float* __restrict__ ts, MatchProblems mp,
                                                                  int Q, int H, int W, float w_cls, float w_dice, float eps,
                                                                  float* __restrict__ cost, int32_t* __restrict__ status) {
    const int q = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int g0 = mp.first[p], G = mp.first[p + 1] - g0;
    const size_t n = (size_t)p * Q + q;
    const bool with_cls = cls != nullptr && w_cls != 0.f, with_dice = w_dice != 0.f;
    if (q == 0 && wave == 0) {                                   // the problem's status word: one wave scans its labels
        int bad = 0;
        if (with_cls)
            for (int g = lane; g < G; g += kWave) {
                const long long l = labels[g0 + g];
                bad |= (l < 0 || l >= C) ? 1 : 0;
            }
        const int any = __ballot(bad) != 0ull;
        if (lane == 0) status[p] = any ? BXI_MATCH_STATUS_BAD_LABEL : 0;
    }
    if (G == 0) return;
    float mx = 0.f, den = 1.f;
    if (with_cls) {                                              // softmax statistics of the query's row (every wave its own copy)
        const float* __restrict__ row = cls + n * C;
        float m = -INFINITY;
        for (int c = lane; c < C; c += kWave) m = pmax(m, row[c]);
        mx = wave_pmax_f32(m);
        float s = 0.f;
        for (int c = lane; c < C; c += kWave) s += expf(row[c] - mx);
        den = wave_total_f32(s);
    }
    float* __restrict__ out = cost + (size_t)g0 * Q + (size_t)q * G;
    for (int g = wave; g < G; g += kCostWaves) {
        const size_t gi = (size_t)g0 + g;
        double dr = 0.0, dc = 0.0;
        if (with_dice) {
            const float* __restrict__ a = pr + n * H;
            const float* __restrict__ b = tr + gi * H;
            for (int j = lane; j < H; j += kWave) dr += (double)a[j] * (double)b[j];
            a = pc + n * W;
            b = tc + gi * W;
            for (int j = lane; j < W; j += kWave) dc += (double)a[j] * (double)b[j];
            dr = wave_total_f64(dr);
            dc = wave_total_f64(dc);
        }
        if (lane == 0) {
            double c = 0.0;
            if (with_dice) {
                const double e = (double)eps;
                const double lr = 1.0 - (2.0 * dr + e) / (((double)ps[2 * n] + (double)ts[2 * gi]) + e);
                const double lc = 1.0 - (2.0 * dc + e) / (((double)ps[2 * n + 1] + (double)ts[2 * gi + 1]) + e);
                c = (double)w_dice * (lr + lc);
            }
            if (with_cls) {
                const long long l = labels[gi];
                if (l < 0 || l >= C) c = (double)qnan();
                else c -= (double)w_cls * (double)(expf(cls[n * C + l] - mx) / den);
            }
            out[g] = (float)c;
        }
    }
}

__global__ void __launch_bounds__(kWave) lsa_kernel(const float* __restrict__ cost, const int64_t* __restrict__ labels, MatchProblems mp, int Q,
                                                    int64_t* __restrict__ assigned_gt_inds, int64_t* __restrict__ assigned_labels,
                                                    int64_t* __restrict__ pos_inds, int64_t* __restrict__ pos_gt, int32_t* __restrict__ status) {
    __shared__ double u[kLsaMax], v[kLsaMax], sh[kLsaMax];       // duals of the rows / columns, shortest path to every column
    __shared__ int path[kLsaMax], col4row[kLsaMax], row4col[kLsaMax];
    __shared__ unsigned char SR[kLsaMax], SC[kLsaMax];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int g0 = mp.first[p], G = mp.first[p + 1] - g0;
    const int npos = min(Q, G);
    int slot = 0;                                                 // first compacted slot of the problem
    for (int k = 0; k < p; ++k) slot += min(Q, mp.first[k + 1] - mp.first[k]);
    const float* __restrict__ Cm = cost + (size_t)g0 * Q;
    int64_t* __restrict__ out_gi = assigned_gt_inds + (size_t)p * Q;
    int64_t* __restrict__ out_lab = assigned_labels + (size_t)p * Q;
    int bad = 0;
    for (int idx = lane; idx < Q * G; idx += kWave) {
        const float c = Cm[idx];
        bad |= (c - c == 0.f) ? 0 : 1;                           // NaN, +inf, -inf
    }
    bad = __ballot(bad) != 0ull;
    if (lane == 0) status[p] = bad ? BXI_MATCH_STATUS_NONFINITE : 0;
    if (bad || G == 0) {
        for (int q = lane; q < Q; q += kWave) { out_gi[q] = 0; out_lab[q] = -1; }
        for (int k = lane; k < npos; k += kWave) { pos_inds[slot + k] = -1; pos_gt[slot + k] = -1; }
        return;
    }
    const bool tr = G < Q;                                        // rows are the smaller side (scipy transposes the same way)
    const int nr = tr ? G : Q, nc = tr ? Q : G;
    auto c_at = [&](int i, int j) { return (double)(tr ? Cm[(size_t)j * G + i] : Cm[(size_t)i * G + j]); };
    for (int i = lane; i < nr; i += kWave) { u[i] = 0.0; col4row[i] = -1; }
    for (int j = lane; j < nc; j += kWave) { v[j] = 0.0; row4col[j] = -1; }
    __syncthreads();
    const double inf = (double)INFINITY;
    for (int cur = 0; cur < nr; ++cur) {
        for (int i = lane; i < nr; i += kWave) SR[i] = 0;
        for (int j = lane; j < nc; j += kWave) { SC[j] = 0; sh[j] = inf; }
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc && sink < 0; ++step) {        // (a path visits a column once: nc steps always reach a sink)
            if (lane == 0) SR[i] = 1;
            const double ui = u[i];
            double low = inf;
            int low_key = 0x7fffffff;
            for (int j = lane; j < nc; j += kWave) {
                if (SC[j]) continue;
                const double r = min_val + c_at(i, j) - ui - v[j];
                if (r < sh[j]) { path[j] = i; sh[j] = r; }
                const double s = sh[j];
                const int key = (row4col[j] < 0 ? 0 : (1 << 20)) | j;          // among equal lengths an unassigned column first
                if (s < low || (s == low && key < low_key)) { low = s; low_key = key; }
            }
            min_val = wave_min_f64(low);
            const int j = wave_min_i32(low == min_val ? low_key : 0x7fffffff) & ((1 << 20) - 1);
            __syncthreads();
            const int owner = row4col[j];
            if (owner < 0) sink = j;
            else i = owner;
            if (lane == 0) SC[j] = 1;
            __syncthreads();
        }
        if (sink < 0) break;
        if (lane == 0) u[cur] += min_val;
        for (int r = lane; r < nr; r += kWave)
            if (SR[r] && r != cur) u[r] += min_val - sh[col4row[r]];
        for (int j = lane; j < nc; j += kWave)
            if (SC[j]) v[j] -= min_val - sh[j];
        __syncthreads();
        if (lane == 0) {                                          // augment along the path
            int j = sink;
            for (int step = 0; step <= nr; ++step) {
                const int r = path[j];
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    int count = 0;
    for (int base = 0; base < Q; base += kWave) {
        const int q = base + lane;
        int gt = -1;
        if (q < Q) {
            gt = tr ? row4col[q] : col4row[q];
            out_gi[q] = gt + 1;
            out_lab[q] = gt >= 0 ? labels[g0 + gt] : -1;
        }
        const unsigned long long who = __ballot(gt >= 0);
        if (gt >= 0) {
            const int at = slot + count + __popcll(who & ((1ull << lane) - 1ull));
            pos_inds[at] = q;
            pos_gt[at] = gt;
        }
        count += __popcll(who);
    }
}

inline int proj_col_tiles(int W) { return (W + kTileCols - 1) / kTileCols; }
inline int proj_row_bands(int H) { return (H + kTileRows - 1) / kTileRows; }
inline bool plane_ok(int a, int b) { return a >= 1 && b >= 1 && (int64_t)a * b < (1LL << 31); }

inline int proj_check(const void* src, int n, int H, int W, float* proj_rows, float* proj_cols, float* sumsq, void* ws, size_t ws_bytes) {
    if (n < 0 || !plane_ok(H, W) || n > 65535) return BXI_ERR_BAD_SHAPE;
    if (n == 0) return BXI_OK;
    if (!src || !proj_rows || !proj_cols || !sumsq) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(ws, ws_bytes, bxi_box_match_workspace_bytes(n, H, W), 4)) return BXI_ERR_WORKSPACE;
    return BXI_OK;
}

inline void proj_parts(void* ws, int n, int H, int W, float*& rowpart, float*& colpart) {
    rowpart = reinterpret_cast<float*>(ws);
    colpart = rowpart + (size_t)n * proj_col_tiles(W) * H;
}

inline int proj_finish(int n, int H, int W, int act, const float* rowpart, const float* colpart, float* proj_rows, float* proj_cols,
                       float* sumsq, hipStream_t s) {
    BXI_LAUNCH("match_project_finish", s, project_finish_kernel, dim3((unsigned)n), dim3(kProjThreads), 0, s, rowpart, colpart, H, W,
               proj_col_tiles(W), proj_row_bands(H), act, proj_rows, proj_cols, sumsq);
    return check_launch();
}

template <typename T>
int project_plain(const T* planes, int n, int H, int W, int act, float* proj_rows, float* proj_cols, float* sumsq, void* ws, size_t ws_bytes,
                  void* stream) {
    const int rc = proj_check(planes, n, H, W, proj_rows, proj_cols, sumsq, ws, ws_bytes);
    if (rc != BXI_OK || n == 0) return rc;
    float *rowpart, *colpart;
    proj_parts(ws, n, H, W, rowpart, colpart);
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH(sizeof(T) == 4 ? "match_project_plain_f32" : "match_project_plain_u8", s, project_plain_kernel<T>,
               dim3((unsigned)proj_col_tiles(W), (unsigned)proj_row_bands(H), (unsigned)n), dim3(kProjThreads), 0, s, planes, H, W, rowpart,
               colpart);
    return proj_finish(n, H, W, act, rowpart, colpart, proj_rows, proj_cols, sumsq, s);
}

// offsets_host -> MatchProblems; BXI_OK, or the status of the first thing that is wrong with it
inline int problems_from(const int* offsets_host, int P, int max_g, MatchProblems& mp) {
    if (P < 0 || P > BXI_MAX_IMAGES) return BXI_ERR_BAD_SHAPE;
    if (P == 0) return BXI_OK;
    if (!offsets_host) return BXI_ERR_NULL_POINTER;
    if (offsets_host[0] != 0) return BXI_ERR_BAD_ARGUMENT;
    for (int p = 0; p <= P; ++p) mp.first[p] = offsets_host[p];
    for (int p = 0; p < P; ++p) {
        if (mp.first[p + 1] < mp.first[p]) return BXI_ERR_BAD_ARGUMENT;
        if (max_g > 0 && mp.first[p + 1] - mp.first[p] > max_g) return BXI_ERR_UNSUPPORTED;
    }
    mp.P = P;
    return BXI_OK;
}

}  // namespace bxi

extern "C" size_t bxi_box_match_workspace_bytes(int n, int H, int W) {
    if (n < 1 || !bxi::plane_ok(H, W)) return 0;
    return sizeof(float) * (size_t)n * ((size_t)bxi::proj_col_tiles(W) * H + (size_t)bxi::proj_row_bands(H) * W);
}

extern "C" int bxi_match_project_pred_f32(const float* logits, int n, int h, int w, int H, int W, int apply_sigmoid, float* proj_rows,
                                          float* proj_cols, float* sumsq, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (!plane_ok(h, w)) return BXI_ERR_BAD_SHAPE;
    if (h == H && w == W) return project_plain<float>(logits, n, H, W, apply_sigmoid ? 1 : 0, proj_rows, proj_cols, sumsq, workspace, workspace_bytes, stream);
    const int rc = proj_check(logits, n, H, W, proj_rows, proj_cols, sumsq, workspace, workspace_bytes);
    if (rc != BXI_OK || n == 0) return rc;
    float *rowpart, *colpart;
    proj_parts(workspace, n, H, W, rowpart, colpart);
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("match_project_pred", s, project_pred_kernel, dim3((unsigned)proj_col_tiles(W), (unsigned)proj_row_bands(H), (unsigned)n),
               dim3(kProjThreads), 0, s, logits, h, w, H, W, (float)h / (float)H, (float)w / (float)W, rowpart, colpart);
    return proj_finish(n, H, W, apply_sigmoid ? 1 : 0, rowpart, colpart, proj_rows, proj_cols, sumsq, s);
}

extern "C" int bxi_match_project_gt_u8(const uint8_t* masks, int g, int H, int W, float* proj_rows, float* proj_cols, float* sumsq,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return bxi::project_plain<uint8_t>(masks, g, H, W, 0, proj_rows, proj_cols, sumsq, workspace, workspace_bytes, stream);
}

extern "C" int bxi_match_project_gt_f32(const float* masks, int g, int H, int W, float* proj_rows, float* proj_cols, float* sumsq,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return bxi::project_plain<float>(masks, g, H, W, 0, proj_rows, proj_cols, sumsq, workspace, workspace_bytes, stream);
}

extern "C" int bxi_match_cost_f32(const float* cls, int C, const int64_t* gt_labels, const float* pred_rows, const float* pred_cols,
                                  const float* pred_sumsq, const float* gt_rows, const float* gt_cols, const float* gt_sumsq, int P, int Q,
                                  const int* offsets_host, int H, int W, float w_cls, float w_dice, float eps, float* cost, int32_t* status,
                                  void* stream) {
    using namespace bxi;
    MatchProblems mp;
    const int rc = problems_from(offsets_host, P, 0, mp);
    if (rc != BXI_OK || P == 0) return rc;
    if (!(w_cls == w_cls) || !(w_dice == w_dice) || !(eps == eps)) return BXI_ERR_BAD_ARGUMENT;
    const bool with_cls = cls != nullptr && w_cls != 0.f, with_dice = w_dice != 0.f;
    if (Q < 1 || Q > 65535 || H < 1 || W < 1 || (with_cls && C < 1)) return BXI_ERR_BAD_SHAPE;
    if (!status) return BXI_ERR_NULL_POINTER;
    const int total = mp.first[P];
    if (total > 0) {
        if (!cost || (with_cls && !gt_labels)) return BXI_ERR_NULL_POINTER;
        if (with_dice && (!pred_rows || !pred_cols || !pred_sumsq || !gt_rows || !gt_cols || !gt_sumsq)) return BXI_ERR_NULL_POINTER;
    }
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("match_cost", s, match_cost_kernel, dim3((unsigned)Q, (unsigned)P), dim3(kCostThreads), 0, s, cls, C, gt_labels, pred_rows,
               pred_cols, pred_sumsq, gt_rows, gt_cols, gt_sumsq, mp, Q, H, W, w_cls, w_dice, eps, cost, status);
    return check_launch();
}

extern "C" int bxi_linear_sum_assignment_f32(const float* cost, const int64_t* gt_labels, int P, int Q, const int* offsets_host,
                                             int64_t* assigned_gt_inds, int64_t* assigned_labels, int64_t* pos_inds,
                                             int64_t* pos_assigned_gt_inds, int32_t* status, void* stream) {
    using namespace bxi;
    if (P < 0 || P > BXI_MAX_IMAGES) return BXI_ERR_BAD_SHAPE;
    if (P == 0) return BXI_OK;
    if (Q < 1 || Q > BXI_MATCH_MAX_SIDE) return BXI_ERR_UNSUPPORTED;
    MatchProblems mp;
    const int rc = problems_from(offsets_host, P, BXI_MATCH_MAX_SIDE, mp);
    if (rc != BXI_OK) return rc;
    if (!assigned_gt_inds || !assigned_labels || !status) return BXI_ERR_NULL_POINTER;
    if (mp.first[P] > 0 && (!cost || !gt_labels || !pos_inds || !pos_assigned_gt_inds)) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("match_lsa", s, lsa_kernel, dim3((unsigned)P), dim3(kWave), 0, s, cost, gt_labels, mp, Q, assigned_gt_inds, assigned_labels,
               pos_inds, pos_assigned_gt_inds, status);
    return check_launch();
}
