// discobox_loss.hip -- the pseudo-label block of DiscoBoxSOLOv2Head.loss for the assigned rows of ALL levels at once
// (mmdet/models/dense_heads/discobox_head.py: loss :1271-1306 and :1335-1339, the tail of corr_loss :1127-1137).
//
// Every label of that block is a bit: the target, its 3x3 dilation ("enlarged target", F.max_pool2d of a 0/1 plane), the mean-field
// state and the pseudo-label.  They live as 64-pixel words [R][H][segs] in one workspace, as meanfield.hip keeps its state:
//   plane 0            target words
//   plane 1            enlarged-target words
//   plane 2 + 2 g + k  state buffer k (0 / 1) of leg g; after `iters` steps the pseudo-label of leg g is buffer iters & 1
// followed by the fp64 partial sums of the dice forward.  Leg 0 is MeanField.forward without inter_img_mask (:1298), leg 1 with it
// (:1132); both start from the same state and read the same affinities, so one launch per iteration advances both
// (meanfield_device.hpp: the same device function per leg as bxi_meanfield_forward_f32 runs).
// No float plane of a label is ever written: the dice sums read `s` once and take e, b from the words; sum b^2 is a popcount.
#include "common.hpp"
#include "meanfield_device.hpp"
#include "../../include/boxinst/boxinst_hip_dbx.h"

namespace bxi {

constexpr int kDbxMaxLevels = BXI_DBX_MAX_LEVELS;
constexpr int kDbxChunkLines = 16;        // lines per workgroup of the dice sums: 4 waves x 4 lines
constexpr int kDbxPartials = 3;           // per leg: sum a b, sum a^2, sum b^2

struct DbxLevels { const float* iiu[kDbxMaxLevels]; int first[kDbxMaxLevels + 1]; int n; };
struct DbxRows { const float* v[BXI_DBX_MAX_MEANS]; };

struct DbxWs { u64* words; double* part; size_t plane; int nchunk; };
__host__ __device__ inline size_t dbx_carve(void* ws, int R, int H, int W, int legs, DbxWs* out) {
    const size_t R1 = R > 0 ? R : 1, segs = (size_t)(W + 63) / 64, plane = R1 * H * segs;
    const size_t nchunk = (size_t)(H + kDbxChunkLines - 1) / kDbxChunkLines;
    const size_t words = (2 + 2 * (size_t)legs) * plane;
    if (out) {
        out->words = reinterpret_cast<u64*>(ws); out->plane = plane; out->nchunk = (int)nchunk;
        out->part = reinterpret_cast<double*>(out->words + words);
    }
    return 8 * (words + R1 * nchunk * kDbxPartials * legs);
}

// ---------------------------------------------------------------------------------------------------
// target, enlarged target (3x3 dilation in the bit domain) and the initial state ((t + s) / 2 * target > 0.5, :621-622 on :1299) of
// every (row, line, segment) item: a wave per IPW items, as mf_init_kernel
template <int IPW>
__global__ __launch_bounds__(256) void dbx_prepare_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                          const uint8_t* __restrict__ tg, int H, int W, int segs, int legs,
                                                          u64* __restrict__ ws, size_t plane) {
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int first = mf_first_item<IPW>(), total = H * segs;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* T = tg + (int64_t)n * HW;
#pragma unroll
    for (int u = 0; u < IPW; ++u) {
        const int item = first + u;
        if (item >= total) break;                                  // wave-uniform
        const int r = item / segs, sg = item % segs, c0 = sg * 64, c = c0 + lane;
        const bool in = c < W;
        const int cc = in ? c : W - 1;                             // clamped: loads need no branch
        const int64_t o = (int64_t)r * W + cc;
        const uint8_t tc = T[o];
        const uint8_t tu = T[(int64_t)(r > 0 ? r - 1 : r) * W + cc], td = T[(int64_t)(r + 1 < H ? r + 1 : r) * W + cc];   // a clamped line repeats line r
        const float sv = s[(int64_t)n * HW + o], tv = t[(int64_t)n * HW + o];
        // the columns next to the segment, lines r - 1, r, r + 1: lanes 0..2 the left one, lanes 3..5 the right one
        const int dy = lane % 3 - 1, c2 = lane < 3 ? c0 - 1 : c0 + 64, r2 = r + dy;
        const bool side_ok = lane < 6 && r2 >= 0 && r2 < H && c2 >= 0 && c2 < W;
        const bool side = side_ok && T[(int64_t)(side_ok ? r2 : r) * W + (side_ok ? c2 : cc)] != 0;
        const u64 mt = __ballot(in && tc != 0);
        const u64 v = mt | __ballot(in && (tu != 0 || td != 0));   // three lines OR-ed
        const u64 sd = __ballot(side);
        const int left = W - c0;
        const u64 inside = left >= 64 ? ~0ull : ((1ull << left) - 1ull);        // clipped to the map: columns >= W stay zero
        const u64 en = (v | (v << 1) | (v >> 1) | ((sd & 7ull) ? 1ull : 0ull) | ((sd & 56ull) ? (1ull << 63) : 0ull)) & inside;
        const float x = __fmul_rn(__fadd_rn(tv, sv), 0.5f);
        const u64 ms = __ballot(in && __fmul_rn(x, (float)tc) > 0.5f);
        if (lane == 0) {
            const size_t w = (size_t)n * total + item;
            ws[w] = mt; ws[plane + w] = en;
            for (int g = 0; g < legs; ++g) {                           // both buffers: items without target are never written again
                ws[(2 + 2 * (size_t)g) * plane + w] = ms; ws[(3 + 2 * (size_t)g) * plane + w] = 0ull;
            }
        }
    }
}

// live[r] = the row has a target pixel; n_live = their number.  One workgroup, no atomics: a wave per row, 16 rows at a time.
__global__ __launch_bounds__(1024) void dbx_live_kernel(const u64* __restrict__ tw, int R, int total, int* __restrict__ live,
                                                        int* __restrict__ n_live) {
    __shared__ int cnt[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int mine = 0;
    for (int r = wave; r < R; r += 16) {
        u64 acc = 0ull;
        for (int i = lane; i < total; i += 64) acc |= tw[(size_t)r * total + i];
        const int any = __any(acc != 0ull) ? 1 : 0;
        if (lane == 0) live[r] = any;
        mine += any;
    }
    if (lane == 0) cnt[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < 16; ++w) sum += cnt[w];
        n_live[0] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------
// one mean-field iteration of every item, both legs: the affinities and the target word are loaded once
template <int KS, int IPW, int LEGS>
__global__ __launch_bounds__(256) void dbx_step_kernel(MfArgs a, DbxLevels lv, const u64* __restrict__ sa1, u64* __restrict__ sb1) {
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int first = mf_first_item<IPW>(), total = a.H * a.segs;
    if (first >= total) return;
    const u64* twp = a.tw + (int64_t)n * total + first;
    u64 mt[IPW];
#pragma unroll
    for (int u = 0; u < IPW; ++u) mt[u] = first + u < total ? twp[u] : 0ull;
    const float* inter = nullptr;                                  // this row's [2,H,W] planes of its level's iiu (uniform)
    if (LEGS == 2) {
#pragma unroll
        for (int l = 0; l < kDbxMaxLevels; ++l)
            if (l < lv.n && n >= lv.first[l] && n < lv.first[l + 1] && lv.iiu[l])
                inter = lv.iiu[l] + (int64_t)(n - lv.first[l]) * 2 * a.H * a.W;
    }
#pragma unroll
    for (int u = 0; u < IPW; ++u) {
        if (!mt[u]) continue;                                      // wave-uniform
        const int r = (first + u) / a.segs, sg = (first + u) % a.segs, c = sg * 64 + lane;
        float kv[KS * KS];
        mf_load_affinity<KS>(a, n, r, c < a.W ? c : a.W - 1, kv);
        mf_eval_loaded<KS>(a, kv, nullptr, a.sa, a.sb, n, r, sg, mt[u], lane);
        if (LEGS == 2) mf_eval_loaded<KS>(a, kv, inter, sa1, sb1, n, r, sg, mt[u], lane);
    }
}

// ---------------------------------------------------------------------------------------------------
// dice_loss(s * enlarged, pseudo) (:1300) and dice_loss(s e gamma + (s e).detach() (1 - gamma), pseudo_corr) (:1135-1137)
__device__ __forceinline__ float dbx_a1(float a0, float g, float omg) { return __fadd_rn(__fmul_rn(a0, g), __fmul_rn(a0, omg)); }

template <int LEGS>
__global__ __launch_bounds__(256) void dbx_dice_partial_kernel(const float* __restrict__ s, int H, int W, int segs, const u64* __restrict__ ew,
                                                               const u64* __restrict__ b0w, const u64* __restrict__ b1w, float g, float omg,
                                                               double* __restrict__ part) {
    __shared__ double red[4][2 * LEGS];
    __shared__ int pcs[4][LEGS];
    const int chunk = blockIdx.x, n = blockIdx.y, nchunk = gridDim.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* S = s + (int64_t)n * H * W;
    double ab[LEGS], aa[LEGS];
    int pc[LEGS];
#pragma unroll
    for (int q = 0; q < LEGS; ++q) { ab[q] = 0.0; aa[q] = 0.0; pc[q] = 0; }
    for (int i = 0; i < 4; ++i) {
        const int r = chunk * kDbxChunkLines + wave * 4 + i;
        if (r >= H) break;
        for (int sg = 0; sg < segs; ++sg) {
            const size_t w = ((size_t)n * H + r) * segs + sg;
            const u64 e = ew[w], b0 = b0w[w];
            const int c = sg * 64 + lane;
            const float sv = c < W ? S[(int64_t)r * W + c] : 0.f;
            const float a0 = ((e >> lane) & 1ull) ? sv : 0.f;         // s * enlarged
            const double a0d = a0;
            if ((b0 >> lane) & 1ull) ab[0] += a0d;
            aa[0] += a0d * a0d;
            pc[0] += __popcll(b0);
            if (LEGS == 2) {
                const u64 b1 = b1w[w];
                const double a1d = dbx_a1(a0, g, omg);
                if ((b1 >> lane) & 1ull) ab[1] += a1d;
                aa[1] += a1d * a1d;
                pc[1] += __popcll(b1);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < LEGS; ++q) {
        const double x = wave_total_f64(ab[q]), y = wave_total_f64(aa[q]);
        if (lane == 0) { red[wave][2 * q] = x; red[wave][2 * q + 1] = y; pcs[wave][q] = pc[q]; }
    }
    __syncthreads();
    if (threadIdx.x < LEGS) {
        const int q = threadIdx.x;
        double x = 0.0, y = 0.0; int p = 0;
        for (int wv = 0; wv < 4; ++wv) { x += red[wv][2 * q]; y += red[wv][2 * q + 1]; p += pcs[wv][q]; }     // fixed order
        double* o = part + (((size_t)n * nchunk + chunk) * LEGS + q) * kDbxPartials;
        o[0] = x; o[1] = y; o[2] = (double)p;
    }
}

__global__ __launch_bounds__(256) void dbx_dice_finish_kernel(const double* __restrict__ part, int R, int nchunk, int legs,
                                                              float* __restrict__ loss, double* __restrict__ sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= legs * R) return;
    const int q = i / R, n = i % R;
    double A = 0.0, aa = 0.0, bb = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {                              // index order
        const double* p = part + (((size_t)n * nchunk + ch) * legs + q) * kDbxPartials;
        A += p[0]; aa += p[1]; bb += p[2];
    }
    const double D = aa + bb + 0.002;
    loss[i] = (float)(1.0 - 2.0 * A / D);
    sums[2 * (size_t)i] = A; sums[2 * (size_t)i + 1] = D;
}

template <int LEGS>
__global__ __launch_bounds__(256) void dbx_dice_bwd_kernel(const float* __restrict__ s, int R, int H, int W, int segs, const u64* __restrict__ ew,
                                                           const u64* __restrict__ b0w, const u64* __restrict__ b1w, float g, float omg,
                                                           const double* __restrict__ sums, const float* __restrict__ g_rows,
                                                           float* __restrict__ g_s) {
    const int64_t HW = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)R * HW) return;
    const int n = (int)(i / HW), p = (int)(i % HW), r = p / W, c = p % W;
    const size_t w = ((size_t)n * H + r) * segs + (c >> 6);
    const int bit = c & 63;
    float out = 0.f;
    if ((ew[w] >> bit) & 1ull) {
        const float a0 = s[i];
        const double A0 = sums[2 * (size_t)n], D0 = sums[2 * (size_t)n + 1];
        const float b0 = (float)((b0w[w] >> bit) & 1ull);
        out = g_rows[n] * ((float)(-2.0 / D0) * b0 + (float)(4.0 * A0 / (D0 * D0)) * a0);
        if (LEGS == 2) {
            const double A1 = sums[2 * ((size_t)R + n)], D1 = sums[2 * ((size_t)R + n) + 1];
            const float b1 = (float)((b1w[w] >> bit) & 1ull);
            out += g * g_rows[R + n] * ((float)(-2.0 / D1) * b1 + (float)(4.0 * A1 / (D1 * D1)) * dbx_a1(a0, g, omg));
        }
    }
    g_s[i] = out;
}

// ---------------------------------------------------------------------------------------------------
// means[k] = sum_r live[r] v_k[r] / max(n_live, 1): one workgroup, fp64, a fixed order
__global__ __launch_bounds__(256) void dbx_means_kernel(DbxRows rows, int K, const int* __restrict__ live, const int* __restrict__ n_live,
                                                        int R, float* __restrict__ means) {
    __shared__ double red[16];
    const double denom = (double)max(n_live[0], 1);
    for (int k = 0; k < K; ++k) {
        double acc = 0.0;
        for (int r = threadIdx.x; r < R; r += 256)
            if (live[r]) acc += (double)rows.v[k][r];
        acc = block_sum_seq_f64(acc, red);
        if (threadIdx.x == 0) means[k] = (float)(acc / denom);
    }
}

__global__ __launch_bounds__(256) void dbx_means_bwd_kernel(const float* __restrict__ g_means, int K, const int* __restrict__ live,
                                                            const int* __restrict__ n_live, int R, float* __restrict__ g_rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * R) return;
    const int k = i / R, r = i % R;
    g_rows[i] = live[r] ? (float)((double)g_means[k] / (double)max(n_live[0], 1)) : 0.f;
}

__global__ __launch_bounds__(256) void dbx_unpack_kernel(const u64* __restrict__ words, int R, int H, int W, int segs, uint8_t* __restrict__ out) {
    const int64_t HW = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)R * HW) return;
    const int n = (int)(i / HW), p = (int)(i % HW), r = p / W, c = p % W;
    out[i] = (uint8_t)((words[((size_t)n * H + r) * segs + (c >> 6)] >> (c & 63)) & 1ull);
}

// what every entry point refuses, before any launch
static int dbx_check(int R, int H, int W, int legs) {
    if (R < 0 || H <= 0 || W <= 0) return BXI_ERR_BAD_SHAPE;
    if (legs != 1 && legs != 2) return BXI_ERR_BAD_ARGUMENT;
    if (R > 65535) return BXI_ERR_UNSUPPORTED;
    if (!fits_i32((int64_t)(R > 0 ? R : 1) * H * W)) return BXI_ERR_BAD_SHAPE;
    return BXI_OK;
}

static dim3 dbx_item_grid(int R, int H, int segs, bool* many) {
    *many = mf_many_items((int64_t)R * H * segs);
    const int per_wg = kMfWaves * (*many ? 4 : 1);
    return dim3((unsigned)((H * segs + per_wg - 1) / per_wg), (unsigned)R);
}

}  // namespace bxi

extern "C" {

size_t bxi_dbx_workspace_bytes(int R, int H, int W, int legs) {
    if (bxi::dbx_check(R, H, W, legs) != BXI_OK) return 0;
    return bxi::dbx_carve(nullptr, R, H, W, legs, nullptr);
}

int bxi_dbx_prepare_f32(const float* s_rows, const float* t_rows, const uint8_t* target_rows, int R, int H, int W, int legs,
                        int32_t* live, int32_t* n_live, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc0 = bxi::dbx_check(R, H, W, legs);
    if (rc0 != BXI_OK) return rc0;
    if (R == 0) return BXI_OK;
    if (!s_rows || !t_rows || !target_rows || !live || !n_live) return BXI_ERR_NULL_POINTER;
    if (!bxi::workspace_ok(workspace, workspace_bytes, bxi::dbx_carve(nullptr, R, H, W, legs, nullptr), 8)) return BXI_ERR_WORKSPACE;
    bxi::DbxWs ws;
    bxi::dbx_carve(workspace, R, H, W, legs, &ws);
    const int segs = (W + 63) / 64;
    bool many;
    const dim3 grid = bxi::dbx_item_grid(R, H, segs, &many), block(64 * bxi::kMfWaves);
    hipStream_t s = bxi::as_stream(stream);
    if (many) BXI_LAUNCH("dbx_prepare", s, bxi::dbx_prepare_kernel<4>, grid, block, 0, s, s_rows, t_rows, target_rows, H, W, segs, legs, ws.words, ws.plane);
    else BXI_LAUNCH("dbx_prepare", s, bxi::dbx_prepare_kernel<1>, grid, block, 0, s, s_rows, t_rows, target_rows, H, W, segs, legs, ws.words, ws.plane);
    int rc = bxi::check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("dbx_live", s, bxi::dbx_live_kernel, dim3(1), dim3(1024), 0, s, ws.words, R, H * segs, live, n_live);
    return bxi::check_launch();
}

int bxi_dbx_steps_f32(const float* kernel, int B, int H, int W, int ksize, const int64_t* img_inds, int R, int iters, float base,
                      double gamma, int legs, const float* const* iiu_levels_host, const int* level_first_host, int n_levels,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const int rc0 = bxi::dbx_check(R, H, W, legs);
    if (rc0 != BXI_OK) return rc0;
    if (B <= 0 || iters < 0) return BXI_ERR_BAD_SHAPE;
    if (ksize != 3 && ksize != 5) return BXI_ERR_UNSUPPORTED;
    if (!(base > 0.f) || !(base < 0.5f)) return BXI_ERR_BAD_ARGUMENT;
    bxi::DbxLevels lv;
    lv.n = 0;
    for (int l = 0; l < bxi::kDbxMaxLevels; ++l) { lv.iiu[l] = nullptr; lv.first[l] = R; }
    lv.first[bxi::kDbxMaxLevels] = R;
    if (legs == 2) {
        if (n_levels < 0) return BXI_ERR_BAD_SHAPE;
        if (n_levels > bxi::kDbxMaxLevels) return BXI_ERR_UNSUPPORTED;
        if (n_levels > 0 && (!iiu_levels_host || !level_first_host)) return BXI_ERR_NULL_POINTER;
        for (int l = 0; l < n_levels; ++l) {           // first[l] .. first[l + 1]: the rows of level l, ascending, ending at R
            const int lo = level_first_host[l], hi = l + 1 < n_levels ? level_first_host[l + 1] : R;
            if (lo < 0 || hi < lo || hi > R || (l == 0 && lo != 0)) return BXI_ERR_BAD_ARGUMENT;
            lv.iiu[l] = iiu_levels_host[l]; lv.first[l] = lo;
        }
        lv.n = n_levels;
    }
    if (R == 0) return BXI_OK;
    if (!kernel) return BXI_ERR_NULL_POINTER;
    if (!bxi::fits_i32((int64_t)B * H * W * ksize * ksize)) return BXI_ERR_BAD_SHAPE;
    if (!bxi::workspace_ok(workspace, workspace_bytes, bxi::dbx_carve(nullptr, R, H, W, legs, nullptr), 8)) return BXI_ERR_WORKSPACE;
    bxi::DbxWs ws;
    bxi::dbx_carve(workspace, R, H, W, legs, &ws);
    bxi::MfArgs a;
    a.K = kernel; a.x = nullptr; a.t = nullptr; a.img = img_inds; a.inter = nullptr; a.ret = nullptr; a.valid = nullptr;
    a.B = B; a.H = H; a.W = W; a.N = R; a.t_u8 = 1; a.segs = (W + 63) / 64;
    a.tw = ws.words; a.sa = ws.words + 2 * ws.plane; a.sb = ws.words + 3 * ws.plane;
    bxi::u64 *sa1 = legs == 2 ? ws.words + 4 * ws.plane : a.sa, *sb1 = legs == 2 ? ws.words + 5 * ws.plane : a.sb;   // read with legs == 2 only
    bxi::mf_set_levels(a, base);
    a.gamma = (float)gamma; a.vlo = 0.f; a.vhi = 0.f;
    bool many;
    const dim3 grid = bxi::dbx_item_grid(R, H, a.segs, &many), block(64 * bxi::kMfWaves);
    hipStream_t s = bxi::as_stream(stream);
    int rc = BXI_OK;
#define BXI_DBX_STEP(KS, IPW, LEGS) BXI_LAUNCH("dbx_step", s, (bxi::dbx_step_kernel<KS, IPW, LEGS>), grid, block, 0, s, a, lv, sa1, sb1)
    for (int it = 0; it < iters && rc == BXI_OK; ++it) {
        if (legs == 2) {
            if (ksize == 3) { if (many) BXI_DBX_STEP(3, 4, 2); else BXI_DBX_STEP(3, 1, 2); }
            else { if (many) BXI_DBX_STEP(5, 4, 2); else BXI_DBX_STEP(5, 1, 2); }
        } else {
            if (ksize == 3) { if (many) BXI_DBX_STEP(3, 4, 1); else BXI_DBX_STEP(3, 1, 1); }
            else { if (many) BXI_DBX_STEP(5, 4, 1); else BXI_DBX_STEP(5, 1, 1); }
        }
        rc = bxi::check_launch();
        bxi::u64* tmp = a.sa; a.sa = a.sb; a.sb = tmp;
        tmp = sa1; sa1 = sb1; sb1 = tmp;
    }
#undef BXI_DBX_STEP
    return rc;
}

int bxi_dbx_dice_forward_f32(const float* s_rows, int R, int H, int W, int legs, int iters, double gamma, void* workspace,
                             size_t workspace_bytes, float* loss, double* sums, void* stream) {
    const int rc0 = bxi::dbx_check(R, H, W, legs);
    if (rc0 != BXI_OK) return rc0;
    if (iters < 0) return BXI_ERR_BAD_SHAPE;
    if (R == 0) return BXI_OK;
    if (!s_rows || !loss || !sums) return BXI_ERR_NULL_POINTER;
    if (!bxi::aligned(sums, 8)) return BXI_ERR_BAD_ARGUMENT;
    if (!bxi::workspace_ok(workspace, workspace_bytes, bxi::dbx_carve(nullptr, R, H, W, legs, nullptr), 8)) return BXI_ERR_WORKSPACE;
    bxi::DbxWs ws;
    bxi::dbx_carve(workspace, R, H, W, legs, &ws);
    const int segs = (W + 63) / 64, fin = iters & 1;
    const bxi::u64 *ew = ws.words + ws.plane, *b0 = ws.words + (2 + fin) * ws.plane, *b1 = ws.words + (4 + fin) * ws.plane;
    const float g = (float)gamma, omg = (float)(1.0 - gamma);
    hipStream_t s = bxi::as_stream(stream);
    const dim3 grid((unsigned)ws.nchunk, (unsigned)R);
    if (legs == 2) BXI_LAUNCH("dbx_dice_partial", s, bxi::dbx_dice_partial_kernel<2>, grid, dim3(256), 0, s, s_rows, H, W, segs, ew, b0, b1, g, omg, ws.part);
    else BXI_LAUNCH("dbx_dice_partial", s, bxi::dbx_dice_partial_kernel<1>, grid, dim3(256), 0, s, s_rows, H, W, segs, ew, b0, b0, g, omg, ws.part);
    int rc = bxi::check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("dbx_dice_finish", s, bxi::dbx_dice_finish_kernel, dim3((unsigned)((legs * R + 255) / 256)), dim3(256), 0, s, ws.part, R, ws.nchunk,
               legs, loss, sums);
    return bxi::check_launch();
}

int bxi_dbx_dice_backward_f32(const float* s_rows, int R, int H, int W, int legs, int iters, double gamma, const void* workspace,
                              size_t workspace_bytes, const double* sums, const float* g_rows, float* g_s, void* stream) {
    const int rc0 = bxi::dbx_check(R, H, W, legs);
    if (rc0 != BXI_OK) return rc0;
    if (iters < 0) return BXI_ERR_BAD_SHAPE;
    if (R == 0) return BXI_OK;
    if (!s_rows || !sums || !g_rows || !g_s) return BXI_ERR_NULL_POINTER;
    if (!bxi::aligned(sums, 8)) return BXI_ERR_BAD_ARGUMENT;
    if (!bxi::workspace_ok(workspace, workspace_bytes, bxi::dbx_carve(nullptr, R, H, W, legs, nullptr), 8)) return BXI_ERR_WORKSPACE;
    bxi::DbxWs ws;
    bxi::dbx_carve(const_cast<void*>(workspace), R, H, W, legs, &ws);
    const int segs = (W + 63) / 64, fin = iters & 1;
    const bxi::u64 *ew = ws.words + ws.plane, *b0 = ws.words + (2 + fin) * ws.plane, *b1 = ws.words + (4 + fin) * ws.plane;
    const float g = (float)gamma, omg = (float)(1.0 - gamma);
    hipStream_t s = bxi::as_stream(stream);
    const unsigned grid = (unsigned)(((int64_t)R * H * W + 255) / 256);
    if (legs == 2) BXI_LAUNCH("dbx_dice_bwd", s, bxi::dbx_dice_bwd_kernel<2>, dim3(grid), dim3(256), 0, s, s_rows, R, H, W, segs, ew, b0, b1, g, omg, sums, g_rows, g_s);
    else BXI_LAUNCH("dbx_dice_bwd", s, bxi::dbx_dice_bwd_kernel<1>, dim3(grid), dim3(256), 0, s, s_rows, R, H, W, segs, ew, b0, b0, g, omg, sums, g_rows, g_s);
    return bxi::check_launch();
}

int bxi_dbx_means_f32(const float* const* rows_host, int K, const int32_t* live, const int32_t* n_live, int R, float* means, void* stream) {
    if (R < 0 || K < 0) return BXI_ERR_BAD_SHAPE;
    if (K > BXI_DBX_MAX_MEANS || R > 65535) return BXI_ERR_UNSUPPORTED;
    if (K == 0) return BXI_OK;
    if (!rows_host || !n_live || !means || (R > 0 && !live)) return BXI_ERR_NULL_POINTER;
    bxi::DbxRows rows;
    for (int k = 0; k < BXI_DBX_MAX_MEANS; ++k) rows.v[k] = k < K ? rows_host[k] : nullptr;
    for (int k = 0; k < K; ++k)
        if (R > 0 && !rows.v[k]) return BXI_ERR_NULL_POINTER;
    hipStream_t s = bxi::as_stream(stream);
    BXI_LAUNCH("dbx_means", s, bxi::dbx_means_kernel, dim3(1), dim3(256), 0, s, rows, K, live, n_live, R, means);
    return bxi::check_launch();
}

int bxi_dbx_means_backward_f32(const float* g_means, int K, const int32_t* live, const int32_t* n_live, int R, float* g_rows, void* stream) {
    if (R < 0 || K < 0) return BXI_ERR_BAD_SHAPE;
    if (K > BXI_DBX_MAX_MEANS || R > 65535) return BXI_ERR_UNSUPPORTED;
    if (K == 0 || R == 0) return BXI_OK;
    if (!g_means || !live || !n_live || !g_rows) return BXI_ERR_NULL_POINTER;
    hipStream_t s = bxi::as_stream(stream);
    BXI_LAUNCH("dbx_means_bwd", s, bxi::dbx_means_bwd_kernel, dim3((unsigned)((K * R + 255) / 256)), dim3(256), 0, s, g_means, K, live, n_live, R, g_rows);
    return bxi::check_launch();
}

int bxi_dbx_unpack_u8(const void* workspace, size_t workspace_bytes, int which, int iters, int R, int H, int W, int legs, uint8_t* out,
                      void* stream) {
    const int rc0 = bxi::dbx_check(R, H, W, legs);
    if (rc0 != BXI_OK) return rc0;
    if (iters < 0) return BXI_ERR_BAD_SHAPE;
    if (which < 0 || which > 1 + legs) return BXI_ERR_BAD_ARGUMENT;
    if (R == 0) return BXI_OK;
    if (!out) return BXI_ERR_NULL_POINTER;
    if (!bxi::workspace_ok(workspace, workspace_bytes, bxi::dbx_carve(nullptr, R, H, W, legs, nullptr), 8)) return BXI_ERR_WORKSPACE;
    bxi::DbxWs ws;
    bxi::dbx_carve(const_cast<void*>(workspace), R, H, W, legs, &ws);
    const size_t plane = which < 2 ? (size_t)which : 2 + 2 * (size_t)(which - 2) + (iters & 1);
    hipStream_t s = bxi::as_stream(stream);
    const unsigned grid = (unsigned)(((int64_t)R * H * W + 255) / 256);
    BXI_LAUNCH("dbx_unpack", s, bxi::dbx_unpack_kernel, dim3(grid), dim3(256), 0, s, ws.words + plane * ws.plane, R, H, W, (W + 63) / 64, out);
    return bxi::check_launch();
}

}  // extern "C"
