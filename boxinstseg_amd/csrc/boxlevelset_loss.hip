// boxlevelset_loss.hip -- the mask losses of BoxSOLOv2Head.loss (mmdet/models/dense_heads/box_solov2_head.py:293-367) for the set cells
// of all levels at once (include/boxinst/boxinst_hip_bls.h).
//
// The reference loops over the levels and, inside a level, copies the resized image and level-set feature once per set cell before it
// multiplies them with the cell's target.  Here a ROW is one set cell; levels of one output size form a size group with its own (h, w),
// image and target planes, and the rows of all groups are evaluated together.  A WORK ITEM is a chunk of lines of one row, so a row of a
// small group costs what its pixels cost:
//   bls_front_partial_kernel   one pass over the chunk's logits: p = sigmoid(x), the lines' arg-max and target bit, the chunk's column
//                              maxima (64-bit integer maxima in the LDS), the fp64 partial sums of the image level-set energy, the
//                              exact count of target bytes and the line dice sums
//   bls_front_finish_kernel    one workgroup per row: the columns' arg-max over the chunks, both dice terms, the energy, pixel_num
//   bls_backward_kernel        every element of every level's gradient: (g_proj + g_img_levelset + g_p) p (1 - p)
//   bls_high_*_kernel          region_levelset on (p T, (1 - p) T) against (y_img T, y_lst T): box2mask_loss.hip's arithmetic, ragged
// An index outside its range makes a row inert: nothing is read through it, zeros are written.
#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_bls.h"

namespace bxi {

typedef unsigned long long u64;

constexpr int kBlsThreads = 256;
constexpr int kBlsRow = 20;        // doubles per row: S[2] | a[2][3] | R[2][3] | line I, U | column I, U | pixel_num | 0
constexpr int kBlsPart = 18;       // doubles per work item: S[2] | A[2][3] | Q[2][3] | count | line sum(x t), sum(x^2), sum(t)
constexpr int kBlsHigh = 10;       // doubles per row (S[2] | a[2][2] | R[2][2]) and per work item (S[2] | A[2][2] | Q[2][2])

struct BlsGroup {
    const float* img;
    const uint8_t* masks;
    int h, w, rows, G;
    int first_row, lpc, chunks, first_item;      // lpc: lines per chunk; first_item: the group's first (row, chunk) work item
    int pix_base, line_base, col_base, colitem_base;     // the group's first row in the ragged per-pixel / per-line / per-column / per-(item, column) arrays
};
struct BlsTable {
    BlsGroup g[BXI_BLS_MAX_GROUPS];
    float* level[BXI_BLS_MAX_LEVELS];
    int level_rows[BXI_BLS_MAX_LEVELS], level_group[BXI_BLS_MAX_LEVELS];
    int n, L, M, B, items;
};
struct BlsState { double* row; double* part; u64* colkey; int* arg_line; int* arg_col; uint8_t* colt; };

__device__ __forceinline__ float bls_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the group of work item `item` / of row `m` (both wave-uniform): a select over the table, no indexed access to the kernel arguments
__device__ __forceinline__ BlsGroup bls_group_of_item(const BlsTable& t, int item, int& gi) {
    BlsGroup G = t.g[0];
    gi = 0;
#pragma unroll
    for (int k = 1; k < BXI_BLS_MAX_GROUPS; ++k)
        if (k < t.n && item >= t.g[k].first_item) { G = t.g[k]; gi = k; }
    return G;
}
__device__ __forceinline__ BlsGroup bls_group_of_row(const BlsTable& t, int m, int& gi) {
    BlsGroup G = t.g[0];
    gi = 0;
#pragma unroll
    for (int k = 1; k < BXI_BLS_MAX_GROUPS; ++k)
        if (k < t.n && m >= t.g[k].first_row) { G = t.g[k]; gi = k; }
    return G;
}

// the row's logit / gradient plane, or nullptr when row_src names none of group gi
__device__ __forceinline__ float* bls_plane(const BlsTable& t, int src, int gi, int hw) {
    if (src < 0) return nullptr;
    const int lvl = src / BXI_BLS_LEVEL_ROWS, n = src % BXI_BLS_LEVEL_ROWS;
    float* base = nullptr;
#pragma unroll
    for (int l = 0; l < BXI_BLS_MAX_LEVELS; ++l)
        if (l == lvl && l < t.L && t.level_group[l] == gi && n < t.level_rows[l]) base = t.level[l];
    return base ? base + (int64_t)n * hw : nullptr;
}

__device__ __forceinline__ void bls_lines(const BlsGroup& G, int c, int& y0, int& y1) {
    y0 = c * G.lpc;
    y1 = y0 + G.lpc < G.h ? y0 + G.lpc : G.h;
}

// ---------------------------------------------------------------------------------------------------
// grid (work items): the chunk's lines, a wave per line.
__global__ __launch_bounds__(kBlsThreads) void bls_front_partial_kernel(BlsTable t, const int* __restrict__ row_src, const int* __restrict__ tgt_of,
                                                                        const int* __restrict__ img_of, float* __restrict__ p, BlsState st) {
    __shared__ u64 s_key[BXI_BLS_MAX_W];
    __shared__ int s_t[BXI_BLS_MAX_W];
    __shared__ double s_red[kBlsThreads / 64][kBlsPart];
    const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int gi;
    const BlsGroup G = bls_group_of_item(t, item, gi);
    const int r = (item - G.first_item) / G.chunks, c = (item - G.first_item) % G.chunks, m = G.first_row + r;
    const int h = G.h, w = G.w, hw = h * w;
    int y0, y1;
    bls_lines(G, c, y0, y1);
    const int tg = tgt_of[m], im = img_of[m];
    const float* X = bls_plane(t, row_src[m], gi, hw);
    const bool live = X != nullptr && tg >= 0 && tg < G.G && im >= 0 && im < t.B;
    const uint8_t* T = G.masks + (int64_t)(live ? tg : 0) * hw;
    const float* I = G.img + (int64_t)(live ? im : 0) * 3 * hw;
    float* P = p + (int64_t)G.pix_base + (int64_t)r * hw;
    for (int x = tid; x < w; x += kBlsThreads) { s_key[x] = 0; s_t[x] = 0; }
    __syncthreads();
    double v[kBlsPart];
#pragma unroll
    for (int k = 0; k < kBlsPart; ++k) v[k] = 0.0;
    for (int y = y0 + wave; y < y1; y += kBlsThreads / 64) {
        u64 best = 0;
        int any = 0;
        for (int x = lane; x < w; x += 64) {
            const int idx = y * w + x;
            float pv = 0.f;
            if (live) {
                const float xv = X[idx];
                const int tb = T[idx] != 0;
                const float i0 = I[idx], i1 = I[hw + idx], i2 = I[2 * hw + idx];
                pv = bls_sigmoid(xv);
                const u64 kx = pack_max(xv, (uint32_t)x);
                best = kx > best ? kx : best;
                any |= tb;
                atomicMax(&s_key[x], pack_max(xv, (uint32_t)y));          // integer maximum: the order cannot matter
                if (tb) atomicOr(&s_t[x], 1);
                const float tv = tb ? 1.f : 0.f;
                const float f = pv * tv, g = (1.f - pv) * tv;             // rounded to fp32, as the reference's stored tensors are
                const float tt[3] = {i0 * tv, i1 * tv, i2 * tv};
                v[0] += (double)f; v[1] += (double)g; v[14] += (double)tv;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double fd = f, gd = g, td = tt[ch];
                    v[2 + ch] += fd * td; v[5 + ch] += gd * td;
                    v[8 + ch] += fd * td * td; v[11 + ch] += gd * td * td;
                }
            }
            P[idx] = pv;
        }
        best = wave_max_u64(best);
        const int line_t = __ballot(any) != 0 ? 1 : 0;
        if (lane == 0) {
            const uint32_t ux = unpack_idx(best);
            const int ax = ux > (uint32_t)(w - 1) ? w - 1 : (int)ux;      // (a line of NaN)
            st.arg_line[G.line_base + r * h + y] = live ? ((ax << 1) | line_t) : 0;
            if (live) {
                const double pm = (double)bls_sigmoid(unpack_val(best));
                v[15] += pm * line_t; v[16] += pm * pm; v[17] += (double)line_t;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kBlsPart; ++k) {
        const double s = wave_total_f64(v[k]);
        if (lane == 0) s_red[wave][k] = s;
    }
    __syncthreads();
    if (tid < kBlsPart) st.part[(int64_t)item * kBlsPart + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];      // fixed order
    const int64_t cb = (int64_t)G.colitem_base + ((int64_t)r * G.chunks + c) * w;
    for (int x = tid; x < w; x += kBlsThreads) { st.colkey[cb + x] = s_key[x]; st.colt[cb + x] = (uint8_t)s_t[x]; }
}

// grid (M): the chunks combined in index order
__global__ __launch_bounds__(kBlsThreads) void bls_front_finish_kernel(BlsTable t, const int* __restrict__ row_src, const int* __restrict__ tgt_of,
                                                                       const int* __restrict__ img_of, double w_proj, double w_img,
                                                                       float* __restrict__ loss_proj, float* __restrict__ loss_img,
                                                                       float* __restrict__ pixel_num, float* __restrict__ live_out, BlsState st) {
    __shared__ double red[16];
    const int m = blockIdx.x, tid = threadIdx.x;
    int gi;
    const BlsGroup G = bls_group_of_row(t, m, gi);
    const int r = m - G.first_row, h = G.h, w = G.w;
    const int tg = tgt_of[m], im = img_of[m];
    const bool live = bls_plane(t, row_src[m], gi, h * w) != nullptr && tg >= 0 && tg < G.G && im >= 0 && im < t.B;
    const int64_t cb = (int64_t)G.colitem_base + (int64_t)r * G.chunks * w;
    double cI = 0.0, cX = 0.0, cT = 0.0;
    for (int x = tid; x < w; x += kBlsThreads) {
        u64 key = 0;
        int tt = 0;
        for (int c = 0; c < G.chunks; ++c) {
            const u64 k = st.colkey[cb + (int64_t)c * w + x];
            key = k > key ? k : key;
            tt |= st.colt[cb + (int64_t)c * w + x];
        }
        const uint32_t uy = unpack_idx(key);
        const int ay = uy > (uint32_t)(h - 1) ? h - 1 : (int)uy;
        st.arg_col[G.col_base + r * w + x] = live ? ((ay << 1) | (tt & 1)) : 0;
        if (live) {
            const double pm = (double)bls_sigmoid(unpack_val(key));
            cI += pm * (tt & 1); cX += pm * pm; cT += (double)(tt & 1);
        }
    }
    cI = block_sum_seq_f64(cI, red);
    cX = block_sum_seq_f64(cX, red);
    cT = block_sum_seq_f64(cT, red);
    if (tid != 0) return;
    double* row = st.row + (int64_t)m * kBlsRow;
    if (!live) {
        for (int k = 0; k < kBlsRow; ++k) row[k] = 0.0;
        loss_proj[m] = 0.f; loss_img[m] = 0.f; pixel_num[m] = 1.f; live_out[m] = 0.f;
        return;
    }
    double s[kBlsPart];
    for (int k = 0; k < kBlsPart; ++k) s[k] = 0.0;
    const double* part = st.part + ((int64_t)G.first_item + (int64_t)r * G.chunks) * kBlsPart;
    for (int c = 0; c < G.chunks; ++c)
        for (int k = 0; k < kBlsPart; ++k) s[k] += part[c * kBlsPart + k];
    const double pn = s[14] > 1.0 ? s[14] : 1.0;                          // torch.clamp(pixel_num, min=1)
    const double lU = s[16] + s[17] + 1e-5, cU = cX + cT + 1e-5;
    loss_proj[m] = (float)(w_proj * ((1.0 - 2.0 * cI / cU) + (1.0 - 2.0 * s[15] / lU)));
    double total = 0.0;
    for (int side = 0; side < 2; ++side) {
        const double S = s[side], sc = S > 1e-5 ? S : 1e-5;                 // .clamp(min=0.00001)
        row[side] = S;
        for (int ch = 0; ch < 3; ++ch) {
            const double a_sum = s[2 + side * 3 + ch], q_sum = s[8 + side * 3 + ch];
            const double a = a_sum / sc;
            total += q_sum - 2.0 * a * a_sum + a * a * S;
            row[2 + side * 3 + ch] = a; row[8 + side * 3 + ch] = a_sum - a * S;
        }
    }
    row[14] = s[15]; row[15] = lU; row[16] = cI; row[17] = cU; row[18] = pn; row[19] = 0.0;
    loss_img[m] = (float)(w_img * total / (3.0 * pn));
    pixel_num[m] = (float)pn;
    live_out[m] = 1.f;
}

// grid (work items): every element of the row's plane of its level's gradient
__global__ __launch_bounds__(kBlsThreads) void bls_backward_kernel(BlsTable t, const int* __restrict__ row_src, const int* __restrict__ tgt_of,
                                                                   const int* __restrict__ img_of, double w_proj, double w_img,
                                                                   const float* __restrict__ p, const float* __restrict__ g_p,
                                                                   const float* __restrict__ g_loss_proj, const float* __restrict__ g_loss_img, BlsState st) {
    const int item = blockIdx.x, tid = threadIdx.x;
    int gi;
    const BlsGroup G = bls_group_of_item(t, item, gi);
    const int r = (item - G.first_item) / G.chunks, c = (item - G.first_item) % G.chunks, m = G.first_row + r;
    const int h = G.h, w = G.w, hw = h * w;
    int y0, y1;
    bls_lines(G, c, y0, y1);
    float* out = bls_plane(t, row_src[m], gi, hw);
    if (!out) return;                                                     // no plane to write (the header's precondition)
    const int tg = tgt_of[m], im = img_of[m];
    const bool live = tg >= 0 && tg < G.G && im >= 0 && im < t.B;
    const int lo = y0 * w, hi = y1 * w;
    if (!live) {
        for (int i = lo + tid; i < hi; i += kBlsThreads) out[i] = 0.f;
        return;
    }
    const double* row = st.row + (int64_t)m * kBlsRow;
    const double pn = row[18];
    const double wgt = (double)g_loss_img[m] * w_img / (3.0 * pn), gpj = (double)g_loss_proj[m] * w_proj;
    const double lI = row[14], lU = row[15], cI = row[16], cU = row[17];
    double a[2][3], R[2][3], a0[2][3], inv[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double S = row[side], sc = S > 1e-5 ? S : 1e-5;
        inv[side] = 1.0 / sc;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            a[side][ch] = row[2 + side * 3 + ch];
            R[side][ch] = row[8 + side * 3 + ch];
            a0[side][ch] = S >= 1e-5 ? a[side][ch] : 0.0;
        }
    }
    const uint8_t* T = G.masks + (int64_t)tg * hw;
    const float* I = G.img + (int64_t)im * 3 * hw;
    const int64_t pb = (int64_t)G.pix_base + (int64_t)r * hw;
    const int* al = st.arg_line + G.line_base + r * h;
    const int* ac = st.arg_col + G.col_base + r * w;
    for (int i = lo + tid; i < hi; i += kBlsThreads) {
        const int y = i / w, x = i - y * w;
        const float pv = p[pb + i];
        double g = (double)g_p[pb + i];
        if (T[i] != 0) {                                                   // T = 1: f = p, g = 1 - p, t = img
            double gm[2];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                double acc = 0.0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double tt = (double)I[ch * hw + i];
                    const double d = tt - a[side][ch];
                    acc += d * d - 2.0 * R[side][ch] * (tt - a0[side][ch]) * inv[side];
                }
                gm[side] = acc;
            }
            g += wgt * (gm[0] - gm[1]);
        }
        const int lv = al[y], cv = ac[x];
        if ((lv >> 1) == x) g += gpj * (-2.0 * (double)(lv & 1) / lU + 4.0 * lI * (double)pv / (lU * lU));
        if ((cv >> 1) == y) g += gpj * (-2.0 * (double)(cv & 1) / cU + 4.0 * cI * (double)pv / (cU * cU));
        out[i] = (float)(g * (double)(pv * (1.f - pv)));
    }
}

// ---------------------------------------------------------------------------------------------------
// region_levelset on the rows' own two-channel target (y_img T, y_lst T): the layout and the arithmetic of box2mask_loss.hip's
// b2m_ls_*_kernel with shared == 0 and C = 2, over the ragged rows.  state: row [M][10] | part [items][10].
__device__ __forceinline__ bool bls_high_live(const BlsGroup& G, const int* __restrict__ tgt_of, const float* __restrict__ live, int m, int& tg) {
    tg = tgt_of[m];
    return live[m] != 0.f && tg >= 0 && tg < G.G;
}

__global__ __launch_bounds__(kBlsThreads) void bls_high_partial_kernel(BlsTable t, const float* __restrict__ p, const float* __restrict__ y_img,
                                                                       const float* __restrict__ y_lst, const int* __restrict__ tgt_of,
                                                                       const float* __restrict__ live_in, double* __restrict__ state) {
    __shared__ double s_red[kBlsThreads / 64][kBlsHigh];
    const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int gi;
    const BlsGroup G = bls_group_of_item(t, item, gi);
    const int r = (item - G.first_item) / G.chunks, c = (item - G.first_item) % G.chunks, m = G.first_row + r;
    const int w = G.w, hw = G.h * w;
    int y0, y1, tg;
    bls_lines(G, c, y0, y1);
    const bool live = bls_high_live(G, tgt_of, live_in, m, tg);
    double v[kBlsHigh];
#pragma unroll
    for (int k = 0; k < kBlsHigh; ++k) v[k] = 0.0;
    if (live) {
        const uint8_t* T = G.masks + (int64_t)tg * hw;
        const int64_t pb = (int64_t)G.pix_base + (int64_t)r * hw;
        for (int i = y0 * w + tid; i < y1 * w; i += kBlsThreads) {
            if (T[i] == 0) continue;                                       // f = g = 0: nothing is added
            const float pv = p[pb + i];
            const double f = pv, g = 1.f - pv;
            const double tt[2] = {(double)y_img[pb + i], (double)y_lst[pb + i]};
            v[0] += f; v[1] += g;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                v[2 + ch] += f * tt[ch]; v[4 + ch] += g * tt[ch];
                v[6 + ch] += f * tt[ch] * tt[ch]; v[8 + ch] += g * tt[ch] * tt[ch];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kBlsHigh; ++k) {
        const double s = wave_total_f64(v[k]);
        if (lane == 0) s_red[wave][k] = s;
    }
    __syncthreads();
    if (tid < kBlsHigh)
        state[((int64_t)t.M + item) * kBlsHigh + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// one thread per row
__global__ __launch_bounds__(64) void bls_high_finish_kernel(BlsTable t, const int* __restrict__ tgt_of, const float* __restrict__ live_in,
                                                             const float* __restrict__ pixel_num, double weight, float* __restrict__ loss,
                                                             double* __restrict__ state) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= t.M) return;
    BlsGroup G = t.g[0];
#pragma unroll
    for (int k = 1; k < BXI_BLS_MAX_GROUPS; ++k)
        if (k < t.n && m >= t.g[k].first_row) G = t.g[k];
    double* row = state + (int64_t)m * kBlsHigh;
    int tg;
    if (!bls_high_live(G, tgt_of, live_in, m, tg)) {
        for (int k = 0; k < kBlsHigh; ++k) row[k] = 0.0;
        loss[m] = 0.f;
        return;
    }
    const double* part = state + ((int64_t)t.M + G.first_item + (int64_t)(m - G.first_row) * G.chunks) * kBlsHigh;
    double total = 0.0;
    for (int side = 0; side < 2; ++side) {
        double S = 0.0;
        for (int c = 0; c < G.chunks; ++c) S += part[c * kBlsHigh + side];
        const double sc = S > 1e-5 ? S : 1e-5;
        row[side] = S;
        for (int ch = 0; ch < 2; ++ch) {
            double a_sum = 0.0, q_sum = 0.0;
            for (int c = 0; c < G.chunks; ++c) { a_sum += part[c * kBlsHigh + 2 + side * 2 + ch]; q_sum += part[c * kBlsHigh + 6 + side * 2 + ch]; }
            const double a = a_sum / sc;
            total += q_sum - 2.0 * a * a_sum + a * a * S;
            row[2 + side * 2 + ch] = a; row[6 + side * 2 + ch] = a_sum - a * S;
        }
    }
    loss[m] = (float)(weight * total / (2.0 * (double)pixel_num[m]));
}

__global__ __launch_bounds__(kBlsThreads) void bls_high_bwd_kernel(BlsTable t, const float* __restrict__ p, const float* __restrict__ y_img,
                                                                   const float* __restrict__ y_lst, const int* __restrict__ tgt_of,
                                                                   const float* __restrict__ live_in, const float* __restrict__ pixel_num, double weight,
                                                                   const double* __restrict__ state, const float* __restrict__ g_loss,
                                                                   float* __restrict__ g_p, float* __restrict__ g_yi, float* __restrict__ g_yl) {
    const int item = blockIdx.x, tid = threadIdx.x;
    int gi;
    const BlsGroup G = bls_group_of_item(t, item, gi);
    const int r = (item - G.first_item) / G.chunks, c = (item - G.first_item) % G.chunks, m = G.first_row + r;
    const int w = G.w, hw = G.h * w;
    int y0, y1, tg;
    bls_lines(G, c, y0, y1);
    const bool live = bls_high_live(G, tgt_of, live_in, m, tg);
    const int64_t pb = (int64_t)G.pix_base + (int64_t)r * hw;
    const int lo = y0 * w, hi = y1 * w;
    if (!live) {
        for (int i = lo + tid; i < hi; i += kBlsThreads) { g_p[pb + i] = 0.f; g_yi[pb + i] = 0.f; g_yl[pb + i] = 0.f; }
        return;
    }
    const double* row = state + (int64_t)m * kBlsHigh;
    const double wgt = (double)g_loss[m] * weight / (2.0 * (double)pixel_num[m]);
    double a[2][2], R[2][2], a0[2][2], inv[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double S = row[side], sc = S > 1e-5 ? S : 1e-5;
        inv[side] = 1.0 / sc;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            a[side][ch] = row[2 + side * 2 + ch];
            R[side][ch] = row[6 + side * 2 + ch];
            a0[side][ch] = S >= 1e-5 ? a[side][ch] : 0.0;
        }
    }
    const uint8_t* T = G.masks + (int64_t)tg * hw;
    for (int i = lo + tid; i < hi; i += kBlsThreads) {
        float gp = 0.f, gy[2] = {0.f, 0.f};
        if (T[i] != 0) {
            const float pv = p[pb + i];
            const double fs[2] = {(double)pv, (double)(1.f - pv)};
            const double tt[2] = {(double)y_img[pb + i], (double)y_lst[pb + i]};
            double gm[2], gt[2] = {0.0, 0.0};
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const double f = fs[side], fi = f * inv[side];
                double acc = 0.0;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const double d = tt[ch] - a[side][ch];
                    acc += d * d - 2.0 * R[side][ch] * (tt[ch] - a0[side][ch]) * inv[side];
                    gt[ch] += 2.0 * d * f - 2.0 * R[side][ch] * fi;
                }
                gm[side] = acc;
            }
            gp = (float)(wgt * (gm[0] - gm[1]));
            gy[0] = (float)(wgt * gt[0]);
            gy[1] = (float)(wgt * gt[1]);
        }
        g_p[pb + i] = gp; g_yi[pb + i] = gy[0]; g_yl[pb + i] = gy[1];
    }
}

// ---------------------------------------------------------------------------------------------------
// The table of a call from the host arrays, with every check that needs no device value.  levels_host may be NULL with L == 0 (the
// level-set pair on the rows' own targets reads no level tensor).
static int bls_table(const bxi_bls_group* groups, int n_groups, float* const* levels, const int* level_rows, const int* level_group, int L,
                     int need /* 0: sizes only, 1: the masks, 2: masks and images */, BlsTable& t) {
    if (n_groups < 1 || L < 0) return BXI_ERR_BAD_SHAPE;
    if (n_groups > BXI_BLS_MAX_GROUPS || L > BXI_BLS_MAX_LEVELS) return BXI_ERR_UNSUPPORTED;
    if (!groups || (L > 0 && (!levels || !level_rows || !level_group))) return BXI_ERR_NULL_POINTER;
    int64_t rows = 0, items = 0, pix = 0, lines = 0, cols = 0, colitems = 0;
    for (int g = 0; g < BXI_BLS_MAX_GROUPS; ++g) {
        BlsGroup& G = t.g[g];
        if (g >= n_groups) { G = BlsGroup{}; G.h = G.w = G.lpc = G.chunks = 1; continue; }
        const bxi_bls_group& s = groups[g];
        if (s.h < 1 || s.w < 1 || s.rows < 0 || s.G < 0) return BXI_ERR_BAD_SHAPE;
        if (s.w > BXI_BLS_MAX_W) return BXI_ERR_UNSUPPORTED;
        if (s.rows > 0 && ((need >= 2 && !s.img) || (need >= 1 && s.G > 0 && !s.masks))) return BXI_ERR_NULL_POINTER;
        if (!fits_i32((int64_t)(s.G > 0 ? s.G : 1) * s.h * s.w)) return BXI_ERR_BAD_SHAPE;
        G.img = s.img; G.masks = s.masks; G.h = s.h; G.w = s.w; G.rows = s.rows; G.G = s.G;
        G.lpc = BXI_BLS_CHUNK_PIXELS / s.w > 1 ? BXI_BLS_CHUNK_PIXELS / s.w : 1;
        G.chunks = (s.h + G.lpc - 1) / G.lpc;
        if (!fits_i32(pix) || !fits_i32(colitems) || !fits_i32(items) || !fits_i32(lines) || !fits_i32(cols)) return BXI_ERR_BAD_SHAPE;
        G.first_row = (int)rows; G.first_item = (int)items; G.pix_base = (int)pix; G.line_base = (int)lines; G.col_base = (int)cols;
        G.colitem_base = (int)colitems;
        rows += s.rows; items += (int64_t)s.rows * G.chunks; pix += (int64_t)s.rows * s.h * s.w; lines += (int64_t)s.rows * s.h;
        cols += (int64_t)s.rows * s.w; colitems += (int64_t)s.rows * G.chunks * s.w;
    }
    if (rows > 65535) return BXI_ERR_UNSUPPORTED;
    if (!fits_i32(pix) || !fits_i32(colitems) || !fits_i32(items)) return BXI_ERR_BAD_SHAPE;
    int64_t planes[BXI_BLS_MAX_GROUPS] = {0, 0, 0, 0};
    for (int l = 0; l < BXI_BLS_MAX_LEVELS; ++l) {
        t.level[l] = nullptr; t.level_rows[l] = 0; t.level_group[l] = 0;
        if (l >= L) continue;
        if (level_rows[l] < 0 || level_group[l] < 0 || level_group[l] >= n_groups) return BXI_ERR_BAD_SHAPE;
        if (level_rows[l] >= BXI_BLS_LEVEL_ROWS) return BXI_ERR_UNSUPPORTED;
        if (level_rows[l] > 0 && !levels[l]) return BXI_ERR_NULL_POINTER;
        t.level[l] = levels[l]; t.level_rows[l] = level_rows[l]; t.level_group[l] = level_group[l];
        planes[level_group[l]] += level_rows[l];
    }
    if (L > 0)
        for (int g = 0; g < n_groups; ++g)
            if (planes[g] != groups[g].rows) return BXI_ERR_BAD_SHAPE;     // the rows of a group are the planes of its levels
    t.n = n_groups; t.L = L; t.M = (int)rows; t.B = 0; t.items = (int)items;
    return BXI_OK;
}

static size_t bls_state(const BlsTable& t, void* base, BlsState& st) {
    const BlsGroup& last = t.g[t.n - 1];
    const size_t lines = (size_t)last.line_base + (size_t)last.rows * last.h, cols = (size_t)last.col_base + (size_t)last.rows * last.w;
    const size_t colitems = (size_t)last.colitem_base + (size_t)last.rows * last.chunks * last.w;
    Carver cv(base, 8);
    st.row = cv.take<double>((size_t)t.M * kBlsRow);
    st.part = cv.take<double>((size_t)t.items * kBlsPart);
    st.colkey = cv.take<u64>(colitems);
    st.arg_line = cv.take<int>(lines);
    st.arg_col = cv.take<int>(cols);
    st.colt = cv.take<uint8_t>(colitems);
    return cv.bytes() > 8 ? cv.bytes() : 8;
}

static size_t bls_high_state(const BlsTable& t) {
    const size_t n = sizeof(double) * kBlsHigh * ((size_t)t.M + (size_t)t.items);
    return n ? n : 8;
}

}  // namespace bxi

extern "C" {

size_t bxi_bls_state_bytes(const bxi_bls_group* groups_host, int n_groups) {
    bxi::BlsTable t;
    if (bxi::bls_table(groups_host, n_groups, nullptr, nullptr, nullptr, 0, 0, t) != BXI_OK) return 0;
    bxi::BlsState st;
    return bxi::bls_state(t, nullptr, st);
}

int bxi_bls_front_f32(const bxi_bls_group* groups_host, int n_groups, const float* const* levels_host, const int* level_rows_host,
                      const int* level_group_host, int L, const int32_t* row_src, const int32_t* tgt_of, const int32_t* img_of, int M, int B,
                      double w_proj, double w_img, float* p, float* loss_proj, float* loss_img, float* pixel_num, float* live, void* state,
                      size_t state_bytes, void* stream) {
    if (L < 1 || M < 0 || B < 0) return BXI_ERR_BAD_SHAPE;
    bxi::BlsTable t;
    int rc = bxi::bls_table(groups_host, n_groups, const_cast<float* const*>(levels_host), level_rows_host, level_group_host, L, 2, t);
    if (rc != BXI_OK) return rc;
    if (M != t.M) return BXI_ERR_BAD_SHAPE;
    if (M == 0) return BXI_OK;
    if (!row_src || !tgt_of || !img_of || !p || !loss_proj || !loss_img || !pixel_num || !live) return BXI_ERR_NULL_POINTER;
    bxi::BlsState st;
    if (!bxi::workspace_ok(state, state_bytes, bxi::bls_state(t, nullptr, st), 8)) return BXI_ERR_WORKSPACE;
    bxi::bls_state(t, state, st);
    t.B = B;
    hipStream_t s = bxi::as_stream(stream);
    BXI_LAUNCH("bls_front_partial", s, bxi::bls_front_partial_kernel, dim3(t.items), dim3(bxi::kBlsThreads), 0, s, t, row_src, tgt_of, img_of, p, st);
    rc = bxi::check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("bls_front_finish", s, bxi::bls_front_finish_kernel, dim3(M), dim3(bxi::kBlsThreads), 0, s, t, row_src, tgt_of, img_of, w_proj, w_img,
               loss_proj, loss_img, pixel_num, live, st);
    return bxi::check_launch();
}

int bxi_bls_backward_f32(const bxi_bls_group* groups_host, int n_groups, float* const* grads_host, const int* level_rows_host,
                         const int* level_group_host, int L, const int32_t* row_src, const int32_t* tgt_of, const int32_t* img_of, int M, int B,
                         double w_proj, double w_img, const float* p, const float* g_p, const float* g_loss_proj, const float* g_loss_img,
                         const void* state, size_t state_bytes, void* stream) {
    if (L < 1 || M < 0 || B < 0) return BXI_ERR_BAD_SHAPE;
    bxi::BlsTable t;
    int rc = bxi::bls_table(groups_host, n_groups, grads_host, level_rows_host, level_group_host, L, 2, t);
    if (rc != BXI_OK) return rc;
    if (M != t.M) return BXI_ERR_BAD_SHAPE;
    if (M == 0) return BXI_OK;
    if (!row_src || !tgt_of || !img_of || !p || !g_p || !g_loss_proj || !g_loss_img) return BXI_ERR_NULL_POINTER;
    bxi::BlsState st;
    if (!bxi::workspace_ok(state, state_bytes, bxi::bls_state(t, nullptr, st), 8)) return BXI_ERR_WORKSPACE;
    bxi::bls_state(t, const_cast<void*>(state), st);
    t.B = B;
    hipStream_t s = bxi::as_stream(stream);
    BXI_LAUNCH("bls_backward", s, bxi::bls_backward_kernel, dim3(t.items), dim3(bxi::kBlsThreads), 0, s, t, row_src, tgt_of, img_of, w_proj, w_img, p, g_p,
               g_loss_proj, g_loss_img, st);
    return bxi::check_launch();
}

size_t bxi_bls_high_state_bytes(const bxi_bls_group* groups_host, int n_groups) {
    bxi::BlsTable t;
    if (bxi::bls_table(groups_host, n_groups, nullptr, nullptr, nullptr, 0, 0, t) != BXI_OK) return 0;
    return bxi::bls_high_state(t);
}

int bxi_bls_high_forward_f32(const bxi_bls_group* groups_host, int n_groups, const float* p, const float* y_img, const float* y_lst,
                             const int32_t* tgt_of, const float* live, const float* pixel_num, int M, double weight, float* loss, void* state,
                             size_t state_bytes, void* stream) {
    if (M < 0) return BXI_ERR_BAD_SHAPE;
    bxi::BlsTable t;
    int rc = bxi::bls_table(groups_host, n_groups, nullptr, nullptr, nullptr, 0, 1, t);
    if (rc != BXI_OK) return rc;
    if (M != t.M) return BXI_ERR_BAD_SHAPE;
    if (M == 0) return BXI_OK;
    if (!p || !y_img || !y_lst || !tgt_of || !live || !pixel_num || !loss) return BXI_ERR_NULL_POINTER;
    if (!bxi::workspace_ok(state, state_bytes, bxi::bls_high_state(t), 8)) return BXI_ERR_WORKSPACE;
    hipStream_t s = bxi::as_stream(stream);
    double* sd = reinterpret_cast<double*>(state);
    BXI_LAUNCH("bls_high_partial", s, bxi::bls_high_partial_kernel, dim3(t.items), dim3(bxi::kBlsThreads), 0, s, t, p, y_img, y_lst, tgt_of, live, sd);
    rc = bxi::check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("bls_high_finish", s, bxi::bls_high_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, s, t, tgt_of, live, pixel_num, weight, loss, sd);
    return bxi::check_launch();
}

int bxi_bls_high_backward_f32(const bxi_bls_group* groups_host, int n_groups, const float* p, const float* y_img, const float* y_lst,
                              const int32_t* tgt_of, const float* live, const float* pixel_num, int M, double weight, const void* state,
                              size_t state_bytes, const float* g_loss, float* g_p, float* g_y_img, float* g_y_lst, void* stream) {
    if (M < 0) return BXI_ERR_BAD_SHAPE;
    bxi::BlsTable t;
    int rc = bxi::bls_table(groups_host, n_groups, nullptr, nullptr, nullptr, 0, 1, t);
    if (rc != BXI_OK) return rc;
    if (M != t.M) return BXI_ERR_BAD_SHAPE;
    if (M == 0) return BXI_OK;
    if (!p || !y_img || !y_lst || !tgt_of || !live || !pixel_num || !g_loss || !g_p || !g_y_img || !g_y_lst) return BXI_ERR_NULL_POINTER;
    if (!bxi::workspace_ok(state, state_bytes, bxi::bls_high_state(t), 8)) return BXI_ERR_WORKSPACE;
    hipStream_t s = bxi::as_stream(stream);
    BXI_LAUNCH("bls_high_bwd", s, bxi::bls_high_bwd_kernel, dim3(t.items), dim3(bxi::kBlsThreads), 0, s, t, p, y_img, y_lst, tgt_of, live, pixel_num, weight,
               reinterpret_cast<const double*>(state), g_loss, g_p, g_y_img, g_y_lst);
    return bxi::check_launch();
}

}  // extern "C"
