// box2mask_loss.hip -- the mask losses of Box2MaskHead.loss (mmdet/models/dense_heads/box2mask_head.py:260-335) for the matched rows
// of all decoder layers at once (include/boxinst/boxinst_hip_b2m.h).
//
// The reference runs loss_single once per layer and, inside it, copies the image, the level-set feature, both trees and the box
// targets once per matched instance before it multiplies them together.  Here a ROW is one matched (layer, image, query); the rows of
// all layers are evaluated together and everything that belongs to an image or to a ground truth is read through an index array:
//   b2m_scores_kernel        sigmoid of the gathered logit planes and their small-grid bilinear resize, one pass
//   b2m_scores_bwd_kernel    the whole gradient of one layer's logits: matched planes (gather-form adjoint of the resize), zeros elsewhere
//   b2m_ls_*_kernel          region_levelset on (p T, (1 - p) T) against target * T, T = T_all[tgt_of[m]]; the arithmetic of levelset.hip
//   bxi_b2m_lcm_refine_f32   levelset.hip's LCM kernels with the affinity read through img_of (lcm_device.hpp)
// An index outside its range makes a row inert: nothing is read through it, zeros are written.
#include "common.hpp"
#include "lcm_device.hpp"
#include "../../include/boxinst/boxinst_hip_b2m.h"

namespace bxi {

struct B2mLayers { const float* p[BXI_B2M_MAX_LAYERS]; };

// One axis of F.interpolate(mode='bilinear', align_corners=False): source index scale * (o + 0.5) - 0.5 clamped at 0, taps i0 and
// i1 = min(i0 + 1, n - 1), weights 1 - l1 and l1 (UpSample.h: area_pixel_compute_source_index, upsample_bilinear2d).  The index is taken in
// double: in float its fraction carries an absolute error of an ulp of the INDEX (1.5e-5 at index 200), which torch's own kernels differ by
// among themselves; the weights here are the correctly rounded ones.  BOTH of them: 1.f - l1 carries l1's absolute error of up to 2^-25
// into a weight that may itself be small (1/24 at 200 -> 96: twelve times the relative error of one rounding, which the adjoint's elements
// with a single tap show in full), so l0 is rounded from the double as well.
__device__ __forceinline__ void b2m_axis(int o, double scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
    double src = scale * ((double)o + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    const double frac = src - (double)i0;
    l1 = (float)frac;
    l0 = (float)(1.0 - frac);
}

__device__ __forceinline__ float b2m_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// grid (chunks, M): the row's h*w scores, then its sh*sw small-grid pixels, each from the four taps' logits.  VEC: h*w a multiple of 4 and
// every layer tensor and p 16-byte aligned (host check), so the scores go four to a thread as float4.
template <bool VEC>
__global__ __launch_bounds__(256) void b2m_scores_kernel(B2mLayers layers, int L, int planes, int h, int w, const int* __restrict__ row_plane,
                                                         int sh, int sw, double sy, double sx, float* __restrict__ p, float* __restrict__ ps) {
    const int m = blockIdx.y, hw = h * w, shw = sh * sw;
    const int rp = row_plane[m];
    const bool live = rp >= 0 && rp / planes < L;
    const float* src = nullptr;
    if (live) { const int l = rp / planes; src = layers.p[l] + (int64_t)(rp - l * planes) * hw; }
    float* pm = p + (int64_t)m * hw;
    float* qm = ps + (int64_t)m * shw;
    const int n_p = VEC ? hw / 4 : hw;                    // work items of the scores
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_p + shw; i += gridDim.x * 256) {
        if (i < n_p) {
            if (VEC) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) {
                    const float4 x = reinterpret_cast<const float4*>(src)[i];
                    v = make_float4(b2m_sigmoid(x.x), b2m_sigmoid(x.y), b2m_sigmoid(x.z), b2m_sigmoid(x.w));
                }
                reinterpret_cast<float4*>(pm)[i] = v;
            } else {
                pm[i] = live ? b2m_sigmoid(src[i]) : 0.f;
            }
        } else {
            const int j = i - n_p, oy = j / sw, ox = j % sw;
            float v = 0.f;
            if (live) {
                int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
                b2m_axis(oy, sy, h, y0, y1, ly0, ly1);
                b2m_axis(ox, sx, w, x0, x1, lx0, lx1);
                const float v00 = b2m_sigmoid(src[y0 * w + x0]), v01 = b2m_sigmoid(src[y0 * w + x1]);
                const float v10 = b2m_sigmoid(src[y1 * w + x0]), v11 = b2m_sigmoid(src[y1 * w + x1]);
                v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
            }
            qm[j] = v;
        }
    }
}

// The small-grid positions o in [lo, hi] that may have element i of an axis among their two taps: the source index of o lies in
// (i - 1, i + 1), i.e. o in ((i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5), widened by one position on either side against the
// rounding of this estimate; every candidate is then tested with the forward's own arithmetic (b2m_axis), so the set is exact.
__device__ __forceinline__ void b2m_candidates(int i, double scale, int n_out, int& lo, int& hi) {
    const float inv = (float)(1.0 / scale);
    lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
    hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
    if (i == 0) lo = 0;                                  // every position whose source index was clamped to 0
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_out - 1 ? n_out - 1 : hi;
}

// grid (chunks, planes): one layer's whole gradient
__global__ __launch_bounds__(256) void b2m_scores_bwd_kernel(const float* __restrict__ g_p, const float* __restrict__ g_ps, const float* __restrict__ p,
                                                             const int* __restrict__ plane_row, int M, int h, int w, int sh, int sw, double sy,
                                                             double sx, float* __restrict__ g_logits) {
    const int plane = blockIdx.y, hw = h * w, shw = sh * sw;
    const int row = plane_row[plane];
    const bool live = row >= 0 && row < M;
    float* out = g_logits + (int64_t)plane * hw;
    const float* gp = g_p + (int64_t)(live ? row : 0) * hw;
    const float* gs = g_ps + (int64_t)(live ? row : 0) * shw;
    const float* pr = p + (int64_t)(live ? row : 0) * hw;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        float g = 0.f;
        if (live) {
            const int y = i / w, x = i % w;
            int ylo, yhi, xlo, xhi;
            b2m_candidates(y, sy, sh, ylo, yhi);
            b2m_candidates(x, sx, sw, xlo, xhi);
            float acc = 0.f;
            for (int oy = ylo; oy <= yhi; ++oy) {
                int y0, y1; float ly0, ly1;
                b2m_axis(oy, sy, h, y0, y1, ly0, ly1);
                const float wy = (y0 == y ? ly0 : 0.f) + (y1 == y ? ly1 : 0.f);
                if (wy == 0.f) continue;
                float line = 0.f;
                for (int ox = xlo; ox <= xhi; ++ox) {
                    int x0, x1; float lx0, lx1;
                    b2m_axis(ox, sx, w, x0, x1, lx0, lx1);
                    const float wx = (x0 == x ? lx0 : 0.f) + (x1 == x ? lx1 : 0.f);
                    if (wx != 0.f) line += wx * gs[oy * sw + ox];
                }
                acc += wy * line;
            }
            const float pv = pr[i];
            g = (gp[i] + acc) * pv * (1.f - pv);
        }
        out[i] = g;
    }
}

// ---------------------------------------------------------------------------------------------------
// region_levelset on the row's scores inside its box.  state per row: S[2] | a[2][C] | R[2][C] (doubles; R = A - a S, zero unless the
// clamp of levelset_loss.py:34-35 is active), followed (after all rows) by the slices' partial sums [M][kB2mSlices][2 + 4C] =
// S[2] | A[2][C] | Q[2][C] -- the layout and the arithmetic of levelset.hip, with f = p T, g = (1 - p) T and t = target T formed in fp32
// as the reference's tensors are.
constexpr int kB2mSlices = 8;
constexpr int kB2mLsThreads = 512;
__host__ __device__ __forceinline__ int b2m_ls_stride(int C) { return 2 + 4 * C; }

// the row's ground truth and image, or false for an inert row
__device__ __forceinline__ bool b2m_row(const int* __restrict__ tgt_of, const int* __restrict__ img_of, bool shared, int m, int G, int B, int& tg,
                                        int& im) {
    tg = tgt_of[m];
    im = shared ? img_of[m] : m;
    return tg >= 0 && tg < G && (!shared || (im >= 0 && im < B));
}

template <bool SHARED>
__global__ __launch_bounds__(kB2mLsThreads) void b2m_ls_partial_kernel(const float* __restrict__ p, const float* __restrict__ T_all,
                                                                       const float* __restrict__ target, const int* __restrict__ tgt_of,
                                                                       const int* __restrict__ img_of, int M, int G, int B, int C, int H, int W,
                                                                       double* __restrict__ state) {
    __shared__ double red[(kB2mLsThreads / 64) * (2 + 4 * BXI_B2M_MAX_C)];
    const int n = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    const int64_t chunk = ((HW + kB2mSlices - 1) / kB2mSlices + 3) & ~(int64_t)3;
    int tg, im;
    const bool live = b2m_row(tgt_of, img_of, SHARED, n, G, B, tg, im);
    const int64_t lo = sl * chunk, hi = !live ? lo : (lo + chunk < HW ? lo + chunk : HW);
    const float* P = p + (int64_t)n * HW;
    const float* Tm = T_all + (int64_t)(live ? tg : 0) * HW;
    const float* X = target + (int64_t)(live ? im : 0) * C * HW;
    double S[2] = {0.0, 0.0}, A[2][BXI_B2M_MAX_C], Q[2][BXI_B2M_MAX_C];
#pragma unroll
    for (int c = 0; c < BXI_B2M_MAX_C; ++c) { A[0][c] = A[1][c] = Q[0][c] = Q[1][c] = 0.0; }
    for (int64_t p0 = lo + tid; p0 < hi; p0 += 4 * kB2mLsThreads) {      // 4 pixels per trip: their loads are independent
        // unconditional loads at a clamped index; a pixel past the end gets zero scores, which add nothing to any sum
        float fv[4], gv[4], tv[4];
        int64_t pc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int64_t q = p0 + u * kB2mLsThreads; pc[u] = q < hi ? q : hi - 1; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { fv[u] = P[pc[u]]; tv[u] = Tm[pc[u]]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float pv = fv[u];
            fv[u] = pv * tv[u]; gv[u] = (1.f - pv) * tv[u];
            if (p0 + u * kB2mLsThreads >= hi) { fv[u] = 0.f; gv[u] = 0.f; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { S[0] += (double)fv[u]; S[1] += (double)gv[u]; }
#pragma unroll
        for (int c = 0; c < BXI_B2M_MAX_C; ++c)
            if (c < C) {
                float xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) xv[u] = X[(int64_t)c * HW + pc[u]] * tv[u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double f = fv[u], g = gv[u], t = xv[u];
                    A[0][c] += f * t; A[1][c] += g * t;
                    Q[0][c] += f * t * t; Q[1][c] += g * t * t;
                }
            }
    }
    double* part = state + (int64_t)M * b2m_ls_stride(C) + ((int64_t)n * kB2mSlices + sl) * b2m_ls_stride(C);
    const int n_sums = b2m_ls_stride(C);
    S[0] = wave_total_f64(S[0]); S[1] = wave_total_f64(S[1]);
#pragma unroll
    for (int c = 0; c < BXI_B2M_MAX_C; ++c)
        if (c < C) {
            A[0][c] = wave_total_f64(A[0][c]); A[1][c] = wave_total_f64(A[1][c]);
            Q[0][c] = wave_total_f64(Q[0][c]); Q[1][c] = wave_total_f64(Q[1][c]);
        }
    if ((tid & 63) == 0) {
        double* r = red + (tid >> 6) * (2 + 4 * BXI_B2M_MAX_C);
        r[0] = S[0]; r[1] = S[1];
#pragma unroll
        for (int c = 0; c < BXI_B2M_MAX_C; ++c)
            if (c < C) {
                r[2 + c] = A[0][c]; r[2 + C + c] = A[1][c];
                r[2 + 2 * C + c] = Q[0][c]; r[2 + 3 * C + c] = Q[1][c];
            }
    }
    __syncthreads();
    if (tid < n_sums) {
        double s = 0.0;
        for (int wv = 0; wv < kB2mLsThreads / 64; ++wv) s += red[wv * (2 + 4 * BXI_B2M_MAX_C) + tid];     // fixed order
        part[tid] = s;
    }
}

// slices summed in index order -> region means, energy, loss; one thread per row
__global__ __launch_bounds__(64) void b2m_ls_finish_kernel(const float* __restrict__ pixel_num, const int* __restrict__ tgt_of,
                                                           const int* __restrict__ img_of, int shared, int M, int G, int B, int C, double weight,
                                                           float* __restrict__ loss, double* __restrict__ state) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= M) return;
    const double* part = state + (int64_t)M * b2m_ls_stride(C) + (int64_t)n * kB2mSlices * b2m_ls_stride(C);
    double* st = state + (int64_t)n * b2m_ls_stride(C);
    int tg, im;
    if (!b2m_row(tgt_of, img_of, shared != 0, n, G, B, tg, im)) {
        for (int k = 0; k < b2m_ls_stride(C); ++k) st[k] = 0.0;
        loss[n] = 0.f;
        return;
    }
    double total = 0.0;
    for (int side = 0; side < 2; ++side) {
        double s = 0.0;
        for (int k = 0; k < kB2mSlices; ++k) s += part[k * b2m_ls_stride(C) + side];
        const double sc = s > 1e-5 ? s : 1e-5;                   // .clamp(min=0.00001)
        st[side] = s;
        for (int c = 0; c < C; ++c) {
            double a_sum = 0.0, q_sum = 0.0;
            for (int k = 0; k < kB2mSlices; ++k) { a_sum += part[k * b2m_ls_stride(C) + 2 + side * C + c]; q_sum += part[k * b2m_ls_stride(C) + 2 + 2 * C + side * C + c]; }
            const double a = a_sum / sc;
            total += q_sum - 2.0 * a * a_sum + a * a * s;
            st[2 + side * C + c] = a; st[2 + 2 * C + side * C + c] = a_sum - a * s;
        }
    }
    loss[n] = (float)(weight * total / ((double)C * (double)pixel_num[tg]));
}

// elementwise from the saved sums (levelset_bwd_kernel), folded through f = p T, g = (1 - p) T, t = x T.  grid (chunks of 1024 pixels, M):
// the row is the workgroup's, so its ground truth, image, weight and saved sums are wave-uniform and fetched once; a thread takes four
// pixels 256 apart (coalesced at any alignment).
template <bool SHARED>
__global__ __launch_bounds__(256) void b2m_ls_bwd_kernel(const float* __restrict__ p, const float* __restrict__ T_all, const float* __restrict__ target,
                                                         const int* __restrict__ tgt_of, const int* __restrict__ img_of,
                                                         const float* __restrict__ pixel_num, int M, int G, int B, int C, int H, int W, double weight,
                                                         const double* __restrict__ state, const float* __restrict__ g_loss,
                                                         float* __restrict__ g_p, float* __restrict__ g_tg) {
    const int HW = H * W, n = blockIdx.y;
    const int q0 = blockIdx.x * 1024 + threadIdx.x;
    int tg, im;
    const bool live = b2m_row(tgt_of, img_of, SHARED, n, G, B, tg, im);
    float* gpn = g_p + (int64_t)n * HW;
    if (!live) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256;
            if (q >= HW) break;
            gpn[q] = 0.f;
            if (g_tg)
                for (int c = 0; c < C; ++c) g_tg[((int64_t)n * C + c) * HW + q] = 0.f;
        }
        return;
    }
    const double* st = state + (int64_t)n * b2m_ls_stride(C);
    const double wgt = (double)g_loss[n] * weight / ((double)C * (double)pixel_num[tg]);
    double a[2][BXI_B2M_MAX_C], R[2][BXI_B2M_MAX_C], inv[2], a0[2][BXI_B2M_MAX_C];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double s = st[side], sc = s > 1e-5 ? s : 1e-5;
        inv[side] = 1.0 / sc;
#pragma unroll
        for (int c = 0; c < BXI_B2M_MAX_C; ++c) {
            a[side][c] = c < C ? st[2 + side * C + c] : 0.0;
            R[side][c] = c < C ? st[2 + 2 * C + side * C + c] : 0.0;
            a0[side][c] = s >= 1e-5 ? a[side][c] : 0.0;
        }
    }
    const float* pn = p + (int64_t)n * HW;
    const float* Tn = T_all + (int64_t)tg * HW;
    const float* Xn = target + (int64_t)im * C * HW;
    float pv[4], Tv[4], xv[4][BXI_B2M_MAX_C];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                          // clamped index: the loads carry no branch
        const int q = q0 + u * 256 < HW ? q0 + u * 256 : HW - 1;
        pv[u] = pn[q]; Tv[u] = Tn[q];
#pragma unroll
        for (int c = 0; c < BXI_B2M_MAX_C; ++c) xv[u][c] = c < C ? Xn[(int64_t)c * HW + q] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = q0 + u * 256;
        if (q >= HW) break;
        const float fs[2] = {pv[u] * Tv[u], (1.f - pv[u]) * Tv[u]};
        double gt[BXI_B2M_MAX_C], gm[2];
#pragma unroll
        for (int c = 0; c < BXI_B2M_MAX_C; ++c) gt[c] = 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const double f = fs[side], fi = f * inv[side];
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < BXI_B2M_MAX_C; ++c)
                if (c < C) {
                    const double t = xv[u][c] * Tv[u];                                     // the fp32 product, as stored by the reference
                    const double d = t - a[side][c];
                    const double da_df = (t - a0[side][c]) * inv[side];
                    acc += d * d - 2.0 * R[side][c] * da_df;
                    gt[c] += 2.0 * d * f - 2.0 * R[side][c] * fi;
                }
            gm[side] = acc;
        }
        gpn[q] = (float)(wgt * (gm[0] - gm[1]) * (double)Tv[u]);
        if (g_tg) {
#pragma unroll
            for (int c = 0; c < BXI_B2M_MAX_C; ++c)
                if (c < C) g_tg[((int64_t)n * C + c) * HW + q] = (float)(wgt * gt[c] * (double)Tv[u]);
        }
    }
}

static int b2m_scores_check(int planes, int M, int h, int w, int sh, int sw) {
    if (planes < 1 || h < 1 || w < 1 || sh < 1 || sw < 1 || M < 0) return BXI_ERR_BAD_SHAPE;
    if ((int64_t)sh > (int64_t)BXI_B2M_MAX_UP * h || (int64_t)sw > (int64_t)BXI_B2M_MAX_UP * w || M > 65535 || planes > 65535) return BXI_ERR_UNSUPPORTED;
    if (!fits_i32((int64_t)h * w + (int64_t)sh * sw) || !fits_i32((int64_t)BXI_B2M_MAX_LAYERS * planes)) return BXI_ERR_UNSUPPORTED;
    return BXI_OK;
}

static int b2m_ls_check(int M, int G, int B, int C, int h, int w) {
    if (M < 0 || G < 0 || B < 0 || C < 1 || h < 1 || w < 1) return BXI_ERR_BAD_SHAPE;
    if (C > BXI_B2M_MAX_C || M > 65535) return BXI_ERR_UNSUPPORTED;
    if (!fits_i32((int64_t)(M > 0 ? M : 1) * h * w * C) || !fits_i32((int64_t)(G > B ? G : B) * h * w * C)) return BXI_ERR_BAD_SHAPE;
    return BXI_OK;
}

}  // namespace bxi

extern "C" {

int bxi_b2m_scores_f32(const float* const* layers_host, int L, int planes, int h, int w, const int32_t* row_plane, int M, int sh, int sw,
                       float* p, float* p_small, void* stream) {
    if (L < 1) return BXI_ERR_BAD_SHAPE;
    int rc = bxi::b2m_scores_check(planes, M, h, w, sh, sw);
    if (rc != BXI_OK) return rc;
    if (L > BXI_B2M_MAX_LAYERS) return BXI_ERR_UNSUPPORTED;
    if (M == 0) return BXI_OK;
    if (!layers_host || !row_plane || !p || !p_small) return BXI_ERR_NULL_POINTER;
    bxi::B2mLayers layers;
    for (int l = 0; l < BXI_B2M_MAX_LAYERS; ++l) {
        layers.p[l] = l < L ? layers_host[l] : nullptr;
        if (l < L && !layers.p[l]) return BXI_ERR_NULL_POINTER;
    }
    hipStream_t s = bxi::as_stream(stream);
    bool vec = (h * w) % 4 == 0 && bxi::aligned(p, 16);
    for (int l = 0; l < L; ++l) vec = vec && bxi::aligned(layers.p[l], 16);
    const int total = (vec ? h * w / 4 : h * w) + sh * sw;
    const unsigned chunks = (unsigned)((total + 1023) / 1024);
    if (vec)
        BXI_LAUNCH("b2m_scores", s, bxi::b2m_scores_kernel<true>, dim3(chunks, M), dim3(256), 0, s, layers, L, planes, h, w, row_plane, sh, sw,
                   (double)h / (double)sh, (double)w / (double)sw, p, p_small);
    else
        BXI_LAUNCH("b2m_scores", s, bxi::b2m_scores_kernel<false>, dim3(chunks, M), dim3(256), 0, s, layers, L, planes, h, w, row_plane, sh, sw,
                   (double)h / (double)sh, (double)w / (double)sw, p, p_small);
    return bxi::check_launch();
}

int bxi_b2m_scores_backward_f32(const float* g_p, const float* g_p_small, const float* p, const int32_t* plane_row, int planes, int M, int h,
                                int w, int sh, int sw, float* g_logits, void* stream) {
    int rc = bxi::b2m_scores_check(planes, M, h, w, sh, sw);
    if (rc != BXI_OK) return rc;
    if (!plane_row || !g_logits || (M > 0 && (!g_p || !g_p_small || !p))) return BXI_ERR_NULL_POINTER;
    hipStream_t s = bxi::as_stream(stream);
    const unsigned chunks = (unsigned)((h * w + 1023) / 1024);
    BXI_LAUNCH("b2m_scores_bwd", s, bxi::b2m_scores_bwd_kernel, dim3(chunks, planes), dim3(256), 0, s, g_p, g_p_small, p, plane_row, M, h, w, sh, sw,
               (double)h / (double)sh, (double)w / (double)sw, g_logits);
    return bxi::check_launch();
}

size_t bxi_b2m_levelset_state_bytes(int M, int C) {
    if (M < 0 || C < 1 || C > BXI_B2M_MAX_C || M > 65535) return 0;
    return sizeof(double) * (size_t)(M > 0 ? M : 1) * (2 + 4 * C) * (1 + bxi::kB2mSlices);
}

int bxi_b2m_levelset_forward_f32(const float* p, const float* T_all, const float* target, int shared, const int32_t* tgt_of,
                                 const int32_t* img_of, const float* pixel_num, int M, int G, int B, int C, int h, int w, float weight,
                                 float* loss, void* state, void* stream) {
    int rc = bxi::b2m_ls_check(M, G, B, C, h, w);
    if (rc != BXI_OK) return rc;
    if (M == 0) return BXI_OK;
    if (!p || !T_all || !target || !tgt_of || !pixel_num || !loss || (shared && !img_of)) return BXI_ERR_NULL_POINTER;
    if (!state || !bxi::aligned(state, 8)) return BXI_ERR_WORKSPACE;
    hipStream_t s = bxi::as_stream(stream);
    if (shared)
        BXI_LAUNCH("b2m_ls_partial", s, bxi::b2m_ls_partial_kernel<true>, dim3(bxi::kB2mSlices, M), dim3(bxi::kB2mLsThreads), 0, s, p, T_all, target,
                   tgt_of, img_of, M, G, B, C, h, w, reinterpret_cast<double*>(state));
    else
        BXI_LAUNCH("b2m_ls_partial", s, bxi::b2m_ls_partial_kernel<false>, dim3(bxi::kB2mSlices, M), dim3(bxi::kB2mLsThreads), 0, s, p, T_all, target,
                   tgt_of, img_of, M, G, B, C, h, w, reinterpret_cast<double*>(state));
    rc = bxi::check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("b2m_ls_finish", s, bxi::b2m_ls_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, s, pixel_num, tgt_of, img_of, shared, M, G, B, C,
               (double)weight, loss, reinterpret_cast<double*>(state));
    return bxi::check_launch();
}

int bxi_b2m_levelset_backward_f32(const float* p, const float* T_all, const float* target, int shared, const int32_t* tgt_of,
                                  const int32_t* img_of, const float* pixel_num, int M, int G, int B, int C, int h, int w, float weight,
                                  const void* state, const float* g_loss, float* g_p, float* g_target, void* stream) {
    int rc = bxi::b2m_ls_check(M, G, B, C, h, w);
    if (rc != BXI_OK) return rc;
    if (shared && g_target) return BXI_ERR_BAD_ARGUMENT;
    if (M == 0) return BXI_OK;
    if (!p || !T_all || !target || !tgt_of || !pixel_num || !g_loss || !g_p || (shared && !img_of)) return BXI_ERR_NULL_POINTER;
    if (!state || !bxi::aligned(state, 8)) return BXI_ERR_WORKSPACE;
    hipStream_t s = bxi::as_stream(stream);
    const unsigned grid = (unsigned)((h * w + 1023) / 1024);
    if (shared)
        BXI_LAUNCH("b2m_ls_bwd", s, bxi::b2m_ls_bwd_kernel<true>, dim3(grid, M), dim3(256), 0, s, p, T_all, target, tgt_of, img_of, pixel_num, M, G, B, C,
                   h, w, (double)weight, reinterpret_cast<const double*>(state), g_loss, g_p, g_target);
    else
        BXI_LAUNCH("b2m_ls_bwd", s, bxi::b2m_ls_bwd_kernel<false>, dim3(grid, M), dim3(256), 0, s, p, T_all, target, tgt_of, img_of, pixel_num, M, G, B, C,
                   h, w, (double)weight, reinterpret_cast<const double*>(state), g_loss, g_p, g_target);
    return bxi::check_launch();
}

int bxi_b2m_lcm_refine_f32(const float* aff, const float* phi, const int32_t* img_of, int B, int M, int h, int w, int dilation, int iters,
                           int transpose, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (M < 0 || B < 0 || h <= 0 || w <= 0 || iters < 0) return BXI_ERR_BAD_SHAPE;
    if (dilation < 1) return BXI_ERR_BAD_ARGUMENT;
    if (M == 0) return BXI_OK;
    if (!aff || !phi || !img_of || !out) return BXI_ERR_NULL_POINTER;
    if (!bxi::fits_i32((int64_t)(M > B ? M : B) * h * w * 8)) return BXI_ERR_BAD_SHAPE;
    return bxi::lcm_refine_launch(aff, phi, img_of, B, M, h, w, dilation, iters, transpose, out, workspace, workspace_bytes, bxi::as_stream(stream));
}

}  // extern "C"
