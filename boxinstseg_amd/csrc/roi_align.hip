// roi_align.hip -- RoIAlign forward / backward and the front of one level of DiscoBox's corr_loss (include/boxinst/boxinst_hip_roi.h).
//
//   roi_target_boxes_kernel    one workgroup per object: the box of its non-zero bytes (16-byte reads between a byte-wise head and tail)
//   roi_labels_kernel          one workgroup: the rank of every kept object, the label it reads
//   roi_forward_kernel         one wave per output element, its lanes over the samples of the bin (adjacent lanes, adjacent columns)
//   roi_feat_norm_forward      one workgroup per (roi, bin): a wave per channel pools, the C pooled values stay in LDS for the norm
//   roi_norm_backward_kernel   one workgroup per (roi, bin): the gradient through f / (n + 1e-6) and the relu
//   roi_backward_kernel        a gather: a thread owns a pixel of 16 channels and adds, in roi order, wy(y) wx(x) g / count of every bin
//
// The arithmetic is the per-sample algorithm restated in the header.  A sample's weight is wy(y) * wx(x) and both the out-of-range rule
// and the border clamp act per axis, so the backward may sum the axis weights of a bin first: no float atomics, a fixed order.
// Every loop over samples is cut to the samples that can reach the canvas (sample_span), so a box far outside costs nothing.
#include "common.hpp"

#include <math.h>

#include "../../include/boxinst/boxinst_hip_roi.h"

namespace bxi {
namespace {

constexpr int kBins = BXI_ROI_FEAT * BXI_ROI_FEAT;
constexpr int kGatherCh = 16;      // channels of one thread of the gather
constexpr float kNormEps = 1e-6f;  // relu_and_l2_norm_feat (:18-19)

struct RoiGeom {
    int b, gh, gw;
    bool ok;
    float xs, ys, rw, rh, bin_w, bin_h, count;
};

__device__ __forceinline__ int to_grid(float v) { return (int)fminf(fmaxf(ceilf(v), 0.f), 1e9f); }

__device__ __forceinline__ RoiGeom roi_geom(const float* __restrict__ r, int B, int PH, int PW, float scale, int sr, int aligned) {
    RoiGeom g;
    const float fb = r[0], x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
    const float off = aligned ? 0.5f : 0.f;
    g.ok = fb >= 0.f && fb < (float)B && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
    g.b = g.ok ? (int)fb : 0;
    g.xs = x1 * scale - off;
    g.ys = y1 * scale - off;
    g.rw = (x2 * scale - off) - g.xs;
    g.rh = (y2 * scale - off) - g.ys;
    if (!aligned) { g.rw = fmaxf(g.rw, 1.f); g.rh = fmaxf(g.rh, 1.f); }
    g.ok = g.ok && isfinite(g.rw) && isfinite(g.rh);
    g.bin_w = g.rw / (float)PW;
    g.bin_h = g.rh / (float)PH;
    g.gh = sr > 0 ? sr : to_grid(g.rh / (float)PH);
    g.gw = sr > 0 ? sr : to_grid(g.rw / (float)PW);
    g.count = fmaxf((float)g.gh * (float)g.gw, 1.f);
    return g;
}

// The samples i of [0, grid) whose coordinate base + (i + 0.5) * bin / grid can lie in [lo, hi]: one more on either side than the
// division says, and the callers apply the exact rule to each.  bin <= 0 puts every sample on `base`: all of them.
__device__ __forceinline__ void sample_span(float base, float bin, int grid, float lo, float hi, int& i0, int& i1) {
    i0 = 0;
    i1 = grid - 1;
    if (bin > 0.f && grid > 0) {
        const float step = bin / (float)grid;
        const float a = floorf((lo - base) / step - 0.5f) - 1.f, b = ceilf((hi - base) / step - 0.5f) + 1.f;
        i0 = max(i0, (int)fminf(fmaxf(a, -1.f), 1e9f));
        i1 = min(i1, (int)fminf(fmaxf(b, -2.f), 1e9f));
    }
}

// one axis of a bilinear sample
struct Tap {
    int lo, hi;
    float l, h;
    bool in;
};
__device__ __forceinline__ Tap axis_tap(float s, int size) {
    Tap t;
    t.in = !(s < -1.f || s > (float)size);
    s = fminf(fmaxf(s, 0.f), (float)size);
    t.lo = (int)s;
    if (t.lo >= size - 1) {
        t.lo = t.hi = size - 1;
        s = (float)t.lo;
    } else {
        t.hi = t.lo + 1;
    }
    t.l = s - (float)t.lo;
    t.h = 1.f - t.l;
    return t;
}

__device__ __forceinline__ float sample_at(float base, float bin, int grid, int i) { return base + ((float)i + 0.5f) * bin / (float)grid; }

// The sum of the samples of bin (ph, pw) of one plane, over the wave: every lane calls it with the same arguments and gets the total.
template <bool SIGMOID>
__device__ __forceinline__ float pool_bin(const float* __restrict__ plane, int H, int W, const RoiGeom& g, int ph, int pw, int lane) {
    const float by = g.ys + (float)ph * g.bin_h, bx = g.xs + (float)pw * g.bin_w;
    int y0, y1, x0, x1;
    sample_span(by, g.bin_h, g.gh, -1.f, (float)H, y0, y1);
    sample_span(bx, g.bin_w, g.gw, -1.f, (float)W, x0, x1);
    float acc = 0.f;
    if (y1 >= y0 && x1 >= x0) {
        const unsigned nx = (unsigned)(x1 - x0 + 1), n = (unsigned)(y1 - y0 + 1) * nx;     // <= (2 * 16384 + 8)^2 < 2^31
        for (unsigned s = (unsigned)lane; s < n; s += 64u) {
            const unsigned ry = s / nx;
            const Tap ty = axis_tap(sample_at(by, g.bin_h, g.gh, y0 + (int)ry), H);
            const Tap tx = axis_tap(sample_at(bx, g.bin_w, g.gw, x0 + (int)(s - ry * nx)), W);
            if (ty.in && tx.in) {
                float v00 = plane[ty.lo * W + tx.lo], v01 = plane[ty.lo * W + tx.hi], v10 = plane[ty.hi * W + tx.lo], v11 = plane[ty.hi * W + tx.hi];
                if (SIGMOID) {
                    v00 = 1.f / (1.f + expf(-v00)); v01 = 1.f / (1.f + expf(-v01));
                    v10 = 1.f / (1.f + expf(-v10)); v11 = 1.f / (1.f + expf(-v11));
                }
                acc += ty.h * tx.h * v00 + ty.h * tx.l * v01 + ty.l * tx.h * v10 + ty.l * tx.l * v11;
            }
        }
    }
    return wave_total_f32(acc) / g.count;
}

template <bool SIGMOID>
__global__ __launch_bounds__(256) void roi_forward_kernel(const float* __restrict__ in, const float* __restrict__ rois, int B, int C, int H, int W,
                                                          int PH, int PW, float scale, int sr, int aligned, float* __restrict__ out, int total) {
    const int lane = threadIdx.x & 63;
    for (long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); o < total; o += (long long)gridDim.x * 4) {
        const int e = __builtin_amdgcn_readfirstlane((int)o);
        const int pw = e % PW, ph = (e / PW) % PH, c = (e / (PW * PH)) % C, k = e / (PW * PH * C);
        const RoiGeom g = roi_geom(rois + 5 * (size_t)k, B, PH, PW, scale, sr, aligned);
        float v = 0.f;
        if (g.ok) v = pool_bin<SIGMOID>(in + ((size_t)g.b * C + c) * H * W, H, W, g, ph, pw, lane);
        if (lane == 0) out[e] = v;
    }
}

// RoIAlign at 7 x 7, relu, the l2 norm over the channels: p[C] and the four wave sums live in the dynamic LDS block (nothing static in front).
__global__ __launch_bounds__(256) void roi_feat_norm_forward_kernel(const float* __restrict__ in, const float* __restrict__ rois, int B, int C, int H,
                                                                    int W, float scale, int sr, int aligned, float* __restrict__ out,
                                                                    float* __restrict__ norms) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* p = reinterpret_cast<float*>(smem);
    float* red = p + ((C + 3) & ~3);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x / kBins, bin = blockIdx.x - k * kBins, ph = bin / BXI_ROI_FEAT, pw = bin - ph * BXI_ROI_FEAT;
    const RoiGeom g = roi_geom(rois + 5 * (size_t)k, B, BXI_ROI_FEAT, BXI_ROI_FEAT, scale, sr, aligned);
    for (int c = wave; c < C; c += 4) {
        float v = 0.f;
        if (g.ok) v = pool_bin<false>(in + ((size_t)g.b * C + c) * H * W, H, W, g, ph, pw, lane);
        if (lane == 0) p[c] = fmaxf(v, 0.f);
    }
    __syncthreads();
    float ss = 0.f;
    for (int c = tid; c < C; c += 256) ss += p[c] * p[c];
    ss = wave_total_f32(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float n = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) + kNormEps);
    for (int c = tid; c < C; c += 256) out[((size_t)k * C + c) * kBins + bin] = p[c] / (n + kNormEps);
    if (tid == 0) norms[(size_t)k * kBins + bin] = n;
}

// out = r / (n + e), n = sqrt(sum r^2 + e), r = relu(pooled):  d / d pooled_c = [out_c > 0] (g_c / (n + e) - (sum_j g_j out_j) out_c / n)
__global__ __launch_bounds__(256) void roi_norm_backward_kernel(const float* __restrict__ out, const float* __restrict__ g_out,
                                                                const float* __restrict__ norms, int C, float* __restrict__ g_pooled) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x / kBins, bin = blockIdx.x - k * kBins;
    const size_t base = (size_t)k * C * kBins + bin;
    float dot = 0.f;
    for (int c = tid; c < C; c += 256) dot += g_out[base + (size_t)c * kBins] * out[base + (size_t)c * kBins];
    dot = wave_total_f32(dot);
    if (lane == 0) red[wave] = dot;
    __syncthreads();
    dot = (red[0] + red[1]) + (red[2] + red[3]);
    const float n = norms[(size_t)k * kBins + bin];
    for (int c = tid; c < C; c += 256) {
        const float o = out[base + (size_t)c * kBins];
        g_pooled[base + (size_t)c * kBins] = o > 0.f ? g_out[base + (size_t)c * kBins] / (n + kNormEps) - dot * o / n : 0.f;
    }
}

// What the samples of one bin put on the integer coordinate `coord` of an axis of `size` cells.
__device__ __forceinline__ float axis_weight(float base, float bin, int grid, int coord, int size) {
    int i0, i1;
    sample_span(base, bin, grid, (float)coord - 1.f, (float)coord + 1.f, i0, i1);
    float w = 0.f;
    for (int i = i0; i <= i1; ++i) {
        const Tap t = axis_tap(sample_at(base, bin, grid, i), size);
        if (t.in) w += (t.lo == coord ? t.h : 0.f) + (t.hi == coord ? t.l : 0.f);     // lo == hi at the border: l is 0 there
    }
    return w;
}

// The bins of [0, P) whose samples, all within [start + p * bin, start + (p + 1) * bin], can lie within one cell of `coord`.
__device__ __forceinline__ void bin_span(float start, float bin, int P, int coord, int& p0, int& p1) {
    p0 = 0;
    p1 = P - 1;
    if (bin > 0.f) {
        const float a = floorf(((float)coord - 1.f - start) / bin) - 1.f, b = floorf(((float)coord + 1.f - start) / bin) + 1.f;
        p0 = max(p0, (int)fminf(fmaxf(a, -1.f), 1e9f));
        p1 = min(p1, (int)fminf(fmaxf(b, -2.f), 1e9f));
    }
}

__global__ __launch_bounds__(256) void roi_backward_kernel(const float* __restrict__ g_out, const float* __restrict__ rois, int B, int C, int H, int W,
                                                           int K, int PH, int PW, float scale, int sr, int aligned, float* __restrict__ g_in) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int c0 = blockIdx.y * kGatherCh, b = blockIdx.z;
    const int y = pix / W, x = pix - y * W;
    const int nc = min(kGatherCh, C - c0);
    const size_t plane = (size_t)PH * PW;
    float acc[kGatherCh];
#pragma unroll
    for (int j = 0; j < kGatherCh; ++j) acc[j] = 0.f;
    for (int k = 0; k < K; ++k) {
        const RoiGeom g = roi_geom(rois + 5 * (size_t)k, B, PH, PW, scale, sr, aligned);
        if (!g.ok || g.b != b) continue;
        // the samples of an axis lie between its two ends (x2 < x1 with a fixed grid puts them to the left of xs), their taps within one cell
        if ((float)y < fminf(g.ys, g.ys + g.rh) - 1.5f || (float)y > fmaxf(g.ys, g.ys + g.rh) + 1.5f ||
            (float)x < fminf(g.xs, g.xs + g.rw) - 1.5f || (float)x > fmaxf(g.xs, g.xs + g.rw) + 1.5f)
            continue;
        int p0, p1, q0, q1;
        bin_span(g.ys, g.bin_h, PH, y, p0, p1);
        bin_span(g.xs, g.bin_w, PW, x, q0, q1);
        for (int ph = p0; ph <= p1; ++ph) {
            const float wy = axis_weight(g.ys + (float)ph * g.bin_h, g.bin_h, g.gh, y, H);
            if (wy == 0.f) continue;
            for (int pw = q0; pw <= q1; ++pw) {
                const float wx = axis_weight(g.xs + (float)pw * g.bin_w, g.bin_w, g.gw, x, W);
                if (wx == 0.f) continue;
                const float w = wy * wx / g.count;
                const float* __restrict__ gp = g_out + (((size_t)k * C + c0) * PH + ph) * PW + pw;
#pragma unroll
                for (int j = 0; j < kGatherCh; ++j)
                    if (j < nc) acc[j] += w * gp[(size_t)j * plane];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kGatherCh; ++j)
        if (j < nc) g_in[(((size_t)b * C + c0 + j) * H + y) * W + x] = acc[j];
}

// ---- the boxes of the target masks ----------------------------------------------------------------------------------------
struct Extent {
    int x0, y0, nx1, ny1;      // min x, min y, -(max x), -(max y): all four are minima
    __device__ __forceinline__ void add(int x, int y) {
        x0 = min(x0, x); y0 = min(y0, y);
        nx1 = min(nx1, -x); ny1 = min(ny1, -y);
    }
};

__global__ __launch_bounds__(256) void roi_target_boxes_kernel(const uint8_t* __restrict__ target, int H, int W, float* __restrict__ boxes,
                                                               uint8_t* __restrict__ keep) {
    __shared__ int red[4][4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int nbytes = H * W;
    const uint8_t* __restrict__ p = target + (size_t)n * nbytes;
    Extent e = {0x7fffffff, 0x7fffffff, 1, 1};
    // [0, head) byte-wise, then 16-byte vectors from the first aligned address, then the tail
    const int head = min(nbytes, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15)) & 15));
    const int nvec = (nbytes - head) >> 4;
    const int tail0 = head + (nvec << 4);
    if (tid < head && p[tid]) e.add(tid % W, tid / W);
    if (tail0 + tid < nbytes && p[tail0 + tid]) e.add((tail0 + tid) % W, (tail0 + tid) / W);
    const uint4* __restrict__ pv = reinterpret_cast<const uint4*>(p + head);
    for (int v = tid; v < nvec; v += 256) {
        const uint4 q = pv[v];
        if ((q.x | q.y | q.z | q.w) == 0u) continue;
        const int i0 = head + (v << 4);
        int y = i0 / W, x = i0 - y * W;
        const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((wd[j >> 2] >> (8 * (j & 3))) & 0xffu) e.add(x, y);
            if (++x == W) { x = 0; ++y; }
        }
    }
    const int m[4] = {wave_min_i32(e.x0), wave_min_i32(e.y0), wave_min_i32(e.nx1), wave_min_i32(e.ny1)};
    if ((tid & 63) == 0)
        for (int j = 0; j < 4; ++j) red[tid >> 6][j] = m[j];
    __syncthreads();
    if (tid == 0) {
        int r[4];
        for (int j = 0; j < 4; ++j) r[j] = min(min(red[0][j], red[1][j]), min(red[2][j], red[3][j]));
        const bool any = r[2] <= 0;
        boxes[4 * (size_t)n + 0] = any ? (float)r[0] : 0.f;
        boxes[4 * (size_t)n + 1] = any ? (float)r[1] : 0.f;
        boxes[4 * (size_t)n + 2] = any ? (float)(1 - r[2]) : 0.f;
        boxes[4 * (size_t)n + 3] = any ? (float)(1 - r[3]) : 0.f;
        keep[n] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void roi_labels_kernel(const uint8_t* __restrict__ keep, const int64_t* __restrict__ kernel_labels, int N, int own,
                                                         int64_t* __restrict__ labels_out) {
    __shared__ int part[4];
    int carry = 0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + threadIdx.x;
        const int kp = i < N && keep[i] ? 1 : 0;
        int total;
        const int rank = carry + block_scan_excl_i32<4>(kp, part, total);
        if (i < N) labels_out[i] = kp ? kernel_labels[own ? i : rank] : (int64_t)-1;
        carry += total;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int check_pool(int B, int C, int H, int W, int K, int PH, int PW, float scale, int sr) {
    if (B < 0 || C < 0 || K < 0 || H < 1 || W < 1 || H > BXI_ROI_MAX_SIDE || W > BXI_ROI_MAX_SIDE || PH < 1 || PW < 1 || PH > BXI_ROI_MAX_POOL ||
        PW > BXI_ROI_MAX_POOL || B > 65535 || (C + kGatherCh - 1) / kGatherCh > 65535 || !fits_i32((int64_t)B * C * H * W) ||
        !fits_i32((int64_t)K * C * PH * PW) || !fits_i32((int64_t)K * 5))
        return BXI_ERR_BAD_SHAPE;
    if (!(scale == scale) || sr < 0 || sr > BXI_ROI_MAX_SAMPLING) return BXI_ERR_BAD_ARGUMENT;
    return BXI_OK;
}

size_t fused_layout(void* ws, int K, int C, float** norms, float** g_pooled) {
    Carver cv(ws, 16);
    float* n = cv.take<float>((size_t)K * kBins);
    float* g = cv.take<float>((size_t)K * C * kBins);
    if (norms) *norms = n;
    if (g_pooled) *g_pooled = g;
    return cv.bytes() < 16 ? 16 : cv.bytes();
}

int launch_gather(const float* g_out, const float* rois, int B, int C, int H, int W, int K, int PH, int PW, float scale, int sr, int aligned,
                  float* g_in, hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)((C + kGatherCh - 1) / kGatherCh), (unsigned)B);
    BXI_LAUNCH("roi_align_backward", s, roi_backward_kernel, grid, dim3(256), 0, s, g_out, rois, B, C, H, W, K, PH, PW, scale, sr, aligned ? 1 : 0, g_in);
    return check_launch();
}

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" int bxi_roi_target_boxes_u8(const uint8_t* target, const int64_t* kernel_labels, int N, int H, int W, int own_labels, float* boxes,
                                       uint8_t* keep, int64_t* labels_out, void* stream) {
    if (N < 0 || H < 1 || W < 1 || !fits_i32((int64_t)H * W)) return BXI_ERR_BAD_SHAPE;
    if (N == 0) return BXI_OK;
    if (!target || !kernel_labels || !boxes || !keep || !labels_out) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("roi_target_boxes", s, roi_target_boxes_kernel, dim3((unsigned)N), dim3(256), 0, s, target, H, W, boxes, keep);
    int rc = check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("roi_labels", s, roi_labels_kernel, dim3(1), dim3(256), 0, s, (const uint8_t*)keep, kernel_labels, N, own_labels ? 1 : 0, labels_out);
    return check_launch();
}

extern "C" int bxi_roi_align_forward_f32(const float* input, const float* rois, int B, int C, int H, int W, int K, int PH, int PW,
                                         float spatial_scale, int sampling_ratio, int aligned, int flags, float* out, void* stream) {
    const int rc = check_pool(B, C, H, W, K, PH, PW, spatial_scale, sampling_ratio);
    if (rc != BXI_OK) return rc;
    if (flags & ~BXI_ROI_SIGMOID) return BXI_ERR_BAD_ARGUMENT;
    if (K == 0 || C == 0) return BXI_OK;
    if (!rois || !out || (B > 0 && !input)) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    const int total = K * C * PH * PW;
    const int64_t want = ((int64_t)total + 3) / 4, cap = (int64_t)device_cus() * 64;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    const int al = aligned ? 1 : 0;
    if (flags & BXI_ROI_SIGMOID)
        BXI_LAUNCH("roi_align_forward_sigmoid", s, roi_forward_kernel<true>, grid, dim3(256), 0, s, input, rois, B, C, H, W, PH, PW, spatial_scale,
                   sampling_ratio, al, out, total);
    else
        BXI_LAUNCH("roi_align_forward", s, roi_forward_kernel<false>, grid, dim3(256), 0, s, input, rois, B, C, H, W, PH, PW, spatial_scale,
                   sampling_ratio, al, out, total);
    return check_launch();
}

extern "C" int bxi_roi_align_backward_f32(const float* g_out, const float* rois, int B, int C, int H, int W, int K, int PH, int PW,
                                          float spatial_scale, int sampling_ratio, int aligned, float* g_input, void* stream) {
    const int rc = check_pool(B, C, H, W, K, PH, PW, spatial_scale, sampling_ratio);
    if (rc != BXI_OK) return rc;
    if (C == 0 || B == 0) return BXI_OK;
    if (!g_input || (K > 0 && (!g_out || !rois))) return BXI_ERR_NULL_POINTER;
    return launch_gather(g_out, rois, B, C, H, W, K, PH, PW, spatial_scale, sampling_ratio, aligned, g_input, as_stream(stream));
}

extern "C" size_t bxi_roi_feat_norm_workspace_bytes(int K, int C) {
    if (K < 0 || C < 1 || C > BXI_ROI_FUSED_MAX_C || !fits_i32((int64_t)K * C * kBins)) return 0;
    return fused_layout(nullptr, K, C, nullptr, nullptr);
}

extern "C" int bxi_roi_feat_norm_forward_f32(const float* input, const float* rois, int B, int C, int H, int W, int K, float spatial_scale,
                                             int sampling_ratio, int aligned, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_pool(B, C, H, W, K, BXI_ROI_FEAT, BXI_ROI_FEAT, spatial_scale, sampling_ratio);
    if (rc != BXI_OK) return rc;
    if (C < 1) return BXI_ERR_BAD_SHAPE;
    if (C > BXI_ROI_FUSED_MAX_C) return BXI_ERR_UNSUPPORTED;
    if (!workspace_ok(workspace, workspace_bytes, fused_layout(nullptr, K, C, nullptr, nullptr), 16)) return BXI_ERR_WORKSPACE;
    if (K == 0) return BXI_OK;
    if (!rois || !out || (B > 0 && !input)) return BXI_ERR_NULL_POINTER;
    float* norms;
    fused_layout(workspace, K, C, &norms, nullptr);
    hipStream_t s = as_stream(stream);
    const size_t lds = (size_t)(((C + 3) & ~3) + 4) * sizeof(float);
    BXI_LAUNCH("roi_feat_norm_forward", s, roi_feat_norm_forward_kernel, dim3((unsigned)K * kBins), dim3(256), lds, s, input, rois, B, C, H, W,
               spatial_scale, sampling_ratio, aligned ? 1 : 0, out, norms);
    return check_launch();
}

extern "C" int bxi_roi_feat_norm_backward_f32(const float* out, const float* g_out, const float* rois, int B, int C, int H, int W, int K,
                                              float spatial_scale, int sampling_ratio, int aligned, float* g_input, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    const int rc = check_pool(B, C, H, W, K, BXI_ROI_FEAT, BXI_ROI_FEAT, spatial_scale, sampling_ratio);
    if (rc != BXI_OK) return rc;
    if (C < 1) return BXI_ERR_BAD_SHAPE;
    if (C > BXI_ROI_FUSED_MAX_C) return BXI_ERR_UNSUPPORTED;
    if (!workspace_ok(workspace, workspace_bytes, fused_layout(nullptr, K, C, nullptr, nullptr), 16)) return BXI_ERR_WORKSPACE;
    if (B == 0) return BXI_OK;
    if (!g_input || (K > 0 && (!out || !g_out || !rois))) return BXI_ERR_NULL_POINTER;
    float *norms, *g_pooled;
    fused_layout(workspace, K, C, &norms, &g_pooled);
    hipStream_t s = as_stream(stream);
    if (K > 0) {
        BXI_LAUNCH("roi_norm_backward", s, roi_norm_backward_kernel, dim3((unsigned)K * kBins), dim3(256), 0, s, out, g_out, (const float*)norms, C,
                   g_pooled);
        const int rc2 = check_launch();
        if (rc2 != BXI_OK) return rc2;
    }
    return launch_gather(g_pooled, rois, B, C, H, W, K, BXI_ROI_FEAT, BXI_ROI_FEAT, spatial_scale, sampling_ratio, aligned, g_input, s);
}
