// msda.hip -- multi-scale deformable attention, forward and backward (include/boxinst/boxinst_hip_msda.h).
//
//   msda_forward_kernel    lanes over the D channels of one (b, q, m), 64 / D items per wave: every corner read is one contiguous D * 4-byte
//                          segment, a wave's output 256 contiguous bytes.  The fused form takes the softmax and the offset normaliser here.
//   msda_prep_kernel       zeroes the int64 accumulator and leaves 256 partial maxima of |grad_out| and |weight| (as float bits: the bits of
//                          a non-negative float order as integers, and a NaN orders above the infinity, so it is never lost)
//   msda_backward_kernel   the same mapping: per sample the per-query gradients as a fixed-order reduction over the D lanes, the
//                          contributions to grad_value in fixed point with 64-bit integer atomics
//   msda_convert_kernel    accumulator -> fp32, every element of grad_value
//
// Fixed point.  Mx = max|grad_out| * max|weight| (fp64 product of two floats: exact).  A contribution c = g * a * k (g one element of grad_out,
// a the attention weight, k a corner weight in [0, 1]) has |c| <= Mx.  It is formed in fp64 from the three fp32 factors -- exact up to one
// fp64 rounding, 2^-53 -- times 2^40 / Mx and rounded to the nearest integer q, |q| <= 2^40 + 1: the stored value is off by at most half a
// unit, 2^-41 Mx.  A cell with n contributions: |sum| <= n (2^40 + 1) < 2^63 for n < 2^22 (header), and the error of its grad_value is at
// most n 2^-41 Mx + one fp32 rounding of the result.
// Against the tolerance of the tests, 4 x the fp32 error of the per-sample statement relative to max|grad_value|: that statement rounds every
// product c to fp32, 2^-24 |c|, and every partial sum likewise.  The fixed-point error 2^-41 Mx per contribution is below the product
// rounding alone of every contribution with |c| > 2^-17 Mx, and for the smaller ones it is 2^-17 of the rounding of ONE contribution of
// full size; summed over a cell it stays below n 2^-41 Mx <= 2^-19 Mx (n < 2^22), i.e. below 2^5 ulp of a result of the size of Mx, and
// below one ulp of such a result for n <= 2^17.  The cases of the tests have n <= 2^12 and max|grad_value| >= Mx / 2^4, where the bound is
// 2^-25 max|grad_value|: under a quarter of ONE fp32 rounding of the result.  The accumulated sum itself is exact, which the fp32
// statement's is not.
#include "common.hpp"

#include <math.h>

#include "../../include/boxinst/boxinst_hip_msda.h"

namespace bxi {
namespace {

constexpr int kParts = 256;                  // workgroups of the prep launch = partial maxima per quantity
constexpr double kFixedOne = 1099511627776.0;   // 2^40
constexpr uint32_t kInfBits = 0x7f800000u;

// The total of v over the D lanes that share one (b, q, m), in every one of them, in a fixed order.  Every lane of the wave takes part.
template <int D>
__device__ __forceinline__ float group_total(float v) {
    v += __int_as_float(dpp_i32(__float_as_int(v), 0xB1));       // quad_perm:[1,0,3,2]
    v += __int_as_float(dpp_i32(__float_as_int(v), 0x4E));       // quad_perm:[2,3,0,1]
    v += __int_as_float(dpp_i32(__float_as_int(v), 0x141));      // row_half_mirror: the other quad of 8 lanes
    if (D >= 16) v += __int_as_float(dpp_i32(__float_as_int(v), 0x140));      // row_mirror: the other half of 16 lanes
    if (D >= 32) v += __shfl_xor(v, 16);
    if (D >= 64) v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ int wave_max_i32(int v) {
    wave_total_steps([&](int c) { v = max(v, dpp_i32(v, c)); });
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

struct Level {
    int H, W;
    long long start;
    bool ok;
};
// A level the kernels may index: both sides at least 1 and its cells inside [0, S).
__device__ __forceinline__ Level load_level(const int64_t* __restrict__ shapes, const int64_t* __restrict__ starts, int l, int S) {
    const long long H = shapes[2 * l], W = shapes[2 * l + 1], st = starts[l];
    Level lv;
    lv.ok = H >= 1 && W >= 1 && H <= S && W <= S && st >= 0 && st + H * W <= (long long)S;
    lv.H = lv.ok ? (int)H : 1;
    lv.W = lv.ok ? (int)W : 1;
    lv.start = lv.ok ? st : 0;
    return lv;
}

// One bilinear sample: the four corners' cells (relative to the level's start, -1 outside the map) and the axis weights.
struct Sample {
    bool valid;
    int c[4];          // (h_low, w_low), (h_low, w_high), (h_high, w_low), (h_high, w_high)
    float lh, lw, hh, hw;
};
__device__ __forceinline__ Sample make_sample(float x, float y, const Level& lv) {
    Sample s;
    const float h = y * (float)lv.H - 0.5f, w = x * (float)lv.W - 0.5f;
    s.valid = lv.ok && h > -1.f && w > -1.f && h < (float)lv.H && w < (float)lv.W;
    s.c[0] = s.c[1] = s.c[2] = s.c[3] = -1;
    s.lh = s.lw = 0.f;
    s.hh = s.hw = 1.f;
    if (s.valid) {
        const float hf = floorf(h), wf = floorf(w);
        const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
        s.lh = h - hf;
        s.lw = w - wf;
        s.hh = 1.f - s.lh;
        s.hw = 1.f - s.lw;
        const bool t = h0 >= 0, bt = h1 <= lv.H - 1, lf = w0 >= 0, rt = w1 <= lv.W - 1;
        if (t && lf) s.c[0] = h0 * lv.W + w0;
        if (t && rt) s.c[1] = h0 * lv.W + w1;
        if (bt && lf) s.c[2] = h1 * lv.W + w0;
        if (bt && rt) s.c[3] = h1 * lv.W + w1;
    }
    return s;
}

// The softmax of the fused form over the LP logits of one item: its maximum and 1 / sum exp, every lane for itself (same addresses
// across the D lanes: one fetch).
__device__ __forceinline__ void softmax_stats(const float* __restrict__ wp, int LP, float& mx, float& inv) {
    mx = -INFINITY;
    for (int s = 0; s < LP; ++s) mx = fmaxf(mx, wp[s]);
    float sum = 0.f;
    for (int s = 0; s < LP; ++s) sum += expf(wp[s] - mx);
    inv = 1.f / sum;
}

// Location of sample s of level l.  fused: ref + off / (W, H).
template <bool FUSED>
__device__ __forceinline__ void sample_xy(const float* __restrict__ a, const float* __restrict__ off, size_t item, int bq, int L, int LP, int l, int s,
                                          const Level& lv, float& x, float& y) {
    if (FUSED) {
        const float* __restrict__ r = a + ((size_t)bq * L + l) * 2;
        const float* __restrict__ o = off + (item * LP + s) * 2;
        x = r[0] + o[0] / (float)lv.W;
        y = r[1] + o[1] / (float)lv.H;
    } else {
        const float* __restrict__ p = a + (item * LP + s) * 2;
        x = p[0];
        y = p[1];
    }
}

template <int D, bool FUSED>
__global__ __launch_bounds__(256) void msda_forward_kernel(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                           const int64_t* __restrict__ starts, const float* __restrict__ a,
                                                           const float* __restrict__ off, const float* __restrict__ w, int S, int M, int Q, int L, int P,
                                                           int items, float* __restrict__ out) {
    constexpr int G = 64 / D;
    const int lane = threadIdx.x & 63, d = lane % D;
    const long long it = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * G + lane / D;
    if (it >= items) return;
    const size_t item = (size_t)it;
    const int m = (int)(it % M), bq = (int)(it / M), b = bq / Q, LP = L * P;
    const float* __restrict__ wp = w + item * LP;
    float mx = 0.f, inv = 1.f;
    if (FUSED) softmax_stats(wp, LP, mx, inv);
    const size_t row = (size_t)M * D;
    const float* __restrict__ vb = value + ((size_t)b * S * M + m) * D + d;
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
        const Level lv = load_level(shapes, starts, l, S);
        const float* __restrict__ vl = vb + (size_t)lv.start * row;
        for (int p = 0; p < P; ++p) {
            const int s = l * P + p;
            float x, y;
            sample_xy<FUSED>(a, off, item, bq, L, LP, l, s, lv, x, y);
            const float aw = FUSED ? expf(wp[s] - mx) * inv : wp[s];
            const Sample sm = make_sample(x, y, lv);
            if (sm.valid) {
                const float v0 = sm.c[0] >= 0 ? vl[(size_t)sm.c[0] * row] : 0.f, v1 = sm.c[1] >= 0 ? vl[(size_t)sm.c[1] * row] : 0.f;
                const float v2 = sm.c[2] >= 0 ? vl[(size_t)sm.c[2] * row] : 0.f, v3 = sm.c[3] >= 0 ? vl[(size_t)sm.c[3] * row] : 0.f;
                acc += aw * (sm.hh * sm.hw * v0 + sm.hh * sm.lw * v1 + sm.lh * sm.hw * v2 + sm.lh * sm.lw * v3);
            }
        }
    }
    out[item * D + d] = acc;
}

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// partial [2][kParts] uint32: row 0 the maxima of |grad_out|, row 1 of |weight| (zeros when n_w == 0).
__global__ __launch_bounds__(256) void msda_prep_kernel(const float* __restrict__ g_out, size_t n_g, const float* __restrict__ w, size_t n_w,
                                                        long long* __restrict__ acc, size_t n_acc, uint32_t* __restrict__ partial) {
    __shared__ int red[2][4];
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)kParts * 256;
    for (size_t i = tid; i < n_acc; i += step) acc[i] = 0;
    uint32_t mg = 0, mw = 0;
    for (size_t i = tid; i < n_g; i += step) mg = max(mg, abs_bits(g_out[i]));
    for (size_t i = tid; i < n_w; i += step) mw = max(mw, abs_bits(w[i]));
    const int wg = wave_max_i32((int)mg), ww = wave_max_i32((int)mw);         // the sign bit is clear: the order of int is the order of the bits
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = wg;
        red[1][threadIdx.x >> 6] = ww;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int* r = red[threadIdx.x];
        partial[threadIdx.x * kParts + blockIdx.x] = (uint32_t)max(max(r[0], r[1]), max(r[2], r[3]));
    }
}

// Mx from the partial maxima, the same in every lane of the wave; false when it is not finite.
template <bool FUSED>
__device__ __forceinline__ bool load_mx(const uint32_t* __restrict__ partial, int lane, double& mx) {
    int mg = 0, mw = 0;
    for (int i = lane; i < kParts; i += 64) {
        mg = max(mg, (int)partial[i]);
        if (!FUSED) mw = max(mw, (int)partial[kParts + i]);
    }
    mg = wave_max_i32(mg);
    mw = wave_max_i32(mw);
    const bool finite = (uint32_t)mg < kInfBits && (uint32_t)mw < kInfBits;
    mx = finite ? (double)__int_as_float(mg) * (FUSED ? 1.0 : (double)__int_as_float(mw)) : 0.0;
    return finite;
}

__device__ __forceinline__ void add_fixed(long long* __restrict__ cell, double c) {
    if (fabs(c) <= 2.0 * kFixedOne) {         // a NaN fails: it adds nothing
        const long long q = __double2ll_rn(c);
        if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)q);
    }
}

template <int D, bool FUSED>
__global__ __launch_bounds__(256) void msda_backward_kernel(const float* __restrict__ g_out, const float* __restrict__ value,
                                                            const int64_t* __restrict__ shapes, const int64_t* __restrict__ starts,
                                                            const float* __restrict__ a, const float* __restrict__ off, const float* __restrict__ w, int S,
                                                            int M, int Q, int L, int P, int items, const uint32_t* __restrict__ partial,
                                                            long long* __restrict__ acc, float* g_a, float* g_w) {
    constexpr int G = 64 / D;
    const int lane = threadIdx.x & 63, d = lane % D;
    const long long raw = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * G + lane / D;
    const bool live = raw < items;                      // a group behind the last item computes the last item again and stores nothing:
    const long long it = live ? raw : items - 1;        // the reductions below run with every lane of the wave
    double mxv;
    const bool finite = load_mx<FUSED>(partial, lane, mxv);
    const double scale = finite && mxv > 0.0 ? kFixedOne / mxv : 0.0;
    const size_t item = (size_t)it;
    const int m = (int)(it % M), bq = (int)(it / M), b = bq / Q, LP = L * P;
    const float* __restrict__ wp = w + item * LP;
    float mx = 0.f, inv = 1.f;
    if (FUSED) softmax_stats(wp, LP, mx, inv);
    const size_t row = (size_t)M * D, base = ((size_t)b * S * M + m) * D + d;
    const float g = g_out[item * D + d];
    float dot = 0.f;
    for (int l = 0; l < L; ++l) {
        const Level lv = load_level(shapes, starts, l, S);
        const size_t lbase = base + (size_t)lv.start * row;
        for (int p = 0; p < P; ++p) {
            const int s = l * P + p;
            float x, y;
            sample_xy<FUSED>(a, off, item, bq, L, LP, l, s, lv, x, y);
            const float aw = FUSED ? expf(wp[s] - mx) * inv : wp[s];
            const Sample sm = make_sample(x, y, lv);
            float val = 0.f, gh = 0.f, gw = 0.f;
            if (sm.valid) {
                const float v0 = sm.c[0] >= 0 ? value[lbase + (size_t)sm.c[0] * row] : 0.f, v1 = sm.c[1] >= 0 ? value[lbase + (size_t)sm.c[1] * row] : 0.f;
                const float v2 = sm.c[2] >= 0 ? value[lbase + (size_t)sm.c[2] * row] : 0.f, v3 = sm.c[3] >= 0 ? value[lbase + (size_t)sm.c[3] * row] : 0.f;
                val = sm.hh * sm.hw * v0 + sm.hh * sm.lw * v1 + sm.lh * sm.hw * v2 + sm.lh * sm.lw * v3;
                gh = (sm.hw * v2 + sm.lw * v3) - (sm.hw * v0 + sm.lw * v1);
                gw = (sm.hh * v1 + sm.lh * v3) - (sm.hh * v0 + sm.lh * v2);
                if (live) {
                    const double tg = (double)g * (double)aw * scale;
                    if (sm.c[0] >= 0) add_fixed(acc + lbase + (size_t)sm.c[0] * row, tg * ((double)sm.hh * (double)sm.hw));
                    if (sm.c[1] >= 0) add_fixed(acc + lbase + (size_t)sm.c[1] * row, tg * ((double)sm.hh * (double)sm.lw));
                    if (sm.c[2] >= 0) add_fixed(acc + lbase + (size_t)sm.c[2] * row, tg * ((double)sm.lh * (double)sm.hw));
                    if (sm.c[3] >= 0) add_fixed(acc + lbase + (size_t)sm.c[3] * row, tg * ((double)sm.lh * (double)sm.lw));
                }
            }
            const float ga = group_total<D>(g * val);
            float gx = group_total<D>(g * gw) * aw, gy = group_total<D>(g * gh) * aw;
            if (!FUSED) {       // d loc = (W, H) d (w, h); the fused form divides its offsets by the same (W, H)
                gx *= (float)lv.W;
                gy *= (float)lv.H;
            }
            if (FUSED) dot += aw * ga;
            if (live && (s % D) == d) {
                const size_t e = item * LP + s;
                g_a[2 * e] = sm.valid ? gx : 0.f;
                g_a[2 * e + 1] = sm.valid ? gy : 0.f;
                g_w[e] = ga;               // fused: d out / d weight for now, turned into the logit's gradient below by the same lane
            }
        }
    }
    if (FUSED && live) {
        for (int s = d; s < LP; s += D) {
            const size_t e = item * LP + s;
            const float aw = expf(wp[s] - mx) * inv;
            g_w[e] = aw * (g_w[e] - dot);
        }
    }
}

template <bool FUSED>
__global__ __launch_bounds__(256) void msda_convert_kernel(const long long* __restrict__ acc, const uint32_t* __restrict__ partial, size_t n,
                                                           float* __restrict__ g_value) {
    double mxv;
    const bool finite = load_mx<FUSED>(partial, threadIdx.x & 63, mxv);
    const double unit = mxv / kFixedOne;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        g_value[i] = finite ? (float)((double)acc[i] * unit) : __int_as_float(0x7fc00000);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int check_shape(int B, int S, int M, int D, int Q, int L, int P, int flags) {
    if (B < 0 || S < 0 || Q < 0 || M < 1 || D < 1 || L < 1 || P < 1) return BXI_ERR_BAD_SHAPE;
    if (flags & ~BXI_MSDA_FUSED) return BXI_ERR_BAD_ARGUMENT;
    if (D < BXI_MSDA_MIN_HEAD_DIM || D > BXI_MSDA_MAX_HEAD_DIM || (D & (D - 1)) || L > BXI_MSDA_MAX_LEVELS || P > BXI_MSDA_MAX_POINTS)
        return BXI_ERR_UNSUPPORTED;
    if (!fits_i32((int64_t)B * S * M * D) || !fits_i32((int64_t)B * Q * M * D) || !fits_i32((int64_t)B * Q * M * L * P * 2)) return BXI_ERR_BAD_SHAPE;
    return BXI_OK;
}

size_t backward_layout(void* ws, size_t n_value, uint32_t** partial, long long** acc) {
    Carver cv(ws, 16);
    uint32_t* p = cv.take<uint32_t>(2 * kParts);
    long long* a = cv.take<long long>(n_value);
    if (partial) *partial = p;
    if (acc) *acc = a;
    return cv.bytes();
}

template <int D, bool FUSED>
void launch_forward(const float* value, const int64_t* shapes, const int64_t* starts, const float* a, const float* off, const float* w, int S, int M,
                    int Q, int L, int P, int items, float* out, hipStream_t s) {
    const int per_block = 4 * (64 / D);
    BXI_LAUNCH(FUSED ? "msda_forward_fused" : "msda_forward", s, (msda_forward_kernel<D, FUSED>), dim3((unsigned)((items + per_block - 1) / per_block)),
               dim3(256), 0, s, value, shapes, starts, a, off, w, S, M, Q, L, P, items, out);
}

template <int D, bool FUSED>
void launch_backward(const float* g_out, const float* value, const int64_t* shapes, const int64_t* starts, const float* a, const float* off,
                     const float* w, int S, int M, int Q, int L, int P, int items, const uint32_t* partial, long long* acc, float* g_a, float* g_w,
                     hipStream_t s) {
    const int per_block = 4 * (64 / D);
    BXI_LAUNCH(FUSED ? "msda_backward_fused" : "msda_backward", s, (msda_backward_kernel<D, FUSED>),
               dim3((unsigned)((items + per_block - 1) / per_block)), dim3(256), 0, s, g_out, value, shapes, starts, a, off, w, S, M, Q, L, P, items, partial,
               acc, g_a, g_w);
}

#define MSDA_DISPATCH(fn, D, fused, ...)                          \
    do {                                                          \
        switch (D) {                                              \
            case 8: if (fused) fn<8, true>(__VA_ARGS__); else fn<8, false>(__VA_ARGS__); break;     \
            case 16: if (fused) fn<16, true>(__VA_ARGS__); else fn<16, false>(__VA_ARGS__); break;  \
            case 32: if (fused) fn<32, true>(__VA_ARGS__); else fn<32, false>(__VA_ARGS__); break;  \
            default: if (fused) fn<64, true>(__VA_ARGS__); else fn<64, false>(__VA_ARGS__); break;  \
        }                                                         \
    } while (0)

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" int bxi_msda_forward_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const float* a,
                                    const float* offsets, const float* w, int B, int S, int M, int D, int Q, int L, int P, int flags, float* out,
                                    void* stream) {
    const int rc = check_shape(B, S, M, D, Q, L, P, flags);
    if (rc != BXI_OK) return rc;
    if (B == 0 || Q == 0) return BXI_OK;
    const bool fused = flags & BXI_MSDA_FUSED;
    if (!spatial_shapes || !level_start_index || !a || !w || !out || (fused && !offsets) || (S > 0 && !value)) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    const int items = B * Q * M;
    MSDA_DISPATCH(launch_forward, D, fused, value, spatial_shapes, level_start_index, a, offsets, w, S, M, Q, L, P, items, out, s);
    return check_launch();
}

extern "C" size_t bxi_msda_backward_workspace_bytes(int B, int S, int M, int D, int Q, int L, int P) {
    if (check_shape(B, S, M, D, Q, L, P, 0) != BXI_OK || (int64_t)Q * L * P >= BXI_MSDA_MAX_CELL_SAMPLES) return 0;
    return backward_layout(nullptr, (size_t)B * S * M * D, nullptr, nullptr);
}

extern "C" int bxi_msda_backward_f32(const float* grad_out, const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                     const float* a, const float* offsets, const float* w, int B, int S, int M, int D, int Q, int L, int P, int flags,
                                     float* grad_value, float* grad_a, float* grad_w, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_shape(B, S, M, D, Q, L, P, flags);
    if (rc != BXI_OK) return rc;
    if ((int64_t)Q * L * P >= BXI_MSDA_MAX_CELL_SAMPLES) return BXI_ERR_UNSUPPORTED;
    const size_t n_value = (size_t)B * S * M * D;
    if (!workspace_ok(workspace, workspace_bytes, backward_layout(nullptr, n_value, nullptr, nullptr), 16)) return BXI_ERR_WORKSPACE;
    const bool fused = flags & BXI_MSDA_FUSED;
    const int items = B * Q * M;
    if (n_value == 0 && items == 0) return BXI_OK;
    if ((n_value > 0 && (!grad_value || !value)) ||
        (items > 0 && (!grad_out || !spatial_shapes || !level_start_index || !a || !w || !grad_a || !grad_w || (fused && !offsets))))
        return BXI_ERR_NULL_POINTER;
    uint32_t* partial;
    long long* acc;
    backward_layout(workspace, n_value, &partial, &acc);
    hipStream_t s = as_stream(stream);
    const size_t n_g = (size_t)items * D, n_w = fused ? 0 : (size_t)items * L * P;
    BXI_LAUNCH("msda_prep", s, msda_prep_kernel, dim3(kParts), dim3(256), 0, s, grad_out, n_g, w, n_w, acc, n_value, partial);
    int rc2 = check_launch();
    if (rc2 != BXI_OK) return rc2;
    if (items > 0) {
        MSDA_DISPATCH(launch_backward, D, fused, grad_out, value, spatial_shapes, level_start_index, a, offsets, w, S, M, Q, L, P, items,
                      (const uint32_t*)partial, acc, grad_a, grad_w, s);
        rc2 = check_launch();
        if (rc2 != BXI_OK) return rc2;
    }
    if (n_value > 0) {
        const size_t want = (n_value + 255) / 256, cap = (size_t)device_cus() * 16;
        const dim3 grid((unsigned)(want < cap ? want : cap));
        if (fused)
            BXI_LAUNCH("msda_convert", s, msda_convert_kernel<true>, grid, dim3(256), 0, s, (const long long*)acc, (const uint32_t*)partial, n_value, grad_value);
        else
            BXI_LAUNCH("msda_convert", s, msda_convert_kernel<false>, grid, dim3(256), 0, s, (const long long*)acc, (const uint32_t*)partial, n_value, grad_value);
        rc2 = check_launch();
    }
    return rc2;
}
