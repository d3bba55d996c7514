// solo_targets.hip -- the training targets of the two SOLOv2-style heads and their category loss (include/boxinst/boxinst_hip_solo.h).
// gfx950 only.
//
//   solo_mask_pass_kernel       one workgroup of 256 per (instance, band of source rows).  Sweeps the band's bytes once as
//                               16-byte vectors (byte-wise head and tail: a mask may start anywhere) for the exact moments -- 64-bit
//                               integer partials through LDS, three integer atomics per workgroup that saw a one -- and writes the
//                               band's rows of every rescaled mask (the four sampled bytes come out of the cache lines just read).
//   solo_assign_kernel          one workgroup per (level, image): every instance's window (one thread per instance, chunks of 256), the
//                               pair list through a workgroup scan, the last writer of a cell through an integer max in LDS, then the
//                               per-cell outputs and the compacted owners through a second scan.
//   solo_cate_focal_kernel<G2>  flat over the [B][C][S*S] logits of a level, as fcos_focal_kernel (same element-to-thread map).
//   solo_cate_finish_kernel     one workgroup adds the fp64 partials in a fixed order and rounds once.
//   flat_rescale_kernel         focal_device.hpp.
#include <algorithm>

#include "focal_device.hpp"
#include "../../include/boxinst/boxinst_hip_solo.h"

// (fp contraction is off for the whole file: focal_device.hpp says why)
#pragma clang fp contract(off)

namespace bxi {
namespace {

constexpr int kMaxF = BXI_SOLO_MAX_FACTORS;
constexpr int kMinOnes = BXI_SOLO_RESCALE_MIN_ONES;
constexpr int kMaxGrid = BXI_SOLO_MAX_GRID;
constexpr int kPairs = BXI_SOLO_PAIRS_PER_INSTANCE;
constexpr int kMinBand = 16;                // source rows per workgroup: the smallest multiple of the largest factor that is >= 16

struct MaskImgs {
    const uint8_t* ptr[BXI_MAX_IMAGES];
    int H[BXI_MAX_IMAGES], W[BXI_MAX_IMAGES];
    int off[BXI_MAX_IMAGES + 1];
    int B;
};
struct MaskOuts {
    uint8_t* out[kMaxF];
    int f[kMaxF], h[kMaxF], w[kMaxF];
    int n, band, nb;                        // factors, source rows per band, bands per instance
};

// ---- mask pass ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_byte(unsigned v, int x, int y, unsigned& m00, unsigned long long& m10, unsigned long long& m01) {
    if (v) { m00 += 1u; m10 += (unsigned)x; m01 += (unsigned)y; }
}

__global__ __launch_bounds__(256) void solo_mask_pass_kernel(MaskImgs im, MaskOuts o, unsigned long long* __restrict__ moments) {
    __shared__ unsigned long long sm[3];
    const int tid = threadIdx.x;
    const int g = blockIdx.x / o.nb, j = blockIdx.x - g * o.nb;
    int b = 0;
    while (b + 1 < im.B && g >= im.off[b + 1]) ++b;
    const int H = im.H[b], W = im.W[b];
    const uint8_t* __restrict__ src = im.ptr[b] + (size_t)(g - im.off[b]) * H * W;
    const int y0 = min(j * o.band, H), y1 = min(y0 + o.band, H);
    if (tid < 3) sm[tid] = 0ull;
    __syncthreads();

    // the band's bytes, once: [0, head) byte-wise, then 16-byte vectors from the first aligned address, then the tail
    const int nbytes = (y1 - y0) * W;
    if (nbytes > 0) {
        const uint8_t* p = src + (size_t)y0 * W;
        const int head = min(nbytes, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15)) & 15));
        const int nvec = (nbytes - head) >> 4;
        const int tail0 = head + (nvec << 4);
        unsigned m00 = 0;
        unsigned long long m10 = 0, m01 = 0;
        if (tid < head) add_byte(p[tid], tid % W, y0 + tid / W, m00, m10, m01);
        if (tail0 + tid < nbytes) { const int i = tail0 + tid; add_byte(p[i], i % W, y0 + i / W, m00, m10, m01); }
        const uint4* pv = reinterpret_cast<const uint4*>(p + head);
        for (int v = tid; v < nvec; v += 256) {
            const uint4 q = pv[v];
            if ((q.x | q.y | q.z | q.w) == 0u) continue;
            const int i0 = head + (v << 4);
            int y = i0 / W, x = i0 - y * W;
            y += y0;
            const unsigned wd[4] = {q.x, q.y, q.z, q.w};
            unsigned c00 = 0, c10 = 0, c01 = 0;                 // 16 bytes: the sums fit 32 bits for every W, H < 2^27
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned on = ((wd[k >> 2] >> (8 * (k & 3))) & 0xffu) ? 1u : 0u;
                c00 += on;
                c10 += on ? (unsigned)x : 0u;
                c01 += on ? (unsigned)y : 0u;
                if (++x == W) { x = 0; ++y; }
            }
            m00 += c00; m10 += c10; m01 += c01;
        }
        if (m00) {
            atomicAdd(&sm[0], (unsigned long long)m00);
            atomicAdd(&sm[1], m10);
            atomicAdd(&sm[2], m01);
        }
    }
    __syncthreads();
    if (tid < 3 && sm[0] != 0ull) atomicAdd(&moments[3 * (size_t)g + tid], sm[tid]);

    // the band's rows of every rescaled mask (zeros outside the source)
    for (int k = 0; k < o.n; ++k) {
        const int f = o.f[k], hk = o.h[k], wk = o.w[k];
        const int r0 = min(j * (o.band / f), hk), r1 = min(r0 + o.band / f, hk);
        const int hs = H / f, ws = W / f;
        uint8_t* __restrict__ dst = o.out[k] + ((size_t)g * hk + r0) * wk;
        const int n = (r1 - r0) * wk;
        for (int i = tid; i < n; i += 256) {
            const int rr = i / wk, c = i - rr * wk, r = r0 + rr;
            unsigned v = 0;
            if (r < hs && c < ws) {
                const uint8_t* a = src + (size_t)(f * r + f / 2 - 1) * W + (f * c + f / 2 - 1);
                const int ones = (a[0] ? 1 : 0) + (a[1] ? 1 : 0) + (a[W] ? 1 : 0) + (a[W + 1] ? 1 : 0);
                v = ones >= kMinOnes ? 1u : 0u;
            }
            dst[i] = (uint8_t)v;
        }
    }
}

// ---- assignment -----------------------------------------------------------------------------------------------------------
// int(a // b) of torch (float) and of Python (double): fmod, (a - mod) / b, the sign fix, floor and the 0.5 correction
template <typename T>
__device__ __forceinline__ int floor_div_int(T a, T b) {
    const T mod = sizeof(T) == 4 ? (T)fmodf((float)a, (float)b) : (T)fmod((double)a, (double)b);
    T div = (a - mod) / b;
    if (mod != T(0) && ((b < T(0)) != (mod < T(0)))) div = div - T(1);
    T fl;
    if (div != T(0)) {
        fl = sizeof(T) == 4 ? (T)floorf((float)div) : (T)floor((double)div);
        if (div - fl > T(0.5)) fl = fl + T(1);
    } else {
        fl = T(0);
    }
    if (!(fl == fl)) return 0;
    const T lim = T(1 << 30);
    return (int)(fl > lim ? lim : (fl < -lim ? -lim : fl));
}

struct AssignCfg {
    int S[kMaxL];
    int first[kMaxL + 1];           // cells of one image in the levels before l
    float lo[kMaxL], hi[kMaxL];
    int n, B, mode, num_classes, Hc, Wc, G;
    float sigma;
};

__global__ __launch_bounds__(256) void solo_assign_kernel(AssignCfg cf, GtOffsets off, const float* __restrict__ gt_boxes,
                                                          const int64_t* __restrict__ gt_labels, const long long* __restrict__ moments,
                                                          int64_t* __restrict__ cate_labels, uint8_t* __restrict__ ins_ind,
                                                          int32_t* __restrict__ cell_owner, int32_t* __restrict__ sel_inst,
                                                          int32_t* __restrict__ pair_cell, int32_t* __restrict__ pair_inst,
                                                          int32_t* __restrict__ counts, int32_t* __restrict__ num_ins,
                                                          int32_t* __restrict__ status) {
    __shared__ int owner[kMaxGrid * kMaxGrid];
    __shared__ int scan[4];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int l = blockIdx.x / cf.B, b = blockIdx.x - l * cf.B;
    const int S = cf.S[l], cells = S * S;
    const int g0 = off.v[b], n_gt = off.v[b + 1] - g0;
    for (int c = tid; c < cells; c += 256) owner[c] = -1;
    if (tid == 0) s_bad = 0;
    __syncthreads();

    const float lo = cf.lo[l], hi = cf.hi[l];
    const float fS = (float)(1.0 / (double)S);             // what `// (1. / num_grid)` holds next to an fp32 tensor
    const double dS = 1.0 / (double)S;
    const float fH = (float)cf.Hc, fW = (float)cf.Wc;
    const size_t pair0 = (size_t)kPairs * ((size_t)l * cf.G + g0);
    int base = 0;
    for (int c0 = 0; c0 < n_gt; c0 += 256) {
        const int i = c0 + tid;
        int top = 0, down = -1, left = 0, right = -1;
        if (i < n_gt) {
            const float* p = gt_boxes + 4 * (size_t)(g0 + i);
            const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
            const float bw = f_sub(x2, x1), bh = f_sub(y2, y1);
            const float area = sqrtf(f_mul(bw, bh));
            const long long m00 = moments[3 * (size_t)(g0 + i)], m10 = moments[3 * (size_t)(g0 + i) + 1], m01 = moments[3 * (size_t)(g0 + i) + 2];
            const bool valid = cf.mode == BXI_SOLO_MODE_DISCOBOX ? m00 > 0 : m00 >= BXI_SOLO_MIN_MASK_SUM;
            if (area >= lo && area <= hi && valid) {
                const int64_t lab = gt_labels[g0 + i];
                if (lab < 0 || lab >= cf.num_classes) {
                    s_bad = 1;
                } else {
                    const float half_w = f_mul(f_mul(0.5f, bw), cf.sigma), half_h = f_mul(f_mul(0.5f, bh), cf.sigma);
                    float cw, ch;
                    int coord_w, coord_h;
                    if (cf.mode == BXI_SOLO_MODE_DISCOBOX) {
                        const float d = (float)m00;                         // clamp(min=1e-6) cannot bind: m00 >= 1
                        cw = f_div((float)m10, d);
                        ch = f_div((float)m01, d);
                        coord_w = floor_div_int<float>(f_div(cw, fW), fS);
                        coord_h = floor_div_int<float>(f_div(ch, fH), fS);
                    } else {
                        const double cwd = (double)m10 / (double)m00, chd = (double)m01 / (double)m00;
                        coord_w = floor_div_int<double>(cwd / (double)cf.Wc, dS);
                        coord_h = floor_div_int<double>(chd / (double)cf.Hc, dS);
                        cw = (float)cwd;
                        ch = (float)chd;
                    }
                    const int top_box = max(0, floor_div_int<float>(f_div(f_sub(ch, half_h), fH), fS));
                    const int down_box = min(S - 1, floor_div_int<float>(f_div(f_add(ch, half_h), fH), fS));
                    const int left_box = max(0, floor_div_int<float>(f_div(f_sub(cw, half_w), fW), fS));
                    const int right_box = min(S - 1, floor_div_int<float>(f_div(f_add(cw, half_w), fW), fS));
                    top = max(top_box, coord_h - 1);
                    down = min(down_box, coord_h + 1);
                    left = max(coord_w - 1, left_box);
                    right = min(right_box, coord_w + 1);
                }
            }
        }
        // 0 <= top, left and down, right <= S - 1 whatever the centre's cell is: every cell below lies inside the grid
        const int rows = down - top + 1, cols = right - left + 1;
        const int cnt = (rows > 0 && cols > 0) ? rows * cols : 0;
        int total;
        const int at = base + block_scan_excl_i32<4>(cnt, scan, total);
        if (cnt > 0) {
            int k = 0;
            for (int y = top; y <= down; ++y)
                for (int x = left; x <= right; ++x, ++k) {
                    const int cell = y * S + x;
                    pair_cell[pair0 + at + k] = cell;
                    pair_inst[pair0 + at + k] = g0 + i;
                    atomicMax(&owner[cell], i);                              // the last writer in loop order: integer, order-free
                }
        }
        base += total;
    }
    for (int k = base + tid; k < kPairs * n_gt; k += 256) {
        pair_cell[pair0 + k] = -1;
        pair_inst[pair0 + k] = -1;
    }
    __syncthreads();

    const size_t row0 = (size_t)cf.B * cf.first[l] + (size_t)b * cells;
    int nset = 0;
    for (int c0 = 0; c0 < cells; c0 += 256) {
        const int c = c0 + tid;
        const int own = c < cells ? owner[c] : -1;
        int total;
        const int at = nset + block_scan_excl_i32<4>(own >= 0 ? 1 : 0, scan, total);
        if (c < cells) {
            cate_labels[row0 + c] = own >= 0 ? gt_labels[g0 + own] : (int64_t)cf.num_classes;
            ins_ind[row0 + c] = own >= 0 ? 1 : 0;
            cell_owner[row0 + c] = own >= 0 ? g0 + own : -1;
            if (own >= 0) sel_inst[row0 + at] = g0 + own;
        }
        nset += total;
    }
    for (int k = nset + tid; k < cells; k += 256) sel_inst[row0 + k] = -1;
    if (tid == 0) {
        counts[2 * (size_t)blockIdx.x] = base;
        counts[2 * (size_t)blockIdx.x + 1] = nset;
        if (nset) atomicAdd(num_ins, nset);
        if (s_bad) atomicOr(status, BXI_SOLO_STATUS_BAD_LABEL);
    }
}

// ---- category loss --------------------------------------------------------------------------------------------------------
struct CateMaps { const float* cls[kMaxL]; float* gcls[kMaxL]; };

template <bool G2>
__global__ __launch_bounds__(256) void solo_cate_focal_kernel(CateMaps m, LocGrid g, FlatGrid f, int C, const int64_t* __restrict__ labels,
                                                              const int32_t* __restrict__ num_ins, float gamma, float alpha, float lw,
                                                              int32_t* __restrict__ partials) {
    __shared__ double s4d[4];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
    while (l + 1 < f.n && blk >= f.blk_first[l + 1]) ++l;
    const int count = f.count[l];
    const int e0 = (blk - f.blk_first[l]) * kElemTile + tid * 4;
    const int hw = g.H[l] * g.W[l];
    const float* __restrict__ src = m.cls[l];
    float* __restrict__ dst = m.gcls[l];
    const float denom = (float)(num_ins[0] + 1) + FLT_EPSILON;          // avg_factor = num_ins + 1, then weight_reduce_loss's eps
    const float scale = lw / denom;
    const double tot = focal_tile<G2>(src, dst, count, e0, hw, C, (size_t)g.B * g.first[l], labels, gamma, alpha, scale, s4d);
    if (tid == 0) {                                         // the partial stays fp64 (two words: the workspace is 4-byte aligned)
        const long long bits = __double_as_longlong(tot * (double)scale);
        partials[2 * (size_t)blk] = (int32_t)bits;
        partials[2 * (size_t)blk + 1] = (int32_t)(bits >> 32);
    }
}

__global__ __launch_bounds__(256) void solo_cate_finish_kernel(const int32_t* __restrict__ partials, int n_blocks, float* __restrict__ out) {
    __shared__ double s4d[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += 256)
        a += __longlong_as_double(((long long)partials[2 * (size_t)i + 1] << 32) | (unsigned int)partials[2 * (size_t)i]);
    a = block_sum_4w_f64(a, s4d);
    if (threadIdx.x == 0) out[0] = (float)a;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int cate_grid(const int* num_grids_host, int n_levels, int B, int C, LocGrid& g, FlatGrid& f, int64_t& blocks) {
    if (n_levels < 1 || n_levels > kMaxL || C < 1) return BXI_ERR_BAD_SHAPE;
    if (!num_grids_host) return BXI_ERR_NULL_POINTER;
    int S[kMaxL], one[kMaxL];
    for (int l = 0; l < n_levels; ++l) {
        S[l] = num_grids_host[l];
        one[l] = 1;
        if (S[l] < 1 || S[l] > kMaxGrid) return BXI_ERR_BAD_SHAPE;
    }
    if (int rc = make_grid(S, S, one, n_levels, B, g)) return rc;
    const int chan[1] = {C};
    blocks = make_flat(g, chan, 1, f);
    return blocks < 0 ? BXI_ERR_BAD_SHAPE : BXI_OK;
}

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" int bxi_solo_mask_pass_u8(const uint8_t* const* masks_host, const int* gt_offsets_host, const int* img_h_host, const int* img_w_host,
                                     int B, const int* factors_host, const int* out_h_host, const int* out_w_host, int n_factors,
                                     uint8_t* const* rescaled_host, int64_t* moments, void* stream) {
    GtOffsets off;
    if (int rc = read_offsets(gt_offsets_host, B, off)) return rc;
    if (n_factors < 0 || n_factors > kMaxF) return BXI_ERR_UNSUPPORTED;
    if (B == 0 || off.v[B] == 0) return BXI_OK;
    const int G = off.v[B];
    if (!masks_host || !img_h_host || !img_w_host || !moments || (n_factors > 0 && (!factors_host || !out_h_host || !out_w_host || !rescaled_host)))
        return BXI_ERR_NULL_POINTER;
    if (reinterpret_cast<uintptr_t>(moments) & 7) return BXI_ERR_BAD_ARGUMENT;
    MaskOuts o;
    o.n = n_factors;
    int maxf = 1;
    for (int k = 0; k < n_factors; ++k) {
        const int f = factors_host[k];
        if (f < 2 || f > BXI_SOLO_MAX_FACTOR || (f & 1)) return BXI_ERR_UNSUPPORTED;
        maxf = f > maxf ? f : maxf;
    }
    for (int k = 0; k < kMaxF; ++k) {
        o.out[k] = nullptr; o.f[k] = 2; o.h[k] = 0; o.w[k] = 0;
        if (k < n_factors) {
            if (maxf % factors_host[k]) return BXI_ERR_UNSUPPORTED;
            if (out_h_host[k] < 1 || out_w_host[k] < 1 || !fits_i32((int64_t)out_h_host[k] * out_w_host[k])) return BXI_ERR_BAD_SHAPE;
            if (!rescaled_host[k]) return BXI_ERR_NULL_POINTER;
            o.out[k] = rescaled_host[k]; o.f[k] = factors_host[k]; o.h[k] = out_h_host[k]; o.w[k] = out_w_host[k];
        }
    }
    o.band = maxf * ((kMinBand + maxf - 1) / maxf);
    MaskImgs im;
    im.B = B;
    int64_t rows = 1;
    for (int k = 0; k < n_factors; ++k) rows = std::max<int64_t>(rows, (int64_t)o.h[k] * o.f[k]);
    for (int b = 0; b < BXI_MAX_IMAGES; ++b) {
        im.ptr[b] = nullptr; im.H[b] = 1; im.W[b] = 1;
        im.off[b] = off.v[b];
        if (b < B && off.v[b + 1] > off.v[b]) {
            const int H = img_h_host[b], W = img_w_host[b];
            if (H < 1 || W < 1 || !fits_i32((int64_t)H * W)) return BXI_ERR_BAD_SHAPE;
            if (H % maxf || W % maxf) return BXI_ERR_UNSUPPORTED;
            if (!masks_host[b]) return BXI_ERR_NULL_POINTER;
            for (int k = 0; k < n_factors; ++k)
                if (o.h[k] < H / o.f[k] || o.w[k] < W / o.f[k]) return BXI_ERR_BAD_SHAPE;
            im.ptr[b] = masks_host[b]; im.H[b] = H; im.W[b] = W;
            rows = std::max<int64_t>(rows, H);
        }
    }
    im.off[BXI_MAX_IMAGES] = off.v[BXI_MAX_IMAGES];
    o.nb = (int)((rows + o.band - 1) / o.band);
    if (!fits_i32((int64_t)G * o.nb)) return BXI_ERR_BAD_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(moments, 0, 24 * (size_t)G, s) != hipSuccess) { check_launch(); return BXI_ERR_LAUNCH; }
    BXI_LAUNCH("solo_mask_pass", s, solo_mask_pass_kernel, dim3((unsigned)(G * o.nb)), dim3(256), 0, s, im, o,
               reinterpret_cast<unsigned long long*>(moments));
    return check_launch();
}

extern "C" int bxi_solo_assign_f32(int mode, int B, int n_levels, const int* num_grids_host, const float* scale_ranges_host, double sigma,
                                   int num_classes, int canvas_h, int canvas_w, const float* gt_boxes, const int64_t* gt_labels,
                                   const int64_t* moments, const int* gt_offsets_host, int64_t* cate_labels, uint8_t* ins_ind_labels,
                                   int32_t* cell_owner, int32_t* sel_inst, int32_t* pair_cell, int32_t* pair_inst, int32_t* counts,
                                   int32_t* num_ins, int32_t* status, void* stream) {
    if (n_levels < 1 || n_levels > kMaxL || num_classes < 1 || canvas_h < 1 || canvas_w < 1) return BXI_ERR_BAD_SHAPE;
    GtOffsets off;
    if (int rc = read_offsets(gt_offsets_host, B, off)) return rc;
    if (mode != BXI_SOLO_MODE_DISCOBOX && mode != BXI_SOLO_MODE_BOXLEVELSET) return BXI_ERR_BAD_ARGUMENT;
    if (B == 0) return BXI_OK;
    if (!num_grids_host || !scale_ranges_host) return BXI_ERR_NULL_POINTER;
    if (sigma != sigma) return BXI_ERR_BAD_ARGUMENT;
    AssignCfg cf;
    cf.n = n_levels; cf.B = B; cf.mode = mode; cf.num_classes = num_classes; cf.Hc = canvas_h; cf.Wc = canvas_w; cf.G = off.v[B];
    cf.sigma = (float)sigma;
    int64_t at = 0;
    for (int l = 0; l < kMaxL; ++l) {
        cf.S[l] = 1; cf.lo[l] = 0.f; cf.hi[l] = 0.f;
        cf.first[l] = (int)at;
        if (l < n_levels) {
            const int S = num_grids_host[l];
            if (S < 1 || S > kMaxGrid) return BXI_ERR_BAD_SHAPE;
            cf.S[l] = S;
            cf.lo[l] = scale_ranges_host[2 * l];
            cf.hi[l] = scale_ranges_host[2 * l + 1];
            if (cf.lo[l] != cf.lo[l] || cf.hi[l] != cf.hi[l]) return BXI_ERR_BAD_ARGUMENT;
            at += (int64_t)S * S;
        }
    }
    cf.first[kMaxL] = (int)at;
    if (!fits_i32((int64_t)kPairs * n_levels * cf.G + 1)) return BXI_ERR_BAD_SHAPE;
    if (!cate_labels || !ins_ind_labels || !cell_owner || !sel_inst || !counts || !num_ins || !status ||
        (cf.G > 0 && (!gt_boxes || !gt_labels || !moments || !pair_cell || !pair_inst)))
        return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(num_ins, 0, 4, s) != hipSuccess || hipMemsetAsync(status, 0, 4, s) != hipSuccess) { check_launch(); return BXI_ERR_LAUNCH; }
    BXI_LAUNCH("solo_assign", s, solo_assign_kernel, dim3((unsigned)(n_levels * B)), dim3(256), 0, s, cf, off, gt_boxes, gt_labels,
               reinterpret_cast<const long long*>(moments), cate_labels, ins_ind_labels, cell_owner, sel_inst, pair_cell, pair_inst, counts,
               num_ins, status);
    return check_launch();
}

extern "C" size_t bxi_solo_cate_workspace_bytes(const int* num_grids_host, int n_levels, int B, int C) {
    LocGrid g;
    FlatGrid f;
    int64_t blocks = 0;
    if (B < 1 || cate_grid(num_grids_host, n_levels, B, C, g, f, blocks) != BXI_OK) return 0;
    return 8 * (size_t)blocks;
}

extern "C" int bxi_solo_cate_loss_f32(const float* const* cate_preds_host, const int* num_grids_host, int n_levels, int B, int C,
                                      const int64_t* cate_labels, const int32_t* num_ins, float gamma, float alpha, float loss_weight,
                                      float* const* grads_host, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    LocGrid g;
    FlatGrid f;
    int64_t blocks = 0;
    if (int rc = cate_grid(num_grids_host, n_levels, B, C, g, f, blocks)) return rc;
    if (B == 0) return BXI_OK;
    if (!(gamma >= 0.f) || alpha != alpha || loss_weight != loss_weight) return BXI_ERR_BAD_ARGUMENT;
    if (!cate_preds_host || !grads_host || !cate_labels || !num_ins || !loss) return BXI_ERR_NULL_POINTER;
    CateMaps m;
    for (int l = 0; l < kMaxL; ++l) {
        m.cls[l] = nullptr; m.gcls[l] = nullptr;
        if (l < n_levels) {
            if (!cate_preds_host[l] || !grads_host[l]) return BXI_ERR_NULL_POINTER;
            m.cls[l] = cate_preds_host[l]; m.gcls[l] = grads_host[l];
        }
    }
    if (!workspace_ok(workspace, workspace_bytes, 8 * (size_t)blocks, 4)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    int32_t* part = static_cast<int32_t*>(workspace);
    if (gamma == 2.f)
        BXI_LAUNCH("solo_cate_focal_g2", s, solo_cate_focal_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, m, g, f, C, cate_labels, num_ins,
                   gamma, alpha, loss_weight, part);
    else
        BXI_LAUNCH("solo_cate_focal", s, solo_cate_focal_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, m, g, f, C, cate_labels, num_ins,
                   gamma, alpha, loss_weight, part);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("solo_cate_finish", s, solo_cate_finish_kernel, dim3(1), dim3(256), 0, s, part, (int)blocks, loss);
    return check_launch();
}

extern "C" int bxi_solo_cate_grad_rescale_f32(const int* num_grids_host, int n_levels, int B, int C, const float* const* unit_host,
                                              const float* upstream, float* const* out_host, void* stream) {
    LocGrid g;
    FlatGrid f;
    int64_t blocks = 0;
    if (int rc = cate_grid(num_grids_host, n_levels, B, C, g, f, blocks)) return rc;
    if (B == 0) return BXI_OK;
    if (!unit_host || !out_host || !upstream) return BXI_ERR_NULL_POINTER;
    RescaleSegs sg;
    for (int s = 0; s < 3 * kMaxL; ++s) {
        sg.src[s] = nullptr; sg.dst[s] = nullptr; sg.which[s] = 0;
        if (s < f.n) {
            sg.src[s] = unit_host[s]; sg.dst[s] = out_host[s];
            if (!sg.src[s] || !sg.dst[s]) return BXI_ERR_NULL_POINTER;
        }
    }
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("solo_cate_grad_rescale", s, flat_rescale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, sg, f, upstream);
    return check_launch();
}
