// inst_post.hip -- Box2Mask at test time on gfx950: what the reference does after the decoder (box2mask_head.py:445-459,
// maskformer_fusion_head.py:112-162 and :207-241, mask2bbox of mmdet/core/mask/utils.py:68-89), without a full-size fp32 canvas.
//
// inst_topk_kernel   one workgroup of 1024 threads per image.
//   1. one wave per query row: the fp32 softmax over its C + 1 logits (wave maximum, every lane's expf in column order, the wave total
//      in the fixed DPP order, one division), the background column dropped; every score becomes a 64-bit key in LDS,
//      (order-preserving score bits << 32) | (2^32 - 1 - flat index), a NaN score the smallest score key there is;
//   2. a bitonic sort of the keys, descending, padded to a power of two with keys below every real one: the first k are the selection in
//      the defined order (descending score, ascending flat index among equals, NaN last); steps inside a block of 512 keys are one
//      wave's own business, in registers, the workgroup meets only around the steps that cross blocks;
//   3. the is_thing filter as an exclusive scan in that order; rows behind the count are written as (0, -1, -1).
// inst_paste_kernel  the tile of paste_device.hpp with STATS and SCORE on the raw logits, read through query[i]: one workgroup = one mask x
//   one band of output rows x one chunk of columns; per row of the chunk the count, first / last set column and the fp32 sum of
//   sigmoid(p) over the set pixels go to the row's own workspace slot by plain stores.
// inst_stats_kernel  one workgroup per mask folds its slots: integer statistics as seg_stats_kernel, the sums in fp64 (every thread its
//   slots in ascending order, the wave total in the fixed DPP order, the four waves in wave order), then mask score, box and det score.
#include "paste_device.hpp"

#include "../../include/boxinst/boxinst_hip_inst.h"

namespace bxi {

constexpr int kTopkThreads = 1024;
constexpr int kTopkWaves = kTopkThreads / kWave;

constexpr int kTopkLocal = 512;                                   // keys of a block one wave sorts on its own

// a score and its flat index as one key whose descending order is the defined one: score descending (NaN below every number), index ascending
__device__ __forceinline__ unsigned long long score_key(float v, uint32_t idx) {
    const uint32_t sk = v == v ? float_key(v) : 0u;
    return ((unsigned long long)sk << 32) | (unsigned long long)(0xffffffffu - idx);
}
// one compare-exchange of the bitonic network: keys i and i + stride, descending where bit `size` of i is clear
__device__ __forceinline__ void key_step(unsigned long long* keys, int i, int stride, int size) {
    const int j = i + stride;
    const unsigned long long a = keys[i], c = keys[j];
    const bool down = (i & size) == 0;
    if ((a < c) == down && a != c) { keys[i] = c; keys[j] = a; }
}
// A wave's block of 512 keys in registers: lane l holds keys l, 64 + l, ..., 448 + l of the block (consecutive lanes read consecutive
// keys: no LDS bank conflicts; eight consecutive keys per lane would hit the same banks 16 ways).  p = block start + l.
__device__ __forceinline__ void load_keys(unsigned long long (&r)[8], const unsigned long long* p) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = p[kWave * j];
}
__device__ __forceinline__ void store_keys(unsigned long long* p, const unsigned long long (&r)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) p[kWave * j] = r[j];
}
// partners 64 S apart (S = 1, 2, 4): both in this lane
template <int S>
__device__ __forceinline__ void lane_step(unsigned long long (&r)[8], int base, int size) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if ((j & S) == 0) {
            const unsigned long long a = r[j], c = r[j + S];
            const bool down = ((base + kWave * j) & size) == 0;
            if ((a < c) == down) { r[j] = c; r[j + S] = a; }
        }
    }
}
// the key of lane ^ LX at the same j: the two quad permutations on the VALU's DPP path, the rest through the LDS crossbar
template <int LX>
__device__ __forceinline__ unsigned long long key_of_lane_xor(unsigned long long v) {
    if (LX == 1 || LX == 2) {
        const int ctrl = LX == 1 ? 0xB1 : 0x4E;                   // quad_perm:[1,0,3,2] / [2,3,0,1]
        return ((unsigned long long)(unsigned int)dpp_i32((int)(v >> 32), ctrl) << 32) | (unsigned int)dpp_i32((int)v, ctrl);
    }
    return __shfl_xor(v, LX);
}
// partners LX < 64 apart: in lane ^ LX at the same j
template <int LX>
__device__ __forceinline__ void cross_step(unsigned long long (&r)[8], int base, int size) {
    const bool low = ((threadIdx.x & 63) & LX) == 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned long long o = key_of_lane_xor<LX>(r[j]);
        const bool take_max = low == (((base + kWave * j) & size) == 0);
        r[j] = take_max ? (o > r[j] ? o : r[j]) : (o < r[j] ? o : r[j]);
    }
}
// the steps of the merge of `size` with partners from `stride` (<= 256) down to 1 apart, on a block in registers; base = the index of
// the lane's first key
__device__ __forceinline__ void wave_steps(unsigned long long (&r)[8], int base, int size, int stride) {
    if (stride >= 256) lane_step<4>(r, base, size);
    if (stride >= 128) lane_step<2>(r, base, size);
    if (stride >= 64) lane_step<1>(r, base, size);
    if (stride >= 32) cross_step<32>(r, base, size);
    if (stride >= 16) cross_step<16>(r, base, size);
    if (stride >= 8) cross_step<8>(r, base, size);
    if (stride >= 4) cross_step<4>(r, base, size);
    if (stride >= 2) cross_step<2>(r, base, size);
    cross_step<1>(r, base, size);
}

__global__ void __launch_bounds__(kTopkThreads) inst_topk_kernel(const float* __restrict__ cls, int Q, int C, int num_things, int k, int P,
                                                                 float* __restrict__ scores, int64_t* __restrict__ labels,
                                                                 int64_t* __restrict__ query, int32_t* __restrict__ count) {
    extern __shared__ unsigned long long keys[];                  // [P]
    __shared__ int part[kTopkWaves];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = Q * C, C1 = C + 1;
    const float* mine = cls + (size_t)b * Q * C1;

    // 1. scores -> keys.  Up to 256 columns a lane holds its (at most four) logits in registers: one trip to memory per row; the sums
    // are taken in the same order on both paths (every lane its columns ascending, then the wave total), so the bits do not depend on it.
    for (int q = wave; q < Q; q += kTopkWaves) {
        const float* row = mine + (size_t)q * C1;
        float m = -INFINITY, s = 0.f;
        if (C1 <= 4 * kWave) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lane + j * kWave < C1 ? row[lane + j * kWave] : -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, v[j]);
            m = wave_max_f32(m);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = expf(v[j] - m);
                if (lane + j * kWave < C1) s += v[j];
            }
            s = wave_total_f32(s);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = lane + j * kWave;
                if (c < C) keys[q * C + c] = score_key(v[j] / s, (uint32_t)(q * C + c));
            }
        } else {
            for (int c = lane; c < C1; c += kWave) m = fmaxf(m, row[c]);
            m = wave_max_f32(m);
            for (int c = lane; c < C1; c += kWave) s += expf(row[c] - m);
            s = wave_total_f32(s);
            for (int c = lane; c < C; c += kWave) keys[q * C + c] = score_key(expf(row[c] - m) / s, (uint32_t)(q * C + c));
        }
    }
    for (int i = N + (int)threadIdx.x; i < P; i += kTopkThreads) keys[i] = 0ull;
    __syncthreads();

    // 2. bitonic sort, descending.  A step whose partners are less than kTopkLocal = 512 apart stays inside an aligned block of 512 keys,
    // and a block belongs to ONE wave for a whole run of such steps: the wave takes the block into registers (8 keys per lane, 64
    // apart), exchanges across lanes for partners 1 .. 32 apart and inside the lane for 64 .. 256, and puts it back.  The workgroup meets
    // after the blocks' own sort (sizes 2 .. 512), after every step with partners 512 or more apart (in LDS), and after every run of
    // local steps: 15 barriers at P = 8192 instead of 91, and no LDS round trip per step in between.
    for (int blk = wave; blk < P / kTopkLocal; blk += kTopkWaves) {
        const int base = blk * kTopkLocal + lane;
        unsigned long long r[8];
        load_keys(r, keys + base);
        for (int size = 2; size <= kTopkLocal; size <<= 1) wave_steps(r, base, size, size >> 1);
        store_keys(keys + base, r);
    }
    __syncthreads();
    for (int size = 2 * kTopkLocal; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= kTopkLocal; stride >>= 1) {
#pragma unroll 4
            for (int t = threadIdx.x; t < (P >> 1); t += kTopkThreads) key_step(keys, 2 * t - (t & (stride - 1)), stride, size);
            __syncthreads();
        }
        for (int blk = wave; blk < P / kTopkLocal; blk += kTopkWaves) {
            const int base = blk * kTopkLocal + lane;
            unsigned long long r[8];
            load_keys(r, keys + base);
            wave_steps(r, base, size, kTopkLocal >> 1);
            store_keys(keys + base, r);
        }
        __syncthreads();
    }

    // 3. the things among the first k, in order
    float* out_s = scores + (size_t)b * k;
    int64_t* out_l = labels + (size_t)b * k;
    int64_t* out_q = query + (size_t)b * k;
    int running = 0;
    for (int base = 0; base < k; base += kTopkThreads) {
        const int i = base + (int)threadIdx.x;
        const bool in = i < k;
        const unsigned long long key = in ? keys[i] : 0ull;
        const uint32_t idx = 0xffffffffu - (uint32_t)key, sk = (uint32_t)(key >> 32);
        const int qi = in ? (int)(idx / (uint32_t)C) : 0;
        const int label = in ? (int)idx - qi * C : 0;
        const int keep = in && label < num_things ? 1 : 0;
        int total;
        const int pos = running + block_scan_excl_i32<kTopkWaves>(keep, part, total);
        if (keep) {
            out_s[pos] = sk ? key_float(sk) : __int_as_float(0x7fc00000);
            out_l[pos] = label;
            out_q[pos] = qi;
        }
        running += total;
    }
    for (int i = running + (int)threadIdx.x; i < k; i += kTopkThreads) { out_s[i] = 0.f; out_l[i] = -1; out_q[i] = -1; }
    if (threadIdx.x == 0) count[b] = running;
}

struct InstArgs {
    const float* logits;
    const int64_t* query;
    uint8_t* masks;
    int4* rows;                                     // workspace: [n][out_h][chunks]
    int n_all, h, w, up_h, up_w;
    int crop_h, crop_w, out_h, out_w;
    float scale1_h, scale1_w, scale2_h, scale2_w;
    int band_rows, rows_cap, kw, bands, chunks;
};

__global__ void __launch_bounds__(kPasteThreads) inst_paste_kernel(const InstArgs a) {
    extern __shared__ float lds[];
    const int band = (int)(blockIdx.x % (unsigned)a.bands);
    const int rest = (int)(blockIdx.x / (unsigned)a.bands);
    const int chunk = rest % a.chunks;
    const int i = rest / a.chunks;
    const int64_t k = a.query[i];
    const bool valid = k >= 0 && k < a.n_all;
    const int Y0 = band * a.band_rows, X0 = chunk * kChunkCols;                 // inside the output: the grid is exact (one image)
    PasteTile t;
    t.plane = a.logits + (size_t)(valid ? k : 0) * a.h * a.w;
    t.base = a.masks + (size_t)i * a.out_h * a.out_w;
    t.w = a.w; t.kw = a.kw; t.rows_cap = a.rows_cap;
    t.crop_h = a.crop_h; t.crop_w = a.crop_w; t.out_h = a.out_h; t.out_w = a.out_w;
    t.s2h = a.scale2_h; t.s2w = a.scale2_w; t.thr = 0.f;
    t.Y0 = Y0; t.Y1 = Y0 + a.band_rows < a.out_h ? Y0 + a.band_rows : a.out_h;
    t.X0 = X0; t.cw = a.out_w - X0 < kChunkCols ? a.out_w - X0 : kChunkCols;
    int4* rows = a.rows + ((size_t)i * a.out_h + Y0) * a.chunks + chunk;
    paste_tile<false, true, true>(lds, t, ResizeAxis{a.h, a.up_h, a.scale1_h}, ResizeAxis{a.w, a.up_w, a.scale1_w}, valid, rows, a.chunks);
}

__global__ void __launch_bounds__(kPasteThreads) inst_stats_kernel(const int4* __restrict__ rows, int out_h, int chunks,
                                                                   const float* __restrict__ cls_scores, int32_t* __restrict__ stats,
                                                                   float* __restrict__ mask_scores, float* __restrict__ boxes) {
    __shared__ int red[5][kPasteThreads / kWave];
    __shared__ double red_sum[kPasteThreads / kWave];
    const int i = blockIdx.x;
    const int4* mine = rows + (size_t)i * out_h * chunks;
    int area = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    double sum = 0.0;
    const int slots = out_h * chunks;
    for (int s = threadIdx.x; s < slots; s += kPasteThreads) {
        const int4 r = mine[s];
        if (r.x > 0) {
            const int y = s / chunks;
            area += r.x;
            sum += (double)__int_as_float(r.w);
            x0 = min(x0, r.y); x1 = max(x1, r.z);
            y0 = min(y0, y); y1 = max(y1, y);
        }
    }
    area = wave_total_i32(area);
    sum = wave_total_f64(sum);
    x0 = wave_min_i32(x0); y0 = wave_min_i32(y0);
    x1 = -wave_min_i32(-x1); y1 = -wave_min_i32(-y1);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        red[0][wv] = area; red[1][wv] = x0; red[2][wv] = y0; red[3][wv] = x1; red[4][wv] = y1;
        red_sum[wv] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < kPasteThreads / kWave; ++wv) {
            area += red[0][wv];
            sum += red_sum[wv];
            x0 = min(x0, red[1][wv]); y0 = min(y0, red[2][wv]);
            x1 = max(x1, red[3][wv]); y1 = max(y1, red[4][wv]);
        }
        int32_t* o = stats + 5 * (size_t)i;
        o[0] = area;
        o[1] = area ? x0 : -1; o[2] = area ? y0 : -1; o[3] = area ? x1 : -1; o[4] = area ? y1 : -1;
        const float ms = (float)(sum / ((double)area + 1e-6));
        mask_scores[i] = ms;
        float* bx = boxes + 5 * (size_t)i;
        bx[0] = area ? (float)x0 : 0.f; bx[1] = area ? (float)y0 : 0.f;
        bx[2] = area ? (float)(x1 + 1) : 0.f; bx[3] = area ? (float)(y1 + 1) : 0.f;
        bx[4] = cls_scores[i] * ms;
    }
}

// shapes the entry point and the size query accept
static bool inst_shape_ok(int n, int out_h, int out_w) {
    if (n < 0 || out_h < 1 || out_w < 1 || !fits_i32((int64_t)out_h * out_w)) return false;
    const int64_t bands = (out_h + kBandRows - 1) / kBandRows, chunks = (out_w + kChunkCols - 1) / kChunkCols;
    return fits_i32((int64_t)n * bands) && fits_i32((int64_t)n * bands * chunks);
}

}  // namespace bxi

extern "C" int bxi_inst_topk_f32(const float* cls, int B, int Q, int C, int num_things, int k, float* scores, int64_t* labels, int64_t* query,
                                 int32_t* count, void* stream) {
    using namespace bxi;
    if (B < 0 || Q < 1 || C < 1 || k < 1 || num_things < 0 || num_things > C) return BXI_ERR_BAD_SHAPE;
    if (!fits_i32((int64_t)B * Q * ((int64_t)C + 1))) return BXI_ERR_BAD_SHAPE;
    const int64_t N = (int64_t)Q * C;
    if (k > N || N > BXI_INST_TOPK_MAX) return BXI_ERR_UNSUPPORTED;
    if (B == 0) return BXI_OK;
    if (!cls || !scores || !labels || !query || !count) return BXI_ERR_NULL_POINTER;
    int P = kTopkLocal;                                                   // a power of two >= Q * C, whole blocks of kTopkLocal keys
    while (P < (int)N) P <<= 1;
    const size_t lds = sizeof(unsigned long long) * (size_t)P;
    if (lds > 48 * 1024) {
        static std::atomic<int> attr_set{0};
        if (!attr_set.load(std::memory_order_relaxed)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(inst_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(sizeof(unsigned long long) * BXI_INST_TOPK_MAX));
            if (e != hipSuccess) { set_last_hip_error((int)e); return BXI_ERR_LAUNCH; }
            attr_set.store(1, std::memory_order_relaxed);
        }
    }
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("inst_topk", s, inst_topk_kernel, dim3((unsigned)B), dim3(kTopkThreads), lds, s, cls, Q, C, num_things, k, P, scores, labels,
               query, count);
    return check_launch();
}

extern "C" size_t bxi_inst_paste_workspace_bytes(int n, int out_h, int out_w) {
    using namespace bxi;
    if (!inst_shape_ok(n, out_h, out_w)) return 0;
    const size_t chunks = (size_t)(out_w + kChunkCols - 1) / kChunkCols;
    return sizeof(int4) * (size_t)n * (size_t)out_h * chunks;
}

extern "C" int bxi_inst_paste_u8(const float* logits, int n_all, int h, int w, const int64_t* query, const float* cls_scores, int n, int up_h,
                                 int up_w, int crop_h, int crop_w, int out_h, int out_w, uint8_t* masks, int32_t* stats, float* mask_scores,
                                 float* boxes, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (n_all < 1 || h < 1 || w < 1 || up_h < 1 || up_w < 1 || crop_h < 1 || crop_w < 1 || crop_h > up_h || crop_w > up_w) return BXI_ERR_BAD_SHAPE;
    if (!inst_shape_ok(n, out_h, out_w) || !fits_i32((int64_t)h * w) || !fits_i32((int64_t)n_all * h * w)) return BXI_ERR_BAD_SHAPE;
    if (n == 0) return BXI_OK;
    if (!logits || !query || !cls_scores || !masks || !stats || !mask_scores || !boxes) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_inst_paste_workspace_bytes(n, out_h, out_w), 16)) return BXI_ERR_WORKSPACE;
    InstArgs a;
    a.n_all = n_all; a.h = h; a.w = w; a.up_h = up_h; a.up_w = up_w;
    a.crop_h = crop_h; a.crop_w = crop_w; a.out_h = out_h; a.out_w = out_w;
    a.scale1_h = (float)h / (float)up_h;                                  // compute_scales_value: (float)in / out
    a.scale1_w = (float)w / (float)up_w;
    a.scale2_h = (float)crop_h / (float)out_h;
    a.scale2_w = (float)crop_w / (float)out_w;
    const int chunk = out_w < kChunkCols ? out_w : kChunkCols;
    a.kw = (chunk + 15) / 16 * 16;
    a.chunks = (out_w + kChunkCols - 1) / kChunkCols;
    size_t lds = 0;
    const bool fits = choose_band(h, w, a.kw, true, [&](int band_rows) {
        return band_rows_needed(band_rows, crop_h, out_h, a.scale2_h, ResizeAxis{h, up_h, a.scale1_h});
    }, a.band_rows, a.rows_cap, lds, true);
    if (!fits) return BXI_ERR_UNSUPPORTED;                                // source rows wider than ~5000 columns
    a.bands = (out_h + a.band_rows - 1) / a.band_rows;
    const int64_t grid = (int64_t)n * a.chunks * a.bands;
    if (grid * kPasteThreads > 0xffffffffLL) return BXI_ERR_UNSUPPORTED;   // the dispatch's 32-bit work-item count
    a.logits = logits; a.query = query; a.masks = masks; a.rows = static_cast<int4*>(workspace);
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("inst_paste", s, inst_paste_kernel, dim3((unsigned)grid), dim3(kPasteThreads), lds, s, a);
    int rc = check_launch();
    if (rc != BXI_OK) return rc;
    BXI_LAUNCH("inst_stats", s, inst_stats_kernel, dim3((unsigned)n), dim3(kPasteThreads), 0, s, a.rows, out_h, a.chunks, cls_scores, stats,
               mask_scores, boxes);
    return check_launch();
}
