// corr.hip -- DiscoBox's cross-image correspondence (include/boxinst/boxinst_hip_corr.h): plan, retrieval, solver with loss_corr and its
// gradient, the inter-image mask iiu, append, and superres_T for callers that want the matrix.  gfx950 only.
//
// Every reduction is kept in fp64 in a fixed order and rounded once; the data is fp32.  No atomics: a launch writes every element of its
// outputs from exactly one thread.
#include "common.hpp"
#include "../../include/boxinst/boxinst_hip_corr.h"

#pragma clang fp contract(off)

namespace bxi {
namespace {

constexpr int kF = BXI_CORR_FEAT, kFF = kF * kF, kM = BXI_CORR_MASK, kMM = kM * kM, kPairs = kFF * kFF;
constexpr int kMaxK = BXI_CORR_MAX_OBJS, kMaxQueue = BXI_CORR_MAX_QUEUE;
constexpr int kChunk = 16;          // channels staged in LDS at a time
constexpr int kCiThreads = 196, kCiParts = kMM / kCiThreads;   // 4 x 196 = 784 source pixels

struct Work {
    float* T; float* gpart; float* cipart; double* rowloss;
};
__host__ __device__ inline size_t carve_work(void* base, int N, int C, int K, Work& w) {
    Carver cv(base, 16);
    const size_t nk = (size_t)N * K;
    w.T = cv.take<float>(nk * kPairs);
    w.gpart = cv.take<float>(nk * (size_t)C * kFF);
    w.cipart = cv.take<float>(nk * 2 * kMM);
    w.rowloss = cv.take<double>(nk);
    const size_t b = cv.bytes();
    return b < 16 ? 16 : b;
}

__device__ __forceinline__ bool flagged(const float* boxes, const int64_t* labels, int j, int num_class, float min_size) {
    const long long c = labels[j];
    const float* b = boxes + 4 * (size_t)j;
    return c >= 0 && c < num_class && (b[2] - b[0]) > min_size && (b[3] - b[1]) > min_size;
}

// ---- plan: one workgroup -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void corr_plan_kernel(const float* boxes, const int64_t* labels, const int32_t* ptr, int N, int num_class, int L,
                                                        float min_size, int32_t* obj_slot, int32_t* obj_role) {
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        int slot = -1, role = 0;
        if (flagged(boxes, labels, j, num_class, min_size)) {
            const long long c = labels[j];
            int rank = 0, total = 0;
            for (int i = 0; i < N; ++i)
                if (labels[i] == c && flagged(boxes, labels, i, num_class, min_size)) { ++total; rank += i < j; }
            int p = ptr[c] % L;
            if (p < 0) p += L;
            slot = (int)(((long long)p + rank) % L);
            role = (rank >= total - L ? 1 : 0) | (rank == total - 1 ? 2 : 0);
        }
        obj_slot[j] = slot;
        obj_role[j] = role;
    }
}

// the 28 -> 7 bilinear value of cell (y, x): the mean of the middle 2 x 2 of its 4 x 4 block, in torch's order
__device__ __forceinline__ float mask7(const float* m, int cell) {
    const int y = cell / kF, x = cell % kF;
    const float* r0 = m + (4 * y + 1) * kM + 4 * x + 1;
    return 0.5f * (0.5f * r0[0] + 0.5f * r0[1]) + 0.5f * (0.5f * r0[kM] + 0.5f * r0[kM + 1]);
}

// the latest earlier object of this call planned for slot s of class c, or -1: the stored entry shows
__device__ __forceinline__ int in_call_source(const int64_t* labels, const int32_t* obj_slot, int i, long long c, int s) {
    int v = -1;
    for (int j = 0; j < i; ++j)
        if (labels[j] == c && obj_slot[j] == s) v = j;
    return v;
}

// ---- retrieval: one workgroup per (object, four slots), one wave per visible slot ------------------------------------------------------------
__global__ __launch_bounds__(256) void corr_retrieve_kernel(const float* s_feat, const float* s_mask, const float* t_feat, const float* t_mask,
                                                            const float* boxes, const int64_t* labels, const int32_t* obj_slot, int C,
                                                            const float* bank_feature, const float* bank_mask, const float* bank_box, int num_class,
                                                            int L, float fg_thresh, float bg_thresh, float appear_thresh, float ratio_lo,
                                                            float ratio_hi, int32_t* slot_pass, float* scores) {
    __shared__ float qm[kMM];
    __shared__ float qm7[kFF];
    __shared__ float mm[4][kFF];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y * 4 + wave;
    const bool live = s < L;
    const long long c = labels[i];
    if (c < 0 || c >= num_class) {       // uniform for the workgroup
        if (live && lane == 0) {
            slot_pass[(size_t)i * L + s] = 0;
            if (scores)
                for (int e = 0; e < 4; ++e) scores[((size_t)i * L + s) * 4 + e] = 0.f;
        }
        return;
    }
    for (int e = tid; e < kMM; e += blockDim.x) qm[e] = s_mask[(size_t)i * kMM + e];
    __syncthreads();
    if (tid < kFF) qm7[tid] = mask7(qm, tid);
    const int CE = C * kFF;
    const int sj = live ? in_call_source(labels, obj_slot, i, c, s) : -1;
    const size_t row = (size_t)c * L + (live ? s : 0);
    const float* km = sj >= 0 ? t_mask + (size_t)sj * kMM : bank_mask + row * kMM;
    const float* kf = sj >= 0 ? t_feat + (size_t)sj * CE : bank_feature + row * CE;
    const float* kb = sj >= 0 ? boxes + 4 * (size_t)sj : bank_box + row * 4;
    __syncthreads();
    if (live && lane < kFF) mm[wave][lane] = qm7[lane] * mask7(km, lane);
    __syncthreads();
    if (!live) return;                   // no barrier below
    const float* qf = s_feat + (size_t)i * CE;
    double fn = 0.0, bn = 0.0, den = 0.0, num = 0.0;
    int fd = 0, bd = 0;
    for (int e = lane; e < kMM; e += 64) {
        const float a = qm[e], b = km[e];
        fn += (double)(a * b);
        fd += (a + b) >= 1.f;
        bn += (double)((1.f - a) * (1.f - b));
        bd += (2.f - a - b) >= 1.f;
    }
    if (lane < kFF) den = (double)mm[wave][lane];
    for (int e = lane; e < CE; e += 64) num += (double)(qf[e] * kf[e] * mm[wave][e % kFF]);
    fn = wave_total_f64(fn); bn = wave_total_f64(bn); den = wave_total_f64(den); num = wave_total_f64(num);
    fd = wave_total_i32(fd); bd = wave_total_i32(bd);
    if (lane == 0) {
        const float* qb = boxes + 4 * (size_t)i;
        const float r0 = (qb[2] - qb[0]) / (qb[3] - qb[1] + 1e-5f);
        const float fg = (float)fn / (float)fd, bg = (float)bn / (float)bd;
        const float sim = (float)num / ((float)den + 1e-6f);
        const float r1 = (kb[2] - kb[0]) / (kb[3] - kb[1] + 1e-5f);
        const float ratio = r0 / r1;
        slot_pass[(size_t)i * L + s] = fg > fg_thresh && bg > bg_thresh && sim > appear_thresh && ratio >= ratio_lo && ratio <= ratio_hi;
        if (scores) {
            float* sc = scores + ((size_t)i * L + s) * 4;
            sc[0] = fg; sc[1] = bg; sc[2] = sim; sc[3] = ratio;
        }
    }
}

// ---- the first K passing slots of every object, in slot order: one thread per object -----------------------------------------------------
__global__ __launch_bounds__(64) void corr_compact_kernel(const int64_t* labels, const int32_t* obj_slot, const int32_t* slot_pass, int N, int L, int K,
                                                          int32_t* ret_slot, int32_t* ret_src, int32_t* count) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    int n = 0;
    for (int s = 0; s < L && n < K; ++s)
        if (slot_pass[(size_t)i * L + s]) {
            ret_slot[(size_t)i * K + n] = s;
            ret_src[(size_t)i * K + n] = in_call_source(labels, obj_slot, i, labels[i], s);
            ++n;
        }
    count[i] = n;
    for (; n < K; ++n) { ret_slot[(size_t)i * K + n] = -1; ret_src[(size_t)i * K + n] = -1; }
}

// where retrieved object k of object i lies: a row of the call's teacher tensors or of the bank (row index in units of one entry)
struct KeyRef { bool in_call; size_t row; };
__device__ __forceinline__ KeyRef key_of(const int64_t* labels, const int32_t* ret_slot, const int32_t* ret_src, int i, int k, int K, int L) {
    const int sj = ret_src[(size_t)i * K + k];
    KeyRef r;
    r.in_call = sj >= 0;
    r.row = sj >= 0 ? (size_t)sj : (size_t)labels[i] * L + (size_t)ret_slot[(size_t)i * K + k];
    return r;
}
__device__ __forceinline__ bool runs(const int64_t* labels, const int32_t* count, int i, int k, int min_objs, int K, int num_class) {
    const long long c = labels[i];
    const int n = count[i];
    return c >= 0 && c < num_class && n >= min_objs && n <= K && k < n;
}

// ---- solver: one workgroup per (object, k) --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void corr_solve_kernel(const float* s_feat, const float* t_feat, const int64_t* labels, int C,
                                                         const float* bank_feature, int num_class, int L, const int32_t* ret_slot,
                                                         const int32_t* ret_src, const int32_t* count, int K, int min_objs, int radius, int num_iter,
                                                         int num_smooth, float* Cu_out, float* C_out, int32_t* assign, int N, void* workspace) {
    __shared__ float Cu[kPairs], Cm[kPairs], V[kPairs], Wp[kPairs];
    __shared__ float a_s[kChunk * kFF], b_s[kChunk * kFF];
    __shared__ float n0[kFF], d0[kFF], d1[kFF], rs[kFF];
    __shared__ double rl[kFF], dpart[5][kFF];
    const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const size_t ik = (size_t)i * K + k;
    Work w;
    carve_work(workspace, N, C, K, w);
    if (!runs(labels, count, i, k, min_objs, K, num_class)) {
        for (int o = tid; o < kPairs; o += 256) { Cu_out[ik * kPairs + o] = 0.f; C_out[ik * kPairs + o] = 0.f; }
        if (tid < kFF) assign[ik * kFF + tid] = -1;
        if (tid == 0) w.rowloss[ik] = 0.0;
        return;
    }
    const int n_objs = count[i];
    const int CE = C * kFF;
    const float* f0 = s_feat + (size_t)i * CE;
    const KeyRef key = key_of(labels, ret_slot, ret_src, i, k, K, L);
    const float* f1 = (key.in_call ? t_feat : bank_feature) + key.row * CE;

    // norms over the channels: threads 0..48 for f0, 64..112 for f1
    if (tid < kFF || (tid >= 64 && tid < 64 + kFF)) {
        const bool first = tid < kFF;
        const int p = first ? tid : tid - 64;
        const float* f = first ? f0 : f1;
        double s = 0.0;
        for (int ch = 0; ch < C; ++ch) { const float v = f[ch * kFF + p]; s += (double)v * (double)v; }
        const float n = (float)sqrt(s);
        if (first) { n0[p] = n; d0[p] = n + 1e-4f; } else d1[p] = n + 1e-4f;
    }
    __syncthreads();
    double acc[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) acc[r] = 0.0;
    for (int c0 = 0; c0 < C; c0 += kChunk) {
        const int cc = min(kChunk, C - c0);
        for (int e = tid; e < cc * kFF; e += 256) {
            a_s[e] = f0[c0 * kFF + e] / d0[e % kFF];
            b_s[e] = f1[c0 * kFF + e] / d1[e % kFF];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const int o = tid + 256 * r;
            if (o < kPairs) {
                const int p = o / kFF, q = o % kFF;
                double a = acc[r];
                for (int ch = 0; ch < cc; ++ch) a += (double)a_s[ch * kFF + p] * (double)b_s[ch * kFF + q];
                acc[r] = a;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int o = tid + 256 * r;
        if (o < kPairs) {
            const int p = o / kFF, q = o % kFF;
            const float v = (float)acc[r];
            const int dy = p / kF - q / kF, dx = p % kF - q % kF;
            const bool near = dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
            Cu[o] = v;
            Cm[o] = near ? v : v * 0.f;
            Cu_out[ik * kPairs + o] = v;
        }
    }
    __syncthreads();

    // rows of `plane` divided by (their sum + eps): sums by 49 threads in fp64, then everybody divides
    auto normalise = [&](float* plane, float eps) {
        if (tid < kFF) {
            double s = 0.0;
            for (int q = 0; q < kFF; ++q) s += (double)plane[tid * kFF + q];
            rs[tid] = (float)s + eps;
        }
        __syncthreads();
        for (int o = tid; o < kPairs; o += 256) plane[o] = plane[o] / rs[o / kFF];
        __syncthreads();
    };
    for (int it = 0; it < num_iter; ++it) {
        const float* in = Cm;
        for (int sm = 0; sm < num_smooth; ++sm) {
            // pass_message: the mean over the in-range shifts, the same (dy, dx) on source and target; the reference's order of the adds
            for (int o = tid; o < kPairs; o += 256) {
                const int p = o / kFF, q = o % kFF;
                const int y = p / kF, x = p % kF, y2 = q / kF, x2 = q % kF;
                float sum = 0.f, cnt = 0.f;
                for (int dx = -1; dx <= 1; ++dx)
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int sy = y - dy, sx = x - dx, ty = y2 - dy, tx = x2 - dx;
                        if (sy >= 0 && sy < kF && sx >= 0 && sx < kF && ty >= 0 && ty < kF && tx >= 0 && tx < kF) {
                            sum += in[(sy * kF + sx) * kFF + ty * kF + tx];
                            cnt += 1.f;
                        }
                    }
                Wp[o] = sum / cnt;
            }
            __syncthreads();
            for (int o = tid; o < kPairs; o += 256) V[o] = Wp[o];
            __syncthreads();
            normalise(V, 1e-4f);
            in = V;
        }
        for (int o = tid; o < kPairs; o += 256) Cm[o] = Cu[o] + in[o];     // in == Cm (no smoothing round): C = Cu + C, as the reference
        __syncthreads();
        normalise(Cm, 1e-4f);
    }
    for (int o = tid; o < kPairs; o += 256) C_out[ik * kPairs + o] = Cm[o];
    __syncthreads();                     // the rows of Cm are overwritten below

    // one thread per row: arg-max of C, p = softmax(Cu) -> V, the cross entropy of p and d loss / d Cu -> Wp, T = C p -> Cm (not yet normalised)
    const double scale = 1.0 / ((double)n_objs * kFF);
    if (tid < kFF) {
        const int p = tid;
        int a = 0;
        float best = Cm[p * kFF];
        for (int q = 1; q < kFF; ++q)
            if (Cm[p * kFF + q] > best) { best = Cm[p * kFF + q]; a = q; }
        assign[ik * kFF + p] = a;
        float mx = Cu[p * kFF];
        for (int q = 1; q < kFF; ++q) mx = fmaxf(mx, Cu[p * kFF + q]);
        double s = 0.0;
        for (int q = 0; q < kFF; ++q) { const float e = expf(Cu[p * kFF + q] - mx); V[p * kFF + q] = e; s += (double)e; }
        const float sf = (float)s;
        double s2 = 0.0;
        for (int q = 0; q < kFF; ++q) { const float pr = V[p * kFF + q] / sf; V[p * kFF + q] = pr; s2 += exp((double)pr); }
        rl[p] = log(s2) - (double)V[p * kFF + a];
        double gp = 0.0;                                                     // sum_q g_q p_q
        for (int q = 0; q < kFF; ++q) {
            const double pr = (double)V[p * kFF + q];
            gp += (exp(pr) / s2 - (q == a ? 1.0 : 0.0)) * pr;
        }
        for (int q = 0; q < kFF; ++q) {
            const double pr = (double)V[p * kFF + q];
            const double g = exp(pr) / s2 - (q == a ? 1.0 : 0.0);
            Wp[p * kFF + q] = (float)(pr * (g - gp) * scale);
            Cm[p * kFF + q] = Cm[p * kFF + q] * V[p * kFF + q];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int p = 0; p < kFF; ++p) s += rl[p];
        w.rowloss[ik] = s;
    }
    normalise(Cm, 1e-5f);
    for (int o = tid; o < kPairs; o += 256) w.T[ik * kPairs + o] = Cm[o];

    // d / d f0: dA[c,p] = sum_q G[p,q] f1n[c,q], then back through f0 / (|f0| + 1e-4).  Thread (g, p) owns channels g, g + 5, ... of cell p
    // in both sweeps, so it reads back only what it wrote itself.
    float* gp_out = w.gpart + ik * (size_t)CE;
    const int p = tid % kFF, g = tid / kFF;
    double dot = 0.0;
    for (int c0 = 0; c0 < C; c0 += kChunk) {
        const int cc = min(kChunk, C - c0);
        for (int e = tid; e < cc * kFF; e += 256) b_s[e] = f1[c0 * kFF + e] / d1[e % kFF];
        __syncthreads();
        if (g < 5)
            for (int ch = g; ch < cc; ch += 5) {
                double a = 0.0;
                for (int q = 0; q < kFF; ++q) a += (double)Wp[p * kFF + q] * (double)b_s[ch * kFF + q];
                const float da = (float)a;
                gp_out[(c0 + ch) * kFF + p] = da;
                dot += (double)da * (double)f0[(c0 + ch) * kFF + p];
            }
        __syncthreads();
    }
    if (g < 5) dpart[g][p] = dot;
    __syncthreads();
    if (g < 5) {
        const double full = (((dpart[0][p] + dpart[1][p]) + dpart[2][p]) + dpart[3][p]) + dpart[4][p];
        const double n = (double)n0[p], d = (double)d0[p];
        const double back = n > 0.0 ? full / (n * d * d) : 0.0;
        for (int c0 = 0; c0 < C; c0 += kChunk) {
            const int cc = min(kChunk, C - c0);
            for (int ch = g; ch < cc; ch += 5) {
                const size_t at = (size_t)(c0 + ch) * kFF + p;
                gp_out[at] = (float)((double)gp_out[at] / d - (double)f0[at] * back);
            }
        }
    }
}

// ---- loss sums and the gradient: workgroup i < N adds the parts of object i, workgroup N the losses --------------------------------------
__global__ __launch_bounds__(256) void corr_loss_kernel(const int32_t* count, int N, int C, int K, int min_objs, float* loss_sum, int32_t* num_ins,
                                                        float* grad, void* workspace) {
    Work w;
    carve_work(workspace, N, C, K, w);
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i == N) {
        if (tid == 0) {
            double s = 0.0;
            int n = 0;
            for (int j = 0; j < N; ++j) {
                const int m = count[j];
                if (m >= min_objs && m <= K) {
                    double r = 0.0;
                    for (int k = 0; k < m; ++k) r += w.rowloss[(size_t)j * K + k];
                    s += r / ((double)m * kFF);
                    ++n;
                }
            }
            loss_sum[0] = (float)s;
            num_ins[0] = n;
        }
        return;
    }
    const int m = count[i];
    const bool ran = m >= min_objs && m <= K;
    const int CE = C * kFF;
    for (int e = tid; e < CE; e += 256) {
        double s = 0.0;
        if (ran)
            for (int k = 0; k < m; ++k) s += (double)w.gpart[((size_t)i * K + k) * CE + e];
        grad[(size_t)i * CE + e] = (float)s;
    }
}

__global__ __launch_bounds__(256) void corr_rescale_kernel(const float* unit, const float* upstream, long long n, float* out) {
    const float u = upstream[0];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) out[e] = unit[e] * u;
}

// the 7 -> 28 bilinear taps of one axis (align_corners=False), torch's arithmetic
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap_up(int d, int in, float scale) {
    float src = scale * ((float)d + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > in - 1) t.i0 = in - 1;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// ---- class-map parts: one workgroup per (object, k, quarter of the 784 source pixels), one thread per source pixel ------------------------
__global__ __launch_bounds__(256) void corr_ci_kernel(const float* s_mask, const float* t_mask, const int64_t* labels, int N, int C,
                                                      const float* bank_mask, int num_class, int L, const int32_t* ret_slot, const int32_t* ret_src,
                                                      const int32_t* count, int K, int min_objs, void* workspace) {
    __shared__ float Ts[kPairs];
    __shared__ float m1[kMM];
    __shared__ float R[kFF * kCiThreads];
    __shared__ Tap taps[kM];
    const int i = blockIdx.x, k = blockIdx.y, part = blockIdx.z, tid = threadIdx.x;
    if (!runs(labels, count, i, k, min_objs, K, num_class)) return;
    Work w;
    carve_work(workspace, N, C, K, w);
    const size_t ik = (size_t)i * K + k;
    const KeyRef key = key_of(labels, ret_slot, ret_src, i, k, K, L);
    const float* km = (key.in_call ? t_mask : bank_mask) + key.row * kMM;
    for (int o = tid; o < kPairs; o += 256) Ts[o] = w.T[ik * kPairs + o];
    for (int e = tid; e < kMM; e += 256) m1[e] = km[e];
    if (tid < kM) taps[tid] = tap_up(tid, kF, (float)kF / (float)kM);
    __syncthreads();
    if (tid >= kCiThreads) return;      // no barrier below
    const int P = part * kCiThreads + tid;
    const Tap ty = taps[P / kM], tx = taps[P % kM];
    const int p00 = ty.i0 * kF + tx.i0, p01 = ty.i0 * kF + tx.i1, p10 = ty.i1 * kF + tx.i0, p11 = ty.i1 * kF + tx.i1;
    for (int q = 0; q < kFF; ++q)
        R[q * kCiThreads + tid] = ty.l0 * (tx.l0 * Ts[p00 * kFF + q] + tx.l1 * Ts[p01 * kFF + q]) + ty.l1 * (tx.l0 * Ts[p10 * kFF + q] + tx.l1 * Ts[p11 * kFF + q]);
    const float m0 = s_mask[(size_t)i * kMM + P], n0 = 1.f - m0;
    double fg = 0.0, bg = 0.0;
    for (int Qy = 0; Qy < kM; ++Qy) {
        const Tap uy = taps[Qy];
        for (int Qx = 0; Qx < kM; ++Qx) {
            const Tap ux = taps[Qx];
            const float r00 = R[(uy.i0 * kF + ux.i0) * kCiThreads + tid], r01 = R[(uy.i0 * kF + ux.i1) * kCiThreads + tid];
            const float r10 = R[(uy.i1 * kF + ux.i0) * kCiThreads + tid], r11 = R[(uy.i1 * kF + ux.i1) * kCiThreads + tid];
            const float tsr = uy.l0 * (ux.l0 * r00 + ux.l1 * r01) + uy.l1 * (ux.l0 * r10 + ux.l1 * r11);
            const float b = m1[Qy * kM + Qx], nb = 1.f - b;
            if (m0 * b > 0.5f) fg += (double)(tsr * fminf(fmaxf(b, 0.1f), 0.9f));
            if (n0 * nb > 0.5f) bg += (double)(tsr * fminf(fmaxf(nb, 0.1f), 0.9f));
        }
    }
    const float sc = (float)kFF / (float)kMM;      // 1 / 16, exact
    w.cipart[(ik * 2 + 0) * kMM + P] = (float)bg * sc;
    w.cipart[(ik * 2 + 1) * kMM + P] = (float)fg * sc;
}

// ---- iiu: the mean over k of the class-map parts, resized to the box and written at the box; everything else zero -------------------------
constexpr int kPasteTile = 4096;
__global__ __launch_bounds__(256) void corr_paste_kernel(const float* boxes, const int64_t* labels, const int32_t* count, int N, int C, int K, int min_objs,
                                                         int num_class, int H, int W, float* iiu, void* workspace) {
    __shared__ float ci[kMM];
    const int i = blockIdx.x >> 1, ch = blockIdx.x & 1, tid = threadIdx.x;
    const bool ran = runs(labels, count, i, 0, min_objs, K, num_class);
    const float* b = boxes + 4 * (size_t)i;
    int y1 = 0, x1 = 0, h = 0, wd = 0;
    if (ran) {
        Work w;
        carve_work(workspace, N, C, K, w);
        const int m = count[i];
        for (int e = tid; e < kMM; e += 256) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += (double)w.cipart[(((size_t)i * K + k) * 2 + ch) * kMM + e];
            ci[e] = (float)(s / (double)m);
        }
        y1 = (int)b[1]; x1 = (int)b[0];
        h = (int)(b[3] - b[1]); wd = (int)(b[2] - b[0]);
    }
    __syncthreads();
    const bool any = ran && h > 0 && wd > 0;
    const float sh = any ? (float)kM / (float)h : 0.f, sw = any ? (float)kM / (float)wd : 0.f;
    const int HW = H * W;
    float* out = iiu + ((size_t)i * 2 + ch) * HW;
    const int end = min(HW, (int)(blockIdx.y + 1) * kPasteTile);
    for (int e = blockIdx.y * kPasteTile + tid; e < end; e += 256) {
        const int y = e / W, x = e % W;
        float v = 0.f;
        if (any && y >= y1 && y - y1 < h && x >= x1 && x - x1 < wd) {
            const Tap ty = tap_up(y - y1, kM, sh), tx = tap_up(x - x1, kM, sw);
            v = ty.l0 * (tx.l0 * ci[ty.i0 * kM + tx.i0] + tx.l1 * ci[ty.i0 * kM + tx.i1]) +
                ty.l1 * (tx.l0 * ci[ty.i1 * kM + tx.i0] + tx.l1 * ci[ty.i1 * kM + tx.i1]);
        }
        out[e] = v;
    }
}

// ---- append: one workgroup per object -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void corr_append_kernel(const float* t_feat, const float* t_mask, const float* boxes, const int64_t* labels,
                                                          const int32_t* obj_slot, const int32_t* obj_role, int C, float* bank_feature, float* bank_mask,
                                                          float* bank_box, int32_t* ptr, int num_class, int L) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const long long c = labels[j];
    const int slot = obj_slot[j], role = obj_role[j];
    if (c < 0 || c >= num_class || slot < 0 || slot >= L) return;
    const size_t row = (size_t)c * L + slot;
    const int CE = C * kFF;
    if (role & 1) {
        for (int e = tid; e < CE; e += 256) bank_feature[row * CE + e] = t_feat[(size_t)j * CE + e];
        for (int e = tid; e < kMM; e += 256) bank_mask[row * kMM + e] = t_mask[(size_t)j * kMM + e];
        if (tid < 4) bank_box[row * 4 + tid] = boxes[4 * (size_t)j + tid];
    }
    if ((role & 2) && tid == 0) ptr[c] = (slot + 1) % L;
}

// ---- superres_T as a matrix: one workgroup per (k, source pixel P), threads over the target pixels Q -------------------------------------
__global__ __launch_bounds__(256) void corr_superres_kernel(const float* T, float* out) {
    __shared__ Tap taps[kM];
    const int k = blockIdx.x / kMM, P = blockIdx.x % kMM, tid = threadIdx.x;
    if (tid < kM) taps[tid] = tap_up(tid, kF, (float)kF / (float)kM);
    __syncthreads();
    const float* Tk = T + (size_t)k * kPairs;
    const float sc = (float)kFF / (float)kMM;
    const Tap py = taps[P / kM], px = taps[P % kM];
    for (int Q = tid; Q < kMM; Q += 256) {
        const Tap uy = taps[Q / kM], ux = taps[Q % kM];
        // the target axes first (F.interpolate bilinear on [.., 49, 7, 7]), then the source axes (the trilinear step)
        auto up = [&](int p) {
            const float* r = Tk + p * kFF;
            return uy.l0 * (ux.l0 * r[uy.i0 * kF + ux.i0] + ux.l1 * r[uy.i0 * kF + ux.i1]) + uy.l1 * (ux.l0 * r[uy.i1 * kF + ux.i0] + ux.l1 * r[uy.i1 * kF + ux.i1]);
        };
        const float v = py.l0 * (px.l0 * up(py.i0 * kF + px.i0) + px.l1 * up(py.i0 * kF + px.i1)) +
                        py.l1 * (px.l0 * up(py.i1 * kF + px.i0) + px.l1 * up(py.i1 * kF + px.i1));
        out[((size_t)k * kMM + P) * kMM + Q] = v * sc;
    }
}

// ---- d / d f0 of Cu for a caller's upstream gradient (the drop-in solve): one workgroup, k after k, every thread adds to its own elements ---
__global__ __launch_bounds__(256) void corr_cu_backward_kernel(const float* f0, const float* f1, const float* dCu, int K, int C, float* grad) {
    __shared__ float G[kPairs];
    __shared__ float b_s[kChunk * kFF];
    __shared__ float n0[kFF], d0[kFF], d1[kFF];
    __shared__ double dpart[5][kFF];
    const int tid = threadIdx.x, p = tid % kFF, g = tid / kFF;
    if (tid < kFF) {
        double s = 0.0;
        for (int ch = 0; ch < C; ++ch) { const float v = f0[ch * kFF + tid]; s += (double)v * (double)v; }
        n0[tid] = (float)sqrt(s);
        d0[tid] = n0[tid] + 1e-4f;
    }
    for (int k = 0; k < K; ++k) {
        const float* fk = f1 + (size_t)k * C * kFF;
        __syncthreads();                 // the previous k is done with G, d1 and dpart
        if (tid < kFF) {
            double s = 0.0;
            for (int ch = 0; ch < C; ++ch) { const float v = fk[ch * kFF + tid]; s += (double)v * (double)v; }
            d1[tid] = (float)sqrt(s) + 1e-4f;
        }
        for (int o = tid; o < kPairs; o += 256) G[o] = dCu[(size_t)k * kPairs + o];
        __syncthreads();
        double back = 0.0;
        for (int sweep = 0; sweep < 2; ++sweep) {
            double dot = 0.0;
            for (int c0 = 0; c0 < C; c0 += kChunk) {
                const int cc = min(kChunk, C - c0);
                for (int e = tid; e < cc * kFF; e += 256) b_s[e] = fk[c0 * kFF + e] / d1[e % kFF];
                __syncthreads();
                if (g < 5)
                    for (int ch = g; ch < cc; ch += 5) {
                        double a = 0.0;
                        for (int q = 0; q < kFF; ++q) a += (double)G[p * kFF + q] * (double)b_s[ch * kFF + q];
                        const float da = (float)a;
                        const size_t at = (size_t)(c0 + ch) * kFF + p;
                        if (sweep == 0) dot += (double)da * (double)f0[at];
                        else grad[at] = (k == 0 ? 0.f : grad[at]) + (float)((double)da / (double)d0[p] - (double)f0[at] * back);
                    }
                __syncthreads();
            }
            if (sweep == 0) {
                if (g < 5) dpart[g][p] = dot;
                __syncthreads();
                if (g < 5) {
                    const double full = (((dpart[0][p] + dpart[1][p]) + dpart[2][p]) + dpart[3][p]) + dpart[4][p];
                    const double n = (double)n0[p], d = (double)d0[p];
                    back = n > 0.0 ? full / (n * d * d) : 0.0;
                }
            }
        }
    }
}

inline int bank_shape(int N, int C, int num_class, int L) {
    if (N < 0 || C < 1 || num_class < 1 || L < 1 || L > kMaxQueue) return BXI_ERR_BAD_SHAPE;
    if (!fits_i32((int64_t)C * kFF) || !fits_i32((int64_t)N * kMaxK * kFF)) return BXI_ERR_BAD_SHAPE;
    return BXI_OK;
}
inline bool objs_ok(int max_objs) { return max_objs >= 1 && max_objs <= kMaxK; }

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" size_t bxi_corr_workspace_bytes(int N, int C, int max_objs) {
    if (N < 0 || C < 1 || !objs_ok(max_objs) || !fits_i32((int64_t)C * kFF)) return 0;
    Work w;
    return carve_work(nullptr, N, C, max_objs, w);
}

extern "C" int bxi_corr_plan_f32(const float* boxes, const int64_t* labels, const int32_t* ptr, int N, int num_class, int L, float min_size,
                                 int32_t* obj_slot, int32_t* obj_role, void* stream) {
    if (int rc = bank_shape(N, 1, num_class, L)) return rc;
    if (min_size != min_size) return BXI_ERR_BAD_ARGUMENT;
    if (N == 0) return BXI_OK;
    if (!boxes || !labels || !ptr || !obj_slot || !obj_role) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_plan", s, corr_plan_kernel, dim3(1), dim3(256), 0, s, boxes, labels, ptr, N, num_class, L, min_size, obj_slot, obj_role);
    return check_launch();
}

extern "C" int bxi_corr_retrieve_f32(const float* s_feat, const float* s_mask, const float* t_feat, const float* t_mask, const float* boxes,
                                     const int64_t* labels, const int32_t* obj_slot, int N, int C, const float* bank_feature,
                                     const float* bank_mask, const float* bank_box, int num_class, int L, float fg_thresh, float bg_thresh,
                                     float appear_thresh, float ratio_lo, float ratio_hi, int max_objs, int32_t* slot_pass, int32_t* ret_slot,
                                     int32_t* ret_src, int32_t* count, float* scores, void* stream) {
    if (int rc = bank_shape(N, C, num_class, L)) return rc;
    if (!objs_ok(max_objs)) return BXI_ERR_BAD_SHAPE;
    if (fg_thresh != fg_thresh || bg_thresh != bg_thresh || appear_thresh != appear_thresh || ratio_lo != ratio_lo || ratio_hi != ratio_hi)
        return BXI_ERR_BAD_ARGUMENT;
    if (N == 0) return BXI_OK;
    if (!s_feat || !s_mask || !t_feat || !t_mask || !boxes || !labels || !obj_slot || !bank_feature || !bank_mask || !bank_box || !slot_pass ||
        !ret_slot || !ret_src || !count)
        return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_retrieve", s, corr_retrieve_kernel, dim3((unsigned)N, (unsigned)((L + 3) / 4)), dim3(256), 0, s, s_feat, s_mask, t_feat, t_mask, boxes,
               labels, obj_slot, C, bank_feature, bank_mask, bank_box, num_class, L, fg_thresh, bg_thresh, appear_thresh, ratio_lo, ratio_hi, slot_pass,
               scores);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("corr_compact", s, corr_compact_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, labels, obj_slot, slot_pass, N, L, max_objs, ret_slot,
               ret_src, count);
    return check_launch();
}

extern "C" int bxi_corr_solve_f32(const float* s_feat, const float* t_feat, const int64_t* labels, int N, int C, const float* bank_feature,
                                  int num_class, int L, const int32_t* ret_slot, const int32_t* ret_src, const int32_t* count, int max_objs,
                                  int min_objs, int dist_kernel, int num_iter, int num_smooth_iter, float* Cu_out, float* C_out,
                                  int32_t* assign, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = bank_shape(N, C, num_class, L)) return rc;
    if (!objs_ok(max_objs)) return BXI_ERR_BAD_SHAPE;
    if (dist_kernel < 1 || !(dist_kernel & 1) || num_iter < 0 || num_smooth_iter < 0 || min_objs < 1) return BXI_ERR_BAD_ARGUMENT;
    if (N == 0) return BXI_OK;
    if (!s_feat || !t_feat || !labels || !bank_feature || !ret_slot || !ret_src || !count || !Cu_out || !C_out || !assign) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_corr_workspace_bytes(N, C, max_objs), 16)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_solve", s, corr_solve_kernel, dim3((unsigned)N, (unsigned)max_objs), dim3(256), 0, s, s_feat, t_feat, labels, C, bank_feature,
               num_class, L, ret_slot, ret_src, count, max_objs, min_objs, dist_kernel / 2, num_iter, num_smooth_iter, Cu_out, C_out, assign, N,
               workspace);
    return check_launch();
}

extern "C" int bxi_corr_loss_f32(const int32_t* count, int N, int C, int max_objs, int min_objs, float* loss_sum, int32_t* num_ins, float* grad,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = bank_shape(N, C, 1, 1)) return rc;
    if (!objs_ok(max_objs)) return BXI_ERR_BAD_SHAPE;
    if (min_objs < 1) return BXI_ERR_BAD_ARGUMENT;
    if (!loss_sum || !num_ins || (N > 0 && (!count || !grad))) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_corr_workspace_bytes(N, C, max_objs), 16)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_loss", s, corr_loss_kernel, dim3((unsigned)N + 1), dim3(256), 0, s, count, N, C, max_objs, min_objs, loss_sum, num_ins, grad,
               workspace);
    return check_launch();
}

extern "C" int bxi_corr_grad_rescale_f32(const float* unit, const float* upstream, int64_t n, float* out, void* stream) {
    if (n < 0) return BXI_ERR_BAD_SHAPE;
    if (n == 0) return BXI_OK;
    if (!unit || !upstream || !out) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    const int64_t blocks = (n + 255) / 256;
    BXI_LAUNCH("corr_grad_rescale", s, corr_rescale_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, unit, upstream,
               (long long)n, out);
    return check_launch();
}

extern "C" int bxi_corr_iiu_f32(const float* s_mask, const float* t_mask, const float* boxes, const int64_t* labels, int N, int C,
                                const float* bank_mask, int num_class, int L, const int32_t* ret_slot, const int32_t* ret_src,
                                const int32_t* count, int max_objs, int min_objs, int H, int W, float* iiu, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (int rc = bank_shape(N, C, num_class, L)) return rc;
    if (!objs_ok(max_objs) || H < 1 || W < 1 || !fits_i32((int64_t)H * W) || !fits_i32((int64_t)N * 2 * H * W)) return BXI_ERR_BAD_SHAPE;
    if (min_objs < 1) return BXI_ERR_BAD_ARGUMENT;
    if (N == 0) return BXI_OK;
    if (!s_mask || !t_mask || !boxes || !labels || !bank_mask || !ret_slot || !ret_src || !count || !iiu) return BXI_ERR_NULL_POINTER;
    if (!workspace_ok(workspace, workspace_bytes, bxi_corr_workspace_bytes(N, C, max_objs), 16)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_ci", s, corr_ci_kernel, dim3((unsigned)N, (unsigned)max_objs, (unsigned)kCiParts), dim3(256), 0, s, s_mask, t_mask, labels, N, C,
               bank_mask, num_class, L, ret_slot, ret_src, count, max_objs, min_objs, workspace);
    if (int rc = check_launch()) return rc;
    const int tiles = (H * W + kPasteTile - 1) / kPasteTile;
    BXI_LAUNCH("corr_paste", s, corr_paste_kernel, dim3((unsigned)N * 2, (unsigned)tiles), dim3(256), 0, s, boxes, labels, count, N, C, max_objs, min_objs,
               num_class, H, W, iiu, workspace);
    return check_launch();
}

extern "C" int bxi_corr_append_f32(const float* t_feat, const float* t_mask, const float* boxes, const int64_t* labels, const int32_t* obj_slot,
                                   const int32_t* obj_role, int N, int C, float* bank_feature, float* bank_mask, float* bank_box, int32_t* ptr,
                                   int num_class, int L, void* stream) {
    if (int rc = bank_shape(N, C, num_class, L)) return rc;
    if (N == 0) return BXI_OK;
    if (!t_feat || !t_mask || !boxes || !labels || !obj_slot || !obj_role || !bank_feature || !bank_mask || !bank_box || !ptr) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_append", s, corr_append_kernel, dim3((unsigned)N), dim3(256), 0, s, t_feat, t_mask, boxes, labels, obj_slot, obj_role, C,
               bank_feature, bank_mask, bank_box, ptr, num_class, L);
    return check_launch();
}

extern "C" int bxi_corr_superres_f32(const float* T, int K, float* out, void* stream) {
    if (K < 0 || !fits_i32((int64_t)K * kMM * kMM)) return BXI_ERR_BAD_SHAPE;
    if (K == 0) return BXI_OK;
    if (!T || !out) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_superres", s, corr_superres_kernel, dim3((unsigned)K * kMM), dim3(256), 0, s, T, out);
    return check_launch();
}

extern "C" int bxi_corr_cu_backward_f32(const float* f0, const float* f1, const float* dCu, int K, int C, float* grad, void* stream) {
    if (K < 1 || K > kMaxK || C < 1 || !fits_i32((int64_t)C * kFF * kMaxK)) return BXI_ERR_BAD_SHAPE;
    if (!f0 || !f1 || !dCu || !grad) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("corr_cu_backward", s, corr_cu_backward_kernel, dim3(1), dim3(256), 0, s, f0, f1, dCu, K, C, grad);
    return check_launch();
}
