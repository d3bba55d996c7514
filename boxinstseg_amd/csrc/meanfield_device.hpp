// meanfield_device.hpp -- one MeanField.simple_forward step (discobox_head.py:640-655) on bit words, as the translation units share it.
// meanfield.hip (bxi_meanfield_forward_f32: one leg) and discobox_loss.hip (bxi_dbx_steps_f32: both legs of DiscoBoxSOLOv2Head.loss in
// one launch) run the SAME device function per leg: there is one copy of the arithmetic, so the thresholded decisions of the two agree
// bit for bit.
//
// State = one bit per pixel, stored as 64-pixel words [N][H][segs] (target mask, state read, state written).  A wave evaluates the 64
// consecutive pixels of one (instance, line, segment) item; `__ballot` of the new decisions IS the new state word.  The per-pixel
// arithmetic is the reference's fp32 op sequence, step by step (products and sums are not contracted, neighbours summed in unfold order).
#pragma once

#include "common.hpp"

namespace bxi {

typedef unsigned long long u64;

struct MfArgs {
    const float* K;           // [B,KS*KS,H,W]
    const float* x;           // [N,H,W]
    const void* t;            // [N,H,W] f32 or u8
    const int64_t* img;       // [N] or null
    const float* inter;       // [N,2,H,W] or null
    float* ret;               // [N,H,W]
    float* valid;             // [N]
    u64* tw;                  // [N,H,segs] target words
    u64* sa;                  // [N,H,segs] state, read
    u64* sb;                  // [N,H,segs] state, written
    int B, H, W, N, t_u8, segs;
    float nl_lo0, nl_lo1, nl_hi0, nl_hi1;   // -log(1-x), -log(x) for x = lo / hi
    float gamma, vlo, vhi;
};

constexpr int kMfWaves = 4;   // waves per workgroup of the per-item kernels
// IPW = consecutive items per wave: 4 when there are many items (4x fewer workgroups to dispatch), 1 when few
// (all the parallelism there is).  The threshold kMfManyItems has one home, meanfield.hip; this is its question (host side).
bool mf_many_items(int64_t items);

// first item of this wave
template <int IPW>
__device__ __forceinline__ int mf_first_item() {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return ((int)blockIdx.x * kMfWaves + wave) * IPW;
}

// the two values a thresholded probability takes, (f > 0.5).float() * (1 - base*2) + base (:622, :653), in fp32 (host side)
inline void mf_set_levels(MfArgs& a, float base) {
    const float span = (float)(1.0 - (double)base * 2.0);
    const float lo = 0.f * span + base, hi = 1.f * span + base;
    a.nl_lo0 = -logf(1.f - lo); a.nl_lo1 = -logf(lo);
    a.nl_hi0 = -logf(1.f - hi); a.nl_hi1 = -logf(hi);
}

// the KS*KS affinity values of this lane's pixel (line r, clamped column cc) of instance n
template <int KS>
__device__ __forceinline__ void mf_load_affinity(const MfArgs& a, int n, int r, int cc, float (&kv)[KS * KS]) {
    constexpr int KK = KS * KS;
    const int64_t HW = (int64_t)a.H * a.W;
    // img_inds is device data: clamp it into [0, B) so that a bad index reads a wrong kernel plane, never foreign memory
    const int64_t bi = a.img ? (a.img[n] < 0 ? 0 : (a.img[n] >= a.B ? a.B - 1 : a.img[n])) : 0;
    const float* Kp = a.K + bi * (int64_t)KK * HW + (int64_t)r * a.W + cc;
#pragma unroll
    for (int k = 0; k < KK; ++k) kv[k] = Kp[(int64_t)k * HW];
}

// one simple_forward (:640-655) of one item from loaded affinities: state `sa` -> `sb`; `inter` = this instance's [2,H,W] planes or null
template <int KS>
__device__ __forceinline__ void mf_eval_loaded(const MfArgs& a, const float (&kv)[KS * KS], const float* inter, const u64* sa, u64* sb,
                                               int n, int r, int sg, u64 mt, int lane) {
    constexpr int HALF = KS / 2;
    const int H = a.H, W = a.W, segs = a.segs, c = sg * 64 + lane;
    const int64_t wbase = (int64_t)n * H * segs;
    const int64_t HW = (int64_t)H * W;
    const int cc = c < W ? c : W - 1;                             // clamped: loads need no branch
    float i0 = 0.f, i1 = 0.f;
    if (inter) { const float* ip = inter + (int64_t)r * W + cc; i0 = ip[0]; i1 = ip[HW]; }
    // the state words of the neighbourhood rows (uniform addresses); outside the map = 0 and never used
    u64 wl[KS], wm[KS], wr[KS];
#pragma unroll
    for (int dy = -HALF; dy <= HALF; ++dy) {
        const int r2 = r + dy;
        const bool rin = r2 >= 0 && r2 < H;
        const u64* row = sa + wbase + (int64_t)(rin ? r2 : r) * segs;
        wm[dy + HALF] = rin ? row[sg] : 0ull;
        wl[dy + HALF] = rin && sg > 0 ? row[sg - 1] : 0ull;
        wr[dy + HALF] = rin && sg + 1 < segs ? row[sg + 1] : 0ull;
    }
    const bool act = (mt >> lane) & 1ull;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int dy = -HALF; dy <= HALF; ++dy) {
        const int r2 = r + dy;
        const bool rin = r2 >= 0 && r2 < H;
#pragma unroll
        for (int dx = -HALF; dx <= HALF; ++dx) {
            const int k = (dy + HALF) * KS + (dx + HALF);
            const u64 m = wm[dy + HALF];
            const u64 sh = dx < 0 ? (m << (-dx)) | (wl[dy + HALF] >> (64 + dx)) : dx > 0 ? (m >> dx) | (wr[dy + HALF] << (64 - dx)) : m;
            const bool bit = (sh >> lane) & 1ull;
            const int c2 = c + dx;
            if (rin && c2 >= 0 && c2 < W) {                   // outside the map nn.Unfold pads -log(U) with 0: adds nothing
                acc0 = __fadd_rn(acc0, __fmul_rn(bit ? a.nl_hi0 : a.nl_lo0, kv[k]));
                acc1 = __fadd_rn(acc1, __fmul_rn(bit ? a.nl_hi1 : a.nl_lo1, kv[k]));
            }
        }
    }
    float f0 = expf(-acc0), f1 = expf(-acc1);
    if (inter) { f0 = __fadd_rn(f0, __fmul_rn(i0, a.gamma)); f1 = __fadd_rn(f1, __fmul_rn(i1, a.gamma)); }
    f1 = act ? f1 : 0.f;                                      // f[:, 1:] *= targets
    f0 = __fadd_rn(f0, 1e-6f); f1 = __fadd_rn(f1, 1e-6f);
    const float r1v = __fdiv_rn(f1, __fadd_rn(f0, f1));
    const u64 nw = __ballot(act && c < W && r1v > 0.5f);
    if (lane == 0) sb[wbase + (int64_t)r * segs + sg] = nw;
}

// one simple_forward (:640-655) of one item
template <int KS>
__device__ __forceinline__ void mf_eval_item(const MfArgs& a, const u64* sa, u64* sb, int n, int r, int sg, u64 mt, int lane) {
    const int c = sg * 64 + lane;
    float kv[KS * KS];
    mf_load_affinity<KS>(a, n, r, c < a.W ? c : a.W - 1, kv);
    mf_eval_loaded<KS>(a, kv, a.inter ? a.inter + (int64_t)n * 2 * a.H * a.W : nullptr, sa, sb, n, r, sg, mt, lane);
}

}  // namespace bxi
