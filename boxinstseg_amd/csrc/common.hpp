// common.hpp -- shared host/device helpers for libboxinst_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../../include/boxinst_hip.h"

namespace bxi {

constexpr int kWave = 64;  // CDNA wavefront

// ---- host side ------------------------------------------------------------------------------
void set_last_hip_error(int e);

inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_hip_error((int)e);
        return BXI_ERR_LAUNCH;
    }
    return BXI_OK;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// measurement hook (bxi_set_launch_hook): brackets one kernel launch
typedef void (*bxi_launch_hook)(const char* kernel_name, int phase, void* stream, void* user);      // include/boxinst_hip_dev.h
extern std::atomic<bxi_launch_hook> g_hook;
extern std::atomic<void*> g_hook_user;
struct LaunchScope {
    const char* name; hipStream_t s; bxi_launch_hook hook; void* user;
    LaunchScope(const char* n, hipStream_t st) : name(n), s(st), hook(g_hook.load(std::memory_order_acquire)), user(nullptr) {
        if (hook) { user = g_hook_user.load(std::memory_order_acquire); hook(name, 0, (void*)s, user); }
    }
    ~LaunchScope() { if (hook) hook(name, 1, (void*)s, user); }
};

#define BXI_LAUNCH(label, stream, ...)                 \
    do {                                               \
        ::bxi::LaunchScope _scope(label, stream);      \
        hipLaunchKernelGGL(__VA_ARGS__);               \
    } while (0)

inline bool fits_i32(int64_t v) { return v >= 0 && v <= 0x7fffffffLL; }

// A caller's buffer as an entry point accepts it: present, large enough, aligned to `align` bytes (a power of two, here and in Carver).
inline bool aligned(const void* p, size_t align) { return !(reinterpret_cast<uintptr_t>(p) & (align - 1)); }
inline bool workspace_ok(const void* ws, size_t have, size_t need, size_t align) { return ws && have >= need && aligned(ws, align); }

// Carves consecutive arrays out of one buffer, every array starting on a multiple of `align` from the base; a null base measures only
// (take() returns null, bytes() is the size to ask for).  The one layout rule of every workspace and `state` block of the library --
// the *_workspace_bytes queries and the kernels that carve again on the device must agree to the byte, so there is one copy.
// Sizes are rounded with a mask, not as x / align * align: from the division form the compiler derives x - x % align, moves the `+ align - 1`
// into the instructions' immediate offsets and leaves base registers that are not dword-aligned -- which a scalar load (it ignores the two
// low bits of its base AND of its offset) then reads the wrong word through.
struct Carver {
    char* base; size_t align, off;
    __host__ __device__ Carver(void* b, size_t a) : base(static_cast<char*>(b)), align(a), off(0) {}
    template <typename T> __host__ __device__ T* take(size_t count) {
        const size_t o = off;
        off += (sizeof(T) * count + align - 1) & ~(align - 1);
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
    __host__ __device__ size_t bytes() const { return off; }
};

// compute units of the current device (256 on an MI355X in SPX mode, 32 per partition in CPX): grids are sized so that a launch is
// resident in one round.  Cached per device ordinal; a wrong value costs time, never correctness.
inline int device_cus() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cached[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

// ---- developer tracing (-DBXI_TRACE builds only; never in the shipped library) ---------------
// BXI_T(kernel_id, block, phase) stores the 100 MHz wall clock of lane 0 into a global buffer.
#ifdef BXI_TRACE
constexpr int kTraceBlocks = 8192, kTracePhases = 8;
static __device__ long long* g_trace = nullptr;   // per translation unit
#define BXI_T(kid, blk, ph)                                                                            \
    do {                                                                                               \
        if (threadIdx.x == 0 && g_trace && (blk) < ::bxi::kTraceBlocks)                                \
            g_trace[((size_t)(kid) * ::bxi::kTraceBlocks + (blk)) * ::bxi::kTracePhases + (ph)] = wall_clock64(); \
    } while (0)
#else
#define BXI_T(kid, blk, ph) do {} while (0)
#endif

// ---- device side ----------------------------------------------------------------------------
// log sigmoid, the reference's formula (pairwise.cu:27-37) in the overflow-free arrangement
// min(x,0) - log(1 + exp(-|x|)).
__device__ __forceinline__ float logsig(float x) { return fminf(x, 0.f) - logf(1.f + expf(-fabsf(x))); }
__device__ __forceinline__ double logsig(double x) { return fmin(x, 0.0) - log(1.0 + exp(-fabs(x))); }

template <typename T> __device__ __forceinline__ T t_exp(T x);
template <> __device__ __forceinline__ float t_exp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double t_exp<double>(double x) { return exp(x); }
template <typename T> __device__ __forceinline__ T t_log(T x);
template <> __device__ __forceinline__ float t_log<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double t_log<double>(double x) { return log(x); }
template <typename T> __device__ __forceinline__ T t_abs(T x) { return x < T(0) ? -x : x; }

// order-preserving map float -> uint32 (larger float <=> larger key); -inf maps above 0.
__device__ __forceinline__ uint32_t float_key(float x) {
    uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    uint32_t u = k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu);
    return __uint_as_float(u);
}
// (value, index) -> one 64-bit key whose max is "largest value, then smallest index".
__device__ __forceinline__ unsigned long long pack_max(float x, uint32_t idx) {
    return ((unsigned long long)float_key(x) << 32) | (unsigned long long)(0xffffffffu - idx);
}
__device__ __forceinline__ float unpack_val(unsigned long long k) { return key_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ uint32_t unpack_idx(unsigned long long k) { return 0xffffffffu - (uint32_t)k; }

// Wave totals on the VALU's data-parallel path (DPP) instead of six dependent trips through the LDS crossbar
// (__shfl_xor = ds_bpermute, ~130 clk each): quad swaps, the two mirrors within a row of 16 lanes, then the four rows by
// v_readlane.  Every lane gets the total; fixed order, so run-to-run identical.
template <typename F>
__device__ __forceinline__ void wave_total_steps(F&& step) {
    step(0xB1);    // quad_perm:[1,0,3,2]
    step(0x4E);    // quad_perm:[2,3,0,1]
    step(0x141);   // row_half_mirror
    step(0x140);   // row_mirror
}
__device__ __forceinline__ int dpp_i32(int v, int ctrl) {
    switch (ctrl) {
        case 0xB1: return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);
        case 0x4E: return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);
        case 0x141: return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);
        default: return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);
    }
}
__device__ __forceinline__ float wave_total_f32(float v) {
    wave_total_steps([&](int c) { v += __int_as_float(dpp_i32(__float_as_int(v), c)); });
    const int b = __float_as_int(v);
    return (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
}
__device__ __forceinline__ int wave_total_i32(int v) {
    wave_total_steps([&](int c) { v += dpp_i32(v, c); });
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) + (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
__device__ __forceinline__ double wave_total_f64(double v) {
    wave_total_steps([&](int c) {
        const long long b = __double_as_longlong(v);
        const int lo = dpp_i32((int)b, c), hi = dpp_i32((int)(b >> 32), c);
        v += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    });
    auto row = [&](int l) {
        const long long b = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
        return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    };
    return (row(0) + row(16)) + (row(32) + row(48));
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    wave_total_steps([&](int c) {
        const unsigned long long o = ((unsigned long long)(unsigned int)dpp_i32((int)(v >> 32), c) << 32) | (unsigned int)dpp_i32((int)v, c);
        v = o > v ? o : v;
    });
    auto row = [&](int l) {
        return ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned int)__builtin_amdgcn_readlane((int)v, l);
    };
    const unsigned long long a = row(0), b = row(16), c2 = row(32), d = row(48);
    const unsigned long long ab = a > b ? a : b, cd = c2 > d ? c2 : d;
    return ab > cd ? ab : cd;
}
__device__ __forceinline__ float wave_max_f32(float v) {
    wave_total_steps([&](int c) { v = fmaxf(v, __int_as_float(dpp_i32(__float_as_int(v), c))); });
    const int b = __float_as_int(v);
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 0)), __int_as_float(__builtin_amdgcn_readlane(b, 16))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 32)), __int_as_float(__builtin_amdgcn_readlane(b, 48))));
}
__device__ __forceinline__ int wave_min_i32(int v) {
    wave_total_steps([&](int c) { v = min(v, dpp_i32(v, c)); });
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// The column a row's arg-max goes to, from per-lane (maximum, its first column) pairs and the wave's maximum: the SMALLEST column among
// the lanes that hold the maximum.  A lane owns four columns of every 256-column chunk, so with one chunk the lowest such lane holds it
// (one ballot + readlane); with several chunks a low lane may hold a column of a later chunk (column 256 is lane 0, column 255 lane 63),
// and the columns themselves are compared.  No lane holds the maximum only for a row of NaN: column 0 then, as before.
__device__ __forceinline__ int first_col_of_max(float lane_max, int lane_col, float wave_max, bool one_chunk) {
    const bool mine = lane_max == wave_max;
    if (one_chunk) {
        const unsigned long long who = __ballot(mine);
        return __builtin_amdgcn_readlane(lane_col, who ? __ffsll((long long)who) - 1 : 0);
    }
    const int col = wave_min_i32(mine ? lane_col : 0x7fffffff);
    return col == 0x7fffffff ? __builtin_amdgcn_readlane(lane_col, 0) : col;
}
// Inclusive prefix sum over the 64 lanes on the DPP path: Hillis-Steele inside a row of 16 lanes (row_shr 1, 2, 4, 8; lanes without a source add 0),
// then the rows' totals by row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3).  Ten VALU instructions, no LDS.
__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ int wave_scan_incl_i32(int v) { return (int)wave_scan_incl_u32((uint32_t)v); }
// Exclusive prefix sum of one int per thread over a workgroup of exactly WAVES waves, in thread order; `total` is the workgroup's sum
// (every thread gets both; a caller that wants the inclusive value adds its own v).  The wave scan, the waves' totals handed over through
// part[WAVES], then every wave scans those totals again (lane w reads wave w's) and picks the sum of the waves before it and the last one
// by v_readlane: one LDS read and a few registers whatever WAVES is.  Called by all threads of the workgroup, every lane active.  The
// barrier BEHIND the reads makes a second call on the same `part` safe right away; the caller sees to it that nobody still uses `part` for
// something else when the first one starts.
template <int WAVES>
__device__ __forceinline__ int block_scan_excl_i32(int v, int* part /*[WAVES]*/, int& total) {
    static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup has at most 1024 threads");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_incl_i32(v);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    const int t = lane < WAVES ? part[lane] : 0;
    const int upto = wave_scan_incl_i32(t);
    __syncthreads();
    total = __builtin_amdgcn_readlane(upto, WAVES - 1);
    return __builtin_amdgcn_readlane(upto - t, __builtin_amdgcn_readfirstlane(wave)) + incl - v;
}

// ---- workgroup sums in a fixed order ---------------------------------------------------------------------------------
// Two orders, two names: these are fp64 loss sums whose order is part of the results, so the forms are not interchangeable.
//
// block_sum_seq_f64: ANY number of waves (blockDim.x / 64 <= 16), the wave totals added one after the other in wave order,
// ((w0 + w1) + w2) + ...; every thread gets the sum.  LDS: red[16] doubles.  Barriers: one BEFORE the hand-over (a second
// call may reuse `red`: nobody still reads the previous call's totals once every wave is past it), one after it; none behind
// the reads -- the next call's leading barrier is what protects them.
__device__ __forceinline__ double block_sum_seq_f64(double v, double* red /*[16]*/) {
    v = wave_total_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];   // fixed order
    return s;
}
// block_sum_4w_f64 / block_sum_4w_i32: EXACTLY four waves (256 threads), the wave totals pairwise, (w0 + w1) + (w2 + w3); every
// thread gets the sum.  LDS: s4[4].  Barriers: one after the hand-over and one AFTER the reads, so `s4` is free again when the
// call returns and calls on the same `s4` may follow each other directly.
__device__ __forceinline__ double block_sum_4w_f64(double v, double* s4) {
    v = wave_total_f64(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ int block_sum_4w_i32(int v, int* s4) {
    v = wave_total_i32(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const int r = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return r;
}

// Workgroup barrier that orders LDS traffic only: unlike __syncthreads() it does not wait for the
// wave's outstanding global stores (vmcnt), so zero-fill / output stores stay in flight across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- stores that are written through to memory as they are issued (sc1 = agent scope) --------------------------------
// Used (a) for bulk output that should drain while the launch is still reading instead of in a burst at the kernel
// boundary, and (b) for data another workgroup of the SAME launch reads after an arrival counter (MI355X_MICROARCH.md,
// "inter-workgroup visibility", form R1: sc1 payload -> s_waitcnt vmcnt(0) -> agent-scope atomic).  16-byte forms: a narrower
// sc1 store is one fabric write per lane.  The asm forms are invisible to the compiler's vmcnt bookkeeping: callers drain
// with drain_vmem() before they publish.
__device__ __forceinline__ void store4_through(float* p, float x, float y, float z, float w) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = {x, y, z, w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_u64x2_through(unsigned long long* p, unsigned long long a, unsigned long long b) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    const u4v v = {(unsigned int)a, (unsigned int)(a >> 32), (unsigned int)b, (unsigned int)(b >> 32)};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// python slice [a:b] on an axis of length n -> [lo,hi)   (condinst_head.py:1429-1430)
__device__ __forceinline__ void py_slice(int a, int b, int n, int& lo, int& hi) {
    if (a < 0) a += n;
    a = a < 0 ? 0 : (a > n ? n : a);
    if (b < 0) b += n;
    b = b < 0 ? 0 : (b > n ? n : b);
    lo = a;
    hi = b > a ? b : a;
}

// Box (x1,y1,x2,y2 in canvas pixels) -> half-open rectangle [r0,r1) x [c0,c1) on the sampled
// grid y = start + r*stride: the cells whose sample lies inside the python slice.
struct Rect { int r0, r1, c0, c1; };
__device__ __forceinline__ void sampled_range(int lo, int hi, int start, int stride, int n, int& a, int& b) {
    // smallest r with start + r*stride >= lo ; smallest r with start + r*stride >= hi
    int ra = lo - start <= 0 ? 0 : (lo - start + stride - 1) / stride;
    int rb = hi - start <= 0 ? 0 : (hi - start + stride - 1) / stride;
    a = ra > n ? n : ra;
    b = rb > n ? n : rb;
    if (b < a) b = a;
}
__device__ __forceinline__ Rect box_rect(const float* box, int Hc, int Wc, int stride, int start, int h, int w) {
    int y0, y1, x0, x1;
    py_slice((int)box[1], (int)box[3] + 1, Hc, y0, y1);
    py_slice((int)box[0], (int)box[2] + 1, Wc, x0, x1);
    Rect rc;
    sampled_range(y0, y1, start, stride, h, rc.r0, rc.r1);
    sampled_range(x0, x1, start, stride, w, rc.c0, rc.c1);
    if (rc.r1 <= rc.r0 || rc.c1 <= rc.c0) { rc.r0 = rc.r1 = rc.c0 = rc.c1 = 0; }
    return rc;
}

// per-image metadata carried in kernel arguments (no device copy, no sync)
struct GtTable {
    const float* boxes[BXI_MAX_IMAGES];  // device pointers, [G_i,4]
    int first[BXI_MAX_IMAGES + 1];       // first[b] = sum_{i<b} G_i
    int B;
};
__device__ __forceinline__ const float* gt_box(const GtTable& t, int g, int& img) {
    int b = 0;
    while (b + 1 < t.B && g >= t.first[b + 1]) ++b;
    img = b;
    return t.boxes[b] + 4 * (g - t.first[b]);
}

}  // namespace bxi
