// eval_protocol_device.hpp -- what every role of the evaluation (fused_eval.hip) agrees on: the constants of the grid and of the bounded
// waits, the developer macros (BXI_WL, BXI_TW), the loads past the caches (load*_past*), the workspace `Ws` with its one layout (carve)
// and the evaluation's tag (with_tag, next_tag).  Assumes loss_common.hpp (InstArgs, LossState) and, for the head-fused
// launch's tile sizes in carve, dynamic_head_device.hpp; nothing of the roles.
#pragma once
#include "loss_common.hpp"
#include "dynamic_head_device.hpp"

namespace bxi {

constexpr int kWaves = 4;                       // waves per workgroup in both launches
constexpr int kSRows = 8;                       // rows per stream wave
constexpr int kSBlk = kWaves * kSRows;          // rows per stream workgroup
constexpr int kChunkC = 256;                    // columns per pass of a stream wave: 64 lanes x float4
constexpr int kMaxDilFused = 4;
#ifndef BXI_SPIN_LIMIT
#define BXI_SPIN_LIMIT 4000000
#endif
constexpr int kSpinLimit = BXI_SPIN_LIMIT;             // bounded waits (0.3 - 1 us per poll: seconds): a bound, not a schedule -- a transient stall (another
                                                // process time-slicing the GPU, a long kernel on another stream while stream workgroups stay on) must
                                                // not turn an iteration's losses into NaN; running out is loud (NaN losses, status word) and the host
                                                // side then takes the two-launch form, whose every wait is for an EARLIER workgroup
// bits of the `flags` argument of bxi_boxinst_eval_f32 (include/boxinst_hip.h: BXI_EVAL_*); per call, no process-wide state
constexpr unsigned kFlagSingle = BXI_EVAL_SINGLE_LAUNCH, kFlagTwo = BXI_EVAL_TWO_LAUNCHES, kFlagRows8 = BXI_EVAL_TILE_ROWS_8, kFlagRows4 = BXI_EVAL_TILE_ROWS_4,
                   kFlagShared = BXI_EVAL_SHARED_DEVICE, kFlagTargetsReady = BXI_EVAL_TARGETS_READY, kFlagGiveUp = BXI_EVAL_WAITS_GIVE_UP;
constexpr int kBoxCap = 1024;                   // GT boxes per batch bxi_boxinst_targets_f32 keeps pair counts for
constexpr int kBoxSplit = 8;                    // count words per box (each in its own 128 bytes): arrivals on one word are performed one after the other
constexpr int kNtStreamFromMB = 20;             // logit maps of this many MB and more are streamed past the L2 (non-temporal loads)
constexpr int kLongFrom = 96;                   // single launch, long form (8-row tiles) from this many instances on
constexpr unsigned int kMaxTag = 0x0fffffffu;   // tags are 28 bits (a predicate word is tag << 4 | bits)
constexpr int kAcc2Split = 8, kAcc2Stride = 16; // tile arrivals: eight words per instance, each in its own 128 bytes
constexpr int kAcc1Words = 64;                  // count-wave arrivals + sum W: 64 words, each in its own 128 bytes
constexpr int kMaxInst = 65536;
constexpr int kOneOcc = 4;                      // workgroups per CU of the single-launch form (<= 128 VGPRs: the tile role's budget)
constexpr int kLongOcc = 3;                     // workgroups per CU of the 8-row single-launch forms (138 VGPRs: profiles/NOTES.md R6-3)
constexpr int kPrepOcc = 5;                     // workgroups per CU of the two-launch form's first launch (prep_kernel: <= 96 VGPRs)
// developer builds (-DBXI_WAITLOG): the longest wait of every bounded in-grid wait, by site, in polls -- which wait a slow launch sat in
#ifdef BXI_WAITLOG
static __device__ unsigned int g_waitlog[16];
#define BXI_WL(site, spins) do { if ((spins) > 1000 && (threadIdx.x & 63) == 0) atomicMax(&g_waitlog[site], (unsigned int)(spins)); } while (0)
#else
#define BXI_WL(site, spins) do {} while (0)
#endif
constexpr unsigned kFaultCounts = 1u, kFaultFinisher = 2u;
// A wave whose bounded wait ran out says so on the evaluation's fault word (zeroed by the first table wave before the entries every waiter checks),
// with a returning atomic it waits for BEFORE its arrival: the round in which the finisher sees the last arrival reads the fault word too.  The sum W
// word and a leader's dice word carry their own fault bit (one writer each); the arrival words of tile waves and predicate workgroups do not any
// more -- a flag ADDED to an arrival carries into the arrival count from the second (predicate) / fourth (tile) fault on one word on, and the
// finisher then waits kSpinLimit polls for a count that cannot come (4.5 s per evaluation with foreign targets, where every tile wave is "bad").
constexpr unsigned long long kCountFault = 1ull << 39, kSumwFault = 1ull << 62, kDiceFault = 1ull << 33;      // (bits 50 / 51 of an arrival word: reserved, checked by the finisher, set by nobody since R6-3)

#ifdef BXI_TRACE
#ifdef BXI_TRACE_LIGHT      // only the first and the last stamp of a wave: two stores per wave instead of eight (the full trace lengthens the launch by half)
#define BXI_TW(kid, idx, ph)                                                                                  \
    do {                                                                                                      \
        if (((ph) == 0 || (ph) == 7 || (kid) >= 2) && (threadIdx.x & 63) == 0 && g_trace && (idx) >= 0 && (idx) < ::bxi::kTraceBlocks) \
            g_trace[((size_t)(kid) * ::bxi::kTraceBlocks + (idx)) * ::bxi::kTracePhases + (ph)] = wall_clock64(); \
    } while (0)
#else
#define BXI_TW(kid, idx, ph)                                                                                  \
    do {                                                                                                      \
        if ((threadIdx.x & 63) == 0 && g_trace && (idx) >= 0 && (idx) < ::bxi::kTraceBlocks)                  \
            g_trace[((size_t)(kid) * ::bxi::kTraceBlocks + (idx)) * ::bxi::kTracePhases + (ph)] = wall_clock64(); \
    } while (0)
#endif
#else
#define BXI_TW(kid, idx, ph) do {} while (0)
#endif

// back-off between the polls of the bounded in-grid waits, in units of 64 clocks (A/B of 1 .. 32 on one box moved the step by +-0.15 us at most:
// the waits are not what the launch ends on)
constexpr int kSleepTab = 16, kSleepPred = 16, kSleepWords = 8, kSleepSumw = 8, kSleepLead = 4, kSleepFin = 2;

#define BXI_RLX __ATOMIC_RELAXED
#define BXI_AGENT __HIP_MEMORY_SCOPE_AGENT

// float add at the L2 without return (global_atomic_add_f32): the gradient is zero-filled by launch 1 and every element
// receives at most two additions, so the result does not depend on their order
__device__ __forceinline__ void add_f32(float* p, float v) {
    (void)__builtin_amdgcn_global_atomic_fadd_f32((__attribute__((address_space(1))) float*)p, v);
}

// 16-byte load past the caches (sc1 = agent scope): what another workgroup of the SAME launch stored with store4_through /
// store_u64x2_through.  One instruction per datum, so a tagged 16-byte record is seen whole or not at all.  The asm form is
// invisible to the compiler's vmcnt bookkeeping, hence the wait inside the statement.
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u4v load16_past(const void* p) {
    u4v v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ void load16_past_x4(const void* p0, const void* p1, const void* p2, const void* p3, u4v& a, u4v& b, u4v& c, u4v& d) {
    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\tglobal_load_dwordx4 %2, %6, off sc1\n\t"
                 "global_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d) : "v"(p0), "v"(p1), "v"(p2), "v"(p3) : "memory");
}
// two 8-byte words past the caches, one round trip
__device__ __forceinline__ void load8_past_x2(const void* p0, const void* p1, unsigned long long& a, unsigned long long& b) {
    asm volatile("global_load_dwordx2 %0, %2, off sc1\n\tglobal_load_dwordx2 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(p0), "v"(p1) : "memory");
}
__device__ __forceinline__ void load16_past_x3(const void* p0, const void* p1, const void* p2, u4v& a, u4v& b, u4v& c) {
    asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\tglobal_load_dwordx4 %2, %5, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c) : "v"(p0), "v"(p1), "v"(p2) : "memory");
}
__device__ __forceinline__ void load16_past_x5(const void* p0, const void* p1, const void* p2, const void* p3, const void* p4, u4v& a, u4v& b, u4v& c, u4v& d,
                                               u4v& e) {
    asm volatile("global_load_dwordx4 %0, %5, off sc1\n\tglobal_load_dwordx4 %1, %6, off sc1\n\tglobal_load_dwordx4 %2, %7, off sc1\n\t"
                 "global_load_dwordx4 %3, %8, off sc1\n\tglobal_load_dwordx4 %4, %9, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d), "=&v"(e) : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4) : "memory");
}
__device__ __forceinline__ u4v load16_past_epoch(const void* p, const unsigned int* epoch, unsigned int& ep_word) {
    u4v v;
    asm volatile("global_load_dword %1, %3, %4\n\tglobal_load_dwordx4 %0, %2, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v), "=&v"(ep_word) : "v"(p), "v"(0), "s"(epoch) : "memory");
    return v;
}
// ... and the workspace's epoch word in the same round trip (a wave that does not know the evaluation's tag yet: with_tag)
__device__ __forceinline__ void load16_past_x5_epoch(const void* p0, const void* p1, const void* p2, const void* p3, const void* p4, const unsigned int* epoch,
                                                     u4v& a, u4v& b, u4v& c, u4v& d, u4v& e, unsigned int& ep_word) {
    asm volatile("global_load_dword %5, %11, %12\n\tglobal_load_dwordx4 %0, %6, off sc1\n\tglobal_load_dwordx4 %1, %7, off sc1\n\t"
                 "global_load_dwordx4 %2, %8, off sc1\n\tglobal_load_dwordx4 %3, %9, off sc1\n\tglobal_load_dwordx4 %4, %10, off sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d), "=&v"(e), "=&v"(ep_word)
                 : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(0), "s"(epoch)
                 : "memory");
}
// N words past the caches in ONE round trip: `base` (a scalar register pair) + a 32-bit byte offset per lane and word.  As a sequence of
// __hip_atomic_load the compiler issues them one at a time, an s_waitcnt vmcnt(0) behind each (atomics are not reordered against each other and
// each one's consumer is scheduled right behind it): R + D dependent trips to the L2 in front of every tile's pair loop -- six at 4-row tiles,
// ten at 8-row tiles, the "pred + masks" phase of the per-wave traces (1.4 / 3.3 us).  profiles/NOTES.md R6-11.
#define BXI_PW_LD(i) "global_load_dword %[v" #i "], %[o" #i "], %[b] sc1\n\t"
#define BXI_PW_OUT(i) [v##i] "=&v"(v[i])
#define BXI_PW_IN(i) [o##i] "v"(off[i])
template <int N>
__device__ __forceinline__ void load_words_past(const unsigned int* base_in, const uint32_t (&off)[N], uint32_t (&v)[N]) {
    static_assert(N >= 5 && N <= 12, "R + D of the tile kernels");
    // the base is wave-uniform by construction (a tile's image); said so explicitly: where the compiler cannot prove it (an ablation build did not)
    // an "s" operand is handed a VGPR pair and the assembler rejects the statement.  Two v_readfirstlane at most, none when the value is scalar already.
    const unsigned long long b64 = reinterpret_cast<unsigned long long>(base_in);
    const unsigned int* base = reinterpret_cast<const unsigned int*>(
        ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(b64 >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)b64));
    if constexpr (N == 5)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), [b] "s"(base) : "memory");
    else if constexpr (N == 6)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), [b] "s"(base) : "memory");
    else if constexpr (N == 7)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), [b] "s"(base) : "memory");
    else if constexpr (N == 8)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) BXI_PW_LD(7) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6), BXI_PW_OUT(7)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), BXI_PW_IN(7), [b] "s"(base) : "memory");
    else if constexpr (N == 9)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) BXI_PW_LD(7) BXI_PW_LD(8) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6), BXI_PW_OUT(7), BXI_PW_OUT(8)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), BXI_PW_IN(7), BXI_PW_IN(8), [b] "s"(base) : "memory");
    else if constexpr (N == 10)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) BXI_PW_LD(7) BXI_PW_LD(8) BXI_PW_LD(9) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6), BXI_PW_OUT(7), BXI_PW_OUT(8), BXI_PW_OUT(9)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), BXI_PW_IN(7), BXI_PW_IN(8), BXI_PW_IN(9), [b] "s"(base) : "memory");
    else if constexpr (N == 11)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) BXI_PW_LD(7) BXI_PW_LD(8) BXI_PW_LD(9) BXI_PW_LD(10) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6), BXI_PW_OUT(7), BXI_PW_OUT(8), BXI_PW_OUT(9), BXI_PW_OUT(10)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), BXI_PW_IN(7), BXI_PW_IN(8), BXI_PW_IN(9), BXI_PW_IN(10), [b] "s"(base) : "memory");
    else if constexpr (N == 12)
        asm volatile(BXI_PW_LD(0) BXI_PW_LD(1) BXI_PW_LD(2) BXI_PW_LD(3) BXI_PW_LD(4) BXI_PW_LD(5) BXI_PW_LD(6) BXI_PW_LD(7) BXI_PW_LD(8) BXI_PW_LD(9) BXI_PW_LD(10) BXI_PW_LD(11) "s_waitcnt vmcnt(0)"
                     : BXI_PW_OUT(0), BXI_PW_OUT(1), BXI_PW_OUT(2), BXI_PW_OUT(3), BXI_PW_OUT(4), BXI_PW_OUT(5), BXI_PW_OUT(6), BXI_PW_OUT(7), BXI_PW_OUT(8), BXI_PW_OUT(9), BXI_PW_OUT(10), BXI_PW_OUT(11)
                     : BXI_PW_IN(0), BXI_PW_IN(1), BXI_PW_IN(2), BXI_PW_IN(3), BXI_PW_IN(4), BXI_PW_IN(5), BXI_PW_IN(6), BXI_PW_IN(7), BXI_PW_IN(8), BXI_PW_IN(9), BXI_PW_IN(10), BXI_PW_IN(11), [b] "s"(base) : "memory");
}
#undef BXI_PW_LD
#undef BXI_PW_OUT
#undef BXI_PW_IN
__device__ __forceinline__ float4 f4_of(const u4v& v) { return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)); }

// ---- workspace ---------------------------------------------------------------------------------------------------------
struct Ws {
    float4* lab4;                               // [B,h,w] (L, a, b, 0)
    float* lab_planar;                          // [B,3,h,w] only the generic pooling path (other strides, unaligned canvases) fills it
    unsigned int* pred;                         // [B,h,w] epoch << 4 | bits; bit d = colour predicate of pair direction d with this pixel as the step pixel
    unsigned long long* colpart;                // [N,n_cb,w] packed (max logit, first row) of a band of rows
    unsigned long long* rowkey;                 // [N,n_rp,h] packed (max logit, first column)
    int n_cb, n_rp;
    int4* tab;                                  // [N+1] {tile prefix | img << 24, r0 | r1 << 16, c0 | c1 << 16, epoch}; [N].x = tiles
    unsigned int* bandflag;                     // [N,n_cb] epoch once a stream block's zero-fill and partial maxima are in memory (single-launch form)
    unsigned int* epoch;                        // [1] tag of the last evaluation FINISHED on this workspace (0 after the one-time zeroing); only the
                                                // finisher writes it, as its last act
    unsigned int ep;                            // this evaluation's tag (1 .. 2^28 - 1) = epoch + 1, read ON THE DEVICE by every kernel (with_tag):
                                                // data another workgroup of the SAME launch reads carries it.  Nothing about it is a kernel
                                                // argument, so a captured launch replayed from a hipGraph draws a fresh tag every time
    // words polled inside pair_kernel; zeroed by prep_kernel's table waves, i.e. before a kernel boundary
    unsigned long long* acc1;                   // [kAcc1Words] (one per 128 B) predicate workgroups: segments evaluated << 40 | sum W
    unsigned long long* sumw;                   // [1]   1 << 63 | sum W, published by the reducer wave once every segment is in (0 = not yet)
    unsigned long long* acc2;                   // [N][kAcc2Split] (one per 128 B) tile waves: arrivals << 52 | sum (W pw + 1) in 2^-24 units
    unsigned long long* dice;                   // [N]   leader: 1 << 32 | bits of the instance's dice loss (0 = not published)
    unsigned int* fault;                        // [1]   bit mask of waits that ran out (never expected)
    // what bxi_boxinst_targets_f32 leaves for evaluations with BXI_EVAL_TARGETS_READY (next to lab4 / pred)
    // (ONE pointer for the three regions: every field of this structure is a pair of scalar registers in every role of every kernel)
    unsigned char* tgt;                         // +0: tkey [1] u32, digest of the geometry / window / threshold the targets were computed for (0 = none)
                                                // +256: boxtab [kBoxCap] int4 per GT box {img << 24, r0 | r1 << 16, c0 | c1 << 16, 0}: what its predicate waves count against
                                                // +256 + 16 kBoxCap: boxcnt [kBoxCap][kBoxSplit] u64 (one per 128 B) per GT box: sum over its pixels p and the 8
                                                //   neighbours k of [sim_k(p) >= thresh]
    unsigned int pred_any;                      // 1: lab4 / pred come from bxi_boxinst_targets_f32 (an earlier launch): their tag field is not this evaluation's
    unsigned int ws_n16;                        // size of the workspace in 16-byte units (the finisher zeroes all of it when the tag counter is about to wrap)
    __host__ __device__ __forceinline__ unsigned int* tkey() const { return reinterpret_cast<unsigned int*>(tgt); }
    __host__ __device__ __forceinline__ int4* boxtab() const { return reinterpret_cast<int4*>(tgt + 256); }
    __host__ __device__ __forceinline__ unsigned long long* boxcnt() const { return reinterpret_cast<unsigned long long*>(tgt + 256 + 16 * (size_t)kBoxCap); }
};

__device__ __forceinline__ unsigned long long* acc2_word(unsigned long long* acc2, int n, int sub) {
    return acc2 + ((size_t)n * kAcc2Split + (sub & (kAcc2Split - 1))) * kAcc2Stride;
}

// This evaluation's tag: one more than the tag of the last evaluation that FINISHED on this workspace.  Every wave of an evaluation
// reads the word; only the finisher -- the last workgroup, which has by then seen every other wave of the launch arrive (each tile
// wave arrives exactly once, with or without tiles) -- writes it.  Evaluations that share a workspace are serialised by their stream,
// so the word is stable while anybody reads it, and a reader is always a LATER kernel than the writer: a scalar load (constant cache,
// invalidated at every dispatch) on one side, a plain store on the other.  What it costs is WHERE it is read: a wave that reads it
// first thing starts one dependent memory round trip late -- the whole launch with it (18.1 against 17.4 us with the tag as a kernel
// argument, same box).  The roles that head the launch's dependency chain (stream, pool) therefore read it behind their first loads
// (`after_loads`), where the round trip hides; the others wait for somebody anyway.  Likewise the finisher's store: written through
// (sc1) it is acknowledged ~0.3 us later than a plain one, and the launch ends on it.
__device__ __forceinline__ unsigned int next_tag(unsigned int e) { const unsigned int t = (e + 1u) & 0x0fffffffu; return t ? t : 1u; }
__device__ __forceinline__ Ws with_tag(Ws ws) {
    unsigned int e;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(e) : "s"(ws.epoch) : "memory");
    ws.ep = next_tag(e);
    return ws;
}
// min(_iter / pairwise_warmup, 1) (condinst_head.py:1330-1331).  warmup >= 0: the caller's value.  warmup < 0: -warmup is
// pairwise_warmup and the factor comes from the device counter as it stands after this call's `self._iter += 1` (:1297; the finisher
// adds the 1 at the very end, behind every reader): a float32 add, then Python's double division, then the f32 operand of the multiply.
__device__ __forceinline__ float resolve_warmup(float warmup, const float* iter) {
    if (warmup >= 0.f) return warmup;
    const float it = __fadd_rn(__hip_atomic_load(iter, BXI_RLX, BXI_AGENT), 1.0f);
    return (float)fmin((double)it / (double)(-warmup), 1.0);
}

static inline int tile_width(int dil) { return 64 - 2 * dil; }
static inline int64_t eval_cap(int N, int h, int w, int dil, int R) {
    const int tw = tile_width(dil);
    return (int64_t)(N > 0 ? N : 1) * ((h + R - 1) / R) * ((w + tw - 1) / tw);
}

static size_t carve(void* base, int B, int N, int h, int w, Ws* ws) {
    const int N1 = N > 0 ? N : 1;
    const size_t Sn = (size_t)(h + kSBlk - 1) / kSBlk;
    const size_t cb_max = (size_t)(h + kYR * 2 - 1) / (kYR * 2), rp_max = (size_t)(w + kYC * 2 - 1) / (kYC * 2);   // the head-fused launch's tiles
    Carver cv(base, 256);
    Ws t;
    const size_t P = (size_t)h * w, B1 = B > 0 ? B : 1;
    // the epoch word FIRST, at offset 0 whatever the shape: evaluations of different shapes share a workspace (one per stream), and the
    // tag counter that tells their records apart must be the same word for all of them (everything behind it moves with the shape)
    t.epoch = cv.take<unsigned int>(1);
    t.lab4 = cv.take<float4>(B1 * P);
    t.lab_planar = cv.take<float>(3 * B1 * P);
    t.pred = cv.take<unsigned int>(B1 * P);
    t.tgt = cv.take<unsigned char>(256 + 16 * (size_t)kBoxCap + 8 * (size_t)kBoxCap * kBoxSplit * kAcc2Stride);
    t.colpart = cv.take<unsigned long long>((size_t)N1 * (cb_max > Sn ? cb_max : Sn) * w);
    t.rowkey = cv.take<unsigned long long>((size_t)N1 * h * (rp_max > 1 ? rp_max : 1));
    t.n_cb = (int)Sn; t.n_rp = 1;
    t.tab = cv.take<int4>((size_t)(N1 + 1));
    t.bandflag = cv.take<unsigned int>((size_t)N1 * (cb_max > Sn ? cb_max : Sn));
    t.ep = 0u; t.pred_any = 0u; t.ws_n16 = 0u;
    t.acc1 = cv.take<unsigned long long>((size_t)kAcc1Words * kAcc2Stride);
    t.sumw = cv.take<unsigned long long>(1);
    t.acc2 = cv.take<unsigned long long>((size_t)N1 * kAcc2Split * kAcc2Stride);
    t.dice = cv.take<unsigned long long>((size_t)N1);
    t.fault = cv.take<unsigned int>(1);
    if (ws) *ws = t;
    return cv.bytes();
}

}  // namespace bxi
