// fused_eval.hip -- the BoxInst loss evaluation (forward AND finished backward) on gfx950: ONE launch (eval1_kernel, the roles below in
// one grid) where the shipped shapes allow it, otherwise TWO (prep_kernel, pair_kernel).
//
// Replaces (reference, LiWentomng/BoxInstSeg) CondInstMaskHead.loss with boxinst_enabled,
// condinst_head.py:1288-1343, together with everything it calls:
//   get_targets / get_original_image / get_bitmasks_from_boxes   :170-186, :1345-1448   (image side)
//   get_image_color_similarity + unfold_wo_center                :190-246
//   compute_project_term + dice_coefficient                      :117-143
//   pairwise_nlog (CUDA op, pairwise.cu:68-149) + weights / normalise / warm-up   :1315-1332
// and what autograd does behind them, with the upstream factors folded in.
//
//   launch 1  prep_kernel   256-thread workgroups, three roles, nothing waits                              HBM stream
//     table waves   per-instance table (tile prefix, box cells, image, valid-cell limits): 16 bytes per instance; zeroes the
//                   words the next launch polls
//     stream blocks 4 waves x 8 rows of one instance map: zero-fill of g_logits (written through), row maxima, column maxima
//                   of the block's 32 rows -> partials for the leaders of the next launch
//     pool blocks   the 4 input rows of 64 pooled pixels -> de-normalise, truncate, 4x4 mean, Lab (fp64) -> ONE 16-byte
//                   store per pooled pixel
//   launch 2  pair_kernel   [predicate blocks][reducer][leaders][tile blocks][finisher]
//     leaders       one block per instance: partial maxima -> maxima -> sigmoid -> dice -> unit projection gradients, ADDED
//                   (float atomic) at the arg-max positions of the zero-filled gradient.  Nobody waits for a leader but the finisher.
//     predicate waves  one wave64 per pooled row segment (64 pixels) of an image: the four colour predicates per pixel (one byte)
//                   -- each unordered pair ONCE PER IMAGE, not once per instance and tile -- and the segment's share of the pair
//                   weights' sum (a function of the image and the boxes only, :1324-1328) -> one packed integer atomic per workgroup;
//                   the reducer (one wave, right behind them in the grid) adds the 64 count words up and publishes ONE word (1 << 63 | sum W)
//     tile waves    one wave64 per box tile (no barrier; LDS only to park its own pair terms): logits tile + halo in registers, every unordered pair
//                   evaluated once -- in the un-split single launch (4-row tiles, dilation 2) the part of a pair that needs the logits alone (log2 S, 1 / S) AHEAD of the
//                   wait for the predicate words, the weighted sums behind it;
//                   g_pw warm/max(sum W,1) d pw is ADDED (float atomic) to the gradient -- an element receives
//                   at most two additions onto 0 (its tile's and its leader's), so the sum does not depend on their order;
//                   the tile's share of sum W pw goes to an integer accumulator by an atomic without return.  Its two waits:
//                   its own predicate bytes (bit 7 = evaluated) before the pair loop, the published sum W (the global
//                   normaliser) after it; both are produced by workgroups that precede it in the grid and never wait
//                   for a tile.  In the single-launch forms the wave ARRIVES (its share) as soon as the pair loop of its last tile
//                   is done, ahead of that tile's wait for sum W and its adds: the finisher reads nothing else of it.  A wait that runs out after the
//                   arrival is loud by itself (NaN gradient elements, fault and status words, NaN losses).
//     finisher      the last workgroup: polls the accumulators (every tile wave arrives exactly once, with or without tiles), writes the two
//                   loss values and, as its last act, advances the workspace's epoch -- while the last tile waves may still be
//                   waiting for sum W and adding (single-launch forms): the launch ends at the later of the two.
// What one workgroup hands to another inside a launch carries the evaluation's TAG = epoch + 1; the epoch is word 0 of the workspace,
// read on the device by every kernel of an evaluation (with_tag) -- nothing about it is a kernel argument, so a captured launch replayed
// from a hipGraph is as correct as an eager one; the warm-up factor likewise (resolve_warmup).  The workspace is zeroed once and keeps ONE
// layout (a function of the canvas and of its size), so a tag field only ever holds tags.  The launch's form is the caller's `flags`
// (include/boxinst_hip.h: BXI_EVAL_*): the library keeps no process-wide state and guesses nothing about what else runs on the device.
// Every wait is bounded and running out of it is loud: NaN losses, a status word, a poisoned gradient (rescale_kernel).
// Table entries instead of a work list: a tile wave finds its tile from 16 bytes per instance that every wave reads (the same
// few cache lines), not from a record of its own behind a list length (two dependent misses right after the kernel boundary).
// Data layout in HBM: everything NCHW / row-major as the reference hands it over; intermediates: Lab [B,h,w] float4 (1.6 MB at
// 2x800x1024), column / row partial maxima, 16-byte table entries.
// Where the parts live (included in this order, each assuming the ones before it): eval_protocol_device.hpp -- constants, loads past the caches,
// workspace, tag; eval_front_device.hpp -- table, stream and pool roles, the head-fused first launch; eval_tile_device.hpp -- predicate and tile
// waves; eval_back_device.hpp -- leaders, reducer, tile role, finisher.  This file: the kernels and the host side.
#include "loss_common.hpp"
#include "dynamic_head_device.hpp"
#include "eval_protocol_device.hpp"
#include "eval_front_device.hpp"
#include "eval_tile_device.hpp"
#include "eval_back_device.hpp"
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <ctime>

namespace bxi {

// ---- launch 1 of the two-launch form ------------------------------------------------------------------------------------------
// what the first launch needs beyond its streams
struct PrepTail {
    int ready;               // BXI_EVAL_TARGETS_READY (the number of GT boxes + 1): no pool workgroups; the first table wave gathers sum W from the boxes' pair counts
    unsigned int key;        // ... and checks that the targets in the workspace are the ones this call means
};

// grid: [table blocks][pool blocks][stream blocks] (pool_first) or [table][stream][pool].  Nobody in this launch waits for anybody.
__global__ __launch_bounds__(256, kPrepOcc) void prep_kernel(PoolArgs pa, int n_pool, int n_items, InstArgs a, int dil, int R, Ws ws_in, LossState st,
                                                       float* __restrict__ g_logits, int vec, int pool_first, PrepTail tl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Ws ws = ws_in;                                        // the tag is read where a role needs it (with_tag), behind its loads
    const int n_tab = ((a.N + 64) / 64 + kWaves - 1) / kWaves;
    const int Sn = (a.h + kSBlk - 1) / kSBlk;
    const int n_stream = a.N * Sn;
    const int blk = (int)blockIdx.x;
    const int tix = blk * kWaves + (int)(threadIdx.x >> 6);
    (void)tix;
    BXI_TW(0, tix, 0);
    int role = 0, idx = blk;                              // 0 table, 1 pool, 2 stream
    if (blk >= n_tab) {
        idx = blk - n_tab;
        const int n_a = pool_first ? n_pool : n_stream, n_b = pool_first ? n_stream : n_pool;
        (void)n_b;
        if (idx < n_a) role = pool_first ? 1 : 2;
        else { idx -= n_a; role = pool_first ? 2 : 1; }
    }
    if (role == 0) {
        const int k = blk * kWaves + (int)(threadIdx.x >> 6);
        if (64 * k <= a.N) { ws = with_tag(ws); table_wave(a, pa.meta, dil, R, ws, st, k, true, tl.ready, tl.key); }
    } else if (role == 2) {
        const LogitRows rows = {a.logits + (int64_t)(idx / Sn) * a.h * a.w, a.w, vec & 1, vec >> 1};
        stream_block<false>(a, ws, g_logits, vec & 1, idx, reinterpret_cast<unsigned long long*>(smem), rows, tix);     // (no tagged record in this form)
    } else {
        double* lut = reinterpret_cast<double*>(smem);
        double* fch = lut + 256;
        int* part = reinterpret_cast<int*>(fch + 3 * 64);
        pool_block(pa, ws, idx, n_pool, n_items, lut, part, fch, tix, [&](Ws& w_) { w_ = with_tag(w_); });
    }
    BXI_TW(0, tix, 7);
}

// workgroups per CU of pair_kernel (four only where the tile role fits 128 VGPRs without spilling: dilation <= 2 -- every shipped configuration uses 2;
// dilation 3 needs 10-row register arrays and ran with 9 spilled VGPRs at four per CU)
constexpr int pair_occ(int D, int R) { return R == 4 ? (D <= 2 ? 4 : 3) : (D <= 2 ? 3 : 2); }

// grid: [n_pb predicate blocks][reducer][N leaders][n_tb tile blocks][finisher].  The only waits: a tile wave for the predicate waves
// (earlier in the grid, never waiting themselves), the finisher for everybody (nobody waits for it).  Every wait is bounded, and
// running out of it is loud: NaN losses, status word, poisoned gradient (the reference surfaces launch failures through
// AT_CUDA_CHECK, pairwise.cu:173,200).
template <int D, int R>
__global__ __launch_bounds__(256, pair_occ(D, R)) void pair_kernel(const float* __restrict__ up_prj, const float* __restrict__ up_pw, float warmup,
                                                       float n2max, int zero_bit, int n_pb, int n_items, int spin_limit, ValidCells vc, float* __restrict__ losses,
                                                       float* __restrict__ g_logits, InstArgs a, Ws ws_in, LossState st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float red[16];
    const int blk = (int)blockIdx.x;
    const int N = a.N;
    if (blk < n_pb) {                                                // ---- predicate waves: first in the grid, everybody asks for their words
        if (zero_bit) return;                                          // every pair weighs 1: sum W has a closed form, the tiles take the log-space path
        pred_role<false>(a, vc, ws_in /* no tag yet: it comes with the wave's first loads (pred_item) */, D, n2max, blk, n_pb, n_items, spin_limit);
        return;
    }
    const Ws ws = with_tag(ws_in);
    const float upp = up_prj ? *up_prj : 1.f, upw = up_pw ? *up_pw : 1.f;
    // (grid order [predicate][reducer][leaders][tiles][finisher].  Measured and dropped -- profiles/NOTES.md R6-10 --: the tile workgroups AHEAD of the leaders,
    // so that 128 more of them are resident from the start: 30.7 vs 28.4 us at 96 instances, 35.0 vs 33.0 at 128 -- the leaders then run last and the
    // finisher waits for their dice words)
    const int n_tb = (int)gridDim.x - 2 - N - n_pb;
    const int lead0 = n_pb + 1, tile0 = n_pb + 1 + N;
    if (blk == n_pb) {                                          // ---- the reducer
        reducer_role<false>(ws, zero_bit, n_pb > 0 ? n_items : 0, spin_limit);      // (no predicate workgroups here: sum W is in memory already)
    } else if (blk == (int)gridDim.x - 1) {
        finisher_role<false>(a, ws, st, upp, upw, resolve_warmup(warmup, st.iter), zero_bit, n_items, spin_limit, R, n_tb * kWaves, losses);
    } else if (blk >= lead0 && blk < lead0 + N) {                      // ---- leader of an instance
        BXI_TW(3, 1 + blk - lead0, 0);
        leader_block<false>(a, D, ws, st, blk - lead0, upp, g_logits, smem, red, spin_limit);
    } else {
        tile_role<D, R, false, kTilesPair>(a, vc, ws, upw * resolve_warmup(warmup, st.iter), n2max, zero_bit, n_items, spin_limit, g_logits, smem, blk - tile0, n_tb, st, losses);
    }
}

// ---- the single-launch form ---------------------------------------------------------------------------------------------------
// All roles in ONE grid, in this order:  [stream blocks (the table is a duty of some of their waves)][pool blocks][predicate blocks][reducer][N leaders][tile blocks][finisher].
// The table wave k (entries 64 k .. 64 k + 63) is wave 0 of stream block k -- or, where the stream blocks stay on and an instance's last band
// leaves a wave without rows, the last wave of instance k's last band: that one writes it at once, the other behind its 8 KB of zero-fill.
// Workgroups are dispatched in grid order and every wait is for a workgroup EARLIER in the grid -- with two exceptions, both of stream
// workgroups that stay on and both only in forms where every stream workgroup holds a slot from the start and at least half of the slots
// stay free: their tile waves wait for predicate workgroups later in the grid, and, with the table in the last bands, for a table wave
// in a stream workgroup that may stand behind their own (it waits for nobody):
//   table, stream, pool   wait for nobody;
//   leader n              for the table entry n and the band flags of instance n (stream blocks);
//   predicate wave        for the Lab pixels it reads (pool blocks; 16-byte records carrying the evaluation's tag) and the table;
//   tile wave             for the table, its predicate words (tagged), sum W (reducer <- predicate blocks) and the band flags of
//                         the rows it adds onto (stream blocks);
//   finisher              for everybody.
// So no waiter can hold a slot that a workgroup it waits for still needs.  What crosses workgroups is written through (sc1) and
// read past the caches; what a flag announces is drained (s_waitcnt vmcnt(0)) before the flag goes out; what announces itself is
// one 16-byte (or 4-byte) record written by one store.  Four workgroups per CU (<= 128 VGPRs: the tile role's budget): at the
// headline size the table + stream + pool workgroups fill the GPU once, and the back half flows into the slots they leave -- the
// kernel boundary of the two-launch form (~2.2 us) is gone.  The two-launch form stays for 8-row tiles (> 96 instances: 2
// workgroups per CU would starve the front half), dilation 4, the head-fused first launch and the generic pooling path.
// R = 8 ("the long form", three workgroups per CU): the same grid for MANY instances.  With 4-row tiles 128 instances are ~4600 tiles on at most
// half the slots' waves -- every tile wave then walks two or three tiles, each a ~7 us dependent chain, one after the other (45 us per
// evaluation).  8-row tiles are ~2300, one per wave, and the whole back half runs while the front half still streams: no kernel boundary,
// the tile waves' arithmetic under the logit stream.  Nothing here waits for a workgroup LATER in the grid (no staying-on: `merge` = 0),
// so the form makes progress at any residency; the pool workgroups go first (`pool_first`), the image side being the longer chain.
// READY (BXI_EVAL_TARGETS_READY): an instantiation of its own -- no pool / predicate role, table workgroups at the head of the grid, sum W
// gathered by the reducer workgroup -- so that the un-split kernel stays what it was (the same registers, no extra argument).
template <int D, int R, bool READY>
__global__ __launch_bounds__(256, (R == 4 ? kOneOcc : kLongOcc)) void eval1_kernel(PoolArgs pa, int n_pool, int n_items, int n_pb, int n_tb, InstArgs a, Ws ws_in, LossState st, ValidCells vc,
                                                        const float* __restrict__ up_prj, const float* __restrict__ up_pw, float warmup, float n2max, int spin_limit,
                                                        float* __restrict__ losses, float* __restrict__ g_logits, int vec, int merge, int ready_in, unsigned int key,
                                                        int n_tabw_in) {
    const int ready = READY ? ready_in : 0, n_tabw = READY ? n_tabw_in : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float red[16];
    Ws ws = ws_in;
    const int N = a.N;
    constexpr int n_tab = 0;                                  // (trace index layout: table, stream, pool)
    const int Sn = (a.h + kSBlk - 1) / kSBlk;
    const int n_stream = N * Sn;
    const int blk = (int)blockIdx.x;
    // n_tabw > 0 (targets ready): the table has workgroups of its own at the head of the grid.  With the image side in memory the table IS the
    // head of every chain (tile waves, leaders), and as a duty of a stream wave behind its zero-fill and loads it came ~5 us into the launch
    // (its drain waits for that wave's 8 KB of written-through stores) and made the first instance's band the last one.
    if (READY && blk < n_tabw) {
        const int k = blk * kWaves + (int)(threadIdx.x >> 6);
        if (64 * k <= N) table_wave(a, pa.meta, D, R, with_tag(ws), st, k, false, -1, 0u);
        return;
    }
    // role of this workgroup: 0 stream, 1 pool, 2 leader, 3 predicate, 4 tile, 5 finisher, 6 reducer
    int role, idx = blk - n_tabw;
    constexpr bool pool_first = R == 8;                      // the long form (a run-time switch here costs the short form a stack slot)
    const int n_a = pool_first ? n_pool : n_stream, n_b = pool_first ? n_stream : n_pool;      // grid: [stream][pool] or [pool][stream], then the back half
    if (idx < n_a) role = pool_first ? 1 : 0;
    else if ((idx -= n_a) < n_b) role = pool_first ? 0 : 1;
    else if ((idx -= n_b) < n_pb) role = 3;
    else if ((idx -= n_pb) < 1) role = 6;                              // the reducer
    else if ((idx -= 1) < N) role = 2;
    else if ((idx -= N) < n_tb) role = 4;
    else role = 5;
    const int tix = (n_tab + (role == 0 ? idx : n_stream + idx)) * kWaves + (int)(threadIdx.x >> 6);
    (void)tix;
    bool stayed = false;
    if (role == 0) {
        BXI_TW(0, tix, 0);
        // the table is a duty of stream waves: a workgroup of its own would be the one workgroup too many for the front half to be
        // resident at once at the headline size.  Wave k of the table (entries 64 k .. 64 k + 63) is wave 0 of stream workgroup k -- or
        // (merge bit 1, the host's choice: plan_eval1, table_last) the last wave of instance k's last band, which has no rows there: no
        // zero-fill stores to drain ahead of the table's own, no loads to wait for, so the table -- the first thing every leader,
        // predicate wave and tile wave polls -- is in memory as the launch starts, and stream workgroup 0, whose waves stay on as tile
        // waves, ends with the others.  Safe: the table wave waits for nobody, and the host takes this placement only where every stream
        // workgroup holds a slot from the start, so a staying wave that polls an entry written LATER in the grid never holds the slot the
        // writer needs.
        const LogitRows rows = {a.logits + (int64_t)(idx / Sn) * a.h * a.w, a.w, vec & 1, vec >> 1};
        stream_block<true>(a, ws, g_logits, vec & 1, idx, reinterpret_cast<unsigned long long*>(smem), rows, tix, [&](Ws& w_) {
            w_ = with_tag(w_);
            if (READY) return;
            // (two call sites on purpose: with one, behind a computed k, the forms that keep the table where it was -- 64 instances, a
            // shared device -- ran 0.3 us slower in this kernel; profiles/NOTES.md R23-1)
            if ((threadIdx.x >> 6) == 0 && 64 * idx <= N && !(merge & 2)) table_wave(a, pa.meta, D, R, w_, st, idx, false, 0, 0u);
            if ((threadIdx.x >> 6) == kWaves - 1 && (merge & 2) && idx % Sn == Sn - 1 && 64 * (idx / Sn) <= N) table_wave(a, pa.meta, D, R, w_, st, idx / Sn, false, 0, 0u);
        });
        BXI_TW(0, tix, 7);
        if (!merge) return;
        // ... and stays as a tile workgroup: its four waves are the first tile waves, resident since the start of the launch, so their
        // table -> tile -> logits -> per-pixel chain runs while the pool workgroups finish instead of behind a slot that has to come
        // free first.  (It now waits for predicate workgroups LATER in the grid.  Those wait only for pool workgroups, which wait for
        // nobody, and the host launches this form only while the stream workgroups leave at least half of the slots free: a
        // predicate workgroup always finds a slot.  With the table in the last bands it also waits for a table wave of a stream
        // workgroup that may stand later in the grid: that one is resident too -- the stream workgroups are at most a quarter of the
        // slots here -- and writes the table before it waits for anything.)
        __syncthreads();                                                  // the column-partial LDS becomes the tile waves' scratch
        role = 4;
        stayed = true;
        idx -= n_stream;                                                   // tile workgroup index idx + n_stream below
    }
    if (!READY && role == 1) {
        BXI_TW(0, tix, 0);
        double* lut = reinterpret_cast<double*>(smem);
        double* fch = lut + 256;
        int* part = reinterpret_cast<int*>(fch + 3 * 64);
        pool_block(pa, ws, idx, n_pool, n_items, lut, part, fch, tix, [&](Ws& w_) { w_ = with_tag(w_); });
        BXI_TW(0, tix, 7);
        return;
    }
    // (a stream workgroup that stays on has its tag already; predicate waves and leaders get it with their first poll)
    if (!stayed && role != 3 && role != 2) ws = with_tag(ws);
    const float upp = up_prj ? *up_prj : 1.f, upw = up_pw ? *up_pw : 1.f;
    if (role == 2) {
        BXI_TW(3, 1 + idx, 0);
        leader_block<true>(a, D, ws, st, idx, upp, g_logits, smem, red, spin_limit);
        return;
    }
    if (!READY && role == 3) { pred_role<true>(a, vc, ws, D, n2max, idx, n_pb, n_items, spin_limit, merge != 0); return; }
    if (role == 6) {
        if (!READY) reducer_role<true>(ws, 0, n_items, spin_limit);
        else if (threadIdx.x < 64) {
            // targets ready: sum W is a gather over the instances' boxes, published once the table says this evaluation's polled words are zeroed
            // (the table wave is a wave of the first stream workgroup: earlier in the grid, waiting for nobody)
            if (table_complete<true>(ws, 0, spin_limit)) publish_gathered_sumw(a, ws, ready - 1, key);
            else if (threadIdx.x == 0) atomicOr(ws.fault, kFaultCounts);
        }
        return;
    }
    if (role == 4) {          // ONE call site for the stream workgroups that stay on and for the tile workgroups proper
        const int shift = merge ? n_stream : 0;
        tile_role<D, R, true, (READY ? kTilesOneReady : kTilesOne)>(a, vc, ws, upw * resolve_warmup(warmup, st.iter), n2max, 0, n_items, spin_limit, g_logits, smem, idx + shift, n_tb + shift, st, losses);
        return;
    }
    finisher_role<true>(a, ws, st, upp, upw, resolve_warmup(warmup, st.iter), 0, n_items, spin_limit, R, (n_tb + (merge ? n_stream : 0)) * kWaves, losses);
}

// ---- bxi_boxinst_targets_f32: the image side alone, ahead of the evaluation ------------------------------------------------------
// CondInstMaskHead.loss computes its targets from `imgs` and `gt_bboxes` alone (get_targets, condinst_head.py:1298-1299, :1345-1448) --
// both exist before the backbone runs (condinst.py:53 vs :73).  Two launches with NO in-kernel wait (a kernel boundary between them), so the
// call makes progress next to anything: launch 1 = the pool workgroups of prep_kernel (Lab records, tag field 0) + one workgroup that writes
// the box table and zeroes the boxes' count words; launch 2 = the predicate waves over the box table, per-box pair counts.
// (seven workgroups per CU -- the pool role needs 66 registers --: the 1600 items of a 2 x 800 x 1024 batch are resident at once, one item each)
__global__ __launch_bounds__(256, 7) void targets_pool_kernel(PoolArgs pa, int n_pool, int n_items, GtTable gt, int Hc, int Wc, int stride, int h, int w, Ws ws,
                                                               unsigned int key) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (blockIdx.x == 0) {
        const int G = gt.first[gt.B];
        for (int g = threadIdx.x; g < G; g += 256) {
            int img = 0;
            const float* bp = gt_box(gt, g, img);
            const Rect rc = box_rect(bp, Hc, Wc, stride, stride / 2, h, w);
            ws.boxtab()[g] = make_int4(img << 24, rc.r0 | (rc.r1 << 16), rc.c0 | (rc.c1 << 16), 0);
#pragma unroll
            for (int j = 0; j < kBoxSplit; ++j) ws.boxcnt()[((size_t)g * kBoxSplit + j) * kAcc2Stride] = 0ull;
        }
        if (threadIdx.x == 0) *ws.tkey() = key;
        return;
    }
    double* lut = reinterpret_cast<double*>(smem);
    double* fch = lut + 256;
    int* part = reinterpret_cast<int*>(fch + 3 * 64);
    pool_block(pa, ws, (int)blockIdx.x - 1, n_pool, n_items, lut, part, fch, 0);
}

__global__ __launch_bounds__(256) void targets_pred_kernel(int h, int w, int G, ValidCells vc, Ws ws, int D, float n2max, int n_pb, int n_items) {
    __shared__ int boxacc[kBoxCap];
    for (int g = threadIdx.x; g < G; g += 256) boxacc[g] = 0;
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6);
    const int segs = (w + 63) >> 6;
    bool ok = true;
    for (int item = (int)blockIdx.x * kWaves + wave; item < n_items; item += n_pb * kWaves)
        (void)pred_item<false, true>(h, w, G, vc, ws, D, n2max, item, segs, 0, ok, boxacc);
    __syncthreads();
    // one arrival per (workgroup, box it met): integer adds commute -- run-to-run identical
    for (int g = threadIdx.x; g < G; g += 256) {
        const int v = boxacc[g];
        if (v) __hip_atomic_fetch_add(ws.boxcnt() + ((size_t)g * kBoxSplit + (blockIdx.x & (kBoxSplit - 1))) * kAcc2Stride, (unsigned long long)v, BXI_RLX, BXI_AGENT);
    }
}

// ---- rescale: g_logits finished for the factors recorded in `state` -> finished for (g_prj, g_pw) ----------------
// grid (8, N).  No-op when the factors are the recorded ones (the usual case: loss.backward() seeds both terms with 1).
// An evaluation whose status word is set has no gradient: it is poisoned here, next to the NaN losses.
__global__ __launch_bounds__(256) void rescale_kernel(InstArgs a, int dil, LossState st, const float* __restrict__ g_prj,
                                                       const float* __restrict__ g_pw, float* __restrict__ g_logits) {
    const int n = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    const int h = a.h, w = a.w;
    float* G = g_logits + (int64_t)n * h * w;
    if (st.status[0] != 0) {
        const int per = (h + gridDim.x - 1) / gridDim.x;
        const int ra = s * per, rb = min(h, ra + per);
        for (int i = tid; i < (rb - ra) * w; i += 256) G[(int64_t)ra * w + i] = __int_as_float(0x7fc00000);
        return;
    }
    const float np = *g_prj, nw = *g_pw, op = st.applied[0], ow = st.applied[1];
    if (np == op && nw == ow) return;
    const int R = st.status[1];
    const InstRec rec = st.inst[n];
    const InstBox ib = inst_from_rec(rec, dil, h, w);
    const int hr0 = ib.any ? (ib.dil.r0 / R) * R : 0, hr1 = ib.any ? min(h, ((ib.dil.r1 + R - 1) / R) * R) : 0;
    const int hc0 = ib.dil.c0, hc1 = ib.any ? ib.dil.c1 : 0;
    const float ratio = nw / ow;                      // recorded g_pw == 0 cannot be rescaled (documented)
    const unsigned long long* ckp = st.colk + (int64_t)n * w; const unsigned long long* rkp = st.rowk + (int64_t)n * h;
    auto carg = [&](int c) { return (int)(unsigned int)ckp[c]; };
    auto rarg = [&](int r) { return (int)(unsigned int)rkp[r]; };
    auto gcol = [&](int c) { return __uint_as_float((unsigned int)(ckp[c] >> 32)); };
    auto grow = [&](int r) { return __uint_as_float((unsigned int)(rkp[r] >> 32)); };
    const int cw = hc1 - hc0, rows = hr1 - hr0;
    const int per = (rows + gridDim.x - 1) / gridDim.x;
    const int ra = hr0 + s * per, rb = min(hr1, ra + per);
    const int npx = cw > 0 && rb > ra ? (rb - ra) * cw : 0;
    for (int i = tid; i < npx; i += 256) {            // G = ow*s*d + op*sp  ->  nw*s*d + np*sp
        const int r = ra + i / cw, c = hc0 + i % cw;
        float sp = 0.f;
        if (carg(c) == r) sp += gcol(c);
        if (rarg(r) == c) sp += grow(r);
        const float v = G[(int64_t)r * w + c];
        G[(int64_t)r * w + c] = (v - op * sp) * ratio + np * sp;
    }
    if (s == 0) {                                     // arg-max positions outside the hull hold op * sp
        for (int c = tid; c < w; c += 256) {
            const int r = carg(c);
            const bool in_t = r >= hr0 && r < hr1 && c >= hc0 && c < hc1;
            if (!in_t) {
                float v = gcol(c);
                if (rarg(r) == c) v += grow(r);
                G[(int64_t)r * w + c] = v * np;
            }
        }
        for (int r = tid; r < h; r += 256) {
            const int c = rarg(r);
            const bool in_t = r >= hr0 && r < hr1 && c >= hc0 && c < hc1;
            if (!in_t && carg(c) != r) G[(int64_t)r * w + c] = grow(r) * np;
        }
    }
}

__global__ void zero_losses2_kernel(float* losses, float* iter) { losses[0] = 0.f; losses[1] = 0.f; if (iter) atomicAdd(iter, 1.0f); }

// ---- host side ---------------------------------------------------------------------------------------------------
// LDS of a pool workgroup: the sRGB table and the three channels of its 64 pooled pixels (fp64), the four waves' partial sums
constexpr size_t kPoolLds = sizeof(double) * (256 + 3 * 64) + sizeof(int) * 4 * 3 * 64;

// pool workgroups for n_items items on `room` slots: as few items per workgroup as fill them, at most max_per (0: no cap; no room: max_per)
static int pool_wgs(int n_items, int room, int max_per) {
    int per = room > 0 ? (n_items + room - 1) / room : max_per;
    if (max_per > 0 && per > max_per) per = max_per;
    if (per < 1) per = 1;
    return (n_items + per - 1) / per;
}
// predicate workgroups: one wave per item, at most `cap` workgroups
static int pred_wgs(int n_items, int cap) {
    const int n = (n_items + kWaves - 1) / kWaves;
    return n < cap ? n : cap;
}
// tile workgroups: one wave per tile (`cap` tiles), at most `slots` workgroups
static int tile_wgs(int64_t cap, int slots) {
    const int64_t n = (cap + kWaves - 1) / kWaves;
    return n < slots ? (int)n : slots;
}

// A stream that is being captured into a hipGraph: the launch is recorded, not run; what the host decides here is frozen into the graph
static bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// Compute units the stream may use: a CU mask (hipExtStreamCreateWithCUMask, ROC_GLOBAL_CU_MASK) leaves fewer than the device has.
// The single-launch form needs to know (its stream workgroups must leave free slots for the workgroups they wait for).  Cached per
// stream handle (a handful of streams per process); a failing query counts as "the whole device".
static int stream_cus(hipStream_t s, int device_total) {
    struct Entry { std::atomic<uintptr_t> key; std::atomic<int> cus; };
    static Entry cache[8];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    const uintptr_t k = (reinterpret_cast<uintptr_t>(s) + 1) ^ ((uintptr_t)(unsigned)dev << 56);   // +1: the null stream is a key too; per device
    for (auto& e : cache)
        if (e.key.load(std::memory_order_acquire) == k) return e.cus.load(std::memory_order_relaxed);
    uint32_t mask[32] = {};
    int n = device_total;
    if (hipExtStreamGetCUMask(s, 32, mask) == hipSuccess) {
        int bits = 0;
        for (uint32_t m : mask) bits += __builtin_popcount(m);
        if (bits > 0 && bits < n) n = bits;
    } else {
        (void)hipGetLastError();
    }
    static std::atomic<unsigned> next{0};
    Entry& e = cache[next.fetch_add(1, std::memory_order_relaxed) % 8];
    e.cus.store(n, std::memory_order_relaxed);
    e.key.store(k, std::memory_order_release);
    return n;
}

// Rows per tile: 4 up to ~95 instances, 8 from there on (two launches; dilation <= 2).  With 4-row tiles 128 instances are ~4600
// tiles on ~2500 tile waves: two rounds of a ~7 us dependent chain (table -> logits -> predicate words -> pair loop -> sum W -> adds).
// 8-row tiles halve the count; at 157 - 161 VGPRs they run three workgroups per CU (round 3 ran them at two, where they lost): one
// round.  Measured (two launches, 200 x 256 maps, same box): 96 instances 29.4 vs 30.1 us, 128: 35.9 vs 38.3, 256: 64.0 vs 69.7;
// 64 instances: 24.2 vs 23.8 (single launch) -- hence the threshold.  BXI_EVAL_TILE_ROWS_8 / BXI_EVAL_TILE_ROWS_4 override.
static int tile_rows_for(int N, int dil) { return (N >= 96 && dil <= 2) ? 8 : 4; }

// digest of what targets are computed FOR -- canvas, stride, window, threshold, per image its shape, rows removed and box count -- kept in
// the workspace by bxi_boxinst_targets_f32 and compared on the device by an evaluation that counts on them (FNV-1a; never 0)
static unsigned int targets_key(const PoolArgs& pa, int B, int Hc, int Wc, int stride, int dil, float n2max, const int* first /* [B + 1] */) {
    unsigned int hsh = 2166136261u;
    auto mix = [&](unsigned int v) { for (int i = 0; i < 4; ++i) { hsh ^= (v >> (8 * i)) & 255u; hsh *= 16777619u; } };
    unsigned int nb;
    memcpy(&nb, &n2max, 4);
    mix((unsigned)B); mix((unsigned)Hc); mix((unsigned)Wc); mix((unsigned)stride); mix((unsigned)dil); mix(nb);
    for (int b = 0; b < B; ++b) { mix((unsigned)pa.meta.img_h[b]); mix((unsigned)pa.meta.img_w[b]); mix((unsigned)pa.meta.first_removed[b]); mix((unsigned)(first[b + 1] - first[b])); }
    return hsh ? hsh : 1u;
}
static void valid_cells_of(const PoolArgs& pa, int B, int stride, int h, int w, ValidCells& vc) {
    for (int b = 0; b < B; ++b) {                  // the device formula (valid_cells), evaluated here once per image
        const int half = stride / 2;
        auto cells = [&](int limit, int n) { const int v = limit - half <= 0 ? 0 : (limit - half + stride - 1) / stride; return v < n ? v : n; };
        vc.vrow[b] = cells(pa.meta.img_h[b] < pa.meta.first_removed[b] ? pa.meta.img_h[b] : pa.meta.first_removed[b], h);
        vc.vcol[b] = cells(pa.meta.img_w[b], w);
    }
}

// (sim >= thresh) for a valid neighbour as a compare on the squared Lab distance: exp(-0.5 * sqrt(n2)) >= thresh  <=>  n2 <= n2max
// (get_image_color_similarity :237 + the threshold of loss() :1324), n2max found by bisecting the f32 expression over the float
// bit patterns (it is non-increasing in n2 >= 0, and positive floats order like their bit patterns).  Host arithmetic: sqrtf is
// correctly rounded everywhere; expf is the C library's, as in the CPU reference path.
struct HostPred { float n2max; int zero_bit; };
static bool host_sim_pred(float n2, float thresh) { return expf(-sqrtf(n2) * 0.5f) >= thresh; }
static HostPred host_pred(float thresh) {
    static std::atomic<uint64_t> cache{~0ull};                          // (thresh bits << 32 | n2max bits) of the last call
    uint32_t tb, nb;
    memcpy(&tb, &thresh, 4);
    const uint64_t c = cache.load(std::memory_order_relaxed);
    HostPred p;
    p.zero_bit = (0.f >= thresh) ? 1 : 0;                               // weight of a padded / masked-out neighbour (sim == 0)
    if ((uint32_t)(c >> 32) == tb && c != ~0ull) { nb = (uint32_t)c; memcpy(&p.n2max, &nb, 4); return p; }
    if (!host_sim_pred(0.f, thresh)) p.n2max = -1.f;                    // thresh > 1: never
    else if (host_sim_pred(3.0e38f, thresh)) p.n2max = INFINITY;        // thresh <= 0 (exp underflows to 0): always
    else {
        uint32_t lo = 0u, hi;
        const float big = 3.0e38f;
        memcpy(&hi, &big, 4);                                           // pred(lo) true, pred(hi) false
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            float fm;
            memcpy(&fm, &mid, 4);
            if (host_sim_pred(fm, thresh)) lo = mid; else hi = mid;
        }
        memcpy(&p.n2max, &lo, 4);
    }
    memcpy(&nb, &p.n2max, 4);
    cache.store(((uint64_t)tb << 32) | nb, std::memory_order_relaxed);
    return p;
}

size_t eval_ws_bytes(int B, int N, int h, int w) { return carve(nullptr, B, N, h, w, nullptr); }
bool fused_eval_supported(int dil) { return dil >= 1 && dil <= kMaxDilFused; }
// the one-time initialisation of a workspace: all zero (epoch 0, no record carries a tag an evaluation will draw)
int eval_ws_init(void* workspace, size_t bytes, void* stream) {
    if (!workspace || !aligned(workspace, 256)) return BXI_ERR_WORKSPACE;
    if (hipMemsetAsync(workspace, 0, bytes, as_stream(stream)) != hipSuccess) { set_last_hip_error((int)hipGetLastError()); return BXI_ERR_LAUNCH; }
    return BXI_OK;
}

// the per-instance capacity a workspace of this size admits for this canvas (the layout is a function of both, never of a call's N)
static int ws_capacity(int B, int h, int w, int N, size_t workspace_bytes) {
    // (a pure function of (B, h, w, size): the last answer is kept per host thread -- a training loop asks the same question every
    // iteration, and the search is sixteen layouts)
    struct Last { int B, h, w, n_cap; size_t bytes; };
    static thread_local Last last = {0, 0, 0, 0, 0};
    if (last.bytes == workspace_bytes && last.B == B && last.h == h && last.w == w && last.n_cap >= N) return last.n_cap;
    int lo = N, hi = kMaxInst - 1;           // carve() is non-decreasing in N
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (carve(nullptr, B, mid, h, w, nullptr) <= workspace_bytes) lo = mid; else hi = mid - 1;
    }
    last = Last{B, h, w, lo, workspace_bytes};
    return lo;
}

// bxi_boxinst_targets_f32: Lab, predicate words and per-GT-box pair counts into the workspace, ahead of the evaluation
int launch_targets(const bxi_image_batch* batch, const float* const* boxes_per_img_host, const int* gt_count_host, int stride, int dil, float color_thresh,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!batch || !workspace) return BXI_ERR_NULL_POINTER;
    if (!fused_eval_supported(dil)) return BXI_ERR_UNSUPPORTED;
    if (batch->B <= 0 || batch->B > BXI_MAX_IMAGES || stride < 1 || batch->Hc % stride || batch->Wc % stride) return BXI_ERR_BAD_SHAPE;
    if (!batch->imgs) return BXI_ERR_NULL_POINTER;
    if (batch->image_masks) return BXI_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    PoolArgs pa = {};
    int rc = fill_pool_args(batch, nullptr, nullptr, pa);
    if (rc != BXI_OK) return rc;
    GtTable gt;
    int G = 0;
    rc = fill_gt_table(boxes_per_img_host, gt_count_host, batch->B, gt, G);
    if (rc != BXI_OK) return rc;
    if (G > kBoxCap) return BXI_ERR_UNSUPPORTED;           // the evaluation then computes its targets itself (no BXI_EVAL_TARGETS_READY)
    const int h = batch->Hc / stride, w = batch->Wc / stride;
    if (h > 65535 || w > 65535) return BXI_ERR_BAD_SHAPE;
    const HostPred pr = host_pred(color_thresh);
    if (pr.zero_bit) return BXI_ERR_UNSUPPORTED;           // every pair weighs 1: nothing of the image is needed ahead
    const size_t need = carve(nullptr, batch->B, 0, h, w, nullptr);
    if (!workspace_ok(workspace, workspace_bytes, need, 256)) return BXI_ERR_WORKSPACE;
    Ws ws;
    carve(workspace, batch->B, ws_capacity(batch->B, h, w, 0, workspace_bytes), h, w, &ws);
    ws.ws_n16 = (unsigned int)(workspace_bytes / 16);
    ValidCells vc = {};
    valid_cells_of(pa, batch->B, stride, h, w, vc);
    const int64_t n_items64 = (int64_t)batch->B * h * ((w + 63) / 64);
    if (n_items64 > 0x7fffffffLL) return BXI_ERR_BAD_SHAPE;
    const int n_items = (int)n_items64;
    const unsigned int key = targets_key(pa, batch->B, batch->Hc, batch->Wc, stride, dil, pr.n2max, gt.first);
    const bool pooled_in_launch = pool_vec_ok(batch, stride);
    const int n_pool = pooled_in_launch ? pool_wgs(n_items, 7 * device_cus(), 0) : 0;      // (seven workgroups per CU: targets_pool_kernel)
    BXI_LAUNCH("targets_pool", s, targets_pool_kernel, dim3((unsigned)(1 + n_pool)), dim3(256), kPoolLds, s, pa, n_pool, n_items, gt, batch->Hc, batch->Wc, stride, h, w,
               ws, key);
    rc = check_launch();
    if (rc != BXI_OK) return rc;
    if (!pooled_in_launch) {       // other strides / unaligned canvases: the generic pooling kernels, then the repacking into 16-byte records
        rc = launch_pool(batch, stride, nullptr, ws.lab_planar, s);
        if (rc != BXI_OK) return rc;
        const int64_t BP = (int64_t)batch->B * h * w;
        BXI_LAUNCH("pack_lab4", s, pack_lab4_kernel, dim3((unsigned)((BP + 255) / 256 > 2048 ? 2048 : (BP + 255) / 256)), dim3(256), 0, s,
                   (const float*)ws.lab_planar, ws.lab4, (const unsigned int*)ws.epoch, batch->B, (int64_t)h * w);
        rc = check_launch();
        if (rc != BXI_OK) return rc;
    }
    const int n_pb = pred_wgs(n_items, 8 * device_cus());
    BXI_LAUNCH("targets_pred", s, targets_pred_kernel, dim3((unsigned)n_pb), dim3(256), 0, s, h, w, G, vc, ws, dil, pr.n2max, n_pb, n_items);
    return check_launch();
}

// ---- the single launch: whether an evaluation is ONE eval1_kernel launch, and its grid ------------------------------------------------
// A function of the shape, the flags and the stream alone; launch_fused_eval launches what it says and bxi_dev_eval1_plan reports it.
struct Eval1Plan {
    int taken;               // the evaluation is one eval1_kernel launch
    int long_form;           // 8-row tiles, three workgroups per CU, pool workgroups first
    int merge;               // the stream workgroups stay on as the first tile workgroups
    int table_last;          // the table is written from the instances' last bands (eval1_kernel: the stream role's hook)
    int n_tabw, n_stream, n_pool, n_pb, n_tb;      // workgroups per role
    unsigned grid;
    size_t lds;
};
// eligible: no head-fused first launch, the image pooled in the launch, a colour threshold above 0
static Eval1Plan plan_eval1(int N, int h, int w, int n_items, int dil, int R, int64_t cap, unsigned flags, bool ready, bool eligible, hipStream_t s) {
    Eval1Plan p = {};
    const int n_tab = ((N + 64) / 64 + kWaves - 1) / kWaves;
    const int Sn = (h + kSBlk - 1) / kSBlk;
    const int n_stream = N * Sn;
    const size_t lds_stream = std::max(kPoolLds, 8 * (size_t)kWaves * w);
    auto lds_pair_of = [&](int kern) { return std::max((size_t)kWaves * tile_wave_lds(dil, R, kern), 2 * sizeof(float) * (size_t)(h + w) + 16); };
    const bool whole_device = stream_cus(s, device_cus()) >= device_cus();                      // a CU-masked stream has fewer
    // The single launch pays off while its front half (stream + pool workgroups) is resident at once: measured 24.8 vs 27.0 us at
    // 64 instances, 35.1 vs 33.9 at 96, 45.1 vs 39.4 at 128 (200 x 256 maps) -- hence: stream workgroups <= half the slots.
    const int one_slots = kOneOcc * device_cus();
    const bool one_fits = 2 * (int64_t)n_stream <= one_slots && whole_device;
    // (built for dilation <= 2: the single launch needs four workgroups per CU, and at dilation 3 the tile role does not fit 128 VGPRs)
    // Two shapes of the single launch: the SHORT form (4-row tiles, four workgroups per CU, the stream workgroups staying on as the first tile
    // workgroups) while its front half is resident at once; the LONG form (8-row tiles, three per CU, pool workgroups first, nobody waits for a
    // later workgroup) for many instances, where the short form's tile waves would each walk several tiles one after the other.
    // The long form only with the targets ready: with the image side in the launch, three workgroups per CU slow the front half down by what
    // the kernel boundary costs.  So the library takes it where it is asked to (BXI_EVAL_SINGLE_LAUNCH with 8-row tiles) and, with the targets
    // ready, from kLongFrom on: 21.6 against 23.9 us for two launches (R6-14)
    const bool long_form = R == 8 && dil <= 2 && ready && ((flags & kFlagSingle) || (N >= kLongFrom && whole_device && !(flags & kFlagShared)));
    // (targets ready: the short single launch while its stream workgroups are a quarter of the slots -- 14.1 vs 14.4-14.9 us for two launches at 32
    // instances; at 64 two launches take 18.3 against 18.7 us: R6-14)
    const bool short_ok = one_fits && !(ready && 4 * (int64_t)n_stream > one_slots);
    p.lds = std::max(lds_stream, lds_pair_of(ready ? kTilesOneReady : kTilesOne));
    p.long_form = long_form ? 1 : 0;
    p.n_stream = n_stream;
    p.taken = !(flags & kFlagTwo) && (short_ok || (flags & kFlagSingle) || long_form) && eligible && (R == 4 || long_form) && dil <= 2 &&
              p.lds <= 36 * 1024;                                         // (four workgroups per CU must fit)
    if (!p.taken) return p;
    const int slots = long_form ? kLongOcc * device_cus() : one_slots;
    // the front half (table, stream, pool) should fill the GPU exactly once: a pool workgroup takes several items (never more than two in
    // the long form, as in the first launch of the two-launch form)
    const int front = slots - n_stream;
    p.n_pool = ready ? 0 : pool_wgs(n_items, front > slots / 4 ? front : slots / 4, long_form ? 2 : 0);
    p.n_pb = ready ? 0 : pred_wgs(n_items, slots / 2);
    // One tile per wave while the slots last: a wave that walks two tiles runs two ~7 us dependent chains one after the other.  The tile
    // workgroups are the LAST workgroups of the grid and wait only for earlier ones, so nothing else depends on their number.
    p.n_tb = tile_wgs(cap, slots);
    // the stream workgroups stay on as the first tile workgroups (only while they leave half of the slots to the rest of the grid)
    // ... unless evaluations run on SEVERAL streams at once: each would hold its stream workgroups' slots while waiting, and three
    // or four of them leave no room for anybody's pool workgroups (measured: 2.4 ms per evaluation with four streams in flight,
    // against 10 us without the staying-on).  The library cannot see what else runs on the device and does not guess: the CALLER
    // says so (BXI_EVAL_SHARED_DEVICE; boxinstseg_amd/functional.py sets it once a second stream has been
    // seen on the device).  A launch that is being captured into a graph may be replayed next to anything: no staying-on either.
    // ... and only while they are at most a QUARTER of the slots: at 64 instances (448 of 1024) the staying-on costs 0.3 us (21.65 vs 21.35 us, their
    // slots are what the pool workgroups -- three items each then -- are short of); at 32 instances it is worth 0.05 us (R6-12)
    p.merge = !long_form && one_fits && 4 * n_stream <= slots && !(flags & kFlagShared) && !stream_is_capturing(s) ? 1 : 0;
    if (p.merge) p.n_tb = p.n_tb > n_stream ? p.n_tb - n_stream : 0;
    // The table from the instances' last bands: where the stream workgroups stay on -- every one of them then holds a slot from the start
    // (4 n_stream <= slots), so a staying wave that polls the table never holds the slot its writer needs -- and the last band of an
    // instance leaves its last wave without rows.  The image side in the launch only (with the targets ready the table has workgroups
    // of its own).
    p.table_last = p.merge && !ready && h - (Sn - 1) * kSBlk <= (kWaves - 1) * kSRows ? 1 : 0;
    p.n_tabw = ready ? n_tab : 0;
    p.grid = (unsigned)(p.n_tabw + n_stream + p.n_pool + p.n_pb + 1 + N + p.n_tb + 1);
    return p;
}

static int eval_tile_rows(unsigned flags, int N, int dil) { return (flags & kFlagRows8) ? 8 : ((flags & kFlagRows4) ? 4 : tile_rows_for(N, dil)); }
static int64_t eval_items(int B, int h, int w) { return (int64_t)B * h * ((w + 63) / 64); }      // one item = a pooled row segment of 64 pixels

// bxi_dev_eval1_plan (developer query, tests): the plan of an evaluation of N instance maps [h, w] over B images whose image side is
// pooled in the launch (stride 4, aligned rows), colour threshold above 0, no head -- from the functions the launch itself asks.
// out[8]: taken, merge, table_last, n_stream, n_pool, n_pb, n_tb, grid
int eval1_plan_query(int B, int N, int h, int w, int dil, unsigned flags, void* stream, int* out) {
    if (!out) return BXI_ERR_NULL_POINTER;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (N == 0) return BXI_OK;                 // no instances: the evaluation writes two zeros, none of these kernels runs
    if (B <= 0 || B > BXI_MAX_IMAGES || N < 0 || N >= kMaxInst || h <= 0 || w <= 0 || h > 65535 || w > 65535) return BXI_ERR_BAD_SHAPE;
    if (!fused_eval_supported(dil)) return BXI_ERR_UNSUPPORTED;
    const int R = eval_tile_rows(flags, N, dil);
    const int64_t cap = eval_cap(N, h, w, dil, R);
    const int64_t n_items64 = eval_items(B, h, w);
    if (cap >= (1 << 24) || n_items64 > 0x7fffffffLL) return BXI_ERR_BAD_SHAPE;
    const Eval1Plan p = plan_eval1(N, h, w, (int)n_items64, dil, R, cap, flags, (flags & kFlagTargetsReady) != 0, true, as_stream(stream));
    const int v[8] = {p.taken, p.merge, p.table_last, p.n_stream, p.n_pool, p.n_pb, p.n_tb, (int)p.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return BXI_OK;
}

// One evaluation: one launch (eval1) or two (prep, pair).
int launch_fused_eval(const bxi_image_batch* batch, float color_thresh, const bxi_instances* in, int dil, float warmup, const float* up_prj,
                 const float* up_pw, float* losses, float* g_logits, void* state, void* workspace, size_t workspace_bytes, unsigned flags,
                 void* stream, const DynArgs* head, int head_C) {
    InstArgs a;
    int rc = fill_inst(in, a);
    if (rc != BXI_OK) return rc;
    if (!fused_eval_supported(dil)) return BXI_ERR_UNSUPPORTED;
    if (!losses || !batch) return BXI_ERR_NULL_POINTER;
    hipStream_t s = as_stream(stream);
    PoolArgs pa = {};
    if (batch->Hc != in->Hc || batch->Wc != in->Wc || batch->B != in->B) return BXI_ERR_BAD_SHAPE;
    // the image side is in the workspace (bxi_boxinst_targets_f32): `imgs` is not read.  (The kernels get the number of GT boxes + 1.)
    const int ready = (flags & kFlagTargetsReady) ? a.gt.first[a.gt.B] + 1 : 0;
    rc = fill_pool_args(batch, nullptr, nullptr, pa);
    if (rc != BXI_OK) return rc;
    if (batch->B > 0 && !batch->imgs && !ready) return BXI_ERR_NULL_POINTER;
    if (batch->image_masks) return BXI_ERR_UNSUPPORTED;   // explicit masks: use bxi_color_affinity_f32 + bits
    if (warmup < 0.f && !in->iter_counter) return BXI_ERR_NULL_POINTER;     // the factor is to come from the device counter
    if (!(warmup == warmup)) return BXI_ERR_BAD_ARGUMENT;
    if (a.N == 0) {
        BXI_LAUNCH("zero_losses", s, zero_losses2_kernel, dim3(1), dim3(1), 0, s, losses, in->iter_counter);
        return check_launch();
    }
    if (a.N >= kMaxInst || a.h > 65535 || a.w > 65535) return BXI_ERR_BAD_SHAPE;
    if (batch->B <= 0) return BXI_ERR_BAD_SHAPE;
    if (g_logits && !state) return BXI_ERR_NULL_POINTER;
    const bool pooled_in_launch = ready || pool_vec_ok(batch, a.stride);     // else: the generic pooling kernels in launches of their own
    const size_t need = carve(nullptr, batch->B, a.N, a.h, a.w, nullptr);
    if (!workspace_ok(workspace, workspace_bytes, need, 256)) return BXI_ERR_WORKSPACE;
    // The layout is a function of (B, h, w) and of the workspace's SIZE, not of this call's instance count: the per-instance regions are
    // carved for the largest count the size admits, so every evaluation of this canvas on this workspace finds every kind of record at
    // the same address, whatever N it has.  A word that ever held a tag then only ever holds tags of the same kind (or the zero of the
    // one-time initialisation), and tags grow monotonically -- a stale word can never pass for a fresh one.  (With the layout moving
    // with N, a small tag could meet an old PAYLOAD word of the same value -- a predicate word is 16 * tag + bits -- found by
    // tools/extended_fuzz.py: intermittent wrong results, status 0.)
    Ws ws;
    carve(workspace, batch->B, ws_capacity(batch->B, a.h, a.w, a.N, workspace_bytes), a.h, a.w, &ws);
    ws.ws_n16 = (unsigned int)(workspace_bytes / 16);
    ws.pred_any = (ready ? 1u : 0u);
    LossState st = {};
    if (state) {
        if (!aligned(state, 256)) return BXI_ERR_WORKSPACE;
        carve_state(state, a.N, a.h, a.w, &st);
    }
    st.iter = in->iter_counter;
    // bit 0: 16-byte rows; bit 1: the logit stream is read non-temporally -- where the maps outgrow the L2 anyway (128 instances: 52 MB) the
    // stream's lines only push the Lab / predicate / table lines out of it: 37.4 -> 34.3 us per evaluation at 128 instances; at 32 (6.5 MB, which
    // the tile waves find in the L2 again) the hint costs 0.4 us.  profiles/NOTES.md R6-7
    const int nt_stream = (int64_t)a.N * a.h * a.w * 4 >= ((int64_t)kNtStreamFromMB << 20) ? 2 : 0;
    const int vec = (((a.w & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0 &&
                      (!g_logits || (reinterpret_cast<uintptr_t>(g_logits) & 15) == 0)) ? 1 : 0) | nt_stream;
    const int R = eval_tile_rows(flags, a.N, dil);
    const int64_t cap = eval_cap(a.N, a.h, a.w, dil, R);
    if (cap >= (1 << 24)) return BXI_ERR_BAD_SHAPE;     // the table packs a tile prefix into 24 bits
    const HostPred pr = host_pred(color_thresh);
    if (ready && pr.zero_bit) return BXI_ERR_UNSUPPORTED;       // (bxi_boxinst_targets_f32 refuses thresholds <= 0 as well)
    ValidCells vc = {};
    valid_cells_of(pa, batch->B, a.stride, a.h, a.w, vc);
    const int64_t n_items64 = eval_items(batch->B, a.h, a.w);
    if (n_items64 > 0x7fffffffLL) return BXI_ERR_BAD_SHAPE;
    const int n_items = (int)n_items64;
    const int spin_limit = (flags & kFlagGiveUp) ? -1 : kSpinLimit;
    const unsigned int key = ready ? targets_key(pa, batch->B, batch->Hc, batch->Wc, a.stride, dil, pr.n2max, a.gt.first) : 0u;
    // what both forms are made of: table workgroups, stream workgroups (kSBlk rows of one instance map each), and the LDS of the
    // stream / pool workgroups and of the tile waves / leaders
    const int n_tab = ((a.N + 64) / 64 + kWaves - 1) / kWaves;
    const int n_stream = a.N * ((a.h + kSBlk - 1) / kSBlk);
    const size_t lds_stream = std::max(kPoolLds, 8 * (size_t)kWaves * a.w);
    // (the tile waves' share is tile_wave_lds: each kernel parks its pair terms or does not)
    auto lds_pair_of = [&](int kern) { return std::max((size_t)kWaves * tile_wave_lds(dil, R, kern), 2 * sizeof(float) * (size_t)(a.h + a.w) + 16); };
    const size_t lds_pair = lds_pair_of(kTilesPair);
    const int cus = stream_cus(s, device_cus());                      // a CU-masked stream has fewer

    // ---- the single-launch form (plan_eval1 above decides and sizes it) ------------------------------------------------------
    const Eval1Plan pl = plan_eval1(a.N, a.h, a.w, n_items, dil, R, cap, flags, ready != 0, !head && pooled_in_launch && !pr.zero_bit, s);
    if (pl.taken) {
        constexpr decltype(&eval1_kernel<1, 8, true>) eval1_kernels[2][3] = {{eval1_kernel<1, 8, true>, eval1_kernel<1, 4, true>, eval1_kernel<1, 4, false>},
                                                                             {eval1_kernel<2, 8, true>, eval1_kernel<2, 4, true>, eval1_kernel<2, 4, false>}};
        BXI_LAUNCH(ready ? "eval1_ready" : "eval1", s, eval1_kernels[dil - 1][pl.long_form ? 0 : (ready ? 1 : 2)], dim3(pl.grid), dim3(256), pl.lds, s, pa, pl.n_pool, n_items, pl.n_pb, pl.n_tb, a, ws, st, vc, up_prj,
                   up_pw, warmup, pr.n2max, spin_limit, losses, g_logits, vec, pl.merge | (pl.table_last ? 2 : 0), ready, key, pl.n_tabw);
        return check_launch();
    }

    // ---- launch 1 --------------------------------------------------------------------------------------------------
    // one item = the 4 input rows of 64 pooled pixels.  The whole launch should be resident at once (kPrepOcc workgroups per CU at
    // <= 96 VGPRs): a pool workgroup takes several items, the next one's loads in flight, when it is not.
    // ... but never more than two items per pool workgroup: its items are a dependent chain (load -> sums -> Lab -> store, ~2.5 us each), and
    // with many instances -- 896 stream workgroups at 128 -- the few pool workgroups the slots leave would each drag four or five of them
    // behind the HBM stream (the first launch's last 5 us at 128 instances).  Then the launch exceeds the slots and its tail workgroups
    // take them as they come free; the pool workgroups go FIRST in that case, the image side being the longer chain.  Measured: 40.1 ->
    // 38.5 us per evaluation at 128 instances, 75.8 -> 70.3 at 256
    const int prep_slots = kPrepOcc * device_cus();
    const int n_pool = pooled_in_launch && !ready ? pool_wgs(n_items, prep_slots - n_tab - (head ? 0 : n_stream), 2) : 0;
    PrepTail tl = {};
    tl.ready = ready; tl.key = key;
    const int pool_first = !head && n_tab + n_stream + n_pool > prep_slots ? 1 : 0;
    // every refusal comes BEFORE the first launch: a refused call has enqueued nothing (callers fall back to other entry points)
    if (lds_pair > 64 * 1024) return BXI_ERR_UNSUPPORTED;
    if (head && head_C != 8 && head_C != 16) return BXI_ERR_UNSUPPORTED;
    if (head) {
        // the head-fused first launch (factor 2, vector rows): tables, pool blocks, head tiles
        if (head->factor != 2 || !(vec & 1) || head->H * 2 != a.h || head->W * 2 != a.w || head->N != a.N || head->B != in->B || !pooled_in_launch)
            return BXI_ERR_UNSUPPORTED;
        const int tiles = ((head->H + kHeadR - 1) / kHeadR) * ((head->W + kYC - 1) / kYC);
        ws.n_cb = (head->H + kHeadR - 1) / kHeadR;
        ws.n_rp = (head->W + kYC - 1) / kYC;
        const size_t lds_head = std::max(kPoolLds, 8 * 4 * 64 + sizeof(float) * (2 * kHeadR * 64 + 512));
        if (lds_head > 64 * 1024) return BXI_ERR_UNSUPPORTED;
        float* logits_out = const_cast<float*>(a.logits);
        constexpr decltype(&head_prep_kernel<16, true>) head_kernels[2][2] = {{head_prep_kernel<16, true>, head_prep_kernel<16, false>},
                                                                              {head_prep_kernel<8, true>, head_prep_kernel<8, false>}};
        BXI_LAUNCH("head_prep", s, head_kernels[head_C == 8][head->rel ? 0 : 1], dim3((unsigned)(n_tab + n_pool + a.N * tiles)), dim3(256), lds_head, s, pa, n_pool, n_items, a, dil, R, ws,
                   st, g_logits, *head, head->params, logits_out, ready, key);
    } else {
        if (lds_stream > 64 * 1024) return BXI_ERR_UNSUPPORTED;
        BXI_LAUNCH(ready ? "prep_ready" : "prep", s, prep_kernel, dim3((unsigned)(n_tab + n_stream + n_pool)), dim3(256), lds_stream, s, pa, n_pool,
                   n_items, a, dil, R, ws, st, g_logits, vec, pool_first, tl);
    }
    rc = check_launch();
    if (rc != BXI_OK) return rc;
    // From here on a launch of this evaluation is enqueued: records carrying its tag are (or will be) in the workspace while the epoch only
    // moves with the finisher.  An error return below would leave them behind an unchanged epoch -- the next evaluation would draw the same
    // tag and take them for its own -- so the workspace is returned to its initial state (stream-ordered) on that path.
    auto fail = [&](int code) { (void)hipMemsetAsync(workspace, 0, workspace_bytes, s); (void)hipGetLastError(); return code; };
    if (!pooled_in_launch) {
        rc = launch_pool(batch, a.stride, nullptr, ws.lab_planar, s);
        if (rc != BXI_OK) return fail(rc);
        const int64_t BP = (int64_t)batch->B * a.h * a.w;
        BXI_LAUNCH("pack_lab4", s, pack_lab4_kernel, dim3((unsigned)((BP + 255) / 256 > 2048 ? 2048 : (BP + 255) / 256)), dim3(256), 0, s,
                   (const float*)ws.lab_planar, ws.lab4, (const unsigned int*)ws.epoch, batch->B, (int64_t)a.h * a.w);
        rc = check_launch();
        if (rc != BXI_OK) return fail(rc);
    }

    // ---- launch 2 --------------------------------------------------------------------------------------------------
    // the tile list's length is device data: the tile waves stride through it.  The launch should be resident in one round
    // (pair_occ workgroups per CU); the predicate waves are short-lived.
    // (the leaders are short-lived and are not counted; with them subtracted, 512 instances at two workgroups per CU left ONE
    // predicate workgroup for the whole image side: 4.4 ms per evaluation)
    const int slots = pair_occ(dil, R) * cus > 64 ? pair_occ(dil, R) * cus : 64;
    const int n_pb = ready ? 0 : pred_wgs(n_items, slots / 2);   // (targets ready: the image side is in memory at this kernel's start; R6-10)
    // (the predicate workgroups are short-lived: the tile workgroups behind them in the grid take their slots as they leave, so the
    // tile workgroups are sized for the slots, not for what the predicate workgroups leave over)
    const int grid = n_pb + 1 + a.N + tile_wgs(cap, slots) + 1;      // predicate blocks + the reducer + leaders + tile blocks + the finisher
    constexpr decltype(&pair_kernel<1, 4>) pair_kernels[4][2] = {{pair_kernel<1, 4>, pair_kernel<1, 8>}, {pair_kernel<2, 4>, pair_kernel<2, 8>},
                                                                 {pair_kernel<3, 4>, pair_kernel<3, 8>}, {pair_kernel<4, 4>, pair_kernel<4, 8>}};
    BXI_LAUNCH(n_pb > 0 ? "pair" : "pair_tiles", s, pair_kernels[dil - 1][R == 8], dim3((unsigned)grid), dim3(256), lds_pair, s, up_prj, up_pw, warmup,
               pr.n2max, pr.zero_bit, n_pb, n_items, spin_limit, vc, losses, g_logits, a, ws, st);
    rc = check_launch();
    return rc == BXI_OK ? rc : fail(rc);
}

// the same from the three numbers the kernel needs of the instances (the autograd node's backward keeps those, not the structs)
int launch_rescale_nhw(int N, int h, int w, const float* g_prj, const float* g_pw, int dil, const void* state, float* g_logits, void* stream) {
    if (N < 0 || h <= 0 || w <= 0) return BXI_ERR_BAD_SHAPE;
    if (!fused_eval_supported(dil)) return BXI_ERR_UNSUPPORTED;
    if (N == 0) return BXI_OK;
    if (!g_prj || !g_pw || !state || !g_logits) return BXI_ERR_NULL_POINTER;
    if (N > 65535) return BXI_ERR_BAD_SHAPE;
    if (!aligned(state, 256)) return BXI_ERR_WORKSPACE;
    InstArgs a = {};
    a.N = N; a.h = h; a.w = w;
    LossState st = {};
    carve_state(const_cast<void*>(state), N, h, w, &st);
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("rescale", s, rescale_kernel, dim3(8, N), dim3(256), 0, s, a, dil, st, g_prj, g_pw, g_logits);
    return check_launch();
}

int launch_rescale(const bxi_instances* in, const float* g_prj, const float* g_pw, int dil, const void* state, float* g_logits, void* stream) {
    InstArgs a;
    const int rc = fill_inst(in, a);
    return rc != BXI_OK ? rc : launch_rescale_nhw(a.N, a.h, a.w, g_prj, g_pw, dil, state, g_logits, stream);
}

}  // namespace bxi

#ifdef BXI_WAITLOG
extern "C" int bxi_debug_waitlog(unsigned int* out16, int reset) {   // developer builds only
    int rc = (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(bxi::g_waitlog), 16 * sizeof(unsigned int));
    if (rc == 0 && reset) { unsigned int z[16] = {0}; rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(bxi::g_waitlog), z, sizeof(z)); }
    return rc;
}
#endif
#ifdef BXI_TRACE
extern "C" int bxi_debug_set_trace2(void* buf) {   // developer builds only
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(bxi::g_trace), &buf, sizeof(buf));
}
#endif
