// eval_back_device.hpp -- the back half of the evaluation: the leader workgroup of an instance (leader_block: maxima -> dice -> unit
// projection gradients), tile_of / locate_tile, dice_round, and the four roles of the second launch as the kernels call them (the
// predicate, reducer, tile and finisher *_role functions).  Assumes the three eval_*_device.hpp headers before it and block_sum4 /
// sigmoid_acc of loss_common.hpp.
#pragma once
#include "eval_tile_device.hpp"

namespace bxi {

// ---- leader workgroup (one per instance) -------------------------------------------------------------------------------
//   partial maxima -> maxima -> sigmoid on those only -> both dice terms (:117-143) -> unit projection gradients, recorded as
//   one 8-byte word per column / row (gradient bits << 32 | arg-max index) for bxi_boxinst_grad_rescale_f32 and ADDED to the
//   gradient at the arg-max positions.  Nobody in this launch reads what a leader writes except the finisher (its dice loss).
template <bool ONE>
__device__ __forceinline__ void leader_block(const InstArgs& a, int dil, Ws ws /* .ep == 0: the first poll fetches the tag */, const LossState& st, int n, float upp,
                                             float* __restrict__ g_logits, unsigned char* smem, float* red, int spin_limit) {
    const int h = a.h, w = a.w, tid = threadIdx.x;
    float* xs = reinterpret_cast<float*>(smem);   // [w] sigmoid of the column maxima, then their unit gradients
    float* ys = xs + w;                           // [h]
    int* carg = reinterpret_cast<int*>(ys + h);   // [w]
    int* rarg = carg + w;                         // [h]
    int4 e;
    bool waited;
    if (ONE) {
        // single-launch form: the instance's partial maxima and the zero-fill of its map come from stream workgroups of THIS
        // launch (earlier in the grid, waiting for nobody); one flag per band says they are in memory.  The table entry and the
        // (first 64) band flags are asked for in ONE round trip -- both are self-announcing words, and by the time a leader gets a
        // slot both are normally there; the partial maxima themselves are only asked for once their flags have been seen.
        const int lane = tid & 63;
        waited = false;
        for (int spins = 0; spins <= spin_limit; ++spins) {
            unsigned int f = lane < ws.n_cb ? __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + lane], BXI_RLX, BXI_AGENT) : 0u;
            u4v v;                                                  // (its wait covers the flag load issued before it)
            if (ws.ep == 0u) {                                      // wave-uniform: the first poll brings the evaluation's tag along (with_tag)
                unsigned int ew;
                v = load16_past_epoch(ws.tab + n, ws.epoch, ew);
                ws.ep = next_tag((unsigned int)__builtin_amdgcn_readfirstlane((int)ew));
            } else
                v = load16_past(ws.tab + n);
            if (lane >= ws.n_cb) f = ws.ep;
            if (__all(f == ws.ep && v.w == ws.ep)) { e = make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w); waited = true; BXI_WL(6, spins); break; }
            __builtin_amdgcn_s_sleep(kSleepLead);
        }
        for (int b0 = 64; b0 < ws.n_cb && waited; b0 += 64) {
            bool got = false;
            for (int spins = 0; spins <= spin_limit; ++spins) {
                const unsigned int f = b0 + lane < ws.n_cb ? __hip_atomic_load(&ws.bandflag[(int64_t)n * ws.n_cb + b0 + lane], BXI_RLX, BXI_AGENT) : ws.ep;
                if (__all(f == ws.ep)) { got = true; BXI_WL(7, spins); break; }
                __builtin_amdgcn_s_sleep(kSleepLead);
            }
            waited = got;
        }
        if (!waited) {        // loud; nothing is computed from partial maxima that may be stale (their indices address the gradient)
            if (tid == 0) __hip_atomic_store(&ws.dice[n], (1ull << 32) | kDiceFault, BXI_RLX, BXI_AGENT);
            return;
        }
    } else {
        waited = tab_entry<false>(ws, n, true, spin_limit, e);
    }
    const int br0 = e.y & 0xffff, br1 = (int)((unsigned int)e.y >> 16), bc0 = e.z & 0xffff, bc1 = (int)((unsigned int)e.z >> 16);
    const bool any = br1 > br0 && bc1 > bc0;
    (void)dil;
    float sums[4] = {0.f, 0.f, 0.f, 0.f};   // I_x, U_x, I_y, U_y
    // the partial maxima of a column / row: up to eight loads in flight at once
    auto best_key = [](const unsigned long long* __restrict__ part, int n_part, int64_t stride) {
        unsigned long long k = 0ull;
        for (int s0 = 0; s0 < n_part; s0 += 8) {
            unsigned long long o[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                o[u] = ONE ? __hip_atomic_load(part + (int64_t)min(s0 + u, n_part - 1) * stride, BXI_RLX, BXI_AGENT) : part[(int64_t)min(s0 + u, n_part - 1) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) k = o[u] > k ? o[u] : k;
        }
        return k;
    };
    for (int i = tid; i < max(w, h); i += 256) {
        const bool is_c = i < w, is_r = i < h;
        // both keys requested before either is used
        const unsigned long long kc = best_key(ws.colpart + (int64_t)n * ws.n_cb * w + (is_c ? i : 0), ws.n_cb, w);
        const unsigned long long kr = best_key(ws.rowkey + (int64_t)n * ws.n_rp * h + (is_r ? i : 0), ws.n_rp, h);
        if (is_c) {
            const int c = i;
            const float X = sigmoid_acc(unpack_val(kc));
            const float TX = (any && c >= bc0 && c < bc1) ? 1.f : 0.f;
            xs[c] = X; carg[c] = (int)unpack_idx(kc);
            sums[0] += X * TX; sums[1] += X * X + TX * TX;
        }
        if (is_r) {
            const int r = i;
            const float Y = sigmoid_acc(unpack_val(kr));
            const float TY = (any && r >= br0 && r < br1) ? 1.f : 0.f;
            ys[r] = Y; rarg[r] = (int)unpack_idx(kr);
            sums[2] += Y * TY; sums[3] += Y * Y + TY * TY;
        }
    }
    BXI_TW(3, 1 + n, 1);
    block_sum4(sums, red);
    const float Ix = sums[0], Ux = sums[1] + 1e-5f, Iy = sums[2], Uy = sums[3] + 1e-5f;
    if (tid == 0)   // :130, summed over both axes :143; the datum is its own flag
        __hip_atomic_store(&ws.dice[n], (1ull << 32) | (unsigned long long)__float_as_uint((1.f - 2.f * Ix / Ux) + (1.f - 2.f * Iy / Uy)),
                           BXI_RLX, BXI_AGENT);
    BXI_TW(3, 1 + n, 2);
    if (g_logits) {
        // dice = 1 - 2I/U ; d dice/d u_j = (-2 t_j U + 4 I u_j) / U^2 ; chain through sigmoid ; mean over N
        const float invN = 1.f / (float)a.N;
        for (int c = tid; c < w; c += 256) {
            const float X = xs[c];
            const float TX = (any && c >= bc0 && c < bc1) ? 1.f : 0.f;
            const float gv = invN * ((-2.f * TX * Ux + 4.f * Ix * X) / (Ux * Ux)) * X * (1.f - X);
            xs[c] = gv;
            st.colk[(int64_t)n * w + c] = ((unsigned long long)__float_as_uint(gv) << 32) | (unsigned int)carg[c];
        }
        for (int r = tid; r < h; r += 256) {
            const float Y = ys[r];
            const float TY = (any && r >= br0 && r < br1) ? 1.f : 0.f;
            const float gv = invN * ((-2.f * TY * Uy + 4.f * Iy * Y) / (Uy * Uy)) * Y * (1.f - Y);
            ys[r] = gv;
            st.rowk[(int64_t)n * h + r] = ((unsigned long long)__float_as_uint(gv) << 32) | (unsigned int)rarg[r];
        }
        lds_barrier();
        // xs / ys now hold the gradients for every thread (LDS only: the record stores above need not have landed)
        // one addition per arg-max position (a pixel that is its column's AND its row's arg-max gets their sum in one)
        float* G = g_logits + (int64_t)n * h * w;
        for (int c = tid; c < w; c += 256) {
            const int r = carg[c];
            float v = xs[c];
            if (rarg[r] == c) v += ys[r];
            add_f32(G + (int64_t)r * w + c, v * upp);
        }
        for (int r = tid; r < h; r += 256) {
            const int c = rarg[r];
            if (carg[c] != r) add_f32(G + (int64_t)r * w + c, ys[r] * upp);
        }
    }
    BXI_TW(3, 1 + n, 3);
}

__device__ __forceinline__ Tile tile_of(const int4& e, const ValidCells& vc, int D, int R, int TW, int n, int idx, int h, int w) {   // e: the instance's table entry (uniform)
    Tile t;
    t.r0 = e.y & 0xffff; t.r1 = (int)((unsigned int)e.y >> 16); t.c0 = e.z & 0xffff; t.c1 = (int)((unsigned int)e.z >> 16);
    t.img = (int)((unsigned int)e.x >> 24); t.n = n;
    t.vrow = vc.vrow[t.img]; t.vcol = vc.vcol[t.img];
    const int dr0 = max(t.r0 - D, 0), hc0 = max(t.c0 - D, 0);
    t.hc1 = min(t.c1 + D, w);
    const int ntc = (t.hc1 - hc0 + TW - 1) / TW;
    const int ti = idx / ntc, tj = idx - ti * ntc;
    t.tile_r0 = (dr0 / R + ti) * R;
    t.tile_c0 = hc0 + tj * TW;
    (void)h;
    return t;
}

// The finisher's rounds.  Leaders: the dice losses of instances [b0, b0 + 64) (self-flagging words).
__device__ __forceinline__ bool dice_round(const Ws& ws, int N, int b0, float* dsum, bool* fault) {
    const int lane = threadIdx.x & 63, i = b0 + lane;
    const unsigned long long dg = i < N ? __hip_atomic_load(&ws.dice[i], BXI_RLX, BXI_AGENT) : (1ull << 32);
    if (!__all((dg >> 32) != 0ull)) return false;
    if (__any((dg & kDiceFault) != 0ull)) *fault = true;
    const float dv = i < N ? __uint_as_float((unsigned int)dg) : 0.f;
    const int m = min(64, N - b0);
    for (int k = 0; k < m; ++k) *dsum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), k));   // index order: run-to-run identical
    return true;
}

// The tile of list position `ti`: the instance whose tile range holds it (table entries: 16 bytes per instance, the same lines
// for every wave), then the tile's place inside the instance's hull.  e0 = this lane's entry of the first 64 (N < 64: all).
template <int D, int R, bool ONE>
__device__ __forceinline__ bool locate_tile(const Ws& ws, const ValidCells& vc, int N, const int4& e0, const int4& e1, int ti, int h, int w, int spin_limit, Tile& out) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    int4 e = make_int4(0, 0, 0, 0);
    if (N < 64) {
        const unsigned long long mask = __ballot(lane < N && (e0.x & 0xffffff) <= ti);
        n = __popcll(mask) - 1;
        e.x = __builtin_amdgcn_readlane(e0.x, n); e.y = __builtin_amdgcn_readlane(e0.y, n);
        e.z = __builtin_amdgcn_readlane(e0.z, n); e.w = __builtin_amdgcn_readlane(e0.w, n);
    } else {
        // (entries 0..63 and 64..127 came with the wave's first round trip -- tile_role --: up to 128 instances the search asks memory for nothing.
        //  Rounds 3-5 loaded chunk after chunk here, two dependent round trips in front of every tile of instances 64.. : the "locate" phase
        //  of a tile wave, 2.0 us at 128 instances)
        for (int m0 = 0; m0 < N; m0 += 64) {
            int4 em = m0 == 0 ? e0 : e1;
            if (m0 >= 128 && !tab_entry<ONE>(ws, m0 + lane, m0 + lane < N, spin_limit, em)) return false;
            const unsigned long long mask = __ballot(m0 + lane < N && (em.x & 0xffffff) <= ti);
            const int cntm = __popcll(mask);
            if (cntm == 0) break;
            n = m0 + cntm - 1;
            e.x = __builtin_amdgcn_readlane(em.x, cntm - 1); e.y = __builtin_amdgcn_readlane(em.y, cntm - 1);
            e.z = __builtin_amdgcn_readlane(em.z, cntm - 1); e.w = __builtin_amdgcn_readlane(em.w, cntm - 1);
            if (cntm < 64) break;
        }
    }
    out = tile_of(e, vc, D, R, TG<D, R>::TW, n, ti - (e.x & 0xffffff), h, w);
    return true;
}

// ---- the roles of the second launch (two-launch form) / of the back half of the single launch ----------------------------------
// predicate workgroup `pblk` of n_pb: 4 independent waves striding through the pooled row segments
template <bool ONE>
__device__ __forceinline__ void pred_role(const InstArgs& a, const ValidCells& vc, Ws ws /* .ep == 0: the first poll fetches the tag */, int D, float n2max, int pblk, int n_pb, int n_items, int spin_limit,
                                          bool high_prio = true) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int segs = (a.w + 63) >> 6, pid = pblk * kWaves + wave;
    BXI_TW(2, pid, 0);
    // short, and the tile waves will ask for these words -- except in the single launch WITHOUT the staying-on (37 .. 73 instances), where the predicate
    // waves mostly wait for Lab records and their priority only takes issue slots from the pool waves they wait for (64 instances: 21.2 -> 21.05 us, R6-27)
    if (high_prio) __builtin_amdgcn_s_setprio(3);
    int cnt = 0, segments = 0;
    bool ok = true;
    for (int item = pid; item < n_items && ok; item += n_pb * kWaves) { cnt += pred_item<ONE>(a.h, a.w, a.N, vc, ws, D, n2max, item, segs, spin_limit, ok); ++segments; }
    // the evaluation whose tag is the last one: the finisher zeroes the workspace behind it (the tag counter starts again), so every store of
    // this evaluation must have landed before its arrival can be seen (the predicate words otherwise announce themselves)
    if (ws.ep == kMaxTag) drain_vmem();
    cnt = wave_total_i32(cnt);
    // ONE arrival per workgroup: arrivals on one word are performed one after the other (~0.15 us each), and the tile waves
    // need the last one
    __shared__ int pred_cnt[kWaves], pred_seg[kWaves], pred_bad[kWaves];
    if (lane == 0) { pred_cnt[wave] = cnt; pred_seg[wave] = segments; pred_bad[wave] = ok ? 0 : 1; }
    // an LDS-only barrier: __syncthreads() would also wait for this wave's predicate-word stores to be acknowledged (~1 us) before the
    // count -- which the tile waves' normaliser hangs on -- could leave; the words announce themselves, nobody infers them from the count
    lds_barrier();
    if (threadIdx.x == 0) {  // (segments evaluated, sum W); integer adds commute: run-to-run identical
        if ((pred_bad[0] | pred_bad[1]) | (pred_bad[2] | pred_bad[3])) {      // loud: on the fault word, ahead of the arrival (a flag bit ADDED to the
            const unsigned int seen = __hip_atomic_fetch_or(ws.fault, kFaultCounts, BXI_RLX, BXI_AGENT);    // arrival carries into its count from the second fault on)
            asm volatile("s_waitcnt vmcnt(0)" ::"v"(seen) : "memory");
        }
        __hip_atomic_fetch_add(&ws.acc1[(size_t)(pblk & (kAcc1Words - 1)) * kAcc2Stride],
                               ((unsigned long long)(unsigned int)((pred_seg[0] + pred_seg[1]) + (pred_seg[2] + pred_seg[3])) << 40) |
                                   (unsigned long long)(unsigned int)((pred_cnt[0] + pred_cnt[1]) + (pred_cnt[2] + pred_cnt[3])),
                               BXI_RLX, BXI_AGENT);
    }
    BXI_TW(2, pid, 1);
}

// the reducer: ONE wave, in a workgroup of its own right behind the predicate workgroups -- EARLIER in the grid than every tile
// workgroup that waits for what it publishes (it used to be a wave of the finisher, the LAST workgroup: on a stream with fewer
// slots than tile workgroups the finisher could not start while the tile waves, holding every slot, waited for it).  It waits
// only for predicate workgroups.  (Single-launch form: the count words are this evaluation's only once the table says so --
// before that they hold the previous evaluation's complete counts.)
template <bool ONE>
__device__ __forceinline__ void reducer_role(const Ws& ws, int zero_bit, int n_items, int spin_limit) {
    if (threadIdx.x >= 64 || zero_bit || n_items <= 0) return;      // n_items <= 0: sum W is already published (an earlier launch, or the table wave)
    if (!(table_complete<ONE>(ws, 0, spin_limit) && reduce_counts(ws, n_items, spin_limit)) && threadIdx.x == 0) atomicOr(ws.fault, kFaultCounts);
}

// the last workgroup: waits only for workgroups that never wait for it -- the leaders and the predicate waves (done early), then
// the tile waves -- and writes the two loss values
template <bool ONE>
__device__ __forceinline__ void finisher_role(const InstArgs& a, const Ws& ws, const LossState& st, float upp, float upw, float warmup, int zero_bit, int n_items,
                                              int spin_limit, int R, int n_tile_waves, float* __restrict__ losses) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int N = a.N;
    // the launch ends on this workgroup's polls and its last few instructions: they go ahead of whatever else the CU holds (128 instances, two or
    // three tile waves on every SIMD: 30.5 -> 29.85 us; 24.9 -> 24.65 with the targets ready; nothing at 32 / 64.  The reducer and the leaders at a
    // higher priority: nothing.  profiles/NOTES.md R6-23)
    __builtin_amdgcn_s_setprio(3);
    BXI_TW(3, 0, 0);
    __shared__ double fin_d[kWaves];
    __shared__ int fin_i[kWaves];
    __shared__ float fin_f;
    __shared__ int fin_ok, fin_flt, fin_b[kWaves];
    bool ok = true, flt0 = false;
    double total_w = 0.0;
    float dsum = 0.f;
    int spins = 0;
    if (spin_limit < 0) ok = false;
    if (wave == 0) {
        if (!table_complete<ONE>(ws, N, spin_limit)) ok = false;      // every polled word of this evaluation is zeroed from here on
        for (int b0 = 0; b0 < N && ok; b0 += 64) {
            while (!dice_round(ws, N, b0, &dsum, &flt0)) {
                if (++spins > spin_limit) { ok = false; break; }
                __builtin_amdgcn_s_sleep(kSleepFin);
            }
        }
        if (zero_bit) total_w = total_weight_all_pairs(a, ws);
        else
            while (ok && !counts_complete(ws, n_items, &total_w, &flt0)) {
                if (++spins > spin_limit) ok = false;
                __builtin_amdgcn_s_sleep(kSleepFin);
            }
        BXI_WL(8, spins);
        if (lane == 0) { fin_f = dsum; fin_d[0] = total_w; fin_ok = ok ? 1 : 0; fin_flt = flt0 ? 1 : 0; }
    }
    __syncthreads();
    ok = fin_ok != 0; dsum = fin_f; total_w = fin_d[0];
    __syncthreads();
    // every thread watches its own arrival words (N * 8 / 256 each: one at the headline size); the launch ends on this loop
    long long mine = 0;
    unsigned int fault_seen = (ok ? 0u : kFaultFinisher) | (fin_flt ? kFaultCounts : 0u);
    spins = 0;
    for (; ok;) {
        mine = 0;
        int arrived = 0;
        bool flt = false;
        // (the words tile waves arrive on: those of instances 0 .. min(N, 64) - 1 -- tile_wave_arrives --, at most two per thread, asked for in one
        // round trip.  Rounds 3-6 walked all N x 8 words with one atomic load each: four dependent trips per poll at 128 instances, two of them for
        // words nobody arrives on.)
        {
            const int n_words = (N < 64 ? N : 64) * kAcc2Split;
            const int i0 = threadIdx.x, i1 = threadIdx.x + 256;
            unsigned long long x0 = 0ull, x1 = 0ull;
            if (n_words > 256) load8_past_x2(ws.acc2 + (size_t)(i0 < n_words ? i0 : 0) * kAcc2Stride, ws.acc2 + (size_t)(i1 < n_words ? i1 : 0) * kAcc2Stride, x0, x1);
            else x0 = __hip_atomic_load(ws.acc2 + (size_t)(i0 < n_words ? i0 : 0) * kAcc2Stride, BXI_RLX, BXI_AGENT);
            if (i0 >= n_words) x0 = 0ull;
            if (i1 >= n_words) x1 = 0ull;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned long long x = k ? x1 : x0;
                arrived += (int)(x >> 52);
                mine += (long long)(x & ((1ull << 52) - 1ull)) - ((long long)(x >> 52) << 24);       // the +1 per tile
                flt |= (x & (3ull << 50)) != 0ull;                                                   // a tile wave's wait ran out
            }
        }
        // the fault word (waves that gave up WITHOUT arriving set it; the finisher then runs out itself) rides in the same round
        if (threadIdx.x == 0) fault_seen |= __hip_atomic_load(ws.fault, BXI_RLX, BXI_AGENT);
        arrived = wave_total_i32(arrived);
        const bool anyflt = __any(flt);
        if (lane == 0) { fin_i[wave] = arrived; fin_b[wave] = anyflt ? 1 : 0; }
        __syncthreads();
        const bool all = (fin_i[0] + fin_i[1]) + (fin_i[2] + fin_i[3]) == n_tile_waves;    // every tile wave arrives once, tiles or not
        if ((fin_b[0] | fin_b[1]) | (fin_b[2] | fin_b[3])) fault_seen |= kFaultCounts;
        __syncthreads();
        if (all) break;
        if (++spins > spin_limit) { ok = false; break; }           // workgroup-uniform: the same count in every thread
    }
    BXI_WL(10, spins);
    // ... and once more past the round that saw the last arrival: the read in that round may have been served before a late wave's fetch_or,
    // which that wave waits for before its arrival (tile_wave_arrives); this read comes after the arrival was seen.  (In flight under the sum below.)
    if (threadIdx.x == 0) fault_seen |= __hip_atomic_load(ws.fault, BXI_RLX, BXI_AGENT);
    const double wsum = wave_total_f64((double)mine);                // exact; fixed order: run-to-run identical
    if (lane == 0) fin_d[wave] = wsum;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const double num = (fin_d[0] + fin_d[1]) + (fin_d[2] + fin_d[3]);
    const unsigned int status = (unsigned int)__builtin_amdgcn_readfirstlane((int)(fault_seen | (ok ? 0u : kFaultFinisher)));
    if (lane == 0) {
        const float denom = fmaxf((float)total_w, 1.f);                      // weights.sum().clamp(min=1.0), :1328
        float l0 = dsum / (float)N;                                          // .mean(), :143
        float l1 = (float)((num / (double)kNumScale) / (double)denom) * warmup;   // :1327-1332
        if (status) { l0 = __int_as_float(0x7fc00000); l1 = l0; }            // loud: mmdet's CheckInvalidLossHook fires
        losses[0] = l0; losses[1] = l1;
        if (st.scale) { st.scale[0] = warmup / denom; st.scale[1] = warmup; st.applied[0] = upp; st.applied[1] = upw; }   // [1]: the warm-up factor applied
        if (st.status) { st.status[0] = (int)status; if (ONE) st.status[1] = R; }
        if (st.iter) atomicAdd(st.iter, 1.0f);                               // self._iter += 1, condinst_head.py:1297
        // the evaluation is over: every other wave of it has been seen to arrive, so nobody reads the epoch any more
        if (ws.ep != kMaxTag) *ws.epoch = ws.ep;      // (a plain store: see with_tag)
    }
    if (ws.ep == kMaxTag) {
        // The tag counter is about to wrap: records of 2^28 evaluations ago would pass for fresh ones (table entries and arrival words of
        // instances beyond the current count keep their tags until an evaluation that large comes again).  So this evaluation ends by
        // returning the workspace to its initial state -- all zero, epoch 0 -- as bxi_boxinst_eval_workspace_init does: every other wave
        // has arrived, and in this evaluation every wave drains its stores before it arrives (pred_role; the others always do) and arrives
        // behind its last read of the workspace (tile waves: after their adds in this evaluation only -- tile_role).
        // Once per 2^28 - 1 evaluations, ~3 MB by one wave.  (Targets an earlier bxi_boxinst_targets_f32 left in the workspace go too:
        // an evaluation that counts on them finds key 0 and says so, loud.)
        uint4* z = reinterpret_cast<uint4*>(ws.epoch);
        const size_t n16 = ws.ws_n16;
        for (size_t i = lane; i < n16; i += 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    BXI_TW(3, 0, 1);
}

// tile workgroup: 4 independent waves striding through the tile list (its length is device data)
template <int D, int R, bool ONE, int KERN>
__device__ __forceinline__ void tile_role(const InstArgs& a, const ValidCells& vc, const Ws& ws, float upw_warm, float n2max, int zero_bit, int n_items, int spin_limit,
                                          float* __restrict__ g_logits, unsigned char* smem, int tblk, int n_tb, const LossState& st, float* __restrict__ losses) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int N = a.N;
    const int wid = tblk * kWaves + wave, nwaves = n_tb * kWaves;
    // (priority 0 like the stream, pool and leader waves.  Rounds 3-6 ran the tile waves at priority 2 -- "the launch ends on the tile waves, not on
    // the leaders next to them" --, and with the targets ready that starved what they themselves wait for: the stream waves whose band flags gate their
    // adds.  At 0: targets ready 14.1 -> 13.7 us at 32 instances, 18.2 -> 17.5 at 64, 21.5 -> 20.9 at 96, 26.0 -> 24.8 at 128; the un-split evaluation
    // 21.5 -> 21.2 at 64, unchanged at 32 / 96 / 128.  Priority 1 loses all of it; the predicate waves' 3 is worth 0.1-0.2 us at 32 instances.  R6-22)
    BXI_TW(1, wid, 0);
    int4 e0, e1 = make_int4(0, 0, 0, 0), eN = make_int4(0, 0, 0, 0);
    bool ok;
    if (ONE && R == 8 && N >= 64) {
        // the long single-launch form (64 instances or more; the short form runs 64..73 instances with the three calls below: see pred_words): entries 0..63, N and 64..127 polled for in ONE round trip (three tab_entry calls are three
        // statements with a wait each: three dependent trips in front of every tile of the long form)
        ok = false;
        const bool want1 = 64 + lane < N;
        for (int spins = 0; spins <= spin_limit; ++spins) {
            u4v v0, vN, v1;
            load16_past_x3(ws.tab + lane, ws.tab + N, ws.tab + (want1 ? 64 + lane : N), v0, vN, v1);
            if (__all(v0.w == ws.ep && vN.w == ws.ep && v1.w == ws.ep)) {
                e0 = make_int4((int)v0.x, (int)v0.y, (int)v0.z, (int)v0.w); eN = make_int4((int)vN.x, (int)vN.y, (int)vN.z, (int)vN.w);
                if (want1) e1 = make_int4((int)v1.x, (int)v1.y, (int)v1.z, (int)v1.w);
                ok = true;
                BXI_WL(1, spins);
                break;
            }
            __builtin_amdgcn_s_sleep(kSleepTab);
        }
    } else {
        ok = tab_entry<ONE>(ws, lane, lane <= N, spin_limit, e0);
        if (N >= 64) ok = ok && tab_entry<ONE>(ws, N, true, spin_limit, eN);
        if (N > 64) ok = ok && tab_entry<ONE>(ws, 64 + lane, 64 + lane < N, spin_limit, e1);      // (with the two above: one round trip in the two-launch form)
    }
    // (a wave whose table wait ran out still arrives, saying so: the finisher then ends at once, loud, instead of running out itself.
    // The table's own zeroing of the arrival words precedes its entries, so without an entry the arrival may be wiped -- then the finisher
    // does run out: as loud)
    if (!ok) { tile_wave_arrives(ws, N, wid, 0, true); return; }
    const int total = N < 64 ? __builtin_amdgcn_readlane(e0.x, N < 64 ? N : 0) : __builtin_amdgcn_readfirstlane(eN.x);
    float* gbuf = reinterpret_cast<float*>(smem + wave * tile_wave_lds(D, R, KERN));
    float scale = 0.f;
    bool have_scale = false, bad = false;
    long long fx_sum = 0;
    // (tiles are dealt wave by wave: the first workgroups' four waves each take one, the last quarter of the workgroups at 128 instances none.
    // Dealt workgroup by workgroup -- three per workgroup, nine per CU instead of twelve or eight -- the launch is SLOWER: 38.4 vs 37.2 us at 128
    // instances, 32.1 vs 31.1 at 96, targets ready 30.3 vs 28.7: the early workgroups' waves start their chains first.  profiles/NOTES.md R6-5)
    // The wave's last tile arrives from inside math_tile, as soon as its share is known (tile_wave_arrives).  Not in the wrap evaluation: there
    // the finisher zeroes the workspace once every tile wave has arrived, so every tile wave arrives behind its last read of the workspace.
    // Single-launch forms only: in the second launch of the two-launch form (128 instances, 8-row tiles) the early arrival measured 0.3-0.4 us
    // SLOWER (30.0 -> 30.4 us; profiles/NOTES.md R6-28), and without it pair_kernel is the code it was.
    const bool may_arrive_early = ONE && ws.ep != kMaxTag;
    bool arrived = false;
    for (int ti = wid; ti < total && !bad; ti += nwaves) {
        Tile t;
        if (!locate_tile<D, R, ONE>(ws, vc, N, e0, e1, ti, a.h, a.w, spin_limit, t)) { bad = true; break; }
        BXI_TW(1, wid, 1);
        const bool last = may_arrive_early && ti + nwaves >= total;
        math_tile<D, R, ONE, KERN>(a, ws, t, upw_warm, n2max, zero_bit, n_items, spin_limit, scale, have_scale, g_logits, gbuf, wid, fx_sum, bad, last, st, losses);
        arrived = last;
    }
    if (!arrived) tile_wave_arrives(ws, N, wid, fx_sum, bad);
    BXI_TW(1, wid, 7);
}

}  // namespace bxi
