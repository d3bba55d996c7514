// mask_rle.hip -- the test-time masks as COCO run-length encodings on gfx950 (include/boxinst/boxinst_hip_rle.h): the uint8 masks
// [n,h,w] the paste kernels leave on the device become, packed mask after mask, the counts of cocoapi's rleEncode and the characters of
// its rleToString, in FOUR launches whatever n, h and w are.  The format is restated in the header (unpinned: pycocotools never ran here).
//
// A count is the distance between two neighbouring TRANSITIONS of the mask read in column-major order (j = x * h + y): the positions
// P[0] < P[1] < ... < P[m-1] with M[j] != M[j-1] (M[-1] = 0).  With P[-1] = 0 and P[m] = h * w the m + 1 counts are P[r] - P[r-1], and the
// string codes counts[r] - counts[r-2] for r > 2: everything about rank r follows from the positions of ranks r-3 .. r.  So no array of
// positions exists (its size would be the capacity's, and the offsets have to be complete when the capacity is not): the bit words and
// a record per column answer "where is the transition of rank r" whenever somebody asks.
//
// rle_bits_kernel     one wave = one mask x 64 columns x 64 rows; a lane owns a column: it reads one byte of every row (the wave a 64-byte
//   row segment) and stores the column's 64 rows as one word, bit y & 63, into the workspace as [n][ceil(h/64)][w] (coalesced for the
//   lanes here and for the column owners below).  With stats only the words and columns of the mask's box are read and written;
//   everybody who reads a word takes an unwritten one as zero (RleMask::word), so the workspace needs no zero-fill.
// rle_scan_kernel     one workgroup of 1024 threads per mask, a thread owns a column: the transitions of a word are word ^ (word << 1 | carry),
//   the carry being the pixel above -- the last pixel of the column before for the first row.  Exclusive scan over the columns -> per
//   column the rank of its first transition and the positions of its last three (RleArgs::col).  Then every column with transitions
//   takes the three positions in front of its first one from the records to its left (rle_prev3: the column before, or a search),
//   walks its own transitions and adds up their string lengths; a second scan -> the column's first character (col_cbase) and the
//   mask's totals.  What these kernels wait for is dependent loads, not bytes: hence the records, the wide workgroup and kRleGroup.
// rle_offsets_kernel  one workgroup: the scans of the masks' totals -> run_offsets, char_offsets (the TRUE totals in [n]) and the status.
// rle_emit_kernel     the walk again, this time storing: every count and every character exactly once, none at or behind its capacity.
// Integer arithmetic, no atomics, nobody waits for anybody: run-to-run bit-identical.
#include "common.hpp"

#include "../../include/boxinst/boxinst_hip_rle.h"

namespace bxi {

constexpr int kRleThreads = 256;
constexpr int kRleScanThreads = 1024;           // the per-mask kernels: a thread owns a column, so 1024 columns go through one round of dependent loads
typedef unsigned long long u64;

struct RleArgs {
    const uint8_t* masks;
    const int32_t* stats;
    u64* bits;                                      // workspace: [n][hw64][w]
    int4* col;                                      // workspace: [n][w] rank of the column's first transition, positions of its last three
    int* col_cbase;                                 // workspace: [n][w] the column's first character inside its mask's string
    int2* mask_tot;                                 // workspace: [n] counts, characters
    int32_t* run_offsets;
    uint32_t* counts;
    int32_t* char_offsets;
    uint8_t* chars;
    int32_t* status;
    int n, h, w, hw64, tiles, cap_runs, cap_chars;
};

// One mask as the scans see it: the words that were written (columns x0..x1, word rows k0..k1; x0 > x1: none) and where a transition can
// be (columns cx0..cx1, word rows kk0..kk1: one column and one word further, where a run that touches the box's edge ends, and from
// word row 0 on when the box holds the last row: such a run ends at the top of the next column).
struct RleMask {
    const u64* bits;
    int h, w, hw64;
    int x0, x1, y0, y1, k0, k1;
    int cx0, cx1, kk0, kk1;

    __device__ __forceinline__ u64 word(int x, int k) const {
        return (x >= x0 && x <= x1 && k >= k0 && k <= k1) ? bits[(size_t)k * w + x] : 0ull;
    }
    // the transitions of rows 64 k .. 64 k + 63 of column x, bit y & 63
    __device__ __forceinline__ u64 trans(int x, int k) const {
        const u64 wd = word(x, k);
        const u64 carry = k > 0 ? word(x, k - 1) >> 63 : (x > 0 ? (word(x - 1, hw64 - 1) >> ((h - 1) & 63)) & 1ull : 0ull);
        u64 t = wd ^ ((wd << 1) | carry);
        const int rows = h - 64 * k;
        if (rows < 64) t &= (1ull << rows) - 1ull;
        return t;
    }
    __device__ __forceinline__ uint32_t pos(int x, int k, int b) const { return (uint32_t)x * (uint32_t)h + (uint32_t)(64 * k + b); }
};

__device__ __forceinline__ RleMask rle_mask(const RleArgs& a, int i) {
    RleMask m;
    m.bits = a.bits + (size_t)i * a.hw64 * a.w;
    m.h = a.h; m.w = a.w; m.hw64 = a.hw64;
    bool any = true;
    m.x0 = 0; m.y0 = 0; m.x1 = a.w - 1; m.y1 = a.h - 1;
    if (a.stats) {
        const int32_t* s = a.stats + 5 * (size_t)i;
        m.x0 = max(s[1], 0); m.y0 = max(s[2], 0);
        m.x1 = min(s[3], a.w - 1); m.y1 = min(s[4], a.h - 1);                 // clamped: no statistics lead out of the mask
        any = s[0] > 0 && m.x0 <= m.x1 && m.y0 <= m.y1;
    }
    if (!any) { m.x0 = 0; m.x1 = -1; m.y0 = 0; m.y1 = -1; }
    m.k0 = m.y0 >> 6; m.k1 = any ? m.y1 >> 6 : -1;
    m.cx0 = m.x0; m.cx1 = any ? min(m.x1 + 1, a.w - 1) : -1;
    m.kk0 = m.y1 == a.h - 1 ? 0 : m.k0;                                       // a run through the last row ends in row 0 of the next column
    m.kk1 = any ? min(m.k1 + 1, a.hw64 - 1) : -1;
    return m;
}

__global__ void __launch_bounds__(kRleThreads) rle_bits_kernel(const RleArgs a) {
    const long long gw = (long long)blockIdx.x * (kRleThreads / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long per_mask = (long long)a.tiles * a.hw64;
    if (gw >= per_mask * a.n) return;
    const int i = (int)(gw / per_mask);
    const int rest = (int)(gw - (long long)i * per_mask);
    const int k = rest / a.tiles, tile = rest - k * a.tiles;
    const RleMask m = rle_mask(a, i);
    if (k < m.k0 || k > m.k1 || 64 * tile > m.x1 || 64 * tile + 63 < m.x0) return;          // also the empty mask: k1 = x1 = -1
    const int x = 64 * tile + lane;
    if (x < m.x0 || x > m.x1) return;
    const int ya = max(64 * k, m.y0), yb = min(64 * k + 63, m.y1);                          // inside the mask: y1 <= h - 1, x <= x1 <= w - 1
    const uint8_t* p = a.masks + ((size_t)i * a.h + ya) * a.w + x;
    u64 word = 0;
#pragma unroll 8
    for (int y = ya; y <= yb; ++y, p += a.w) word |= (u64)(*p != 0) << (y & 63);
    a.bits[((size_t)i * a.hw64 + k) * a.w + x] = word;
}

// What the scan leaves per column (RleArgs::col): x = the rank of the column's first transition, y / z / w = the positions of its last,
// second-to-last and third-to-last transition (as many as it has).
//
// The positions of the transitions of ranks R-1, R-2, R-3 of a mask, looked for in columns cx0..xhi (which hold every rank < R and
// nothing else); 0 where the rank is negative: P[-1] = 0, and nothing reads further back than a rank that exists.  Every round ends
// one column further left, so the loop ends whatever the records hold.
__device__ __forceinline__ void rle_prev3(const int4* col, int cx0, int R, int xhi, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    uint32_t f1 = 0, f2 = 0, f3 = 0;                                          // found so far: ranks R-1, R-2, R-3
    int got = 0, hi = xhi;
    while (got < 3 && R - 1 - got >= 0 && hi >= cx0) {
        const int target = R - 1 - got;
        // the largest x in [cx0, hi] with col[x].x <= target (col[cx0].x = 0): the column itself inside a blob, so look there first, then
        // at distances 1, 2, 4, ... and halve the bracket that leaves -- a dependent load each, which is what these kernels wait for
        int lo = hi;
        int4 c = col[hi];
        if (c.x > target) {
            int up = hi - 1;
            lo = cx0;
            for (int s = 1; hi - s > cx0; s <<= 1) {
                if (col[hi - s].x <= target) { lo = hi - s; break; }
                up = hi - s - 1;
            }
            while (lo < up) {
                const int mid = (lo + up + 1) >> 1;
                if (col[mid].x <= target) lo = mid; else up = mid - 1;
            }
            c = col[lo];
        }
        const int have = target - c.x + 1;                                    // the column holds ranks c.x .. target
        // the column's last transitions c.y, c.z, c.w (as many as `have`) are the next ones: shift them in behind what was found
        if (got == 0) { f1 = (uint32_t)c.y; f2 = (uint32_t)c.z; f3 = (uint32_t)c.w; }
        else if (got == 1) { f2 = (uint32_t)c.y; f3 = (uint32_t)c.z; }
        else { f3 = (uint32_t)c.y; }
        got += have < 1 ? 0 : have;                                           // values behind `got` are overwritten or unused
        hi = lo - 1;
    }
    p1 = got >= 1 ? f1 : 0;
    p2 = got >= 2 ? f2 : 0;
    p3 = got >= 3 ? f3 : 0;
}

// rleToString of one value: its length, and with EMIT its characters at chars[at ...] as far as they lie in front of the capacity
template <bool EMIT>
__device__ __forceinline__ int rle_chars(int x, uint8_t* chars, int at, int cap) {
    int len = 0;
    bool more;
    do {
        int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (EMIT && at + len < cap) chars[at + len] = (uint8_t)(c + 48);
        ++len;
    } while (more);
    return len;
}

// The words of a column are loaded kRleGroup at a time before any of them is walked: the walks branch on what they find, and a load
// behind such a branch waits for it.
constexpr int kRleGroup = 4;

// Column x for the scan: the number of its transitions and the positions of the last three (q1 the last)
__device__ __forceinline__ int rle_column(const RleMask& m, int x, uint32_t& q1, uint32_t& q2, uint32_t& q3) {
    int c = 0;
    q1 = q2 = q3 = 0;
    for (int k0 = m.kk0; k0 <= m.kk1; k0 += kRleGroup) {
        u64 t[kRleGroup];
#pragma unroll
        for (int j = 0; j < kRleGroup; ++j) t[j] = k0 + j <= m.kk1 ? m.trans(x, k0 + j) : 0ull;
#pragma unroll
        for (int j = 0; j < kRleGroup; ++j) {
            u64 r = t[j];
            if (!r) continue;
            c += __popcll(r);
            uint32_t n1 = 0, n2 = 0, n3 = 0;                                  // the word's highest transitions
            int nn = 0;
            while (r && nn < 3) {
                const int b = 63 - __clzll((long long)r);
                r &= ~(1ull << b);
                const uint32_t p = m.pos(x, k0 + j, b);
                if (nn == 0) n1 = p; else if (nn == 1) n2 = p; else n3 = p;
                ++nn;
            }
            if (nn == 1) { q3 = q2; q2 = q1; q1 = n1; }
            else if (nn == 2) { q3 = q1; q2 = n2; q1 = n1; }
            else { q1 = n1; q2 = n2; q3 = n3; }
        }
    }
    return c;
}

// The transitions of column x, whose first one has rank R: the counts that END at them and their characters.  Returns the characters.
template <bool EMIT>
__device__ __forceinline__ int rle_walk(const RleMask& m, const RleArgs& a, const int4* col, int x, int R, int run_off, int char_at) {
    uint32_t p1, p2, p3;
    rle_prev3(col, m.cx0, R, x - 1, p1, p2, p3);
    int r = R, len = 0;
    for (int k0 = m.kk0; k0 <= m.kk1; k0 += kRleGroup) {
        u64 t[kRleGroup];
#pragma unroll
        for (int j = 0; j < kRleGroup; ++j) t[j] = k0 + j <= m.kk1 ? m.trans(x, k0 + j) : 0ull;
#pragma unroll
        for (int j = 0; j < kRleGroup; ++j) {
            u64 tj = t[j];
            while (tj) {
                const int b = __ffsll((long long)tj) - 1;
                tj &= tj - 1;
                const uint32_t p = m.pos(x, k0 + j, b);
                const uint32_t cnt = p - p1;
                const int d = r > 2 ? (int)cnt - (int)(p2 - p3) : (int)cnt;
                if (EMIT && run_off + r < a.cap_runs) a.counts[run_off + r] = cnt;
                len += rle_chars<EMIT>(d, a.chars, char_at + len, a.cap_chars);
                p3 = p2; p2 = p1; p1 = p;
                ++r;
            }
        }
    }
    return len;
}

// The last count of a mask with mt transitions, h * w - P[mt-1]: the count and the value the string codes for it
__device__ __forceinline__ void rle_last(const RleMask& m, const int4* col, int mt, uint32_t& cnt, int& d) {
    uint32_t p1, p2, p3;
    rle_prev3(col, m.cx0, mt, m.cx1, p1, p2, p3);
    cnt = (uint32_t)m.h * (uint32_t)m.w - p1;
    d = mt > 2 ? (int)cnt - (int)(p2 - p3) : (int)cnt;
}

__global__ void __launch_bounds__(kRleScanThreads) rle_scan_kernel(const RleArgs a) {
    __shared__ int part[kRleScanThreads / kWave];
    const int i = blockIdx.x;
    const RleMask m = rle_mask(a, i);
    int4* col = a.col + (size_t)i * a.w;
    int* cbase = a.col_cbase + (size_t)i * a.w;
    int mt = 0;
    for (int xb = m.cx0; xb <= m.cx1; xb += kRleScanThreads) {
        const int x = xb + (int)threadIdx.x;
        uint32_t q1 = 0, q2 = 0, q3 = 0;
        const int c = x <= m.cx1 ? rle_column(m, x, q1, q2, q3) : 0;
        int total;
        const int ex = block_scan_excl_i32<kRleScanThreads / kWave>(c, part, total);
        if (x <= m.cx1) col[x] = make_int4(mt + ex, (int)q1, (int)q2, (int)q3);
        mt += total;
    }
    __syncthreads();                                                          // the workgroup's own column records, complete
    int ct = 0;
    for (int xb = m.cx0; xb <= m.cx1; xb += kRleScanThreads) {
        const int x = xb + (int)threadIdx.x;
        int len = 0;
        if (x <= m.cx1) {
            const int R = col[x].x;
            if ((x < m.cx1 ? col[x + 1].x : mt) > R) len = rle_walk<false>(m, a, col, x, R, 0, 0);
        }
        int total;
        const int ex = block_scan_excl_i32<kRleScanThreads / kWave>(len, part, total);
        if (x <= m.cx1) cbase[x] = ct + ex;
        ct += total;
    }
    if (threadIdx.x == 0) {
        uint32_t cnt;
        int d;
        rle_last(m, col, mt, cnt, d);
        a.mask_tot[i] = make_int2(mt + 1, ct + rle_chars<false>(d, nullptr, 0, 0));
    }
}

__global__ void __launch_bounds__(kRleThreads) rle_offsets_kernel(const RleArgs a) {
    __shared__ int part[kRleThreads / kWave];
    int runs = 0, chars = 0;
    for (int ib = 0; ib < a.n; ib += kRleThreads) {
        const int i = ib + (int)threadIdx.x;
        const int2 t = i < a.n ? a.mask_tot[i] : make_int2(0, 0);
        int tr, tc;
        const int er = block_scan_excl_i32<kRleThreads / kWave>(t.x, part, tr);
        const int ec = block_scan_excl_i32<kRleThreads / kWave>(t.y, part, tc);
        if (i < a.n) {
            a.run_offsets[i] = runs + er;
            a.char_offsets[i] = chars + ec;
        }
        runs += tr; chars += tc;
    }
    if (threadIdx.x == 0) {
        a.run_offsets[a.n] = runs;
        a.char_offsets[a.n] = chars;
        a.status[0] = (runs > a.cap_runs ? BXI_RLE_STATUS_OVER_RUNS : 0) | (chars > a.cap_chars ? BXI_RLE_STATUS_OVER_CHARS : 0);
    }
}

__global__ void __launch_bounds__(kRleScanThreads) rle_emit_kernel(const RleArgs a) {
    const int i = blockIdx.x;
    const RleMask m = rle_mask(a, i);
    const int4* col = a.col + (size_t)i * a.w;
    const int* cbase = a.col_cbase + (size_t)i * a.w;
    const int run_off = a.run_offsets[i], char_off = a.char_offsets[i];
    const int2 tot = a.mask_tot[i];
    const int mt = tot.x - 1;
    for (int x = m.cx0 + (int)threadIdx.x; x <= m.cx1; x += kRleScanThreads) {
        const int R = col[x].x;
        if ((x < m.cx1 ? col[x + 1].x : mt) > R) rle_walk<true>(m, a, col, x, R, run_off, char_off + cbase[x]);
    }
    if (threadIdx.x == 0) {
        uint32_t cnt;
        int d;
        rle_last(m, col, mt, cnt, d);
        if (run_off + mt < a.cap_runs) a.counts[run_off + mt] = cnt;
        const int len = rle_chars<false>(d, nullptr, 0, 0);
        rle_chars<true>(d, a.chars, char_off + tot.y - len, a.cap_chars);
    }
}

// shapes the entry point and the size query accept: BXI_OK, or the status the entry point refuses them with
static int rle_shape_status(int n, int h, int w) {
    if (n < 0 || h < 1 || w < 1) return BXI_ERR_BAD_SHAPE;
    const int64_t hw = (int64_t)h * w;
    if (hw >= ((int64_t)1 << 29)) return BXI_ERR_UNSUPPORTED;
    if ((int64_t)n * (hw + 1) * 6 > 0x7fffffffLL) return BXI_ERR_UNSUPPORTED;
    return BXI_OK;
}

static size_t rle_carve(void* ws, int n, int h, int w, RleArgs* a) {
    Carver c(ws, 16);
    const size_t hw64 = (size_t)(h + 63) / 64;
    u64* bits = c.take<u64>((size_t)n * hw64 * (size_t)w);
    int4* col = c.take<int4>((size_t)n * (size_t)w);
    int* col_cbase = c.take<int>((size_t)n * (size_t)w);
    int2* mask_tot = c.take<int2>((size_t)n);
    if (a) { a->bits = bits; a->col = col; a->col_cbase = col_cbase; a->mask_tot = mask_tot; }
    return c.bytes();
}

}  // namespace bxi

extern "C" size_t bxi_mask_rle_workspace_bytes(int n, int h, int w) {
    using namespace bxi;
    if (rle_shape_status(n, h, w) != BXI_OK) return 0;
    return rle_carve(nullptr, n, h, w, nullptr);
}

extern "C" int bxi_mask_rle_u8(const uint8_t* masks, int n, int h, int w, const int32_t* stats, int cap_runs, int cap_chars,
                               int32_t* run_offsets, uint32_t* counts, int32_t* char_offsets, uint8_t* chars, int32_t* status,
                               void* workspace, size_t workspace_bytes, void* stream) {
    using namespace bxi;
    if (n < 0 || h < 1 || w < 1 || cap_runs < 0 || cap_chars < 0) return BXI_ERR_BAD_SHAPE;
    const int rc_shape = rle_shape_status(n, h, w);
    if (rc_shape != BXI_OK) return rc_shape;
    if ((n > 0 && !masks) || !run_offsets || !char_offsets || !status || (cap_runs > 0 && !counts) || (cap_chars > 0 && !chars))
        return BXI_ERR_NULL_POINTER;
    if (n > 0 && !workspace_ok(workspace, workspace_bytes, bxi_mask_rle_workspace_bytes(n, h, w), 16)) return BXI_ERR_WORKSPACE;
    RleArgs a;
    rle_carve(workspace, n, h, w, &a);
    a.masks = masks; a.stats = stats;
    a.run_offsets = run_offsets; a.counts = counts; a.char_offsets = char_offsets; a.chars = chars; a.status = status;
    a.n = n; a.h = h; a.w = w; a.hw64 = (h + 63) / 64; a.tiles = (w + 63) / 64;
    a.cap_runs = cap_runs; a.cap_chars = cap_chars;
    hipStream_t s = as_stream(stream);
    int rc;
    if (n > 0) {
        const int64_t waves = (int64_t)n * a.tiles * a.hw64;                  // <= n * h * w: far inside the 32-bit work-item count
        const unsigned grid = (unsigned)((waves + kRleThreads / kWave - 1) / (kRleThreads / kWave));
        BXI_LAUNCH("rle_bits", s, rle_bits_kernel, dim3(grid), dim3(kRleThreads), 0, s, a);
        if ((rc = check_launch()) != BXI_OK) return rc;
        BXI_LAUNCH("rle_scan", s, rle_scan_kernel, dim3((unsigned)n), dim3(kRleScanThreads), 0, s, a);
        if ((rc = check_launch()) != BXI_OK) return rc;
    }
    BXI_LAUNCH("rle_offsets", s, rle_offsets_kernel, dim3(1), dim3(kRleThreads), 0, s, a);
    if ((rc = check_launch()) != BXI_OK) return rc;
    if (n > 0) {
        BXI_LAUNCH("rle_emit", s, rle_emit_kernel, dim3((unsigned)n), dim3(kRleScanThreads), 0, s, a);
        if ((rc = check_launch()) != BXI_OK) return rc;
    }
    return BXI_OK;
}
