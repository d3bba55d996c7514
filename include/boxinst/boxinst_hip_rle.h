/*
 * boxinst_hip_rle.h -- the test-time masks as COCO run-length encodings in libboxinst_hip.so: the final uint8 masks of an image (what
 * bxi_seg_paste_u8, bxi_inst_paste_u8 and bxi_mask_paste_u8 leave on the device) -> the counts of every mask and their compressed string,
 * packed mask after mask, so that tens of kilobytes instead of the mask block cross to the host.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   test.py   = mmdet/apis/test.py         (:65,72,112,119 every image's masks go through encode_mask_results)
 *   utils.py  = mmdet/core/mask/utils.py   (:38-65 encode_mask_results: pycocotools.mask.encode once per mask, on the host)
 *
 * The format is RESTATED from the published algorithm of cocoapi's maskApi.c (rleEncode, rleToString) and UNPINNED: pycocotools never
 * ran next to this library.  tests/rle_ref.py holds the restatement the kernels are tested against, byte for byte.
 *   rleEncode    the mask in column-major order, j = x * h + y; p = 0, c = 0; at every j with M[j] != p: emit c, c = 0, p = M[j]; then
 *                ++c; after the last pixel emit c.  The counts alternate zeros and ones starting with zeros (counts[0] == 0 when pixel
 *                (0,0) is set), an all-zero mask is the single count h * w, and the counts of a mask sum to h * w.
 *   rleToString  for count i: x = counts[i], and for i > 2: x = counts[i] - counts[i-2] (signed); repeat { c = x & 0x1f; x >>= 5
 *                (arithmetic); more = (c & 0x10) ? x != -1 : x != 0; if (more) c |= 0x20; emit c + 48 } while (more).
 * Deviation: any non-zero byte counts as set (the original compares bytes, M[j] != p; every producer here writes 0 / 1, where the two agree).
 */
#ifndef BOXINST_HIP_RLE_H
#define BOXINST_HIP_RLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bits of *status of bxi_mask_rle_u8: which capacity ran out (0 = both sufficed) */
#define BXI_RLE_STATUS_OVER_RUNS 1
#define BXI_RLE_STATUS_OVER_CHARS 2

/* Bytes of `workspace` of bxi_mask_rle_u8 (0 for n == 0, where none is asked for, and for a shape the entry point refuses): the masks as column bit words
 * (8 bytes per mask, column and 64 rows), 16 + 4 bytes per mask and column, 8 bytes per mask, each array rounded up to 16 bytes.  16-byte aligned, contents undefined on
 * entry; the call writes only what it reads back (with `stats`, the words and columns of every mask's box). */
size_t bxi_mask_rle_workspace_bytes(int n, int h, int w);

/* bxi_mask_rle_u8  <->  [mask_util.encode(np.array(m[:, :, None], order='F', dtype='uint8'))[0] for m in masks]   (utils.py:55-61)
 *   FOUR launches whatever n, h and w are (bit words; per-mask scans; the offsets; the emission) -- ONE, the offsets, for n == 0.
 *   No host synchronisation, no memset, no atomics; integer arithmetic in a fixed order: run-to-run bit-identical.
 *   masks [n,h,w] uint8 at ANY byte address; a non-zero byte is a set pixel.
 *   stats [n,5] int32 or NULL: area, x_min, y_min, x_max, y_max of every mask (inclusive), (0,-1,-1,-1,-1) for an empty one -- the
 *   layout of bxi_seg_paste_u8 / bxi_inst_paste_u8.  With stats only rows y_min..y_max of columns x_min..x_max are read (everything
 *   outside is zero by the statistics' contract) and a mask with area <= 0 costs no pixel read; a box that leaves the mask is clamped to
 *   it, so that no statistics make the call read or write out of bounds.  With NULL every pixel is read.
 *   run_offsets [n+1] int32, counts [cap_runs] uint32: the counts of mask i are counts[run_offsets[i] : run_offsets[i+1]].
 *   char_offsets [n+1] int32, chars [cap_chars] uint8: its string is chars[char_offsets[i] : char_offsets[i+1]] (no terminator).
 *   status [1] int32: 0, or BXI_RLE_STATUS_OVER_RUNS | BXI_RLE_STATUS_OVER_CHARS.
 *   Every element of both offset arrays and the status word are written by every call, whatever the capacities: run_offsets[n] and
 *   char_offsets[n] are the TRUE totals.  counts[0 : min(total_runs, cap_runs)] and chars[0 : min(total_chars, cap_chars)] are written
 *   exactly once each and nothing behind them is touched; over capacity the status says which one ran out and the bytes in front of
 *   the capacity are still right.  counts / chars may be NULL for a capacity of 0.
 * Checked before anything touches a device, in this order: n < 0, h < 1, w < 1 or a negative capacity: BXI_ERR_BAD_SHAPE;
 * h * w >= 2^29 (no count then needs more than 6 characters) or n * (h * w + 1) * 6 >= 2^31 (every offset is an int32; encode a larger
 * batch in several calls): BXI_ERR_UNSUPPORTED; a NULL pointer (masks for n > 0, an offset array, status, counts / chars with a non-zero
 * capacity): BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned (n > 0): BXI_ERR_WORKSPACE. */
int bxi_mask_rle_u8(const uint8_t* masks, int n, int h, int w, const int32_t* stats, int cap_runs, int cap_chars, int32_t* run_offsets,
                    uint32_t* counts, int32_t* char_offsets, uint8_t* chars, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
