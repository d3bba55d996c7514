/*
 * boxinst_hip_post.h -- test-time post-processing of the SOLOv2-style heads (DiscoBox, BoxLevelSet) in libboxinst_hip.so:
 * mask thresholding / area / mask scoring in one pass, and Matrix NMS on bit-packed masks.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device
 * pointers owned by the caller, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative
 * bxi_status).  Paths are relative to the upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   matrix_nms.py       = mmdet/core/post_processing/matrix_nms.py
 *   box_solov2_head.py  = mmdet/models/dense_heads/box_solov2_head.py
 *   discobox_head.py    = mmdet/models/dense_heads/discobox_head.py
 */
#ifndef BOXINST_HIP_POST_H
#define BOXINST_HIP_POST_H

#include <stddef.h>
#include <stdint.h>

#include "../boxinst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_NMS_MAX_CANDIDATES 2048   /* n of bxi_matrix_nms_f32: decay_iou is at most 16 MB */
#define BXI_NMS_KERNEL_GAUSSIAN 0
#define BXI_NMS_KERNEL_LINEAR 1

/* bxi_mask_pack_f32  <->  `seg_masks = seg_preds > cfg.mask_thr; sum_masks = seg_masks.sum((1, 2))` and the numerator of
 *     `seg_scores = (seg_preds * seg_masks.float()).sum((1, 2)) / sum_masks`
 *     (box_solov2_head.py:547-548,561, discobox_head.py:1611-1612,1626), one pass over the probabilities.
 *   probs [n_all,h,w] fp32, any 4-byte aligned address; the test is p > mask_thr in fp32 (ATen rounds the Python scalar to
 *   fp32 the same way).
 *   bits  [n_all, ceil(h*w/64)] 64-bit words.  The position of a pixel inside its candidate's words is private to the library
 *         (the same for every candidate of one h*w); every word is written and bits beyond h*w are zero.
 *   area  [n_all] int32 = number of set pixels;  psum [n_all] fp32 = sum of p over the set pixels, reduced in a fixed order
 *         (four partials per lane, wave, workgroup: run-to-run identical).
 * n_all == 0 is a no-op.  h*w >= 2^24 (fp32 counts stop being exact): BXI_ERR_BAD_SHAPE. */
int bxi_mask_pack_f32(const float* probs, int n_all, int h, int w, float mask_thr, uint64_t* bits, int32_t* area, float* psum,
                      void* stream);

/* bxi_mask_pack_u8  <->  `masks.sum((1, 2))` and the `masks.reshape(num_masks, -1)` operand of matrix_nms.py:48,65 for masks the
 * caller already holds: masks [n_all,h,w] uint8 / bool at any byte address, non-zero = set.  bits and area as above. */
int bxi_mask_pack_u8(const uint8_t* masks, int n_all, int h, int w, uint64_t* bits, int32_t* area, void* stream);

/* Bytes of `workspace` of bxi_matrix_nms_f32 for n candidates (0 when n is outside 1..BXI_NMS_MAX_CANDIDATES):
 * compensate [n] fp32 first, then the per-tile-row column maxima.  Contents undefined on entry. */
size_t bxi_matrix_nms_workspace_bytes(int n);

/* bxi_matrix_nms_f32  <->  mask_matrix_nms, matrix_nms.py:60-99: from `masks[sort_inds]` to `scores * decay_coefficient`.
 *   bits, area [n_all]  from bxi_mask_pack_* at the same h, w;  labels [n_all] int64;
 *   order [n] int64     indices into the n_all candidates, by descending score and cut to nms_pre (rows are fetched through it;
 *                       an index outside [0, n_all) is treated as an empty mask of its own label);
 *   scores_sorted [n]   the scores in that order.
 *   decay_iou [n,n]     for i < j with labels equal: inter / (area_i + area_j - inter) in fp32 on the integers converted to fp32,
 *                       inter = sum of popcount(bits_i & bits_j) -- bit-equal to the reference's fp32 matrix product and division
 *                       (:67-72,85); every other entry 0.  0 / 0 is NaN, as there.
 *   workspace           compensate[j] = max_i decay_iou[i][j] (:80) in its first n floats.  Second pass over per-tile-row
 *                       maxima, no atomics: deterministic.
 *   decayed [n]         scores_sorted[j] * min over i of the decay ratio (:88-99), kernel 0 'gaussian':
 *                       exp(-sigma d_ij^2) / exp(-sigma c_i^2), 1 'linear': (1 - d_ij) / (1 - c_i), with expf.  The minimum is
 *                       taken over i < j with equal labels and 1 (every other entry of the reference's matrix is >= 1 or +inf);
 *                       a NaN ratio, or any NaN compensate, gives NaN as torch.min does.
 * 1 <= n <= BXI_NMS_MAX_CANDIDATES else BXI_ERR_UNSUPPORTED; n_all < 1, h*w outside 1..2^24-1: BXI_ERR_BAD_SHAPE; another kernel
 * or a NaN sigma: BXI_ERR_BAD_ARGUMENT; workspace NULL / too small / not 4-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_matrix_nms_f32(const uint64_t* bits, const int32_t* area, const int64_t* labels, const int64_t* order,
                       const float* scores_sorted, int n_all, int n, int h, int w, int kernel, float sigma, float* decayed,
                       float* decay_iou, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
