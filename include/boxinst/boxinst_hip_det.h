/*
 * boxinst_hip_det.h -- CondInst's test-time detections in libboxinst_hip.so: the decode of the FCOS-style box head for every FPN
 * level and image, the score filter, and greedy box NMS, with one host synchronisation (the caller's, to read the counts) at the
 * very end.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device
 * pointers owned by the caller, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative
 * bxi_status; where a failure depends on data a per-segment `status` word on the device says so).  Paths are relative to the
 * upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   condinst_head.py     = mmdet/models/dense_heads/condinst_head.py   (nms_with_others :18-83, get_bboxes / _get_bboxes :640-853)
 *   transforms.py        = mmdet/core/bbox/transforms.py               (distance2bbox :136-186)
 *   point_generator.py   = mmdet/core/anchor/point_generator.py        (MlvlPointGenerator :119-176)
 * and `mmcv.ops.nms.nms / batched_nms`, which the reference calls and whose source is not part of it (restated, unpinned).
 *
 * Locations.  The maps of one FPN level are NCHW as get_bboxes receives them.  A location's point is
 * ((x + 0.5) * stride, (y + 0.5) * stride) (point_generator.py:152-159; exact in fp32, so no points tensor is read).  The locations
 * of all levels are numbered level-major, then y, then x: M_all = sum of H * W.  This is the order of the reference's concatenation.
 *
 * Two deviations from mmcv's NMS, both documented in INTEGRATION.md ("Level 3d"):
 *  (a) the threshold test is the multiplication form  inter > iou_thr * (Sa + Sb - inter)  in fp32, as mmcv's device kernel is
 *      remembered to have it; a division form differs only where an IoU is within a few fp32 roundings of the threshold;
 *  (b) mmcv makes NMS class-aware by ADDING label * (max coordinate + 1) to the boxes in fp32, which rounds the coordinates;
 *      here the labels are compared and the IoU is computed on the original coordinates.  The two agree wherever the offset boxes
 *      are exact in fp32 and the boxes are well formed (x1 <= x2, y1 <= y2, which the FCOS decode guarantees).  With an inverted box
 *      (negative area) mmcv lets a box of another class "suppress"; that case is not matched.
 */
#ifndef BOXINST_HIP_DET_H
#define BOXINST_HIP_DET_H

#include <stddef.h>
#include <stdint.h>

#include "../boxinst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_DET_MAX_LEVELS 8
#define BXI_DET_SORT_MAX 16384        /* count of a segment the library sorts by itself: 16384 64-bit keys are 128 KiB of LDS */
#define BXI_DET_NMS_ROUND 256         /* candidates one round of the NMS kernel takes (4 waves of 64) */
#define BXI_DET_KEEP_TILE 2048        /* kept boxes the NMS kernel holds in LDS; the rest of max_keep lives in the workspace */
#define BXI_DET_ROW_TILE 64           /* rows of `sel` per workgroup of bxi_det_candidates_f32 */
#define BXI_DET_STATUS_OVER_CAP 1     /* status word of bxi_box_nms_f32: count[p] > cap (or negative) */
#define BXI_DET_STATUS_OVER_SORT 2    /* order == NULL and count[p] > BXI_DET_SORT_MAX */
#define BXI_DET_STATUS_BAD_ORDER 4    /* an entry of the caller's order was outside [0, count[p]) and has been skipped */

/* The NCHW maps of one FPN level: cls [B,C,H,W] logits, bbox [B,4,H,W] distances l,t,r,b in pixels, ctr [B,1,H,W] logits,
 * params [B,P,H,W] (NULL where an entry point does not read it). */
typedef struct { const float *cls, *bbox, *ctr, *params; int H, W, stride; } bxi_det_level;

/* bxi_det_location_score_f32  <->  `(scores * centerness[..., None]).max(-1)` (condinst_head.py:781) for every level and image in
 *     one launch, computed as sigmoid(max_c cls) * sigmoid(ctr): fp32 multiplication by a positive number is monotone, and so is the
 *     sigmoid.  A NaN logit wins the maximum, as in torch.max.  The per-level top-k stays with the caller (torch.topk on slices).
 *   levels_host [n_levels] is a HOST array, passed to the kernel by value;  loc_score [B, M_all] fp32.
 * B == 0 is a no-op; n_levels outside 1..BXI_DET_MAX_LEVELS, B < 0 or > BXI_MAX_IMAGES, C < 1, a level with H, W or stride < 1 or
 * M_all * C >= 2^31: BXI_ERR_BAD_SHAPE. */
int bxi_det_location_score_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, float* loc_score, void* stream);

/* Bytes of `workspace` of bxi_det_candidates_f32 for B images of M rows (0 for a bad shape): int32 [B][ceil(M / BXI_DET_ROW_TILE)]
 * candidate counts per row tile, every word written by the first launch before the second reads it. */
size_t bxi_det_candidates_workspace_bytes(int B, int M);

/* bxi_det_candidates_f32  <->  distance2bbox with the clamp to img_shape (condinst_head.py:796, transforms.py:153-184), the division
 *     by scale_factor when `rescale` (:808-810) and the filter of nms_with_others (:25-62): the test sigmoid(cls) > score_thr on the
 *     class score BEFORE centerness, the candidate score sigmoid(cls) * sigmoid(ctr).  Two launches (count, then write).
 *   sel [B,M] int64 indices into M_all (the concatenated per-level top-k), NULL: every location in order (M is ignored, M_all taken).
 *     An index outside [0, M_all) is a row without candidates.
 *   img_dims_host [B][6] fp32 HOST array, by value: clamp_h, clamp_w (img_shape), then the four scale factors (w, h, w, h).
 *   Boxes are bit-equal to the reference: each coordinate is one fp32 subtraction or addition, `x < 0 ? 0 : x`, `x > max ? max : x`
 *   (a NaN passes, as through torch.where) and a correctly rounded division.
 *   Candidates of image b are written in the order of the reference's `nonzero`: ascending (row m of sel, class c);
 *   cand_boxes [B,cap,4], cand_scores [B,cap], cand_labels [B,cap] int64 = c, cand_pos [B,cap] int32 = m.  count [B] int32 is the
 *   TRUE number of candidates, also beyond cap; only the first min(count, cap) rows are written, the others are left as they were.
 * B == 0 is a no-op; shapes as above, M < 0, cap < 0 or M * C >= 2^31: BXI_ERR_BAD_SHAPE; a NaN score_thr: BXI_ERR_BAD_ARGUMENT;
 * workspace NULL / too small / not 4-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_det_candidates_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, const int64_t* sel, int M,
                           const float* img_dims_host, int rescale, float score_thr, int cap, float* cand_boxes, float* cand_scores,
                           int64_t* cand_labels, int32_t* cand_pos, int32_t* count, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Bytes of `workspace` of bxi_box_nms_f32 (0 for a bad shape).  Layout, 32-bit words: order [P][cap] (written and read only when the
 * library sorts), then [P][max(min(max_keep, cap) - BXI_DET_KEEP_TILE, 0)][6] kept boxes that do not fit in LDS.  Contents undefined on entry;
 * words the call does not need are not written. */
size_t bxi_box_nms_workspace_bytes(int P, int cap, int max_keep);

/* bxi_box_nms_f32  <->  mmcv.ops.nms.nms / batched_nms: greedy box NMS of P segments in one launch (two when the library sorts).
 *   Segment p holds count[p] boxes at a fixed stride: boxes [P,cap,4] x1,y1,x2,y2, scores [P,cap], labels [P,cap] int64 (NULL:
 *   class-agnostic), count [P] int32 ON THE DEVICE (bxi_det_candidates_f32 writes it; no synchronisation in between).
 *   Order of processing: descending score, ties by ascending index within the segment (what a stable sort gives; torch's device sort
 *   and mmcv leave ties open), NaN scores first (where torch.sort(descending=True) puts them), -0 equal to +0.
 *     order == NULL: the library sorts, in LDS; needs count[p] <= BXI_DET_SORT_MAX.
 *     order [P,cap] int32: the indices by the rule above, from the caller; any count[p] <= cap.
 *   Greedy rule: in that order a box is kept unless a box kept earlier, of the same label, has
 *       inter > iou_thr * (Sa + Sb - inter),   inter = max(min(x2) - max(x1) + offset, 0) * max(min(y2) - max(y1) + offset, 0),
 *       S = (x2 - x1 + offset) * (y2 - y1 + offset),   offset 0 or 1,
 *   every operation a single fp32 operation on the ORIGINAL coordinates (deviations (a) and (b) above).
 *   max_keep = max_num when max_num > 0, else cap -- also where max_num > cap: max_keep is the row stride of `keep`, and the value to
 *   pass to bxi_box_nms_workspace_bytes and bxi_det_gather_f32.  NMS stops at max_keep kept boxes (a segment keeps at most count[p]).
 *   keep [P,max_keep] int32: indices into the segment in score order, -1 from n_keep[p] on;  n_keep [P] int32.
 *   status [P] int32, every word written: 0, or BXI_DET_STATUS_OVER_CAP / _OVER_SORT -- then n_keep[p] = -1 and nothing of the segment
 *   is kept --, or BXI_DET_STATUS_BAD_ORDER.
 *   One workgroup per segment, nothing accumulated atomically, no workgroup waits for another: run-to-run identical.
 * P == 0 is a no-op; P < 0 or > 65535, cap < 1, P * cap * 4 >= 2^31 or P * max_keep >= 2^31: BXI_ERR_BAD_SHAPE; offset not 0 or 1, a NaN iou_thr:
 * BXI_ERR_BAD_ARGUMENT; workspace NULL / too small / not 4-byte aligned (when bxi_box_nms_workspace_bytes is not 0 and it is needed):
 * BXI_ERR_WORKSPACE. */
int bxi_box_nms_f32(const float* boxes, const float* scores, const int64_t* labels, const int32_t* count, const int32_t* order, int P,
                    int cap, float iou_thr, int offset, int max_num, int32_t* keep, int32_t* n_keep, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);

/* bxi_det_gather_f32  <->  `dets[:max_num]`, `labels[keep]` and `item[positions][keep]` of the others (condinst_head.py:72-83): the kept
 *     detections' params, points and level indices are fetched straight from the NCHW maps, at most max_keep rows per image.
 *   n_params = channels of the levels' params maps (0: det_params is not written); sel / M as in bxi_det_candidates_f32;
 *   cand_* [B,cap,...], keep [B,max_keep], n_keep [B] as the two entry points above wrote them (n_keep < 0 counts as 0).
 *   dets [B,max_keep,5] x1,y1,x2,y2,score;  det_labels [B,max_keep] int64;  det_params [B,max_keep,n_params];
 *   det_coors [B,max_keep,2] the point (x, y);  det_level_inds [B,max_keep] int64.  Rows at and beyond n_keep[b] are zeros.
 * B == 0 or max_keep == 0 is a no-op. */
int bxi_det_gather_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, int n_params, const int64_t* sel, int M,
                       const float* cand_boxes, const float* cand_scores, const int64_t* cand_labels, const int32_t* cand_pos, int cap,
                       const int32_t* keep, const int32_t* n_keep, int max_keep, float* dets, int64_t* det_labels, float* det_params,
                       float* det_coors, int64_t* det_level_inds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
