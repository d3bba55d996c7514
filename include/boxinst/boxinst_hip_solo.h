/*
 * boxinst_hip_solo.h -- the step between a batch and the loss kernels of the two SOLOv2-style heads in libboxinst_hip.so: the mask
 * pass (exact moments and rescaled masks of every ground-truth mask), the grid-cell assignment of every image and level, and the
 * category (sigmoid focal) loss with its finished gradient.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h and
 * boxinst_hip_fcos.h (device pointers owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable,
 * BXI_OK or a negative bxi_status; where a failure depends on data a `status` word on the device says so).  Paths are relative to
 * the upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   discobox_head.py    = mmdet/models/dense_heads/discobox_head.py   (center_of_mass :522-532, loss :1143-1360,
 *                                                                      solov2_target_single :1442-1529)
 *   box_solov2_head.py  = mmdet/models/dense_heads/box_solov2_head.py (loss :262-388, solo_target_single :390-472)
 *   focal_loss.py, utils.py as in boxinst_hip_fcos.h (py_sigmoid_focal_loss restated; mmcv's device op is not part of the reference).
 * Neither OpenCV nor mmcv is part of the reference: `mmcv.imrescale` is RESTATED here from OpenCV's documented fixed-point bilinear
 * resize and is UNPINNED -- no fixture made by OpenCV itself stands behind it (see bxi_solo_mask_pass_u8).
 *
 * Flatten order of the per-cell outputs: the training order of boxinst_hip_fcos.h with H_l = W_l = S_l (the level's num_grid):
 * level-major, then image, then y, then x.  N_cells = B * sum_l S_l^2; cell (l, b, y, x) is row  B * first_l + b * S_l^2 + y * S_l + x
 * with first_l = sum_{k<l} S_k^2.  Instances are numbered globally: image b owns gt_offsets[b] .. gt_offsets[b+1]-1.
 *
 * Deviations from the reference: (1) the rescale rule is restated, unpinned; (2) the centre of mass comes from the EXACT integer
 * moments, rounded once (the reference's fp32 sums are exact below 2^24 and depend on torch's summation order above); (3) an image
 * without boxes is all background (the reference indexes gt_labels_raw[0] and raises).
 */
#ifndef BOXINST_HIP_SOLO_H
#define BOXINST_HIP_SOLO_H

#include <stddef.h>
#include <stdint.h>

#include "boxinst_hip_fcos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_SOLO_MODE_DISCOBOX 0         /* DiscoBoxSOLOv2Head.solov2_target_single: torch fp32 centre, valid = m00 > 0 */
#define BXI_SOLO_MODE_BOXLEVELSET 1      /* BoxSOLOv2Head.solo_target_single: float64 centre (scipy), valid = m00 >= 10 */
#define BXI_SOLO_MAX_FACTORS 4           /* distinct rescale factors of one mask pass */
#define BXI_SOLO_MAX_FACTOR 64
#define BXI_SOLO_RESCALE_MIN_ONES 2      /* THE threshold of the restated rescale rule: ones among the four sampled pixels for a 1 */
#define BXI_SOLO_MIN_MASK_SUM 10         /* box_solov2_head.py:439: `if seg_mask.sum() < 10: continue` */
#define BXI_SOLO_MAX_GRID 64             /* largest num_grid (the configs use 12..40) */
#define BXI_SOLO_PAIRS_PER_INSTANCE 9    /* the +-1 window: at most 3 x 3 cells per instance and level */
#define BXI_SOLO_STATUS_BAD_LABEL 1      /* status word of bxi_solo_assign_f32: a gt label outside [0, num_classes) */

/* bxi_solo_mask_pass_u8: ONE launch over the mask bytes of the whole batch (and one memset node for `moments`).
 *   masks_host [B]: DEVICE pointers to the uint8 masks [G_b, H_b, W_b] of image b (values 0 / 1; a non-zero byte counts as 1), each
 *   image with its own padded size img_h_host[b] x img_w_host[b]; any byte alignment.  gt_offsets_host [B+1] as in bxi_fcos_targets_f32.
 *   The arrays are HOST arrays passed to the kernel by value.  A pointer may be NULL where G_b = 0.
 *   moments [G,3] int64: m00 = sum m, m10 = sum x m, m01 = sum y m -- exact integers (workgroup partials in 64-bit integers, combined
 *   with integer atomics: exact and order-free, run-to-run identical).  8-byte aligned.
 *   rescaled_host [n_factors]: DEVICE pointers to uint8 [G, out_h[k], out_w[k]], the masks rescaled by 1 / factors_host[k].  EVERY
 *   byte is written: everything outside [:H_b/f, :W_b/f] is zero (the reference's `cur_ins_label[:h', :w'] = seg_mask`).
 *   RESCALE RULE (restates mmcv.imrescale(mask, 1/f) = cv2.resize(INTER_LINEAR) on uint8; UNPINNED): for an even factor f the sample
 *   point of output pixel (r, c) lies exactly between source rows f r + f/2 - 1, f r + f/2 and the same two columns, weight 1/2 each;
 *   the output is 1 where at least BXI_SOLO_RESCALE_MIN_ONES of those four pixels are 1 (OpenCV's fixed point rounds exactly 0.5 up).
 *   The bytes are read as 16-byte vectors between a byte-wise head and tail, so a mask may start at any address.
 * n_factors may be 0 (moments only).  B == 0 or G == 0 is a no-op.
 * B < 0 or > BXI_MAX_IMAGES, gt_offsets not starting at 0 or decreasing, an image with masks whose H or W < 1 or H * W >= 2^31, an
 * output plane smaller than H_b/f x W_b/f: BXI_ERR_BAD_SHAPE.  n_factors > BXI_SOLO_MAX_FACTORS, a factor that is odd, < 2,
 * > BXI_SOLO_MAX_FACTOR or does not divide the largest one, H_b or W_b not a multiple of the largest factor: BXI_ERR_UNSUPPORTED. */
int bxi_solo_mask_pass_u8(const uint8_t* const* masks_host, const int* gt_offsets_host, const int* img_h_host, const int* img_w_host, int B,
                          const int* factors_host, const int* out_h_host, const int* out_w_host, int n_factors,
                          uint8_t* const* rescaled_host, int64_t* moments, void* stream);

/* bxi_solo_assign_f32  <->  solov2_target_single (mode 0) / solo_target_single (mode 1) of all images and levels: ONE launch, one
 *   workgroup per (level, image), and one memset node each for num_ins and status.
 *   num_grids_host [n_levels], scale_ranges_host [n_levels][2] fp32, gt_offsets_host [B+1]: HOST arrays.  sigma: the config's double
 *   (used as (float)sigma, what `tensor * self.sigma` does).  canvas_h / canvas_w: upsampled_size = 4 x the mask feature size
 *   (mode 1: 4 x featmap_sizes[0]).  gt_boxes [G,4] fp32, gt_labels [G] int64, moments [G,3] int64 as the mask pass wrote them.
 *   Mirrored operation by operation, never contracted: gt_areas = sqrt((x2-x1) * (y2-y1)) (correctly rounded), both range ends
 *   inclusive (a box may hit two levels); half = (0.5 * (x2-x1)) * (float)sigma; the centre is fp32(m10) / fp32(m00) with valid =
 *   m00 > 0 (mode 0), or double(m10) / double(m00) with valid = m00 >= BXI_SOLO_MIN_MASK_SUM (mode 1);
 *   FLOOR DIVISION: `(v / upsampled) // (1. / S)` is the fmod-based floor division of torch (fp32, divisor (float)(1.0 / S)) and of
 *   Python (double) -- fmod, (a - mod) / b, the sign fix, floor and the 0.5 correction -- and NOT floor(v * S): the centre's cell is
 *   fp32 in mode 0 and double in mode 1; the four window edges are fp32 in both (in mode 1 `center - half` is a NumPy double minus an
 *   fp32 tensor, which torch evaluates in fp32 on the centre rounded to fp32).  Then max(0, .), min(S-1, .), the +-1 window, and an
 *   empty window (top > down or left > right) writes nothing.
 *   Outputs, every element written:
 *     cate_labels [N_cells] int64 (num_classes = background);  ins_ind_labels [N_cells] uint8 0/1;
 *     cell_owner [N_cells] int32: the global index of the LAST instance, in the reference's loop order, that wrote the cell, or -1;
 *     sel_inst [N_cells] int32: per (level, image), at the offset of its cells, the owners of its set cells in ascending cell order
 *       (the planes `ins_label[ins_ind_label]` selects in mode 1), then -1;
 *     pair_cell, pair_inst [9 * n_levels * G] int32: the reference's grid_order of (level l, image b) and the instance of each entry,
 *       at offset 9 * (l * G + gt_offsets[b]): instance order within hit_indices, then i, then j (a cell may appear twice); then -1;
 *     counts [n_levels * B][2] int32: pairs and set cells of (level, image);  num_ins [1] int32: set cells in all;
 *     status [1] int32: 0 or BXI_SOLO_STATUS_BAD_LABEL -- such an instance is skipped.
 * B == 0 is a no-op.  n_levels outside 1..BXI_DET_MAX_LEVELS, B out of range, a num_grid outside 1..BXI_SOLO_MAX_GRID, num_classes
 * < 1, canvas < 1, bad gt_offsets, 9 * n_levels * G >= 2^31: BXI_ERR_BAD_SHAPE; NaN range or sigma, unknown mode: BXI_ERR_BAD_ARGUMENT. */
int bxi_solo_assign_f32(int mode, int B, int n_levels, const int* num_grids_host, const float* scale_ranges_host, double sigma,
                        int num_classes, int canvas_h, int canvas_w, const float* gt_boxes, const int64_t* gt_labels,
                        const int64_t* moments, const int* gt_offsets_host, int64_t* cate_labels, uint8_t* ins_ind_labels,
                        int32_t* cell_owner, int32_t* sel_inst, int32_t* pair_cell, int32_t* pair_inst, int32_t* counts, int32_t* num_ins,
                        int32_t* status, void* stream);

/* Bytes of `workspace` of bxi_solo_cate_loss_f32 (0 for a bad shape): one fp64 partial (two 32-bit words) per workgroup. */
size_t bxi_solo_cate_workspace_bytes(const int* num_grids_host, int n_levels, int B, int C);

/* bxi_solo_cate_loss_f32  <->  loss_cate (discobox_head.py:1341-1355, box_solov2_head.py:366-381): the sigmoid focal loss of every
 *   level's [B,C,S,S] category map where it lies (no permuted copies), against cate_labels in the order above, avg_factor =
 *   num_ins + 1 read ON THE DEVICE (num_ins [1] int32 as bxi_solo_assign_f32 wrote it), weight_reduce_loss's "+ FLT_EPSILON" applied.
 *   cate_preds_host / grads_host [n_levels]: DEVICE pointers (host arrays).  loss [1];  grads: d loss / d map for a unit upstream
 *   gradient, EVERY element written.  The focal code is that of bxi_fcos_loss_f32 (gamma == 2 a compile-time case); per-workgroup
 *   partials kept in fp64, then one workgroup adds them in a fixed order and rounds once: two launches, no float atomics, run-to-run identical.
 * B == 0 is a no-op.  Shapes as above, C < 1, B * C * S^2 >= 2^31: BXI_ERR_BAD_SHAPE; gamma, alpha or loss_weight NaN, gamma < 0:
 * BXI_ERR_BAD_ARGUMENT; workspace NULL / too small / not 4-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_solo_cate_loss_f32(const float* const* cate_preds_host, const int* num_grids_host, int n_levels, int B, int C,
                           const int64_t* cate_labels, const int32_t* num_ins, float gamma, float alpha, float loss_weight,
                           float* const* grads_host, float* loss, void* workspace, size_t workspace_bytes, void* stream);

/* bxi_solo_cate_grad_rescale_f32: the backward step, one launch: out = unit * upstream[0] for every element of every level; the
 *   upstream scalar is read ON THE DEVICE.  `out` may be `unit` (in place) or must not overlap it.  B == 0 is a no-op. */
int bxi_solo_cate_grad_rescale_f32(const int* num_grids_host, int n_levels, int B, int C, const float* const* unit_host,
                                   const float* upstream, float* const* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
