/*
 * boxinst_hip_fcos.h -- the training step of CondInst's box head in libboxinst_hip.so: the FCOS target assignment of every level and
 * image, sigmoid focal loss, the IoU / GIoU loss and the centerness loss with their finished gradients.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h and
 * boxinst_hip_det.h (device pointers owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable,
 * BXI_OK or a negative bxi_status; where a failure depends on data a `status` word on the device says so).  Paths are relative to
 * the upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   condinst_head.py   = mmdet/models/dense_heads/condinst_head.py   (loss :365-476, get_targets :478-548, _get_target_single :550-633,
 *                                                                     centerness_target :855-874)
 *   focal_loss.py      = mmdet/models/losses/focal_loss.py           (py_sigmoid_focal_loss :12-57)
 *   iou_loss.py        = mmdet/models/losses/iou_loss.py             (iou_loss :16-50, giou_loss :102-117)
 *   iou2d_calculator.py= mmdet/core/bbox/iou_calculators/iou2d_calculator.py (bbox_overlaps, is_aligned :218-261)
 *   utils.py           = mmdet/models/losses/utils.py                (weight_reduce_loss :30-59: sum / (avg_factor + FLT_EPSILON))
 * and `mmcv.ops.sigmoid_focal_loss`, which the reference calls on a device and whose source is not part of it (restated, unpinned:
 * what is restated here is py_sigmoid_focal_loss, the reference's own formula for the same quantity).
 *
 * Flatten order.  The reference's TRAINING order (condinst_head.py:404-435), not the [B, M_all] order of boxinst_hip_det.h:
 * level-major, then image, then y, then x.  N_all = B * M_all; level l begins at B * sum_{k<l} H_k W_k; location (l, b, y, x) is
 * row  B * first_l + b * H_l W_l + y * W_l + x.  A location's point is ((x + 0.5) * stride, (y + 0.5) * stride), exact in fp32, so no
 * points tensor is read.
 *
 * Deviation from the reference: a batch that contains an image WITHOUT ground truth.  The reference raises there
 * (_get_target_single returns two values for such an image, get_targets unpacks three: "ValueError: not enough values to unpack").
 * Here such an image gives what that branch evidently intends: labels = num_classes, bbox_targets = 0, gt_inds = -1.
 *
 * Units.  With norm_on_bbox the targets are divided by the level's stride and the head predicts distances in stride units, while the
 * points stay in pixels; the reference decodes both with distance2bbox(point, distance) all the same (condinst_head.py:456-459).
 * The mixed units are mirrored: the IoU of the two decoded boxes is what the reference computes.
 */
#ifndef BOXINST_HIP_FCOS_H
#define BOXINST_HIP_FCOS_H

#include <stddef.h>
#include <stdint.h>

#include "boxinst_hip_det.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_FCOS_GT_CHUNK 64            /* boxes of an image staged in LDS at a time; any number of boxes per image works */
#define BXI_FCOS_LOC_TILE 256           /* locations per workgroup of the per-location kernels (one (level, image) per workgroup) */
#define BXI_FCOS_ELEM_TILE 1024         /* elements per workgroup of the flat kernels (focal loss, gradient rescale) */
#define BXI_FCOS_STATUS_BAD_LABEL 1     /* status word of bxi_fcos_targets_f32: a gt label outside [0, num_classes) */
#define BXI_FCOS_BBOX_GIOU 0            /* bbox_loss_kind: GIoULoss */
#define BXI_FCOS_BBOX_IOU_LOG 1         /*                 IoULoss(mode='log')     */
#define BXI_FCOS_BBOX_IOU_LINEAR 2      /*                 IoULoss(mode='linear')  */
#define BXI_FCOS_BBOX_IOU_SQUARE 3      /*                 IoULoss(mode='square')  */

/* One FPN level of the head: the size of its maps and its stride. */
typedef struct { int H, W, stride; } bxi_fcos_level;
/* The gradient maps of one level, in the layout of the maps themselves: cls [B,C,H,W], bbox [B,4,H,W], ctr [B,1,H,W]. */
typedef struct { float *cls, *bbox, *ctr; } bxi_fcos_grads;

/* Bytes of `workspace` of bxi_fcos_targets_f32 and bxi_fcos_loss_f32 (one size serves both; 0 for a bad shape): four 32-bit words per
 * workgroup, the per-workgroup partial sums.  Contents undefined on entry; every word that is read has been written by the same call. */
size_t bxi_fcos_workspace_bytes(const bxi_fcos_level* levels_host, int n_levels, int B, int C);

/* bxi_fcos_targets_f32  <->  CondInstBoxHead.get_targets / _get_target_single / centerness_target and the index tensors `loss`
 *     builds (condinst_head.py:396-435, :478-633, :855-874) for all images and levels: one launch, and a one-workgroup launch for the sums.
 *   levels_host [n_levels], regress_ranges_host [n_levels][2] fp32 (what `new_tensor(self.regress_ranges[i])` holds) and
 *   gt_offsets_host [B+1] (image b owns the boxes gt_offsets[b] .. gt_offsets[b+1]-1; gt_offsets[0] = 0, gt_offsets[B] = G) are HOST
 *   arrays, passed to the kernel by value.  gt_boxes [G,4] fp32 x1,y1,x2,y2 and gt_labels [G] int64 on the device (NULL when G = 0).
 *   One thread per location; the image's boxes pass through LDS in chunks of BXI_FCOS_GT_CHUNK.  Every quantity a decision rests on is
 *   the reference's single fp32 operation, never contracted: xs - x1, (x1 + x2) / 2, center -+ (float)(stride * radius), the `where`
 *   clamps, min(...) > 0, max(...) >= lo && <= hi (both ends inclusive), (x2 - x1) * (y2 - y1).  A box that fails a condition counts
 *   with area 1e8f, and a location is background exactly where the minimum == 1e8f (the reference's sentinel: a real box of that area
 *   is background there too).
 *   TIE RULE: among equal minimal areas the LOWEST box index wins (what torch.min returns on the CPU; a device torch.min leaves it open).
 *   Consequence, mirrored: a background location of an image that has boxes carries the bbox_targets of that image's box 0.
 *   Outputs, N_all rows each, every element written:
 *     labels int64 (num_classes = background);  bbox_targets [N_all,4] l,t,r,b (divided by the stride when norm_on_bbox);
 *     gt_inds int64, global (offset by gt_offsets[b]), -1 = background;  points [N_all,2];  level_inds, img_inds int64;
 *     ctr_targets: centerness_target of a positive location, 0 elsewhere;
 *     stats [2] fp32: the number of positives and the sum of ctr_targets, summed in a fixed order (per-workgroup partials, the
 *     centerness sum kept in fp64 and rounded once at the end; one workgroup adds the partials, also in a fixed order; no float
 *     atomics, no workgroup waits for another: run-to-run identical);
 *     status [1] int32: 0, or BXI_FCOS_STATUS_BAD_LABEL -- a location such a box would have won is written as background.
 * B == 0 is a no-op.  n_levels outside 1..BXI_DET_MAX_LEVELS, B < 0 or > BXI_MAX_IMAGES, num_classes < 1, a level with H, W or
 * stride < 1, N_all * 4 >= 2^31, gt_offsets not starting at 0 or decreasing: BXI_ERR_BAD_SHAPE; a NaN regress range or a radius that is
 * NaN or negative with center_sampling: BXI_ERR_BAD_ARGUMENT; workspace NULL / too small / not 4-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_fcos_targets_f32(const bxi_fcos_level* levels_host, int n_levels, int B, const float* regress_ranges_host, int center_sampling,
                         double center_sample_radius, int norm_on_bbox, int num_classes, const float* gt_boxes, const int64_t* gt_labels,
                         const int* gt_offsets_host, int64_t* labels, float* bbox_targets, int64_t* gt_inds, float* points,
                         int64_t* level_inds, int64_t* img_inds, float* ctr_targets, float* stats, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);

/* bxi_fcos_loss_f32  <->  the three losses of CondInstBoxHead.loss (condinst_head.py:437-474) and their finished gradients.
 *   levels_host [n_levels]: the NCHW maps where they lie (`params` is not read; may be NULL);  labels, bbox_targets, ctr_targets as
 *   bxi_fcos_targets_f32 wrote them;  norm [2] fp32 ON THE DEVICE: the cross-rank mean of `stats`, or `stats` itself in one process.
 *   The kernels apply max(norm[0], 1) and max(norm[1], 1e-6) themselves, and weight_reduce_loss's "+ FLT_EPSILON" on both.
 *   losses [3] = loss_cls, loss_bbox, loss_centerness;  grads_host [n_levels]: d losses[k] / d map for a unit upstream gradient, in the
 *   maps' own NCHW layout.  EVERY element is written, zeros included: no memset by the caller.
 *     loss_cls         sigmoid focal loss over every class logit, avg_factor = num_pos (focal_loss.py:12-57, restated, unpinned), in the
 *                      form max(x,0) - x t + log1p(exp(-|x|)) with closed-form derivatives; gamma == 2 is a compile-time special case.
 *     loss_bbox        positives only: distance2bbox(point, pred) against distance2bbox(point, target), bbox_overlaps(is_aligned=True),
 *                      then giou_loss or iou_loss(mode) (`eps`: GIoULoss.eps / IoULoss.eps; the union's own clamp inside iou_loss is the
 *                      reference's fixed 1e-6), weight = ctr_targets, avg_factor = norm[1].
 *                      DIoULoss, CIoULoss, BoundedIoULoss are not built: any other bbox_loss_kind is BXI_ERR_UNSUPPORTED.
 *     loss_centerness  BCE-with-logits of the centerness logit against ctr_targets on positives, avg_factor = num_pos.
 *   Gradients at exact ties follow torch: elementwise min / max of two equal tensors' elements split the gradient in halves (this
 *   includes torch.max(union, eps) and torch.max(enclose_area, eps), which are elementwise maxima of two tensors);
 *   clamp(min=...) passes the gradient at equality and blocks it below.
 *   Loss sums: per-workgroup partials, then one workgroup adds them in a fixed order.  No float atomics: run-to-run identical.
 * B == 0 is a no-op.  Shapes as above, C < 1 or B * C * H * W >= 2^31 on a level: BXI_ERR_BAD_SHAPE; gamma, alpha, eps or a loss weight
 * NaN, gamma < 0, eps <= 0: BXI_ERR_BAD_ARGUMENT; unknown bbox_loss_kind: BXI_ERR_UNSUPPORTED; workspace: BXI_ERR_WORKSPACE. */
int bxi_fcos_loss_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, const int64_t* labels, const float* bbox_targets,
                      const float* ctr_targets, const float* norm, float gamma, float alpha, float loss_weight_cls, float loss_weight_bbox,
                      float loss_weight_ctr, int bbox_loss_kind, float eps, const bxi_fcos_grads* grads_host, float* losses, void* workspace,
                      size_t workspace_bytes, void* stream);

/* bxi_fcos_grad_rescale_f32: the backward step.  out = unit * upstream[k] for every element of every map of every level in one launch
 *   (k = 0 cls, 1 bbox, 2 ctr); upstream [3] fp32 is read ON THE DEVICE, as bxi_boxinst_grad_rescale_f32 reads its scalars: no host
 *   synchronisation.  unit_host / out_host [n_levels]; `out` may be `unit` (in place) or must not overlap it.
 * B == 0 is a no-op; shapes as above. */
int bxi_fcos_grad_rescale_f32(const bxi_fcos_level* levels_host, int n_levels, int B, int C, const bxi_fcos_grads* unit_host,
                              const float* upstream, const bxi_fcos_grads* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
