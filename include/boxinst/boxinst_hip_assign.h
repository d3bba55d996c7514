/*
 * boxinst_hip_assign.h -- the target-assignment step of one Box2Mask decoder layer in libboxinst_hip.so: projection matching
 * cost and Hungarian assignment for all images of the batch, with no host synchronisation and without the up-sampled
 * predictions ever existing in memory.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device
 * pointers owned by the caller, allocation-free, asynchronous on `stream`, hipGraph capturable -- the data-dependent loops of
 * the solver stay on the device --, BXI_OK or a negative bxi_status).  Paths are relative to the upstream checkout of the
 * reference (LiWentomng/BoxInstSeg):
 *   box2mask_head.py            = mmdet/models/dense_heads/box2mask_head.py
 *   match_cost.py               = mmdet/core/bbox/match_costs/match_cost.py
 *   mask_hungarian_assigner.py  = mmdet/core/bbox/assigners/mask_hungarian_assigner.py
 *
 * A batch is P problems (images) of the same Q queries and G_p ground truths each; `offsets_host` [P+1] is a HOST array,
 * offsets_host[p] = G_0 + ... + G_{p-1}, that indexes the concatenated ground-truth arrays (labels, projections).  It is
 * passed to the kernels by value: nothing is read from it after the call returns.  P <= BXI_MAX_IMAGES.
 */
#ifndef BOXINST_HIP_ASSIGN_H
#define BOXINST_HIP_ASSIGN_H

#include <stddef.h>
#include <stdint.h>

#include "../boxinst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_MATCH_MAX_SIDE 1024      /* Q and every G_p of bxi_linear_sum_assignment_f32 */
#define BXI_MATCH_TILE_ROWS 128      /* destination rows per workgroup of the projection kernels */
#define BXI_MATCH_TILE_COLS 1024     /* destination columns per workgroup */
#define BXI_MATCH_STATUS_NONFINITE 1 /* status word of the solver: the problem's cost has a NaN or an infinity */
#define BXI_MATCH_STATUS_BAD_LABEL 2 /* status word of the cost: a label of the problem is outside [0, C) */

/* Bytes of `workspace` of the three projection entry points for n planes projected at H x W (0 for a bad shape).  Layout, fp32:
 *   rowpart [n][ceil(W / BXI_MATCH_TILE_COLS)][H]   the maximum of every destination row inside one column tile,
 *   colpart [n][ceil(H / BXI_MATCH_TILE_ROWS)][W]   the maximum of every destination column inside one row band.
 * Contents undefined on entry; every element is written by the first launch before the second reads it. */
size_t bxi_box_match_workspace_bytes(int n, int H, int W);

/* bxi_match_project_pred_f32  <->  `F.interpolate(mask_pred.unsqueeze(1), target_shape, mode='bilinear', align_corners=False)`
 *     (box2mask_head.py:159-163), `mask_preds.sigmoid()` when pred_act, `max(dim=3)` / `max(dim=2)` (match_cost.py:410-418) and
 *     `mask_preds.pow(2).sum(1)` of both projections (match_cost.py:393).
 *   logits [n,h,w] fp32;  (H, W) the target size, any ratio (up- or down-sampling; H == h and W == w reads the logits as they are).
 *   The up-sampled value is ATen's: src = (dst + 0.5) * (in / out) - 0.5 in fp32, clamped below at 0, neighbour clamped at in - 1,
 *   l0y * (l0x a + l1x b) + l1y * (l0x c + l1x d).  It lives in registers only.
 *   proj_rows [n,H] = act(max over the up-sampled row), proj_cols [n,W] = act(max over the up-sampled column), act = sigmoid when
 *   apply_sigmoid != 0 (sigma is monotone: max sigma(x) = sigma(max x), applied to the n (H + W) maxima only), else the identity.
 *   The running maximum starts at -inf; a NaN wins, as in torch.max.
 *   sumsq [n,2] = sum of p^2 over proj_rows / proj_cols, accumulated in fp64 in a fixed order (element j in thread j mod 256,
 *   wave, workgroup) and rounded once.  Maxima are order-independent and nothing is accumulated atomically: run-to-run identical.
 * n == 0 is a no-op.  n < 0 or > 65535, h, w, H, W < 1 or a plane of 2^31 elements or more: BXI_ERR_BAD_SHAPE; workspace NULL / too small /
 * not 4-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_match_project_pred_f32(const float* logits, int n, int h, int w, int H, int W, int apply_sigmoid, float* proj_rows,
                               float* proj_cols, float* sumsq, void* workspace, size_t workspace_bytes, void* stream);

/* bxi_match_project_gt_u8 / _f32  <->  `gt_box_masks.max(dim=3)` / `max(dim=2)` and `gt_box_masks.pow(2).sum(1)` of the float
 *     projections (match_cost.py:415,418,389,394).  masks [g,H,W]: uint8 / bool at any byte address (the projection is the largest
 *     byte as a float), or fp32 at any 4-byte aligned address.  Outputs as above, without an activation.  g == 0 is a no-op. */
int bxi_match_project_gt_u8(const uint8_t* masks, int g, int H, int W, float* proj_rows, float* proj_cols, float* sumsq,
                            void* workspace, size_t workspace_bytes, void* stream);
int bxi_match_project_gt_f32(const float* masks, int g, int H, int W, float* proj_rows, float* proj_cols, float* sumsq,
                             void* workspace, size_t workspace_bytes, void* stream);

/* bxi_match_cost_f32  <->  ClassificationCost.__call__ (match_cost.py:191-193), BoxMatchingCost.bin_dice_loss on both projections
 *     (match_cost.py:386-398, 420-425) and their sum (mask_hungarian_assigner.py:94-111), for all P problems in one launch.
 *   cls [P*Q, C] fp32 logits (NULL or w_cls == 0: no class term);  gt_labels [G_total] int64;
 *   pred_rows [P*Q, H], pred_cols [P*Q, W], pred_sumsq [P*Q, 2], gt_rows [G_total, H], gt_cols [G_total, W], gt_sumsq [G_total, 2]
 *   from the projection entry points (NULL allowed when w_dice == 0: no dice term).
 *   cost: problem p is a row-major [Q, G_p] block at element offsets_host[p] * Q,
 *     cost[q,g] = -w_cls softmax(cls[q,:])[label_g] + w_dice (d_rows + d_cols),   d = 1 - (2 sum_j p_j t_j + eps) / (sum p^2 + sum t^2 + eps).
 *   The sums over j run in fp64 in a fixed order, the softmax in fp32; the result is rounded to fp32 once.
 *   status [P] int32: BXI_MATCH_STATUS_BAD_LABEL when a label of the problem is outside [0, C) and the class term is on -- that
 *   column's costs are NaN, nothing is read out of range -- else 0.  Every word is written.
 * P == 0 is a no-op; P < 0 or > BXI_MAX_IMAGES, Q, H, W < 1, C < 1 with a class term: BXI_ERR_BAD_SHAPE; offsets_host not
 * ascending from 0, a NaN weight or eps: BXI_ERR_BAD_ARGUMENT. */
int bxi_match_cost_f32(const float* cls, int C, const int64_t* gt_labels, const float* pred_rows, const float* pred_cols,
                       const float* pred_sumsq, const float* gt_rows, const float* gt_cols, const float* gt_sumsq, int P, int Q,
                       const int* offsets_host, int H, int W, float w_cls, float w_dice, float eps, float* cost, int32_t* status,
                       void* stream);

/* bxi_linear_sum_assignment_f32  <->  `linear_sum_assignment(cost)` with steps 1 and 4 of MaskHungarianAssigner.assign
 *     (mask_hungarian_assigner.py:77-90, 113-130) and the pos_inds / pos_assigned_gt_inds of the pseudo sampler, for the P problems
 *     of bxi_match_cost_f32 in one launch.
 *   Exact rectangular assignment by shortest augmenting paths with dual variables (Jonker-Volgenant; the smaller side is augmented
 *   row by row, as scipy's solver does).  Duals and path lengths are fp64; the fp32 costs convert exactly.  One wave per problem,
 *   its state in LDS; the loops are on the device.
 *   assigned_gt_inds [P,Q] int64: 0 background, g + 1 matched;  assigned_labels [P,Q] int64: -1 or gt_labels of the match;
 *   pos_inds, pos_assigned_gt_inds: problem p owns min(Q, G_p) slots from sum_{k<p} min(Q, G_k) on, its matched queries in ascending
 *   order and their ground truths.  G_p == 0: every query is background.
 *   status [P] int32: BXI_MATCH_STATUS_NONFINITE when the problem's cost has a non-finite entry -- then all its queries are background
 *   and its compacted slots hold -1 --, else 0.  Every word is written; nothing waits for it.
 * P == 0 is a no-op; P < 0 or > BXI_MAX_IMAGES: BXI_ERR_BAD_SHAPE; Q outside 1..BXI_MATCH_MAX_SIDE or a G_p above it:
 * BXI_ERR_UNSUPPORTED; offsets_host not ascending from 0: BXI_ERR_BAD_ARGUMENT. */
int bxi_linear_sum_assignment_f32(const float* cost, const int64_t* gt_labels, int P, int Q, const int* offsets_host,
                                  int64_t* assigned_gt_inds, int64_t* assigned_labels, int64_t* pos_inds,
                                  int64_t* pos_assigned_gt_inds, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
