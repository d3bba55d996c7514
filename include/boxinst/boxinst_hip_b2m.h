/*
 * boxinst_hip_b2m.h -- the mask losses of Box2MaskHead.loss for the matched rows of ALL decoder layers in libboxinst_hip.so: the rows'
 * scores and their small-grid resize in one pass over the gathered planes, the level-set energy "inside the box" without its
 * operands, and the local-consistency refinement with one affinity per image.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises, reads a device value on the host, calls memset or uses an atomic; every sum has a fixed order, so two
 * runs are bit-identical; every element of every output and of `state` is written exactly once per call.  Paths are relative to the
 * upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   head.py  = mmdet/models/dense_heads/box2mask_head.py   (:224-335 loss_single, run once per decoder layer by :192-221)
 *   ls.py    = mmdet/models/losses/levelset_loss.py        (:7-45 LevelsetLoss / region_levelset, :53-126 LCM)
 *
 * ROWS.  A row m is one matched (layer, image, query): row_plane[m] = l * planes + b * Q + q names its logit plane among the L layer
 * tensors of [planes = B * Q, h, w] each, tgt_of[m] its ground truth among G, img_of[m] its image among B.  The reference copies the
 * image, the targets and the affinity once per row (head.py:280-297); here they are read through these index arrays, in any order.
 * INERT ROWS.  An index of -1 -- or any index outside its range: nothing is read through it -- makes the row inert: its planes of
 * every output are zeros, its loss is 0, its gradients are zeros.  That is how the compacted slots of an image whose matching cost was
 * not finite arrive (boxinst_hip_assign.h: they hold -1).
 */
#ifndef BOXINST_HIP_B2M_H
#define BOXINST_HIP_B2M_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_B2M_MAX_LAYERS 16   /* layer tensors per call of bxi_b2m_scores_f32 */
#define BXI_B2M_MAX_UP 8        /* sh <= 8 h and sw <= 8 w: at most this up-scaling per axis to the small grid; any down-scaling */
#define BXI_B2M_MAX_C 4         /* target channels of the level-set energy (the image: 3, the two filter outputs: 2) */

/* bxi_b2m_scores_f32  <->  mask_preds = sigmoid(mask_preds[mask_weights > 0]) (head.py:260,301) and _scale_target(mask_preds) (:317)
 *   for the rows of all layers, in ONE launch: p [M,h,w] = sigmoid(logit), p_small [M,sh,sw] = the align_corners=False bilinear
 *   resize of p (its four taps are recomputed from the logits: the same values, nothing is read back).  The source index
 *   scale * (o + 0.5) - 0.5 is taken in double, so the two weights per axis are the correctly rounded ones (torch's fp32 kernels carry
 *   an ulp of the INDEX in them); the backward below uses the same weights.
 *   layers_host [L]: HOST array of L device pointers, each to [planes,h,w] fp32 logits; the tensors are separate allocations and are
 *   read in place.  row_plane [M] int32.  Inert rows are written as zeros.
 * M == 0 is a no-op.  L < 1, planes < 1, h, w, sh, sw < 1, M < 0: BXI_ERR_BAD_SHAPE; L > BXI_B2M_MAX_LAYERS, sh > 8 h, sw > 8 w,
 * M > 65535 or a plane count beyond int32: BXI_ERR_UNSUPPORTED; a NULL pointer: BXI_ERR_NULL_POINTER. */
int bxi_b2m_scores_f32(const float* const* layers_host, int L, int planes, int h, int w, const int32_t* row_plane, int M, int sh, int sw,
                       float* p, float* p_small, void* stream);

/* The backward of bxi_b2m_scores_f32 for ONE layer: EVERY element of that layer's [planes,h,w] gradient, in one launch.
 *   plane_row [planes] int32: the row of plane b * Q + q of this layer, or -1.  A matched plane gets
 *   (g_p + adjoint_resize(g_p_small)) * p * (1 - p), the adjoint in gather form (every small-grid pixel that read the element is
 *   enumerated with the forward's own weights, in ascending order); every other plane gets zeros.
 *   g_p, p [M,h,w], g_p_small [M,sh,sw].  The same support set and statuses as the forward. */
int bxi_b2m_scores_backward_f32(const float* g_p, const float* g_p_small, const float* p, const int32_t* plane_row, int planes, int M, int h,
                                int w, int sh, int sw, float* g_logits, void* stream);

/* Bytes of `state` of the level-set pair (8-byte aligned; 0 for a shape the entry points refuse). */
size_t bxi_b2m_levelset_state_bytes(int M, int C);

/* bxi_b2m_levelset_forward_f32  <->  self.loss_mask(mask_scores_phi, target * box_mask_targets, pixel_num) (head.py:305-312,325-327)
 *   with mask_scores_phi = (p T, (1 - p) T) and T = T_all[tgt_of[m]], none of which is stored.  The products are rounded to fp32 as
 *   the reference's tensors are; the region sums are fp64 in a fixed order and the 1e-5 clamps are ls.py:34-35's (levelset.hip).
 *   p [M,h,w]; T_all [G,h,w]; pixel_num [G] (already clamped, :310), read through tgt_of [M].
 *   shared != 0: target [B,C,h,w], read through img_of [M] (the image; no gradient).
 *   shared == 0: target [M,C,h,w], the row's own (the up-sampled filter outputs); img_of may be NULL.
 *   loss [M] = weight * energy / (C * pixel_num).  Two launches.
 * M == 0 is a no-op.  C outside 1..BXI_B2M_MAX_C or M > 65535: BXI_ERR_UNSUPPORTED; state NULL or not 8-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_b2m_levelset_forward_f32(const float* p, const float* T_all, const float* target, int shared, const int32_t* tgt_of,
                                 const int32_t* img_of, const float* pixel_num, int M, int G, int B, int C, int h, int w, float weight,
                                 float* loss, void* state, void* stream);

/* Its backward, one launch: g_p [M,h,w] (both score channels folded: T * (g_fore - g_back)) and, unless NULL, g_target [M,C,h,w]
 * already multiplied by T (shared == 0 only; with shared != 0 it must be NULL: BXI_ERR_BAD_ARGUMENT).  Every element of both is written. */
int bxi_b2m_levelset_backward_f32(const float* p, const float* T_all, const float* target, int shared, const int32_t* tgt_of,
                                  const int32_t* img_of, const float* pixel_num, int M, int G, int B, int C, int h, int w, float weight,
                                  const void* state, const float* g_loss, float* g_p, float* g_target, void* stream);

/* bxi_b2m_lcm_refine_f32 = bxi_lcm_refine_f32 (../boxinst_hip.h) with the affinity aff [B,8,h,w] of row m read through img_of [M]:
 * phi, out [M,h,w]; transpose != 0 is the adjoint.  The same kernels, dispatch and workspace rule (bxi_lcm_workspace_bytes(M, h, w)). */
int bxi_b2m_lcm_refine_f32(const float* aff, const float* phi, const int32_t* img_of, int B, int M, int h, int w, int dilation, int iters,
                           int transpose, float* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
