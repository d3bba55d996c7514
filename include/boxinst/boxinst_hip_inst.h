/*
 * boxinst_hip_inst.h -- Box2Mask at test time in libboxinst_hip.so: the query x class top-k of the last decoder layer's class logits,
 * and the final uint8 masks of the selected queries with the mask score, the area and the box of each.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   box2mask_head.py          = mmdet/models/dense_heads/box2mask_head.py   (:445-459 simple_test: F.interpolate to batch_input_shape)
 *   maskformer_fusion_head.py = mmdet/models/seg_heads/panoptic_fusion_heads/maskformer_fusion_head.py
 *                               (:112-162 instance_postprocess, :207-241 simple_test: the crop and the second F.interpolate)
 *   mask_utils.py             = mmdet/core/mask/utils.py                    (:68-89 mask2bbox)
 */
#ifndef BOXINST_HIP_INST_H
#define BOXINST_HIP_INST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The largest Q * C bxi_inst_topk_f32 sorts (the keys of one image live in the LDS of one workgroup: 8 bytes each, 128 KB). */
#define BXI_INST_TOPK_MAX 16384

/* bxi_inst_topk_f32  <->  maskformer_fusion_head.py:133-151: scores = F.softmax(mask_cls, dim=-1)[:, :-1]; topk(max_per_image) over the
 *                         Q * C scores; labels = index % C, query = index // C; the is_thing filter.
 *   ONE launch for the batch, one workgroup per image.
 *   cls [B,Q,C+1] fp32 class logits (the last column is the background), any 4-byte aligned address.  The softmax is fp32: the row's
 *   maximum subtracted, expf, one division by the sum (the sum in a fixed order).  A row that holds a NaN gives NaN scores.
 *   The ORDER IS DEFINED (torch's sorted=False leaves it open): descending score, equal scores by ascending flat index q * C + c; a NaN
 *   score orders after every number.  The first k entries of that order are the selection.
 *   Then entries with label >= num_things are dropped and the rest moved up in order.  Per image b:
 *   scores [B,k] fp32, labels [B,k] int64, query [B,k] int64: rows [0, count[b]) hold the result, rows [count[b], k) hold score 0,
 *   label -1, query -1 (bxi_inst_paste_u8 writes an empty mask for query -1): every element is written.
 *   count [B] int32 stays on the device.
 * Support set: 1 <= k <= Q * C <= BXI_INST_TOPK_MAX (100 x 133 fits).  Checked before anything touches a device, in this order: B < 0,
 * Q < 1, C < 1, k < 1, num_things < 0 or num_things > C, B * Q * (C + 1) >= 2^31: BXI_ERR_BAD_SHAPE; k > Q * C or Q * C >
 * BXI_INST_TOPK_MAX: BXI_ERR_UNSUPPORTED; B == 0 returns BXI_OK and touches nothing; a NULL pointer: BXI_ERR_NULL_POINTER. */
int bxi_inst_topk_f32(const float* cls, int B, int Q, int C, int num_things, int k, float* scores, int64_t* labels, int64_t* query,
                      int32_t* count, void* stream);

/* Bytes of `workspace` of bxi_inst_paste_u8 (0 for n == 0 and for a shape the entry point refuses): one 16-byte record per mask,
 * output row and chunk of 1024 output columns.  16-byte aligned, contents undefined on entry, every byte written by the call. */
size_t bxi_inst_paste_workspace_bytes(int n, int out_h, int out_w);

/* bxi_inst_paste_u8  <->  box2mask_head.py:452-457, maskformer_fusion_head.py:211-221 and :145-160 for one image:
 *       x = F.interpolate(mask_pred, size=up, mode='bilinear')[query][:, :crop_h, :crop_w];  p = F.interpolate(x, size=out, 'bilinear')
 *       mask = p > 0;  mask_score = (sigmoid(p) * mask).sum() / (mask.sum() + 1e-6);  box = mask2bbox(mask), cls_score * mask_score
 *   TWO launches: the masks with per-row counts and sums into the workspace, then the per-mask statistics.
 *   logits [n_all,h,w] fp32 mask logits of the image's queries, any 4-byte aligned address; query [n] int64 rows of logits in result
 *   order (repeats allowed; an index outside [0, n_all) gives an all-zero mask, empty statistics, a zero score and a zero box, and
 *   reads nothing).  No copy of the selected rows is made.  cls_scores [n] fp32: the class score of each row.
 *   up = stage 1's size (batch_input_shape; up == (h, w) when the head has resized already), crop = img_shape <= up, out = ori_shape
 *   with rescale, the crop without.  Both stages are ATen's fp32 bilinear kernel with align_corners=False and scale = (float)in / out;
 *   equal sizes are the identity.  The products of the two stages are regrouped (one horizontal, one vertical pass): the same taps and
 *   weights, p within ~16 ulp of the largest |logit| of the plane.  The test is p > 0 in fp32; a NaN compares false.
 *   masks [n,out_h,out_w] uint8 0 / 1 at ANY byte address, every byte written exactly once.
 *   stats [n,5] int32: area, x_min, y_min, x_max, y_max (inclusive, output pixels); an empty mask gives (0, -1, -1, -1, -1).
 *   mask_scores [n] fp32 = sum / (area + 1e-6), sum = the sigmoid 1 / (1 + expf(-p)) over the set pixels AT THE OUTPUT RESOLUTION: fp32
 *   over 16 consecutive pixels in element order, fp32 over a row's 16-pixel segments in ascending order, fp64 over the rows (and chunks)
 *   in a fixed order; the division in fp64, rounded once.  No float atomics: run-to-run bit-identical.
 *   boxes [n,5] fp32 = (x_min, y_min, x_max + 1, y_max + 1, cls_scores[i] * mask_scores[i]); (0, 0, 0, 0, cls_scores[i] * 0) for an
 *   empty mask.  Every element of every output is written; nothing is asked of the caller's contents.
 * n == 0 returns BXI_OK and touches nothing.  Checked before anything touches a device, in this order: a non-positive size, crop > up,
 * n < 0, n * bands * chunks >= 2^31 (bands of 16 rows, chunks of 1024 columns), out_h * out_w >= 2^31 or n_all * h * w >= 2^31:
 * BXI_ERR_BAD_SHAPE; a NULL pointer: BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned: BXI_ERR_WORKSPACE; source
 * rows too wide for the staging buffer (~5000 columns) or more than 2^24 workgroups: BXI_ERR_UNSUPPORTED. */
int bxi_inst_paste_u8(const float* logits, int n_all, int h, int w, const int64_t* query, const float* cls_scores, int n, int up_h, int up_w,
                      int crop_h, int crop_w, int out_h, int out_w, uint8_t* masks, int32_t* stats, float* mask_scores, float* boxes,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
