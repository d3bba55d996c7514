/*
 * boxinst_hip_seg.h -- the final masks of the SOLOv2-style heads (DiscoBox, BoxLevelSet) in libboxinst_hip.so: the probabilities of the
 * candidates Matrix NMS kept -> two bilinear resizes, crop and threshold -> uint8 masks at the original image size, with the area and the
 * tight box of every mask.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   box_solov2_head.py   = mmdet/models/dense_heads/box_solov2_head.py   (:576-588 the two F.interpolate and `> cfg.mask_thr`)
 *   discobox_head.py     = mmdet/models/dense_heads/discobox_head.py     (:1641-1655 the same)
 *   single_stage_ts.py   = mmdet/models/detectors/single_stage_ts.py     (:88-103 format_results: the area test and the box of a mask)
 */
#ifndef BOXINST_HIP_SEG_H
#define BOXINST_HIP_SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `workspace` of bxi_seg_paste_u8 (0 for n == 0 and for a shape the entry point refuses): one 16-byte record per kept mask,
 * output row and chunk of 1024 output columns.  16-byte aligned, contents undefined on entry, every byte written by the call. */
size_t bxi_seg_paste_workspace_bytes(int n, int out_h, int out_w);

/* bxi_seg_paste_u8  <->  seg_masks = F.interpolate(F.interpolate(seg_preds[keep_inds], size=up, mode='bilinear')[:, :, :crop_h, :crop_w],
 *                                                   size=out, mode='bilinear') > mask_thr
 *   TWO launches: the masks with per-row counts into the workspace, then the per-mask statistics.
 *   probs [n_all,h,w] fp32 probabilities, any 4-byte aligned address; keep_inds [n] int64 rows of probs in result order (repeats allowed;
 *   an index outside [0, n_all) gives an all-zero mask and empty statistics and reads nothing).  No copy of the kept rows is made.
 *   up = stage 1's size (4 h x 4 w in the heads), crop = img_shape <= up, out = ori_shape.  Both stages are ATen's fp32 bilinear kernel with
 *   align_corners=False and scale = (float)in / out; equal sizes are the identity.  The products of the two stages are regrouped (one
 *   horizontal, one vertical pass): the same taps and weights, p within ~1e-7 of the composition.  The test is p > threshold in fp32; a
 *   NaN compares false.
 *   masks [n,out_h,out_w] uint8 0 / 1 at ANY byte address, every byte written exactly once.
 *   stats [n,5] int32: area (the number of set bytes), x_min, y_min, x_max, y_max (inclusive, output pixels); an empty mask gives
 *   (0, -1, -1, -1, -1).  Every element is written; nothing is asked of the caller's contents.  Integer arithmetic only and no workgroup
 *   waits for another: run-to-run bit-identical.
 * n == 0 returns BXI_OK and touches nothing.  Checked before anything touches a device, in this order: a non-positive size, crop > up,
 * n < 0, n * bands * chunks >= 2^31 (bands of 16 rows, chunks of 1024 columns), out_h * out_w >= 2^31 (the area is an int32) or
 * n_all * h * w >= 2^31: BXI_ERR_BAD_SHAPE; a NaN threshold: BXI_ERR_BAD_ARGUMENT; a NULL pointer: BXI_ERR_NULL_POINTER; workspace NULL /
 * too small / not 16-byte aligned: BXI_ERR_WORKSPACE; source rows too wide for the staging buffer (~5000 columns) or more than 2^24
 * workgroups: BXI_ERR_UNSUPPORTED. */
int bxi_seg_paste_u8(const float* probs, int n_all, int h, int w, const int64_t* keep_inds, int n, int up_h, int up_w, int crop_h, int crop_w,
                     int out_h, int out_w, float threshold, uint8_t* masks, int32_t* stats, void* workspace, size_t workspace_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
