/*
 * boxinst_hip_roi.h -- RoIAlign (forward and backward) and the front of one level of DiscoBox's corr_loss in libboxinst_hip.so: the boxes
 * of the target masks, the 7 x 7 feature path fused with relu_and_l2_norm_feat, the 28 x 28 mask path with the sigmoid on the taps.
 * gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   discobox_head.py = mmdet/models/dense_heads/discobox_head.py  (relu_and_l2_norm_feat :16-20, the RoIAlign modules :740-742, the
 *                      front of one level of corr_loss :1018-1057)
 *
 * RoIAlign is mmcv's op (mmcv.ops.roi_align), which is not part of the reference tree.  Its arithmetic is RESTATED here from its
 * documented algorithm (the one Detectron2 and torchvision share) and is UNPINNED: mmcv never ran next to this library.  For a roi
 * (b, x1, y1, x2, y2):  off = aligned ? 0.5 : 0;  xs = x1 * scale - off, likewise ys, xe, ye;  rw = xe - xs, rh = ye - ys, clamped to
 * >= 1 only when not aligned;  bin_h = rh / PH, bin_w = rw / PW;  gh = sampling_ratio > 0 ? sampling_ratio : ceil(rh / PH), gw
 * likewise;  count = max(gh * gw, 1);  samples y = ys + ph * bin_h + (iy + 0.5) * bin_h / gh, x likewise;  the output is the sum of the
 * bilinear samples / count.  One sample: 0 if y < -1 or y > H or x < -1 or x > W; else y = max(y, 0), y_low = (int)y; if y_low >= H - 1
 * then y_low = y_high = H - 1 and y = y_low, else y_high = y_low + 1; x the same; weights hy hx, hy lx, ly hx, ly lx.  The backward
 * distributes g / count with the same weights.
 *
 * All data is fp32, rois are [K, 5] fp32.  Sums run in a fixed order and there are no float atomics: results are run-to-run identical.
 * A roi whose batch index is outside [0, B), or that holds a NaN or an infinity, gives a zero row and takes no gradient.
 * Limits: PH, PW <= BXI_ROI_MAX_POOL, sampling_ratio <= BXI_ROI_MAX_SAMPLING, H, W <= BXI_ROI_MAX_SIDE, every tensor below 2^31
 * elements; the fused feature path takes C <= BXI_ROI_FUSED_MAX_C and returns BXI_ERR_UNSUPPORTED beyond (compose it from
 * bxi_roi_align_forward_f32 then).  pool_mode = 'max' is not built.
 */
#ifndef BOXINST_HIP_ROI_H
#define BOXINST_HIP_ROI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_ROI_MAX_POOL 64
#define BXI_ROI_MAX_SAMPLING 64
#define BXI_ROI_MAX_SIDE 16384
#define BXI_ROI_FUSED_MAX_C 8192
#define BXI_ROI_FEAT 7               /* the output size of the fused feature path (feat_roi_align, :740) */
#define BXI_ROI_SIGMOID 1            /* `flags` of bxi_roi_align_forward_f32: the sigmoid of every tap is pooled (:1018, :1050-1053) */

/* bxi_roi_target_boxes_u8  <->  :1025-1038 and the label each object of the loop reads (:1064, :1070, :1118), TWO launches: one workgroup
 *   per object over its bytes (16-byte reads between a byte-wise head and tail: `target` may start at any address), then one workgroup
 *   for the ranks.
 *   target [N, H, W] uint8, contiguous.  boxes [N, 4] fp32 = (min_x, min_y, max_x + 1, max_y + 1) of the non-zero pixels, (0, 0, 0, 0)
 *   where there are none.  keep [N] uint8 = 1 where there are some.  labels_out [N] int64: -1 for a dropped object; for a kept one
 *   kernel_labels[its rank among the kept] (the reference filters the objects but not kernel_labels, :1029), or with own_labels != 0
 *   kernel_labels[its own index].  kernel_labels [N] int64.  Every output element is written.
 * N == 0 is a no-op.  N < 0, H or W < 1, H * W >= 2^31: BXI_ERR_BAD_SHAPE. */
int bxi_roi_target_boxes_u8(const uint8_t* target, const int64_t* kernel_labels, int N, int H, int W, int own_labels, float* boxes,
                            uint8_t* keep, int64_t* labels_out, void* stream);

/* bxi_roi_align_forward_f32  <->  mmcv's RoIAlign forward, pool_mode = 'avg' (self.feat_roi_align / self.mask_roi_align, :740-742,
 *   :1040-1053), ONE launch, one wave per output element, its lanes over the samples of the bin.
 *   input [B, C, H, W], rois [K, 5], out [K, C, PH, PW], every element written.  flags: 0 or BXI_ROI_SIGMOID.
 * K == 0 or C == 0 is a no-op.  Sizes outside the limits above: BXI_ERR_BAD_SHAPE; a NaN spatial_scale, a negative sampling_ratio, unknown
 * flags: BXI_ERR_BAD_ARGUMENT. */
int bxi_roi_align_forward_f32(const float* input, const float* rois, int B, int C, int H, int W, int K, int PH, int PW,
                              float spatial_scale, int sampling_ratio, int aligned, int flags, float* out, void* stream);

/* bxi_roi_align_backward_f32  <->  mmcv's RoIAlign backward, ONE launch, a gather: a thread owns one pixel of 16 channels and adds, in
 *   roi order, what the rois of its image give it (the op is separable: the weight of a pixel is wy(y) * wx(x) / count per bin).
 *   g_out [K, C, PH, PW], g_input [B, C, H, W]: EVERY element written, zeros where no roi reaches (K == 0 writes zeros).
 * C == 0 is a no-op. */
int bxi_roi_align_backward_f32(const float* g_out, const float* rois, int B, int C, int H, int W, int K, int PH, int PW,
                               float spatial_scale, int sampling_ratio, int aligned, float* g_input, void* stream);

/* Bytes of `workspace` of the fused feature path (0 for a bad shape or C > BXI_ROI_FUSED_MAX_C; at least 16): the norms [K, 49] fp32
 * that the forward leaves for the backward, and the gradient of the pooled values [K, C, 49] fp32.  16-byte aligned. */
size_t bxi_roi_feat_norm_workspace_bytes(int K, int C);

/* bxi_roi_feat_norm_forward_f32  <->  relu_and_l2_norm_feat(self.feat_roi_align(feat, rois)) (:1040-1044, :16-20), ONE launch, one
 *   workgroup per (roi, bin): RoIAlign at 7 x 7, relu, n = sqrt(sum_c f^2 + 1e-6), f / (n + 1e-6).  The pooled values stay in LDS.
 *   out [K, C, 7, 7], every element written; n goes to the workspace. */
int bxi_roi_feat_norm_forward_f32(const float* input, const float* rois, int B, int C, int H, int W, int K, float spatial_scale,
                                  int sampling_ratio, int aligned, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* bxi_roi_feat_norm_backward_f32: d / d input of the fused path, TWO launches: through the norm and the relu per (roi, bin) into the
 *   workspace, then the gather of bxi_roi_align_backward_f32.  out [K, C, 7, 7] as the forward wrote it, g_out its upstream gradient,
 *   the workspace as the forward left it.  g_input [B, C, H, W]: EVERY element written. */
int bxi_roi_feat_norm_backward_f32(const float* out, const float* g_out, const float* rois, int B, int C, int H, int W, int K,
                                   float spatial_scale, int sampling_ratio, int aligned, float* g_input, void* workspace,
                                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
