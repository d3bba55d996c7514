/*
 * boxinst_hip_dconvl.h -- BoxLevelSet's training masks in libboxinst_hip.so: the dynamic 1x1 mask convolution of the ASSIGNED grid cells
 * only, followed by the per-level bilinear resize, forward and backward.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   box_solov2_head.py = mmdet/models/dense_heads/box_solov2_head.py
 *     :205-216  forward: F.conv2d(feature_pred, kernel, groups=N) over ALL cells of a level, F.interpolate(size=2 x featmap_size,
 *               mode='bilinear') of the whole result
 *     :317-320  loss: ins_preds_level_img[ins_ind_labels_level_img] -- the rows of the set cells, ascending, are all that is kept
 *
 * What is computed.  For level l, image b and set cell c (ascending), with S_l = grids[l] and (oh_l, ow_l) = level_sizes[2l], [2l+1]:
 *     out_l[i] = resize_l( sum_e kernel_maps[l][b, e, c / S_l, c % S_l] * feat[b, e, :, :] )        (logits; the sigmoid is the loss's)
 * resize_l is F.interpolate(size=(oh_l, ow_l), mode='bilinear'), align_corners=False, with torch's weights for a given size, per axis in
 * fp32:  scale = in / out;  src = max(scale * (dst + 0.5) - 0.5, 0);  i0 = floor(src);  i1 = min(i0 + 1, in - 1);  l1 = src - i0;
 * l0 = 1 - l1;  value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).  A level of the feature's own size is not resampled.
 *
 * DEVIATION: the product (over e) and the resize (over pixels) act on different axes and commute in real arithmetic; here the FEATURE is
 * resized once per size group and the product is taken on the resized feature, so the results equal the reference's to rounding, not
 * in operation order.  Nothing of the size (cells of a level) x H x W exists, and no [N_l, H, W] copy of the rows of a down-sized level.
 *
 * Size groups.  A size group is a run of consecutive levels of one (oh, ow) (the FPN order makes equal sizes consecutive: the configs
 * give three groups, levels {0, 1}, {2}, {3, 4}).  Per group: the resized feature [B,E,oh,ow] of the images that have rows in the group
 * goes to the workspace (not for a group of the feature's own size), then the gather and the product of boxinst_hip_dconv.h run on it
 * for the group's levels: v_mfma_f32_32x32x2_f32, every logit ONE fp32 fmaf chain over e ascending.  The feature of an image is read once
 * per size group, and not at all for an image without rows.  A row's bits depend on its own kernel values, its image's feature and its
 * level's size only -- not on the other rows, their number or their order.  A NaN kernel value stays in its row; a NaN feature value
 * reaches the output pixels whose taps (i0 or i1 on both axes) name it, and no other.
 *
 * Rows and segments as in boxinst_hip_dconv.h: the N rows are level-major, inside a level image by image, inside an image in the order
 * of `cells`; `seg_counts` (HOST, [L*B], index l*B + b) sums to N; `cells` (DEVICE, int64 [N]) holds each row's cell in [0, S_l^2).  A
 * cell outside its map is never read: its row is that of an all-zero kernel, it contributes no gradient, and status[0] is set to
 * BXI_DCONV_STATUS_BAD_CELL (a plain store; the caller zeroes status[0] before the call).
 *
 * Support set (mirrored in boxinstseg_amd/_lib.py): fp32 only; B in [1, BXI_MAX_IMAGES], L in [1, BXI_DCONV_MAX_LEVELS], E in
 * [1, BXI_DCONV_MAX_E]; per axis in <= BXI_DCONVL_MAX_DOWN * out (down-sizing by any ratio up to 8, integer or not) and
 * out <= BXI_DCONVL_MAX_UP * in (up-sizing up to 2x: 2 * ceil(h / 2) is h + 1 for an odd h).  A level size outside it:
 * BXI_ERR_UNSUPPORTED, before any launch.
 */
#ifndef BOXINST_HIP_DCONVL_H
#define BOXINST_HIP_DCONVL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_DCONVL_MAX_DOWN 8          /* per axis: in <= 8 * out */
#define BXI_DCONVL_MAX_UP 2            /* per axis: out <= 2 * in */

/* Bytes of `workspace` of bxi_solo_dconvl_forward_f32: per resampled size group with rows B*E*oh*ow floats of resized feature, then the
 * largest forward workspace of boxinst_hip_dconv.h over the groups.  0 when no level has rows and for arguments the entry point
 * refuses.  16-byte aligned, contents undefined on entry; every byte the call reads it has written. */
size_t bxi_solo_dconvl_forward_workspace_bytes(int B, int E, int H, int W, const int* level_sizes, const int* seg_counts, int L);

/* bxi_solo_dconvl_forward_f32: the rows above.  feat [B,E,H,W] fp32; kernel_maps (host, [L]) the device maps [B,E,S_l,S_l]; grids (host,
 * [L]); level_sizes (host, [2L]) = oh_0, ow_0, oh_1, ...; out: the levels back to back, level l as [N_l, oh_l, ow_l] fp32, every element
 * written once.  Per size group with rows up to three launches (the resize, the gather, the product); no memset, no atomics, run-to-run
 * bit-identical.  N == 0 returns BXI_OK and touches nothing.
 * Checked before anything touches a device, in this order: NULL kernel_maps / grids / level_sizes / seg_counts: BXI_ERR_NULL_POINTER;
 * the shape checks of bxi_solo_dconv_forward_f32, a level size < 1 or sum_l N_l*oh_l*ow_l >= 2^31: BXI_ERR_BAD_SHAPE; a level size
 * outside the support set: BXI_ERR_UNSUPPORTED; then (N > 0) a NULL feat, map, cells, out or status: BXI_ERR_NULL_POINTER; workspace
 * NULL / too small / not 16-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_solo_dconvl_forward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                const int* level_sizes, int L, const int64_t* cells, const int* seg_counts, int N, float* out,
                                int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of `workspace` of bxi_solo_dconvl_backward_f32: per size group with rows B*E*oh*ow floats for the gradient of its (resized)
 * feature; once, for the largest resampled group, as many for the resized feature; then the largest backward workspace of
 * boxinst_hip_dconv.h over the groups.  0 when no level has rows and for arguments the entry point refuses. */
size_t bxi_solo_dconvl_backward_workspace_bytes(int B, int E, int H, int W, const int* level_sizes, const int* seg_counts, int L);

/* bxi_solo_dconvl_backward_f32: the forward's inputs and grad_out (the layout of out)  ->
 *   grad_feat [B,E,H,W]            (may be NULL) the gradient with respect to each group's resized feature is written ONCE to the
 *                                  workspace (rows of an image in ascending order, zeros for an image without rows in the group); a last
 *                                  kernel writes EVERY element of grad_feat as the sum over the groups, in group order, of the adjoint
 *                                  resize: for each source pixel the output pixels whose taps name it, rows then columns ascending.
 *   grad_kernel_maps (host, [L])   (may be NULL; then the feature is not read) device maps in the layout of kernel_maps:
 *                                  grad_kernel(i,e) = sum_p g(i,p) * resized feat[b,e,p] as per-tile partial sums reduced in a fixed
 *                                  order; EVERY element of every map is written, zero for a cell no row names.
 * No memset, no float atomics, run-to-run bit-identical, no host synchronisation.  With both gradients NULL the call checks its
 * arguments and returns.  N == 0 writes all-zero gradients and touches nothing else (no workspace is needed).  Checks as the
 * forward's, then grad_out NULL (N > 0) or a NULL grad map: BXI_ERR_NULL_POINTER; workspace as the forward's while N > 0. */
int bxi_solo_dconvl_backward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids,
                                 const int* level_sizes, int L, const int64_t* cells, const int* seg_counts, int N, const float* grad_out,
                                 float* grad_feat, void* const* grad_kernel_maps, int32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
