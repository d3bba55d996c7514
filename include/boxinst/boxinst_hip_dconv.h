/*
 * boxinst_hip_dconv.h -- the dynamic 1x1 mask convolution of the SOLOv2-style heads (DiscoBox) in libboxinst_hip.so: the mask feature
 * times the kernels of the assigned grid cells (training) or of the candidate rows (test time), and the sigmoid after it; forward and
 * backward.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   discobox_head.py = mmdet/models/dense_heads/discobox_head.py
 *     :1180-1246  loss: kernel_pred.view(E, -1)[:, grid_order], one F.conv2d(ins_pred[idx], kernel) per (level, image), the cats
 *     :1275-1279  the sigmoid of a level's masks           :936-1000, :1018-1022  the same block in corr_loss
 *     :1607-1608  get_seg_single: F.conv2d(seg_preds, kernel_preds.view(I, N, 1, 1)).squeeze(0).sigmoid()
 *
 * DEVIATION: this family is fp32.  The reference runs these statements under fp16 autocast; here every operand is fp32, every logit is
 * ONE fp32 chain fma(k(i,E-1), f(E-1,p), ... fma(k(i,0), f(0,p), 0)) over e = 0 .. E-1 in ascending order (v_mfma_f32_32x32x2_f32, bit
 * for bit a k-ordered fmaf chain), and the result is fp32.  The reference's own precision -- fp16 or bf16 tensors read in place, fp32
 * accumulation -- is the sibling family of boxinst_hip_dconv16.h.
 *
 * Rows and segments.  The N output rows are ordered as the reference concatenates them: level-major, inside a level image by image,
 * inside an image in grid_order's order.  `seg_counts` (HOST, [L*B], index l*B + b) holds the number of rows of every (level, image)
 * segment and sums to N; `cells` (DEVICE, int64 [N]) holds the cell of every row inside its map (a grid_order entry in [0, S_l^2), or a
 * row of the test-time matrix; repeats allowed).  The record of row i is therefore (image, level, cell) = (its segment's b, its segment's
 * l, cells[i]).  The kernel values are gathered by the library, in a small launch of its own, into the workspace (per chunk of 32 rows of an image the values of
 * four k steps of a row side by side, zeros where a chunk has no row): the caller makes no [N,E] copy.
 *   layout BXI_DCONV_MAPS  kernel_maps[l] is the head's output [B,E,S_l,S_l] of level l, read in place; grids[l] = S_l.
 *   layout BXI_DCONV_ROWS  L = 1, B = 1, kernel_maps[0] is one row-major [rows,E] matrix, grids[0] = rows; cells may be NULL (row i is
 *                          matrix row i).
 * A cell outside its map is never read: the row is that of an all-zero kernel, it contributes no gradient, and status[0] is set to
 * BXI_DCONV_STATUS_BAD_CELL (a plain store; the caller zeroes status[0] before the call and reads it when it likes).
 */
#ifndef BOXINST_HIP_DCONV_H
#define BOXINST_HIP_DCONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_DCONV_MAPS 0
#define BXI_DCONV_ROWS 1
#define BXI_DCONV_NONE 0
#define BXI_DCONV_SIGMOID 1
#define BXI_DCONV_MAX_LEVELS 8
#define BXI_DCONV_MAX_E 1024
#define BXI_DCONV_TILE 64              /* pixels per backward tile: the unit of the workspace's partial sums */
#define BXI_DCONV_STATUS_BAD_CELL 1

/* Bytes of `workspace` of bxi_solo_dconv_forward_f32: the gathered kernel values, (N / 32 + B) chunks of 32 rows x (E rounded up to a
 * multiple of 8) floats.  Monotone in N; 0 for N == 0 and for sizes the entry point refuses.  16-byte aligned, contents undefined on entry, every byte
 * written by the call. */
size_t bxi_solo_dconv_forward_workspace_bytes(int N, int B, int E);

/* bxi_solo_dconv_forward_f32: out[i, p] = act( sum_e kernel(i, e) * feat[image_i, e, p] ), TWO launches: the gather, then the product.
 *   feat [B,E,H,W] fp32; out [N,H,W] fp32, every element written once; img_inds (may be NULL) int64 [N], the image of every row.
 *   A workgroup owns a tile of 64 pixels (32 for E > 512) of one image, holds its E feature values in LDS and walks the image's rows in
 *   chunks of 32: the feature of an image is read once per call, and not at all for an image without rows.  A chunk's missing rows and
 *   the tail of E up to a multiple of 8 are zeros on both operands.  A row's values depend on its kernel values and its image's feature only -- not on the
 *   other rows, its position, or the layout.  sigmoid is 1 / (1 + expf(-x)).
 * N == 0 returns BXI_OK and touches nothing.  Checked before anything touches a device, in this order: NULL kernel_maps / grids /
 * seg_counts: BXI_ERR_NULL_POINTER; B outside [1, BXI_MAX_IMAGES], L outside [1, 8], E outside [1, 1024], H or W < 1, N < 0,
 * B*E*H*W or N*H*W >= 2^31, a grid < 1, a map of 2^31 elements or more, a negative count, counts that do not sum to N, BXI_DCONV_ROWS
 * with L != 1 or B != 1: BXI_ERR_BAD_SHAPE; an unknown layout or activation: BXI_ERR_BAD_ARGUMENT; then (N > 0) a NULL feat, map, out,
 * status, or cells with BXI_DCONV_MAPS: BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_solo_dconv_forward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                               int layout, const int64_t* cells, const int* seg_counts, int N, int activation, float* out,
                               int64_t* img_inds, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of `workspace` of bxi_solo_dconv_backward_f32: the forward's gathered kernel values, then N*E partial sums per tile of
 * BXI_DCONV_TILE pixels of ONE image and the N*E reduced sums, 4 bytes each.  Monotone in N and in the tiles; 0 for N == 0 and for sizes
 * the entry point refuses.  16-byte aligned, contents undefined on entry, every byte written by a call that has gradient maps. */
size_t bxi_solo_dconv_backward_workspace_bytes(int N, int B, int E, int H, int W);

/* bxi_solo_dconv_backward_f32: the forward's inputs, its saved `out` and grad_out [N,H,W]  ->  g = grad_out (* out * (1 - out) with
 * BXI_DCONV_SIGMOID, formed in the kernel), and
 *   grad_feat [B,E,H,W]            grad_feat[b,e,p] = sum_{i in b} kernel(i,e) * g(i,p), rows in ascending order; EVERY element written,
 *                                  zeros for an image without rows.  May be NULL.
 *   grad_kernel_maps (host, [L])   device maps in the layout of kernel_maps; grad_kernel(i,e) = sum_p g(i,p) * feat[b,e,p] as per-tile
 *                                  partial sums in the workspace, reduced in a fixed order; a last pass writes EVERY element of every
 *                                  map: zero for a cell no row names, and for a cell named more than once the sum of its rows' gradients
 *                                  in row order.  May be NULL (then the feature is not read).
 * Up to four launches (the gather, the two products in one kernel, the reduction, the pass over the maps); no memset, no float atomics, run-to-run bit-identical, no host synchronisation.  With both gradients NULL the
 * call checks its arguments and returns.  N == 0 writes all-zero gradients.  Checks as the forward's, then grad_out / out NULL (N > 0) or
 * a NULL grad map: BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned while N > 0: BXI_ERR_WORKSPACE. */
int bxi_solo_dconv_backward_f32(const float* feat, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                                int layout, const int64_t* cells, const int* seg_counts, int N, int activation, const float* out,
                                const float* grad_out, float* grad_feat, void* const* grad_kernel_maps, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
