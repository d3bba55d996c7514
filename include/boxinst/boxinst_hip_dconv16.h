/*
 * boxinst_hip_dconv16.h -- the dynamic 1x1 mask convolution of the SOLOv2-style heads (DiscoBox) on fp16 / bf16 tensors read in place:
 * the half-precision sibling of boxinst_hip_dconv.h, forward and backward.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h; rows, segments,
 * layouts (BXI_DCONV_MAPS / BXI_DCONV_ROWS), activations, limits and the BXI_DCONV_STATUS_BAD_CELL rule are those of boxinst_hip_dconv.h
 * (included below), which also names the reference's statements.  The reference runs those statements under fp16 autocast
 * (`fp16 = dict(loss_scale=512.)`, @autocast() on loss / corr_loss / get_seg_single): this family is that precision in HIP.  No entry
 * point synchronises or reads a device value on the host; no memset, no float atomics; run-to-run bit-identical; hipGraph capturable.
 *
 * Types.  `dtype` (BXI_DCONV16_F16 or BXI_DCONV16_BF16) is the type of the feature, of every kernel map and of both gradients
 * (grad_feat, grad_kernel_maps).  `out_dtype` is the same code as `dtype`, or BXI_DCONV16_OUT_F32: the type of `out`, of the saved `out`
 * the backward reads and of `grad_out`.  Every tensor needs the alignment of its element only (2 bytes for the half types).
 *
 * Arithmetic.  All three products run on v_mfma_f32_32x32x16_f16 / _bf16: operands in the half type, products exact, sums in fp32.
 *   - What holds: every output element is the sum of its own E (rows, pixels) exact products, accumulated in fp32 from +0, 16 values of
 *     k per instruction in ascending blocks of 16; k is padded with zeros on BOTH operands (E up to a multiple of 16, a chunk's missing
 *     rows, a tile's missing pixels).  The order is fixed by the shape alone, so results are bit-identical from run to run.  Where every
 *     partial sum is exactly representable in fp32 (integers below 2^24), the result is exact whatever the order.
 *   - What does not hold: the sum is no longer ONE k-ordered fmaf chain.  Inside an instruction the 16 products are added in an order and
 *     with intermediate roundings the ISA does not state, so a result may differ in its last bits from any fmaf chain and from the fp32
 *     family on the same values.  Bounds belong against the error of a half-precision reference, not against bit patterns.
 *   - A row still depends only on its own kernel values and its image's feature: not on the other rows, not on its position in its
 *     chunk, its image's slot or the layout (an output element is its A row times its B column; a NaN stays in its row / its pixel).
 *   - fp16 subnormal operands are multiplied at their value.  Per the ISA's MFMA notes the C input and the D output of an MFMA never
 *     flush, and the A / B inputs honour the wave's MODE denormal fields like VALU operations do; the library's kernels run in hipcc's
 *     default mode, which keeps denormals (float_denorm_mode_32 = 3 and float_denorm_mode_16_64 = 3 in every kernel descriptor; the
 *     build does not pass -fgpu-flush-denormals-to-zero).  Measured on an MI355X and pinned by tests/test_gpu_solo_conv16.py:
 *     2^-24 * 2^10 = 2^-14 and 2^-24 * 2^-24 = 2^-48, on either operand.  A bf16 subnormal is an fp32 subnormal and is kept alike.
 *   - act = 1 / (1 + expf(-x)) in fp32, then ONE rounding to nearest even to `out_dtype`; overflow to +-inf and NaN as torch's cast from
 *     fp32 gives them (a bf16 NaN is 0x7FC0).
 *   - Backward: g = grad_out (* out * (1 - out) with BXI_DCONV_SIGMOID) is formed in fp32 from the saved output and rounded ONCE to
 *     `dtype`, because it is an MFMA operand -- where the reference's fp16 autograd has it too (its sigmoid backward returns fp16 to the
 *     convolution's backward).  A g beyond the half type's range rounds to +-inf: the loss scale is the caller's.
 */
#ifndef BOXINST_HIP_DCONV16_H
#define BOXINST_HIP_DCONV16_H

#include "boxinst_hip_dconv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_DCONV16_F16 0
#define BXI_DCONV16_BF16 1
#define BXI_DCONV16_OUT_F32 2
#define BXI_DCONV16_TILE 64            /* pixels per tile, forward and backward, for every E: 64 x (1024 + 8) halves = 129 KiB of LDS */

/* Bytes of `workspace` of the forward: the gathered kernel values as the A fragments of the 32x32x16 MFMA, (N / 32 + B) chunks of 32
 * rows x (E rounded up to a multiple of 16) x 2 bytes -- per chunk and k step of 16, lane l's 16 bytes are A[row l & 31][k = 8 (l >> 5)
 * + j], j = 0..7.  Monotone in N; 0 for N == 0 and for sizes the entry point refuses.  16-byte aligned, contents undefined on entry,
 * every byte written by the call (zeros where a chunk has no row, for the tail of E and for a cell outside its map). */
size_t bxi_solo_dconv16_forward_workspace_bytes(int N, int B, int E);

/* out[i, p] = act( sum_e kernel(i, e) * feat[image_i, e, p] ), TWO launches: the gather, then the product.
 *   feat [B,E,H,W] and the maps in `dtype`; out [N,H,W] in `out_dtype`, every element written once; img_inds (may be NULL) int64 [N].
 *   A workgroup owns a tile of 64 pixels of one image, stages its E feature values in LDS once (pixel-major, so that a lane's eight k
 *   values are one 16-byte read) and walks the image's rows in chunks of 32: rows on A, pixels on the lanes of B and C.  An image without
 *   rows reads nothing.  A feature whose base is 16-byte aligned with H*W a multiple of 8 is read in 16-byte pieces; any other is read
 *   per feature row in the 16-byte pieces that lie whole inside the tile and by elements at the row's head and tail.
 * N == 0 returns BXI_OK and touches nothing.  Checked before anything touches a device, in the order of bxi_solo_dconv_forward_f32:
 * NULL kernel_maps / grids / seg_counts: BXI_ERR_NULL_POINTER; the shape limits: BXI_ERR_BAD_SHAPE; an unknown layout or activation:
 * BXI_ERR_BAD_ARGUMENT; BXI_DCONV_ROWS with L != 1 or B != 1, a bad grid or count: BXI_ERR_BAD_SHAPE; then an unknown `dtype`, or an
 * `out_dtype` that is neither `dtype` nor BXI_DCONV16_OUT_F32: BXI_ERR_BAD_ARGUMENT; then (N > 0) a NULL feat, map, out, status, or
 * cells with BXI_DCONV_MAPS: BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_solo_dconv16_forward(const void* feat, int dtype, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                             int layout, const int64_t* cells, const int* seg_counts, int N, int activation, void* out, int out_dtype,
                             int64_t* img_inds, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of `workspace` of the backward: the gathered kernel values ((N / 32 + B) chunks x (E rounded up to 16) x 32 rows x 2 bytes, here
 * with a channel's 32 rows side by side: the A fragments of grad_feat's product), then N*E fp32 partial sums per tile of BXI_DCONV16_TILE
 * pixels of ONE image and the N*E reduced fp32 sums.  Monotone in N and in the tiles; 0 for N == 0 and for sizes the entry point refuses.
 * 16-byte aligned, contents undefined on entry, every byte written by a call that has gradient maps. */
size_t bxi_solo_dconv16_backward_workspace_bytes(int N, int B, int E, int H, int W);

/* The forward's inputs, its saved `out` and grad_out [N,H,W] (both `out_dtype`)  ->  g (see Arithmetic), and
 *   grad_feat [B,E,H,W] `dtype`    grad_feat[b,e,p] = sum_{i in b} kernel(i,e) * g(i,p): k = the image's rows, padded to 16; fp32 sums
 *                                  rounded once; EVERY element written, zeros for an image without rows.  May be NULL.
 *   grad_kernel_maps (host, [L])   device maps in `dtype` and the layout of kernel_maps; grad_kernel(i,e) = sum_p g(i,p) * feat[b,e,p]:
 *                                  k = the tile's pixels; fp32 per-tile partial sums in the workspace, reduced in fp32 in a fixed order;
 *                                  a last pass writes EVERY element of every map: zero for a cell no row names, and for a cell named more
 *                                  than once the fp32 sum of its rows' gradients in row order, rounded once.  May be NULL (then the
 *                                  feature is not read).
 * Up to four launches (the gather, the two products in one kernel, the reduction, the pass over the maps).  With both gradients NULL the
 * call checks its arguments and returns.  N == 0 writes all-zero gradients.  Checks as the forward's, then grad_out / out NULL (N > 0) or
 * a NULL grad map: BXI_ERR_NULL_POINTER; workspace NULL / too small / not 16-byte aligned while N > 0: BXI_ERR_WORKSPACE. */
int bxi_solo_dconv16_backward(const void* feat, int dtype, int B, int E, int H, int W, const void* const* kernel_maps, const int* grids, int L,
                              int layout, const int64_t* cells, const int* seg_counts, int N, int activation, const void* out,
                              const void* grad_out, int out_dtype, void* grad_feat, void* const* grad_kernel_maps, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
