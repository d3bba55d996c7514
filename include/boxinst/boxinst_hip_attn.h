/*
 * boxinst_hip_attn.h -- the masked cross-attention of Box2Mask's transformer decoder (mmcv's MultiheadAttention over
 * torch.nn.MultiheadAttention, called once per decoder layer with the mask that forward_head makes) in libboxinst_hip.so: the mask as
 * bits, the attention core forward and backward.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   box2mask_head.py = mmdet/models/dense_heads/box2mask_head.py  (:346-355 the mask of forward_head, :397 its repair in forward)
 *
 * All data is fp32.  Layouts are those F.linear leaves with batch_first=False:  q [Q, B, M * D],  k and v [S, B, M * D],  out [Q, B, M * D],
 * contiguous, head m in columns m * D .. m * D + D - 1;  lse [B, M, Q].  The arithmetic is torch.nn.MultiheadAttention's with a bool mask:
 * score(q, s) = sum_d (q[q, d] * scale) * k[s, d] (q scaled FIRST, as torch does), -inf where the mask is set, softmax over s, times v.
 *
 * THE MASK IS BITS.  bits [R, Q, words] as 32-bit words, words = ceil(S / 32); bit (s & 31) of word (s >> 5) set = key s is masked for that
 * query; the tail bits of the last word are clear.  R = B (bits_per_head = 0: one mask per image, shared by its M heads -- DEVIATION: the
 * reference repeats the mask over the heads, box2mask_head.py:352) or R = B * M (bits_per_head = 1, row b * M + m).  bits = NULL: no mask.
 *
 * DEVIATION (bxi_attn_mask_bits_f32): the reference masks where sigmoid(v) < 0.5.  In fp32 that is false for v in about (-1.2e-7, 0),
 * where the sigmoid rounds to 0.5; the kernel decides v < 0.
 *
 * Parallelisation and reproducibility.  The keys are cut into spans of BXI_ATTN_SPAN: a function of S alone, so the order of every sum
 * depends on (Q, S, D) only.  One workgroup per (b, m, span) streams its K and V rows through LDS (forward) or registers (backward) once;
 * the products run on v_mfma_f32_32x32x2_f32 (exact fp32 inputs, every element one fmaf chain: keys ascending in P V and dQ, queries
 * ascending in dK and dV, d ascending in the scores).  The forward writes per span (max, sum, acc [Q, D]) and a second launch combines the
 * spans in span order; the backward recomputes the probabilities from lse, finishes dk and dv of its span and writes its share of dq,
 * which a last launch adds in span order.  No float atomics, no memset, every element of every output written; run-to-run bit-identical.
 * Nothing of size B * M * Q * S is ever stored.
 *
 * A span in which a row has no unmasked key contributes (-inf, 0, 0).  A row with no unmasked key at all (only bxi_attn_pack_mask_u8 can
 * make one) gives NaN in out and lse, as torch does.
 *
 * Support set: D in {16, 32, 64}; anything else is BXI_ERR_UNSUPPORTED.  1 <= Q <= BXI_ATTN_MAX_Q, 1 <= S <= BXI_ATTN_MAX_S,
 * 1 <= B * M <= BXI_ATTN_MAX_HEADS, every tensor below 2^31 elements; otherwise BXI_ERR_BAD_SHAPE.  With Q > 128 the forward reads K and V
 * once per 128 queries.
 */
#ifndef BOXINST_HIP_ATTN_H
#define BOXINST_HIP_ATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_ATTN_SPAN 256          /* keys per span */
#define BXI_ATTN_MAX_Q 1048576     /* 2^20 */
#define BXI_ATTN_MAX_S 16777216    /* 2^24 */
#define BXI_ATTN_MAX_HEADS 65535   /* B * M */

/* bxi_attn_mask_bits_f32  <->  box2mask_head.py:346-355 and :397, ONE launch, one workgroup per (b, q) row.
 *   mask_pred [B, Q, H, W] is resized to (h, w) bilinearly (align_corners=False, torch's upsample_bilinear2d source index: scale = in / out
 *   in fp32, src = max(scale * (dst + 0.5) - 0.5, 0), any scale), position s = y * w + x, bit s set iff the value is < 0.  A row whose h * w
 *   bits are all set is written as all clear (the repair of :397).  bits [B, Q, ceil(h * w / 32)]: every word written, tail bits clear. */
int bxi_attn_mask_bits_f32(const float* mask_pred, int B, int Q, int H, int W, int h, int w, uint32_t* bits, void* stream);

/* bxi_attn_pack_mask_u8: an existing bool mask [rows, S] (one byte per element, non-zero = masked; rows = R * Q) as bits [rows, ceil(S / 32)].
 *   ONE launch.  A row that is all set stays all set. */
int bxi_attn_pack_mask_u8(const uint8_t* mask, int rows, int S, uint32_t* bits, void* stream);

/* Bytes of `workspace` of the forward: the spans' (max, sum, acc), ceil(S / BXI_ATTN_SPAN) * B * M * Q * (D + 2) floats; 0 for a shape
 * outside the support set.  16-byte aligned, contents undefined on entry, every byte written. */
size_t bxi_masked_attn_forward_workspace_bytes(int B, int M, int Q, int S, int D);

/* bxi_masked_attn_forward_f32: TWO launches (the spans, the combine).  out [Q, B, M * D] and lse [B, M, Q] (max + log sum of the scores of
 *   the row): every element written. */
int bxi_masked_attn_forward_f32(const float* q, const float* k, const float* v, const uint32_t* bits, int bits_per_head, int B, int M, int Q,
                                int S, int D, float scale, float* out, float* lse, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of `workspace` of the backward: delta [B, M, Q] and the spans' shares of dq, ceil(S / BXI_ATTN_SPAN) * B * M * Q * D floats; 0 for
 * a shape outside the support set.  16-byte aligned, contents undefined on entry, every byte written. */
size_t bxi_masked_attn_backward_workspace_bytes(int B, int M, int Q, int S, int D);

/* bxi_masked_attn_backward_f32: THREE launches (delta = sum_d dout * out per row; per (b, m, span) dk and dv of the span and its share of
 *   dq; the sum of the shares in span order, times scale).  dout and out [Q, B, M * D], lse [B, M, Q] as the forward wrote them; dq, dk, dv
 *   in the layouts of q, k, v: every element written. */
int bxi_masked_attn_backward_f32(const float* dout, const float* q, const float* k, const float* v, const uint32_t* bits, int bits_per_head,
                                 const float* out, const float* lse, int B, int M, int Q, int S, int D, float scale, float* dq, float* dk,
                                 float* dv, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
