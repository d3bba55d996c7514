/*
 * boxinst_hip_msda.h -- multi-scale deformable attention (the sampling core of mmcv's MultiScaleDeformableAttention, the self-attention
 * of every layer of Box2Mask's MSDeformAttnPixelDecoder) in libboxinst_hip.so, forward and backward.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises or reads a device value on the host.  Paths are relative to the upstream checkout of the reference
 * (LiWentomng/BoxInstSeg):
 *   msdeformattn_pixel_decoder.py = mmdet/models/plugins/msdeformattn_pixel_decoder.py  (:48-67 six layers, num_heads=8, num_levels=3,
 *                                   num_points=4; every config under configs/box2mask, :41-46)
 *
 * The op is mmcv's (mmcv.ops.multi_scale_deform_attn), which is not part of the reference tree.  Its arithmetic is RESTATED here from its
 * documented algorithm and is UNPINNED: mmcv never ran next to this library.  All data is fp32.
 *
 * Tensors (mmcv's layouts):  value [B, S, M, D] with S = sum_l H_l * W_l;  spatial_shapes [L, 2] int64 as (H, W) and level_start_index [L]
 * int64, both ON THE DEVICE;  out [B, Q, M * D];  Q is independent of S.  Two input forms, one code path:
 *   plain  (flags = 0)              a = sampling_locations [B, Q, M, L, P, 2] as (x, y) in [0, 1] coordinates, offsets = NULL,
 *                                   w = attention_weights [B, Q, M, L, P], any real values.
 *   fused  (flags = BXI_MSDA_FUSED) a = reference_points [B, Q, L, 2], offsets = raw sampling_offsets [B, Q, M, L, P, 2], w = raw attention
 *                                   logits [B, Q, M, L * P].  The kernel forms loc = ref + off / (W_l, H_l) -- x by the WIDTH, y by the
 *                                   height -- and the softmax exp(w - max) / sum over the L * P logits of one (b, q, m); neither the
 *                                   locations nor the weights are stored anywhere.
 * One sample of level l at (x, y):  h = y * H - 0.5, w = x * W - 0.5;  it counts only if h > -1 and w > -1 and h < H and w < W (strict; a
 * NaN or an infinity fails and contributes nothing, with zero gradients);  h_low = floor(h), h_high = h_low + 1, lh = h - h_low, hh = 1 - lh,
 * w likewise;  the value is hh hw v(h_low, w_low) + hh lw v(h_low, w_high) + lh hw v(h_high, w_low) + lh lw v(h_high, w_high), a corner
 * outside the map contributing nothing;  out[b, q, m, :] = sum over (l, p) of weight * value.  This is F.grid_sample(bilinear, zeros,
 * align_corners=False) except for the gradient w.r.t. the location ON the lines h = -1, w = -1: zero here (the sample does not count).
 *
 * The kernels bound every cell index by the level's range and the level's range by S (a level with H or W < 1, a negative start or
 * start + H * W > S contributes nothing), so inconsistent shape tensors cannot reach outside `value`.
 *
 * Support set: D a power of two in [BXI_MSDA_MIN_HEAD_DIM, BXI_MSDA_MAX_HEAD_DIM], 1 <= L <= BXI_MSDA_MAX_LEVELS,
 * 1 <= P <= BXI_MSDA_MAX_POINTS; anything else is BXI_ERR_UNSUPPORTED.  Every tensor below 2^31 elements.
 *
 * Reproducibility: no float atomics anywhere.  The per-query gradients are complete sums inside the lanes that own one (b, q, m).
 * grad_value, a scatter, is accumulated in FIXED POINT: with Mx = max|grad_out| * max|weight| (reduced on the device; the weight maximum is
 * 1 in the fused form) every contribution grad_out * weight * corner weight, |.| <= Mx, is multiplied by 2^40 / Mx in fp64, rounded to the
 * nearest integer and added with 64-bit INTEGER atomics, whose sums do not depend on the order; a last pass converts to fp32 and writes
 * every element.  Run-to-run results are bit-identical.
 *   overflow:      a cell that receives n contributions holds at most n * (2^40 + 1/2) in magnitude: no overflow of the int64 while
 *                  n < 2^22 (there is a factor two to spare).  A sample reaches a cell at most once, and a cell belongs to one level, so
 *                  n <= Q * P; the library asks for the plainer Q * L * P < BXI_MSDA_MAX_CELL_SAMPLES and answers beyond it with 0 bytes /
 *                  BXI_ERR_UNSUPPORTED.
 *   quantisation:  at most 2^-41 * Mx per contribution (the derivation of the tolerance is next to the code, csrc/msda.hip).
 *   non-finite:    a NaN or an infinity in grad_out (or in the plain form's weights) makes Mx non-finite: every element of grad_value is
 *                  then NaN.  A non-finite weight of the fused form (a NaN logit) contributes nothing to grad_value.
 */
#ifndef BOXINST_HIP_MSDA_H
#define BOXINST_HIP_MSDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_MSDA_MAX_LEVELS 8
#define BXI_MSDA_MAX_POINTS 8
#define BXI_MSDA_MIN_HEAD_DIM 8
#define BXI_MSDA_MAX_HEAD_DIM 64
#define BXI_MSDA_FUSED 1                   /* `flags`: reference points, raw offsets and raw logits instead of locations and weights */
#define BXI_MSDA_MAX_CELL_SAMPLES 4194304  /* 2^22: the backward takes Q * L * P below this */

/* bxi_msda_forward_f32  <->  MultiScaleDeformableAttnFunction.forward (and, fused, the offset normaliser and the softmax in front of it),
 *   ONE launch: the lanes of a wave over the D channels of one (b, q, m), 64 / D of them per wave; a corner read is one contiguous
 *   D * 4-byte segment, the output of a wave 256 contiguous bytes.  out [B, Q, M * D]: every element written.
 * B == 0 or Q == 0 is a no-op.  Negative sizes, M < 1, a tensor of 2^31 elements or more: BXI_ERR_BAD_SHAPE; unknown flags:
 * BXI_ERR_BAD_ARGUMENT; outside the support set: BXI_ERR_UNSUPPORTED. */
int bxi_msda_forward_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const float* a,
                         const float* offsets, const float* w, int B, int S, int M, int D, int Q, int L, int P, int flags, float* out,
                         void* stream);

/* Bytes of `workspace` of the backward (0 for a bad or unsupported shape or Q * L * P >= BXI_MSDA_MAX_CELL_SAMPLES; at least 16): the
 * partial maxima of the Mx reduction and the int64 accumulator [B, S, M, D].  16-byte aligned, contents undefined on entry. */
size_t bxi_msda_backward_workspace_bytes(int B, int S, int M, int D, int Q, int L, int P);

/* bxi_msda_backward_f32  <->  MultiScaleDeformableAttnFunction.backward, THREE launches: (1) zero the accumulator and reduce the two
 *   maxima, (2) per (b, q, m) the complete per-query gradients (a wave reduction over D) and the fixed-point scatter, (3) the
 *   accumulator to fp32.  grad_out [B, Q, M * D].
 *   grad_value [B, S, M, D]: EVERY element written, zeros where no sample reaches (also with Q == 0).
 *   grad_a: plain grad_sampling_locations [B, Q, M, L, P, 2]; fused grad of the raw offsets, same shape (reference_points get none).
 *   grad_w: plain grad_attention_weights [B, Q, M, L, P]; fused grad of the raw logits, the softmax backward over the L * P values.
 *   Every element of both is written. */
int bxi_msda_backward_f32(const float* grad_out, const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                          const float* a, const float* offsets, const float* w, int B, int S, int M, int D, int Q, int L, int P, int flags,
                          float* grad_value, float* grad_a, float* grad_w, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
