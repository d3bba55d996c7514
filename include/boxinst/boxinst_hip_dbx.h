/*
 * boxinst_hip_dbx.h -- the pseudo-label block of DiscoBoxSOLOv2Head.loss for the assigned rows of ALL levels in libboxinst_hip.so: target,
 * enlarged target and initial state as bit words, the mean-field iterations of both legs (without / with inter_img_mask) in one launch
 * per iteration, the two dice terms from the words, and the means over the live rows.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises, reads a device value on the host, calls memset or uses a float atomic; every sum has a fixed order, so
 * two runs are bit-identical; every output element and every workspace word that is read later is written first.  Paths are relative to
 * the upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   head.py = mmdet/models/dense_heads/discobox_head.py   (loss :1271-1306, :1335-1339; the tail of corr_loss :1127-1137;
 *                                                          MeanField :585-655, dice_loss :542-550)
 *
 * ROWS.  A row is one assigned (level, image, cell), level-major as bxi_solo_dconv_forward_f32 writes them: s_rows / t_rows [R,H,W] fp32
 * (the student's and the teacher's sigmoid masks; they may be the same buffer), target_rows [R,H,W] uint8 (0 / 1: any non-zero byte marks the target, and the
 * initial state multiplies by the byte's value, as the reference's x * targets and bxi_meanfield_forward_f32 do), img_inds [R]
 * int64.  A row whose target plane is all zero is not live (head.py:1281-1286, decided on the device): it stays in place, its labels are
 * empty, its gradient is zero and the means skip it.
 * LEGS.  legs = 1: leg 0 alone, MeanField.forward without inter_img_mask (head.py:1298).  legs = 2: also leg 1, with it (head.py:1132).
 * WORKSPACE.  bxi_dbx_workspace_bytes(R, H, W, legs) bytes, 8-byte aligned, contents undefined before bxi_dbx_prepare_f32 and opaque
 * afterwards; the same block, R, H, W and legs go to every later call, `iters` to the calls behind bxi_dbx_steps_f32.
 * Common support set: fp32, R <= 65535, R H W within int32; legs other than 1 / 2: BXI_ERR_BAD_ARGUMENT; R > 65535:
 * BXI_ERR_UNSUPPORTED; R == 0 is a no-op; workspace NULL, too small or misaligned: BXI_ERR_WORKSPACE.  Nothing is launched on an error.
 */
#ifndef BOXINST_HIP_DBX_H
#define BOXINST_HIP_DBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_DBX_MAX_LEVELS 8   /* levels (iiu tensors) per call of bxi_dbx_steps_f32 */
#define BXI_DBX_MAX_MEANS 4    /* per-row arrays per call of bxi_dbx_means_f32 */

/* Bytes of the workspace (0 for a shape the entry points refuse). */
size_t bxi_dbx_workspace_bytes(int R, int H, int W, int legs);

/* Target words (target != 0), enlarged-target words (F.max_pool2d(target.float(), 3, 1, 1), head.py:1294, as a 3x3 dilation of the
 * bits, clipped to the map), the initial state ((t + s) / 2 * target > 0.5, head.py:1299 into :621-622; the same for both legs) in one
 * launch, a wave per (row, line, 64-column segment) items; then live [R] int32 (1: the row has a target pixel) and n_live [1] int32 by
 * ONE workgroup from the target words (no atomics). */
int bxi_dbx_prepare_f32(const float* s_rows, const float* t_rows, const uint8_t* target_rows, int R, int H, int W, int legs,
                        int32_t* live, int32_t* n_live, void* workspace, size_t workspace_bytes, void* stream);

/* `iters` mean-field iterations of every leg, ONE launch per iteration: the affinities kernel [B,ksize*ksize,H,W] (bxi_meanfield_kernel_f32)
 * of a pixel and its target word are loaded once, each leg has its own pair of state buffers and runs the device function that
 * bxi_meanfield_forward_f32 runs, so its labels are that entry point's, bit for bit.
 *   legs == 2: iiu_levels_host [n_levels]: HOST array of device pointers, level l's [N_l,2,H,W] inter_img_mask or NULL (then leg 1 adds
 *   nothing for that level's rows: what zeros add); level_first_host [n_levels]: HOST array, the first row of level l (ascending,
 *   level_first_host[0] == 0; level l ends where level l + 1 starts, the last one at R).  legs == 1: both are ignored.
 * ksize other than 3 / 5 or n_levels > BXI_DBX_MAX_LEVELS: BXI_ERR_UNSUPPORTED; base outside (0, 0.5) or a bad level table:
 * BXI_ERR_BAD_ARGUMENT. */
int bxi_dbx_steps_f32(const float* kernel, int B, int H, int W, int ksize, const int64_t* img_inds, int R, int iters, float base,
                      double gamma, int legs, const float* const* iiu_levels_host, const int* level_first_host, int n_levels,
                      void* workspace, size_t workspace_bytes, void* stream);

/* dice_loss(s * enlarged, pseudo) of leg 0 (head.py:1300) and, with legs == 2, dice_loss(a1, pseudo_corr) with
 * a1 = fl(fl(a0 gamma) + fl(a0 fl32(1 - gamma))), a0 = s * enlarged (head.py:1135-1137).  s_rows is read once; e and b are bits of the
 * workspace; sum a b, sum a^2 and sum b^2 (a popcount) are fp64 partials per 16 lines combined in index order; the loss is computed in
 * fp64 and rounded once.  loss [legs,R] fp32; sums [legs,R,2] fp64 = (sum a b, sum a^2 + sum b^2 + 0.002) for the backward.  Two launches. */
int bxi_dbx_dice_forward_f32(const float* s_rows, int R, int H, int W, int legs, int iters, double gamma, void* workspace,
                             size_t workspace_bytes, float* loss, double* sums, void* stream);

/* Its backward, one launch, EVERY element of g_s [R,H,W]: e (g_rows[0,r] (-2 b0 / D0 + 4 A0 a0 / D0^2) + gamma g_rows[1,r] (-2 b1 / D1 +
 * 4 A1 a1 / D1^2)); zero where e = 0, so for every row that is not live.  g_rows [legs,R]. */
int bxi_dbx_dice_backward_f32(const float* s_rows, int R, int H, int W, int legs, int iters, double gamma, const void* workspace,
                              size_t workspace_bytes, const double* sums, const float* g_rows, float* g_s, void* stream);

/* means[k] = sum_r live[r] rows_host[k][r] / max(n_live, 1) for K <= BXI_DBX_MAX_MEANS arrays of [R] (rows_host: HOST array of device
 * pointers), fp64 in a fixed order, one workgroup.  R == 0 gives zeros. */
int bxi_dbx_means_f32(const float* const* rows_host, int K, const int32_t* live, const int32_t* n_live, int R, float* means, void* stream);

/* Its backward: g_rows [K,R] = live[r] ? g_means[k] / max(n_live, 1) : 0. */
int bxi_dbx_means_backward_f32(const float* g_means, int K, const int32_t* live, const int32_t* n_live, int R, float* g_rows, void* stream);

/* A word plane as uint8 [R,H,W] (for details= and the tests): which = 0 target, 1 enlarged target, 2 + g the pseudo-label of leg g after
 * `iters` iterations.  which outside 0 .. 1 + legs: BXI_ERR_BAD_ARGUMENT. */
int bxi_dbx_unpack_u8(const void* workspace, size_t workspace_bytes, int which, int iters, int R, int H, int W, int legs, uint8_t* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
