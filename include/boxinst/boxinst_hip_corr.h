/*
 * boxinst_hip_corr.h -- DiscoBox's cross-image correspondence in libboxinst_hip.so: the object bank, the retrieval of similar objects
 * with the reference loop's order kept, the correspondence solver, loss_corr with its gradient, the inter-image mask `iiu` that
 * MeanField.forward takes, and the append.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * Paths are relative to the upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   discobox_head.py = mmdet/models/dense_heads/discobox_head.py  (ObjectQueues :132-227, SemanticCorrSolver.pass_message / solve
 *                      :349-411, superres_T :851-865, the object loop of corr_loss :1056-1127)
 *
 * Fixed sizes: features are 7 x 7 (BXI_CORR_FEAT), masks 28 x 28 (BXI_CORR_MASK), as in all four configs/discobox.  All data is fp32;
 * sums run in a fixed order (reductions are kept in fp64 and rounded once), there are no float atomics: results are run-to-run identical.
 *
 * The bank: feature [num_class, L, C, 7, 7], mask [num_class, L, 28, 28], box [num_class, L, 4] fp32 and ptr [num_class] int32, zeros
 * before the first append.  A zero slot fails the predicates through 0/0 and x/0: NaN and inf fail every comparison, as in torch.
 *
 * The objects of one call (one level): N rows of s_feat / t_feat [N, C, 7, 7] (student / teacher, after relu_and_l2_norm_feat),
 * s_mask / t_mask [N, 28, 28], boxes [N, 4] (x1, y1, x2, y2: integer-valued floats, the box of the target mask), labels [N] int64.
 * An object whose label is outside [0, num_class) retrieves nothing and is never appended.
 *
 * Lists of retrieved objects have K = max_objs (<= BXI_CORR_MAX_OBJS) entries per object: ret_slot [N, K] the bank slot or -1,
 * ret_src [N, K] the EARLIER OBJECT OF THIS CALL whose teacher entry the slot shows, or -1 for the stored entry, count [N].
 *
 * Deviations from the reference: every bank lives on the device (the reference moves banks past num_gpu_bank to the host; no numerical
 * effect); the double relu_and_l2_norm_feat of the very first query of a run (ObjectFactory.create_one :40) is not reproduced; the
 * image crops (save_corr_img, vis_corr, vis_seg) are not built; a box that leaves the canvas is clipped where the reference raises.
 */
#ifndef BOXINST_HIP_CORR_H
#define BOXINST_HIP_CORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_CORR_FEAT 7
#define BXI_CORR_MASK 28
#define BXI_CORR_MAX_OBJS 8          /* largest max_retrieval_objs (the configs use 5) */
#define BXI_CORR_MAX_QUEUE 1024      /* largest len_object_queues (the configs use 100) */

/* Bytes of `workspace` of bxi_corr_solve_f32 / bxi_corr_loss_f32 / bxi_corr_iiu_f32 of one call (0 for a bad shape; at least 16).
 * The three carve it the same way: T [N,K,49,49] fp32, the per-(object, k) gradient parts [N,K,C,49] fp32, the class-map parts
 * [N,K,2,784] fp32 and the row-loss sums [N,K] fp64.  16-byte aligned. */
size_t bxi_corr_workspace_bytes(int N, int C, int max_objs);

/* bxi_corr_plan_f32: where the append of this call will put every object, ONE launch of one workgroup.
 *   area flag a_j = (x2 - x1 > min_size) & (y2 - y1 > min_size)  (:1056);  slot_j = (ptr[c_j] + #{i < j : c_i = c_j, a_i}) mod L.
 *   obj_slot [N] int32: slot_j, or -1 for an object that is not appended.  obj_role [N] int32: bit 0 = the LAST writer of its slot in
 *   this call (more than L objects of one class wrap around), bit 1 = the last appended object of its class (it advances ptr).
 * `ptr` is only read.  N == 0 is a no-op.  N < 0, num_class < 1, L outside 1..BXI_CORR_MAX_QUEUE: BXI_ERR_BAD_SHAPE; NaN min_size:
 * BXI_ERR_BAD_ARGUMENT. */
int bxi_corr_plan_f32(const float* boxes, const int64_t* labels, const int32_t* ptr, int N, int num_class, int L, float min_size,
                      int32_t* obj_slot, int32_t* obj_role, void* stream);

/* bxi_corr_retrieve_f32  <->  ObjectQueues.get_similar_obj for all N objects, TWO launches: one workgroup per (object, four slots), then the
 *   lists of every object.
 *   Object i sees the stored bank of its class with the appends of the earlier objects of this call applied (obj_slot as the plan wrote
 *   it): a slot shows the teacher feature, teacher mask and box of the latest j < i with c_j = c_i and obj_slot[j] = slot, else the
 *   stored entry.  The query is the STUDENT feature and mask.  Per slot, as cal_fg_iou / cal_bg_iou / cal_appear_identity_sim /
 *   cal_shape_ratio: sum(A B) / #{A + B >= 1}; sum((1-A)(1-B)) / #{2 - A - B >= 1}; sum(f0 f1 m0 m1) / (sum(m0 m1) + 1e-6) with both masks
 *   brought 28 -> 7 by the bilinear rule (the mean of the middle 2 x 2 of each 4 x 4 block); the ratio of the two w / (h + 1e-5).
 *   A slot passes with fg > fg_thresh, bg > bg_thresh, appearance > appear_thresh, ratio_lo <= ratio <= ratio_hi.
 *   slot_pass [N, L] int32: 1 where the slot passes, else 0, every element written.
 *   ret_slot / ret_src [N, max_objs]: the first max_objs passing slots in slot order, then -1; count [N]: how many (<= max_objs).
 *   scores: NULL, or [N, L, 4] fp32 (fg, bg, appearance, ratio of every slot), every element written.
 * N == 0 is a no-op.  Shapes as above, C < 1, max_objs outside 1..BXI_CORR_MAX_OBJS: BXI_ERR_BAD_SHAPE; a NaN threshold:
 * BXI_ERR_BAD_ARGUMENT. */
int bxi_corr_retrieve_f32(const float* s_feat, const float* s_mask, const float* t_feat, const float* t_mask, const float* boxes,
                          const int64_t* labels, const int32_t* obj_slot, int N, int C, const float* bank_feature, const float* bank_mask,
                          const float* bank_box, int num_class, int L, float fg_thresh, float bg_thresh, float appear_thresh, float ratio_lo,
                          float ratio_hi, int max_objs, int32_t* slot_pass, int32_t* ret_slot, int32_t* ret_src, int32_t* count, float* scores,
                          void* stream);

/* bxi_corr_solve_f32  <->  SemanticCorrSolver.solve and the loss / T steps of :1080-1090, ONE launch, one workgroup per (object, k).
 *   Runs for the objects with count >= min_objs, k < count.  Cu = (f0 / (|f0| + 1e-4))^T (f1 / (|f1| + 1e-4)) [49,49] from the student
 *   feature and retrieved object k; C = Cu * dist_mask (Chebyshev distance <= dist_kernel / 2 on the 7 x 7 grid); num_iter rounds of
 *   { num_smooth_iter x (pass_message, row normalisation + 1e-4);  C = Cu + votes, row normalisation + 1e-4 }.
 *   assign = argmax_q C (the lowest index wins a tie); p = softmax(Cu, q); the row loss is CrossEntropyLoss applied to p (a second
 *   log-softmax, :1080-1084); T = C p, row-normalised with + 1e-5.
 *   Outputs, every element written (zeros / -1 for the (object, k) that do not run): Cu_out, C_out [N,K,49,49] fp32, assign [N,K,49] int32.
 *   Into the workspace: T, the row-loss sum, and d loss_i / d s_feat[i] of this k (through both softmaxes, the cosine and the norms;
 *   loss_i is the mean over count_i * 49 rows).
 * N == 0 is a no-op.  dist_kernel even or < 1, num_iter or num_smooth_iter < 0, min_objs < 1: BXI_ERR_BAD_ARGUMENT; workspace NULL /
 * too small / not 16-byte aligned: BXI_ERR_WORKSPACE. */
int bxi_corr_solve_f32(const float* s_feat, const float* t_feat, const int64_t* labels, int N, int C, const float* bank_feature,
                       int num_class, int L, const int32_t* ret_slot, const int32_t* ret_src, const int32_t* count, int max_objs,
                       int min_objs, int dist_kernel, int num_iter, int num_smooth_iter, float* Cu_out, float* C_out, int32_t* assign,
                       void* workspace, size_t workspace_bytes, void* stream);

/* bxi_corr_loss_f32: the sums of one call, ONE launch.  loss_sum [1] fp32 = sum over the objects that ran of their loss, in object
 *   order; num_ins [1] int32 = how many ran; grad [N,C,7,7] = d loss_sum / d s_feat for a unit upstream gradient, the parts added in k
 *   order, zeros for the objects that did not run; EVERY element written.  N == 0 writes loss_sum = 0 and num_ins = 0. */
int bxi_corr_loss_f32(const int32_t* count, int N, int C, int max_objs, int min_objs, float* loss_sum, int32_t* num_ins, float* grad,
                      void* workspace, size_t workspace_bytes, void* stream);

/* bxi_corr_grad_rescale_f32: the backward step, one launch: out = unit * upstream[0] over n elements; the upstream scalar is read ON
 *   THE DEVICE.  `out` may be `unit` (in place) or must not overlap it.  n == 0 is a no-op. */
int bxi_corr_grad_rescale_f32(const float* unit, const float* upstream, int64_t n, float* out, void* stream);

/* bxi_corr_iiu_f32  <->  :1087-1106, TWO launches; the [K,784,784] super-resolved T and the two outer-product masks are never stored.
 *   superres_T is separable: the 7 -> 28 bilinear matrix (align_corners=False) on the target and on the source cells, times 49 / 784.
 *   fg_ci[P] = mean_k sum_Q Tsr_k[P,Q] [m0[P] m1_k[Q] > 0.5] clamp(m1_k[Q], 0.1, 0.9); bg_ci with (1 - m0)(1 - m1) and clamp(1 - m1);
 *   m0 = s_mask[i], m1_k = the mask of retrieved object k.  Both maps are resized to (int(y2 - y1), int(x2 - x1)) by the bilinear rule
 *   and written to iiu[i,0] (bg) and iiu[i,1] (fg) at rows int(y1).., columns int(x1)..; everything else, and the objects that did not
 *   run, is zero.  iiu [N,2,H,W]: EVERY element written.  T is read from the workspace as bxi_corr_solve_f32 left it.
 * N == 0 is a no-op.  H or W < 1, N * 2 * H * W >= 2^31: BXI_ERR_BAD_SHAPE. */
int bxi_corr_iiu_f32(const float* s_mask, const float* t_mask, const float* boxes, const int64_t* labels, int N, int C,
                     const float* bank_mask, int num_class, int L, const int32_t* ret_slot, const int32_t* ret_src, const int32_t* count,
                     int max_objs, int min_objs, int H, int W, float* iiu, void* workspace, size_t workspace_bytes, void* stream);

/* bxi_corr_append_f32  <->  ObjectQueues.append of every flagged object (:1113-1125), ONE launch: the teacher feature, teacher mask and
 *   box of every object with bit 0 of obj_role go to slot obj_slot of its class; the object with bit 1 sets ptr[c] = (slot + 1) mod L. */
int bxi_corr_append_f32(const float* t_feat, const float* t_mask, const float* boxes, const int64_t* labels, const int32_t* obj_slot,
                        const int32_t* obj_role, int N, int C, float* bank_feature, float* bank_mask, float* bank_box, int32_t* ptr,
                        int num_class, int L, void* stream);

/* bxi_corr_superres_f32  <->  superres_T for callers that want the matrix itself: T [K,49,49] -> out [K,784,784], every element written.
 * K == 0 is a no-op.  K * 784 * 784 >= 2^31: BXI_ERR_BAD_SHAPE. */
int bxi_corr_superres_f32(const float* T, int K, float* out, void* stream);

/* bxi_corr_cu_backward_f32: d / d f0 of Cu for a caller's upstream gradient, for SemanticCorrSolver.solve used on its own (the fused path
 *   has its gradient from bxi_corr_solve_f32).  f0 [C,7,7], f1 [K,C,7,7], dCu [K,49,49] -> grad [C,7,7], every element written; one launch,
 *   the k added in order.  K outside 1..BXI_CORR_MAX_OBJS, C < 1: BXI_ERR_BAD_SHAPE. */
int bxi_corr_cu_backward_f32(const float* f0, const float* f1, const float* dCu, int K, int C, float* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
