/*
 * boxinst_hip_plan.h -- developer query of libboxinst_hip.so: the form the single-launch evaluation would take.  NOT part of the
 * production ABI.  It stands in a header of its own, outside the ABI families of boxinstseg_amd/_lib.py: the families' conformance
 * test sorts every entry point into "run guarded over caller memory" or "exempt", and this one launches nothing and touches no caller
 * memory but `out8`.  boxinstseg_amd/_lib.py: eval1_plan() wraps it for the tests.
 */
#ifndef BOXINST_HIP_PLAN_H
#define BOXINST_HIP_PLAN_H

#ifdef __cplusplus
extern "C" {
#endif

/* What bxi_boxinst_eval_f32 would launch for N instance maps [h, w] over B images under `flags` (BXI_EVAL_*) on `stream` -- a batch whose
 * image side is pooled in the launch (stride 4, aligned rows), colour threshold above 0 --, computed by the host code that launches
 * (csrc/fused_eval.hip: plan_eval1).  out8:
 *   [0] 1: the evaluation is ONE eval1_kernel launch (0: two launches; of the rest only [3] is set then)
 *   [1] 1: the stream workgroups stay on as the first tile workgroups
 *   [2] 1: the table is written from the instances' last bands (0: by the first waves of the first stream workgroups, or, with the
 *          targets ready, by table workgroups)
 *   [3] stream workgroups   [4] pool workgroups   [5] predicate workgroups   [6] tile workgroups behind the leaders   [7] grid size
 * N == 0: all zero.  Returns BXI_OK or the status the evaluation would refuse the shape with. */
int bxi_dev_eval1_plan(int B, int N, int h, int w, int dilation, unsigned int flags, void* stream, int* out8);

#ifdef __cplusplus
}
#endif
#endif
