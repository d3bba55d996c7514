"""ctypes binding of libboxinst_hip.so -- the C ABI declared in include/boxinst_hip.h.

There is no fallback: if the shared library is missing (or a status is non-zero) this raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import build as _build

c_void_p, c_int, c_float, c_size_t = C.c_void_p, C.c_int, C.c_float, C.c_size_t

BXI_MAX_IMAGES = 64
BXI_ABI_VERSION = 7
# `flags` of bxi_boxinst_eval_f32 / bxi_boxinst_head_eval_f32 (include/boxinst_hip.h)
EVAL_SINGLE_LAUNCH, EVAL_TWO_LAUNCHES, EVAL_TILE_ROWS_8, EVAL_TILE_ROWS_4, EVAL_SHARED_DEVICE, EVAL_TARGETS_READY, EVAL_WAITS_GIVE_UP = 1, 2, 4, 8, 16, 32, 64

STATUS = {0: 'BXI_OK', -1: 'BXI_ERR_NULL_POINTER', -2: 'BXI_ERR_BAD_SHAPE', -3: 'BXI_ERR_BAD_ARGUMENT',
          -4: 'BXI_ERR_UNSUPPORTED', -5: 'BXI_ERR_WORKSPACE', -6: 'BXI_ERR_LAUNCH', -7: 'BXI_ERR_NO_DEVICE'}
BXI_ERR_UNSUPPORTED = -4


class ImageBatch(C.Structure):
    """struct bxi_image_batch"""
    _fields_ = [('imgs', c_void_p), ('B', c_int), ('Hc', c_int), ('Wc', c_int),
                ('img_h_host', C.POINTER(c_int)), ('img_w_host', C.POINTER(c_int)),
                ('rows_removed_host', C.POINTER(c_int)),
                ('mean', C.c_double * 3), ('std', C.c_double * 3), ('to_rgb', c_int),
                ('image_masks', c_void_p)]


class Instances(C.Structure):
    """struct bxi_instances"""
    _fields_ = [('logits', c_void_p), ('N', c_int), ('h', c_int), ('w', c_int),
                ('gt_inds', c_void_p), ('boxes_per_img_host', C.POINTER(c_void_p)),
                ('gt_count_host', C.POINTER(c_int)), ('B', c_int), ('Hc', c_int), ('Wc', c_int),
                ('stride', c_int), ('iter_counter', c_void_p)]


# name -> (restype, argtypes); must list every symbol of include/boxinst_hip.h and include/boxinst_hip_dev.h (tests check this)
SIGNATURES = {
    'bxi_abi_version': (c_int, []),
    'bxi_status_string': (C.c_char_p, [c_int]),
    'bxi_last_hip_error': (c_int, []),
    'bxi_check_device': (c_int, [c_int]),
    'bxi_dev_set_launch_hook': (None, [c_void_p, c_void_p]),           # boxinst_hip_dev.h (bench / tests only)
    'bxi_dev_set_tree_level_walk': (None, [c_int]),                    # boxinst_hip_dev.h (tests only)
    'bxi_dev_sol_eval_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),                        # boxinst_hip_dev.h (bench only)
    'bxi_dev_sol_pairwise_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),   # boxinst_hip_dev.h (bench only)
    'bxi_pairwise_nlog_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_pairwise_nlog_forward_f64': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_pairwise_nlog_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p]),
    'bxi_pairwise_nlog_backward_f64': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p]),
    'bxi_color_affinity_f32': (c_int, [C.POINTER(ImageBatch), c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    'bxi_box_bitmasks_f32': (c_int, [C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p]),
    'bxi_boxinst_loss_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_boxinst_loss_state_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_boxinst_loss_state_status_offset': (c_size_t, [c_int, c_int, c_int]),
    'bxi_boxinst_loss_state_warmup_offset': (c_size_t, [c_int, c_int, c_int]),
    'bxi_boxinst_loss_fwd_bwd_f32': (c_int, [C.POINTER(Instances), c_void_p, c_int, c_int, c_float, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_boxinst_loss_backward_f32': (c_int, [C.POINTER(Instances), c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p]),
    'bxi_boxinst_eval_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'bxi_boxinst_eval_workspace_lab_offset': (c_size_t, []),
    'bxi_boxinst_eval_workspace_init': (c_int, [c_void_p, c_size_t, c_void_p]),
    'bxi_boxinst_targets_f32': (c_int, [C.POINTER(ImageBatch), C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_int, c_float, c_void_p,
                                        c_size_t, c_void_p]),
    'bxi_boxinst_eval_f32': (c_int, [C.POINTER(ImageBatch), C.POINTER(Instances), c_int, c_int, c_float, c_float,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, C.c_uint, c_void_p]),
    'bxi_boxinst_head_eval_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, C.c_uint, c_void_p]),
    'bxi_boxinst_grad_rescale_f32': (c_int, [C.POINTER(Instances), c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p]),
    'bxi_boxinst_grad_rescale_nhw_f32': (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'bxi_dynamic_mask_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_dynamic_mask_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'bxi_dynamic_mask_generic_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_dynamic_mask_generic_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'bxi_dynamic_mask_generic_backward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_size_t, c_void_p]),
    'bxi_dynamic_mask_backward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_size_t, c_void_p]),
    'bxi_mask_paste_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p,
                                  c_void_p]),
    'bxi_meanfield_kernel_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.c_float, C.c_float, C.c_float,
                                         c_void_p, c_void_p]),
    'bxi_meanfield_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_meanfield_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                          c_int, C.c_float, c_void_p, C.c_float, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    'bxi_dice_loss_forward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, C.c_int64, c_void_p, c_void_p, c_void_p]),
    'bxi_dice_loss_backward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, C.c_int64, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    'bxi_mil_loss_state_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_mil_loss_forward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'bxi_mil_loss_backward_f32': (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_projection_loss_forward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, C.c_float, c_void_p, c_void_p, c_void_p]),
    'bxi_levelset_state_bytes': (c_size_t, [c_int, c_int]),
    'bxi_levelset_loss_forward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, C.c_float, c_void_p,
                                              c_void_p, c_void_p]),
    'bxi_levelset_loss_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, C.c_float, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_lcm_affinity_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.c_float, c_void_p, c_void_p]),
    'bxi_lcm_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_lcm_refine_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    'bxi_mst_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_mst_forward_i32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_bfs_workspace_bytes': (c_size_t, [c_int, c_int]),
    'bxi_bfs_forward_i32': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_tree_refine_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_tree_refine_forward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_tree_refine_backward_feature_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                                     c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_tree_refine_backward_weight_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_tree_refine_backward_weight_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                    c_void_p, c_size_t, c_void_p]),
}

# csrc/meanfield.hip: kMfManyItems.  bxi_meanfield_forward_f32 runs four (instance, row, segment) items per wave when N * H * ceil(W / 64)
# exceeds this, one otherwise (tests/test_host_meanfield_decided.py holds the two together; tests/test_gpu_meanfield_paths.py runs both sides)
MF_MANY_ITEMS = 32768

# include/boxinst/boxinst_hip_post.h (test-time post-processing of the SOLOv2-style heads)
NMS_KERNELS = {'gaussian': 0, 'linear': 1}
NMS_MAX_CANDIDATES = 2048
POST_SIGNATURES = {
    'bxi_mask_pack_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_mask_pack_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'bxi_matrix_nms_workspace_bytes': (c_size_t, [c_int]),
    'bxi_matrix_nms_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/boxinst/boxinst_hip_assign.h (Box2Mask target assignment: matching cost and Hungarian)
MATCH_MAX_SIDE = 1024
MATCH_STATUS_NONFINITE, MATCH_STATUS_BAD_LABEL = 1, 2
ASSIGN_SIGNATURES = {
    'bxi_box_match_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_match_project_pred_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    'bxi_match_project_gt_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_match_project_gt_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_match_cost_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                   C.POINTER(c_int), c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    'bxi_linear_sum_assignment_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, C.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
}

# include/boxinst/boxinst_hip_det.h (CondInst test-time detections: decode, score filter, box NMS)
DET_MAX_LEVELS, DET_SORT_MAX, DET_NMS_ROUND, DET_KEEP_TILE, DET_ROW_TILE = 8, 16384, 256, 2048, 64
DET_STATUS_OVER_CAP, DET_STATUS_OVER_SORT, DET_STATUS_BAD_ORDER = 1, 2, 4


class DetLevel(C.Structure):
    """struct bxi_det_level"""
    _fields_ = [('cls', c_void_p), ('bbox', c_void_p), ('ctr', c_void_p), ('params', c_void_p), ('H', c_int), ('W', c_int), ('stride', c_int)]


DET_SIGNATURES = {
    'bxi_det_location_score_f32': (c_int, [C.POINTER(DetLevel), c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_det_candidates_workspace_bytes': (c_size_t, [c_int, c_int]),
    'bxi_det_candidates_f32': (c_int, [C.POINTER(DetLevel), c_int, c_int, c_int, c_void_p, c_int, C.POINTER(c_float), c_int, c_float, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_box_nms_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_box_nms_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_det_gather_f32': (c_int, [C.POINTER(DetLevel), c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/boxinst/boxinst_hip_fcos.h (the box head's training step: FCOS targets, focal / IoU / centerness loss)
FCOS_GT_CHUNK, FCOS_LOC_TILE, FCOS_ELEM_TILE, FCOS_STATUS_BAD_LABEL = 64, 256, 1024, 1
FCOS_BBOX_KINDS = {'giou': 0, 'iou_log': 1, 'iou_linear': 2, 'iou_square': 3}


class FcosLevel(C.Structure):
    """struct bxi_fcos_level"""
    _fields_ = [('H', c_int), ('W', c_int), ('stride', c_int)]


class FcosGrads(C.Structure):
    """struct bxi_fcos_grads"""
    _fields_ = [('cls', c_void_p), ('bbox', c_void_p), ('ctr', c_void_p)]


FCOS_SIGNATURES = {
    'bxi_fcos_workspace_bytes': (c_size_t, [C.POINTER(FcosLevel), c_int, c_int, c_int]),
    'bxi_fcos_targets_f32': (c_int, [C.POINTER(FcosLevel), c_int, c_int, C.POINTER(c_float), c_int, C.c_double, c_int, c_int, c_void_p, c_void_p,
                                     C.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    'bxi_fcos_loss_f32': (c_int, [C.POINTER(DetLevel), c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float,
                                  c_float, c_float, c_int, c_float, C.POINTER(FcosGrads), c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_fcos_grad_rescale_f32': (c_int, [C.POINTER(FcosLevel), c_int, c_int, c_int, C.POINTER(FcosGrads), c_void_p, C.POINTER(FcosGrads),
                                          c_void_p]),
}

# include/boxinst/boxinst_hip_solo.h (training targets of the SOLOv2-style heads and their category loss)
SOLO_MODES = {'discobox': 0, 'boxlevelset': 1}
SOLO_MAX_FACTORS, SOLO_MAX_FACTOR, SOLO_RESCALE_MIN_ONES, SOLO_MIN_MASK_SUM, SOLO_MAX_GRID, SOLO_PAIRS_PER_INSTANCE = 4, 64, 2, 10, 64, 9
SOLO_STATUS_BAD_LABEL = 1
SOLO_SIGNATURES = {
    'bxi_solo_mask_pass_u8': (c_int, [C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int), c_int, C.POINTER(c_int),
                                      C.POINTER(c_int), C.POINTER(c_int), c_int, C.POINTER(c_void_p), c_void_p, c_void_p]),
    'bxi_solo_assign_f32': (c_int, [c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_float), C.c_double, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, C.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    'bxi_solo_cate_workspace_bytes': (c_size_t, [C.POINTER(c_int), c_int, c_int, c_int]),
    'bxi_solo_cate_loss_f32': (c_int, [C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float,
                                       C.POINTER(c_void_p), c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_solo_cate_grad_rescale_f32': (c_int, [C.POINTER(c_int), c_int, c_int, c_int, C.POINTER(c_void_p), c_void_p, C.POINTER(c_void_p),
                                               c_void_p]),
}

# include/boxinst/boxinst_hip_corr.h (DiscoBox's cross-image correspondence: bank, retrieval, solver, loss_corr, iiu)
CORR_FEAT, CORR_MASK, CORR_MAX_OBJS, CORR_MAX_QUEUE = 7, 28, 8, 1024
CORR_SIGNATURES = {
    'bxi_corr_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_corr_plan_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    'bxi_corr_retrieve_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    'bxi_corr_solve_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                   c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_corr_loss_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_corr_grad_rescale_f32': (c_int, [c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p]),
    'bxi_corr_iiu_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                 c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_corr_append_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, c_int, c_void_p]),
    'bxi_corr_superres_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'bxi_corr_cu_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
}

# include/boxinst/boxinst_hip_roi.h (RoIAlign forward / backward and the front of one level of DiscoBox's corr_loss)
ROI_MAX_POOL, ROI_MAX_SAMPLING, ROI_MAX_SIDE, ROI_FUSED_MAX_C, ROI_FEAT, ROI_SIGMOID = 64, 64, 16384, 8192, 7, 1
ROI_SIGNATURES = {
    'bxi_roi_target_boxes_u8': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_roi_align_forward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p,
                                          c_void_p]),
    'bxi_roi_align_backward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                                           c_void_p]),
    'bxi_roi_feat_norm_workspace_bytes': (c_size_t, [c_int, c_int]),
    'bxi_roi_feat_norm_forward_f32': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                              c_size_t, c_void_p]),
    'bxi_roi_feat_norm_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                                               c_void_p, c_size_t, c_void_p]),
}

# include/boxinst/boxinst_hip_msda.h (multi-scale deformable attention, forward and backward)
MSDA_MAX_LEVELS, MSDA_MAX_POINTS, MSDA_MIN_HEAD_DIM, MSDA_MAX_HEAD_DIM, MSDA_FUSED, MSDA_MAX_CELL_SAMPLES = 8, 8, 8, 64, 1, 1 << 22
MSDA_SIGNATURES = {
    'bxi_msda_forward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p]),
    'bxi_msda_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'bxi_msda_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/boxinst/boxinst_hip_seg.h (the final masks of the SOLOv2-style heads: resize, crop, threshold, area and box of the kept candidates)
SEG_SIGNATURES = {
    'bxi_seg_paste_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_seg_paste_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/boxinst/boxinst_hip_dconv.h (the dynamic 1x1 mask convolution of the SOLOv2-style heads, training and test time)
DCONV_MAPS, DCONV_ROWS, DCONV_NONE, DCONV_SIGMOID, DCONV_MAX_LEVELS, DCONV_MAX_E, DCONV_TILE, DCONV_STATUS_BAD_CELL = 0, 1, 0, 1, 8, 1024, 64, 1
DCONV_SIGNATURES = {
    'bxi_solo_dconv_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_void_p,
                                           C.POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_solo_dconv_forward_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_solo_dconv_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'bxi_solo_dconv_backward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_void_p,
                                            C.POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_void_p, C.POINTER(c_void_p), c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
}

# include/boxinst/boxinst_hip_attn.h (the masked cross-attention of Box2Mask's transformer decoder: the mask as bits, forward and backward)
ATTN_SPAN, ATTN_MAX_Q, ATTN_MAX_S, ATTN_MAX_HEADS, ATTN_HEAD_DIMS = 256, 1 << 20, 1 << 24, 65535, (16, 32, 64)
ATTN_SIGNATURES = {
    'bxi_attn_mask_bits_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_attn_pack_mask_u8': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'bxi_masked_attn_forward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'bxi_masked_attn_forward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p,
                                            c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_masked_attn_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'bxi_masked_attn_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                             c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# every ABI family, in the order it arrived: (name, its headers relative to the repository root, its signature table).  load()
# applies the tables; tests/test_abi_families.py holds each against its headers and the library's exports.
FAMILIES = [
    ('base', ('include/boxinst_hip.h', 'include/boxinst_hip_dev.h'), SIGNATURES),
    ('post', ('include/boxinst/boxinst_hip_post.h',), POST_SIGNATURES),
    ('assign', ('include/boxinst/boxinst_hip_assign.h',), ASSIGN_SIGNATURES),
    ('det', ('include/boxinst/boxinst_hip_det.h',), DET_SIGNATURES),
    ('fcos', ('include/boxinst/boxinst_hip_fcos.h',), FCOS_SIGNATURES),
    ('solo', ('include/boxinst/boxinst_hip_solo.h',), SOLO_SIGNATURES),
    ('corr', ('include/boxinst/boxinst_hip_corr.h',), CORR_SIGNATURES),
    ('roi', ('include/boxinst/boxinst_hip_roi.h',), ROI_SIGNATURES),
    ('msda', ('include/boxinst/boxinst_hip_msda.h',), MSDA_SIGNATURES),
    ('seg', ('include/boxinst/boxinst_hip_seg.h',), SEG_SIGNATURES),
    ('dconv', ('include/boxinst/boxinst_hip_dconv.h',), DCONV_SIGNATURES),
    ('attn', ('include/boxinst/boxinst_hip_attn.h',), ATTN_SIGNATURES),
]

# include/boxinst/boxinst_hip_inst.h (Box2Mask at test time: query x class top-k, final masks with mask score, area and box)
INST_TOPK_MAX = 16384
INST_SIGNATURES = {
    'bxi_inst_topk_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_inst_paste_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_inst_paste_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# the families that arrived after tests/test_abi_families.py pinned FAMILIES to its twelve names: the same triples, applied by load()
# behind FAMILIES with the same check across both lists; tests/test_abi_family_inst.py holds them against headers, exports and guards.
LATE_FAMILIES = [
    ('inst', ('include/boxinst/boxinst_hip_inst.h',), INST_SIGNATURES),
]

# include/boxinst/boxinst_hip_dconv16.h (the dynamic mask convolution on fp16 / bf16 tensors read in place, fp32 accumulation on the MFMA)
DCONV16_F16, DCONV16_BF16, DCONV16_OUT_F32, DCONV16_TILE = 0, 1, 2, 64
DCONV16_SIGNATURES = {
    'bxi_solo_dconv16_forward_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_solo_dconv16_forward': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_void_p,
                                         C.POINTER(c_int), c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_solo_dconv16_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'bxi_solo_dconv16_backward': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), c_int, c_int, c_void_p,
                                          C.POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, C.POINTER(c_void_p), c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
}

# the half-precision siblings of families above: a third list, because tests/test_abi_family_inst.py pins LATE_FAMILIES to ['inst'];
# the same triples, applied by load() behind the other two with the same check across all lists (tests/test_abi_family_dconv16.py)
HALF_FAMILIES = [
    ('dconv16', ('include/boxinst/boxinst_hip_dconv16.h',), DCONV16_SIGNATURES),
]

# include/boxinst/boxinst_hip_dconvl.h (BoxLevelSet's training masks: the assigned cells' dynamic convolution and the per-level bilinear resize)
DCONVL_MAX_DOWN, DCONVL_MAX_UP = 8, 2
DCONVL_SIGNATURES = {
    'bxi_solo_dconvl_forward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), c_int]),
    'bxi_solo_dconvl_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_int,
                                            c_void_p, C.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_solo_dconvl_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), c_int]),
    'bxi_solo_dconvl_backward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_int,
                                             c_void_p, C.POINTER(c_int), c_int, c_void_p, c_void_p, C.POINTER(c_void_p), c_void_p, c_void_p,
                                             c_size_t, c_void_p]),
}

# the families on top of the dynamic convolution: a fourth list, because tests/test_abi_family_dconv16.py pins HALF_FAMILIES to
# ['dconv16']; the same triples, applied by load() behind the other three with the same check across all lists
# (tests/test_abi_family_dconvl.py)
LEVEL_FAMILIES = [
    ('dconvl', ('include/boxinst/boxinst_hip_dconvl.h',), DCONVL_SIGNATURES),
]

# include/boxinst/boxinst_hip_rle.h (the test-time masks as COCO run-length encodings: counts and strings of every mask, packed)
RLE_STATUS_OVER_RUNS, RLE_STATUS_OVER_CHARS, RLE_MAX_PIXELS, RLE_MAX_CHARS_PER_COUNT = 1, 2, 1 << 29, 6
RLE_SIGNATURES = {
    'bxi_mask_rle_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'bxi_mask_rle_u8': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
}

# what the test pipelines end in: a fifth list, because tests/test_abi_family_dconvl.py pins LEVEL_FAMILIES to ['dconvl']; the same
# triples, applied by load() behind the other four with the same check across all lists (tests/test_abi_family_rle.py)
RESULT_FAMILIES = [
    ('rle', ('include/boxinst/boxinst_hip_rle.h',), RLE_SIGNATURES),
]

# include/boxinst/boxinst_hip_b2m.h (Box2MaskHead.loss for the matched rows of all decoder layers: scores and their small-grid resize,
# the level-set energy inside the box without its operands, the LCM refinement with one affinity per image)
B2M_MAX_LAYERS, B2M_MAX_UP, B2M_MAX_C = 16, 8, 4
B2M_SIGNATURES = {
    'bxi_b2m_scores_f32': (c_int, [C.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'bxi_b2m_scores_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'bxi_b2m_levelset_state_bytes': (c_size_t, [c_int, c_int]),
    'bxi_b2m_levelset_forward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                             c_int, c_float, c_void_p, c_void_p, c_void_p]),
    'bxi_b2m_levelset_backward_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                              c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'bxi_b2m_lcm_refine_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
}

# the training steps that are whole compositions: a sixth list, because tests/test_abi_family_rle.py pins RESULT_FAMILIES to ['rle']; the
# same triples, applied by load() behind the other five with the same check across all lists (tests/test_abi_family_b2m.py)
TRAIN_FAMILIES = [
    ('b2m', ('include/boxinst/boxinst_hip_b2m.h',), B2M_SIGNATURES),
]

# include/boxinst/boxinst_hip_dbx.h (the pseudo-label block of DiscoBoxSOLOv2Head.loss for the rows of all levels: labels as bit words, both
# mean-field legs in one launch per iteration, the dice terms from the words, the means over the live rows)
DBX_MAX_LEVELS, DBX_MAX_MEANS, DBX_TARGET, DBX_ENLARGED, DBX_LABEL = 8, 4, 0, 1, 2
DBX_SIGNATURES = {
    'bxi_dbx_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'bxi_dbx_prepare_f32': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_dbx_steps_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, C.c_double, c_int, C.POINTER(c_void_p),
                                  C.POINTER(c_int), c_int, c_void_p, c_size_t, c_void_p]),
    'bxi_dbx_dice_forward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    'bxi_dbx_dice_backward_f32': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, C.c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    'bxi_dbx_means_f32': (c_int, [C.POINTER(c_void_p), c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'bxi_dbx_means_backward_f32': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'bxi_dbx_unpack_u8': (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# the training steps of the second SOLOv2-style method: a seventh list, because tests/test_abi_family_b2m.py pins TRAIN_FAMILIES to
# ['b2m']; the same triples, applied by load() behind the other six with the same check across all lists (tests/test_abi_family_dbx.py)
PSEUDO_FAMILIES = [
    ('dbx', ('include/boxinst/boxinst_hip_dbx.h',), DBX_SIGNATURES),
]

# include/boxinst/boxinst_hip_bls.h (the mask losses of BoxSOLOv2Head.loss for the set cells of all levels: scores, projection term, pixel_num
# and image level-set energy in one pass, the level-set energy on the rows' own filter outputs, one backward launch for every level's gradient)
BLS_MAX_GROUPS, BLS_MAX_LEVELS, BLS_MAX_W, BLS_CHUNK_PIXELS, BLS_LEVEL_ROWS = 4, 8, 2048, 1024, 1 << 20


class BlsGroup(C.Structure):
    """struct bxi_bls_group"""
    _fields_ = [('img', c_void_p), ('masks', c_void_p), ('h', c_int), ('w', c_int), ('rows', c_int), ('G', c_int)]


BLS_SIGNATURES = {
    'bxi_bls_state_bytes': (c_size_t, [C.POINTER(BlsGroup), c_int]),
    'bxi_bls_front_f32': (c_int, [C.POINTER(BlsGroup), c_int, C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_int, c_void_p, c_void_p,
                                  c_void_p, c_int, c_int, C.c_double, C.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    'bxi_bls_backward_f32': (c_int, [C.POINTER(BlsGroup), c_int, C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_int, c_void_p, c_void_p,
                                     c_void_p, c_int, c_int, C.c_double, C.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    'bxi_bls_high_state_bytes': (c_size_t, [C.POINTER(BlsGroup), c_int]),
    'bxi_bls_high_forward_f32': (c_int, [C.POINTER(BlsGroup), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, C.c_double,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    'bxi_bls_high_backward_f32': (c_int, [C.POINTER(BlsGroup), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, C.c_double,
                                          c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# the training steps of the third SOLOv2-style method: an eighth list, because tests/test_abi_family_dbx.py pins PSEUDO_FAMILIES to
# ['dbx']; the same triples, applied by load() behind the other seven with the same check across all lists (tests/test_abi_family_bls.py)
LEVELSET_FAMILIES = [
    ('bls', ('include/boxinst/boxinst_hip_bls.h',), BLS_SIGNATURES),
]

LAUNCH_HOOK = C.CFUNCTYPE(None, C.c_char_p, c_int, c_void_p, c_void_p)

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    return _build.LIB_PATH


def load() -> C.CDLL:
    """dlopen the in-tree shared library (never a fallback: raises if it is not there)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f'{path} is missing: the BoxInst HIP extension has not been built '
                '(run `python -c "import __graft_entry__ as g; g.build()"` or `python -m boxinstseg_amd.build`). '
                'boxinstseg_amd has no CPU or PyTorch fallback for this path.')
        lib = C.CDLL(path)
        owner = {}
        for family, _, table in FAMILIES + LATE_FAMILIES + HALF_FAMILIES + LEVEL_FAMILIES + RESULT_FAMILIES + TRAIN_FAMILIES + PSEUDO_FAMILIES + LEVELSET_FAMILIES:
            for name, (res, args) in table.items():
                if owner.setdefault(name, family) != family:
                    raise RuntimeError(f'{name} is in the signature tables of two ABI families: {owner[name]} and {family}')
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        if lib.bxi_abi_version() != BXI_ABI_VERSION:
            raise RuntimeError(f'{path}: ABI version {lib.bxi_abi_version()} != {BXI_ABI_VERSION}')
        _lib = lib
    return _lib


def status_string(status: int) -> str:
    return load().bxi_status_string(status).decode()


EVAL1_PLAN_FIELDS = ('taken', 'merge', 'table_last', 'n_stream', 'n_pool', 'n_pb', 'n_tb', 'grid')


def eval1_plan(B: int, N: int, h: int, w: int, dilation: int = 2, flags: int = 0, stream: int = 0) -> dict:
    """The form bxi_boxinst_eval_f32 would launch for this shape (include/boxinst_hip_plan.h: bxi_dev_eval1_plan, a developer query
    that belongs to no ABI family: it launches nothing).  Raises with the status the evaluation would refuse the shape with."""
    fn = load().bxi_dev_eval1_plan
    fn.restype, fn.argtypes = c_int, [c_int, c_int, c_int, c_int, c_int, C.c_uint, c_void_p, c_void_p]
    out = (c_int * len(EVAL1_PLAN_FIELDS))()
    rc = fn(B, N, h, w, dilation, flags, stream, C.cast(out, c_void_p))
    if rc != 0:
        raise RuntimeError(f'bxi_dev_eval1_plan: {STATUS.get(rc, rc)}')
    return dict(zip(EVAL1_PLAN_FIELDS, out))


class BoxInstHipError(RuntimeError):
    def __init__(self, fn: str, status: int):
        self.status = status
        detail = status_string(status)
        if status == -6:
            detail += f' [hipError_t {load().bxi_last_hip_error()}]'
        super().__init__(f'{fn}: {STATUS.get(status, status)} -- {detail}')


def check(fn: str, status: int) -> None:
    if status != 0:
        raise BoxInstHipError(fn, status)


def check_supported(fn: str, status: int, header: str) -> None:
    """check(), except that BXI_ERR_UNSUPPORTED is a NotImplementedError naming the header (of include/boxinst/) that states the support set."""
    if status == BXI_ERR_UNSUPPORTED:
        raise NotImplementedError(f'{fn}: outside the support set of include/boxinst/{header}')
    check(fn, status)


def int_array(values) -> C.Array:
    values = [int(v) for v in values]
    return (c_int * max(len(values), 1))(*values)


def float_array(values) -> C.Array:
    values = [float(v) for v in values]
    return (c_float * max(len(values), 1))(*values)


def ptr_array(values) -> C.Array:
    values = [int(v) for v in values]
    return (c_void_p * max(len(values), 1))(*values)
