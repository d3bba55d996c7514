"""boxinstseg_amd -- the BoxInst box-supervised mask-loss path of LiWentomng/BoxInstSeg, rebuilt
MI355X-native (gfx950 HIP kernels behind a C ABI; see include/boxinst_hip.h and DESIGN.md).

Public surface (mirrors the reference's for this path):
    pairwise_nlog                      <-> mmdet.ops.pairwise.pairwise_nlog
    pairwise_nlog_forward / _backward  <-> mmdet.ops.pairwise.pairwise_ext
    CondInstMaskHead                   <-> mmdet.models.dense_heads.CondInstMaskHead (loss path, simple_test)
    paste_masks, paste_masks_device    : the test-time mask post-processing of simple_test as one kernel
    boxinst_mask_loss, color_affinity, box_bitmasks : functional form of the same kernels
    MeanField, dice_loss, mil_loss     <-> mmdet.models.dense_heads.discobox_head
    BoxProjectionLoss, LevelsetLoss, LocalConsistencyModule, LCM <-> mmdet.models.losses
    MinimumSpanningTree, TreeFilter2D, mst, bfs, refine <-> mmdet.ops.tree_filter
    mask_matrix_nms                    <-> mmdet.core.post_processing.mask_matrix_nms
    seg_nms, box_solov2_get_seg_single, discobox_get_seg_single : the test-time block of the SOLOv2-style heads (get_seg_single)
    seg_paste                          : the two resizes and the threshold that end get_seg_single as one kernel, with area and box per mask
    solo_get_seg, solo_format_results  <-> get_seg of both SOLOv2-style heads / format_results of their detectors (one host copy, one sync)
    ClassificationCost, BoxMatchingCost, MaskHungarianAssigner <-> mmdet.core.bbox match costs / assigner of Box2Mask
    box2mask_get_targets               <-> Box2MaskHead.get_targets (matching cost and Hungarian assignment of a whole batch)
    nms, batched_nms                   <-> mmcv.ops.nms.nms / batched_nms (greedy box NMS, one workgroup per image)
    nms_with_others                    <-> mmdet.models.dense_heads.condinst_head.nms_with_others
    condinst_get_bboxes                <-> CondInstBoxHead.get_bboxes (decode, score filter and box NMS of a whole batch, one sync)
    condinst_box_targets               <-> CondInstBoxHead.get_targets / centerness_target (FCOS assignment of a whole batch, one launch)
    condinst_box_loss                  <-> CondInstBoxHead.loss (focal, IoU / GIoU and centerness loss with gradients, no sync)
    parse_box_head_cfg                 : the bbox_head block of the reference's configs as condinst_box_loss takes it
    solov2_targets                     <-> DiscoBoxSOLOv2Head.solov2_target_single over a batch (mask pass + assignment, one sync)
    box_solov2_targets                 <-> BoxSOLOv2Head.solo_target_single over a batch (without its two F.interpolate)
    solo_cate_loss                     <-> loss_cate of both SOLOv2-style heads (focal loss on the NCHW maps, avg_factor on the device)
    parse_solo_head_cfg                : the bbox_head block of configs/discobox and configs/boxlevelset as the functions take it
    ObjectBank, SemanticCorrSolver, superres_T <-> ObjectQueues, SemanticCorrSolver, superres_T of discobox_head.py (cross-image correspondence)
    corr_objects                       <-> the object loop of DiscoBoxSOLOv2Head.corr_loss (retrieval, solver, loss_corr, iiu, append; no sync)
    parse_corr_cfg                     : the loss_corr / obj_bank block of configs/discobox as the classes take it
    roi_align, RoIAlign                <-> mmcv.ops.roi_align / RoIAlign (pool_mode='avg'; restated arithmetic, forward and backward)
    relu_and_l2_norm_feat, roi_feat_norm, sigmoid_roi_masks, target_boxes : the pieces of the front of corr_loss (discobox_head.py:1018-1057)
    corr_level                         <-> one level of DiscoBoxSOLOv2Head.corr_loss (:1018-1127): the front, then corr_objects; no sync
    multi_scale_deformable_attn        <-> mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttnFunction.apply (restated arithmetic)
    multi_scale_deformable_attn_fused  : the same from reference points, raw offsets and raw logits (normaliser and softmax in the kernel)
    MultiScaleDeformableAttention      <-> mmcv's module, the self-attention of Box2Mask's MSDeformAttnPixelDecoder; ATTENTION, build_attention
    solo_dynamic_masks                 <-> the dynamic 1x1 convolution and sigmoid of DiscoBoxSOLOv2Head.loss / corr_loss (one launch, autograd)
    solo_dynamic_masks_pair            : the same for the student's and the teacher's maps with one grid_order (the teacher without a backward)
    solo_candidate_masks               <-> F.conv2d(seg_preds, kernel_preds[rows]).sigmoid() of get_seg_single, the kernel rows read in place
      (all three) compute='half'       : the same statements as the reference's autocast runs them -- fp16 / bf16 tensors read in place,
                                         fp32 accumulation, half masks and gradients (csrc/solo_dconv16.hip); discobox_get_seg_single(conv='hip_half')
    box_solov2_ins_preds               <-> BoxSOLOv2Head.forward :205-216 + loss :317-320: the set cells' dynamic convolution and the per-level bilinear
                                         resize, nothing of all cells' size (csrc/solo_dconv_level.hip; autograd, fp32)
    box_solov2_set_cells               : the set cells of every (level, image) of a SoloTargets, ascending, without a host synchronisation
    box_solov2_get_seg_single_kernels  <-> BoxSOLOv2Head.get_seg_single from the mask feature and the kernels: only the candidates' masks exist
    box2mask_attn_mask, attn_mask_bits <-> the attention mask of Box2MaskHead.forward_head and its repair in forward, as bits (PackedAttnMask), one launch
    pack_attn_mask                     : an existing bool attention mask [B*M,Q,S] or [Q,S] packed to a PackedAttnMask on the device
    masked_attention                   : the attention core of torch.nn.MultiheadAttention with that mask, forward and backward, no [Q,S] tensor
    MultiheadAttention                 <-> mmcv's module, the cross- and self-attention of Box2Mask's transformer decoder; ATTENTION, build_attention
    instance_topk                      <-> softmax, topk and is_thing filter of MaskFormerFusionHead.instance_postprocess (one launch, defined order)
    box2mask_instances                 <-> Box2Mask after the decoder: both F.interpolate, crop, ``> 0``, mask score, mask2bbox (no fp32 canvas)
    MaskFormerFusionHead               <-> mmdet's panoptic_fusion_head of configs/box2mask (instance results; registered in HEADS)
    box2mask_format_results            <-> the formatting loop of MaskFormer.simple_test (bbox2result, masks to numpy: one host copy, one sync)
    rle_encode, EncodedMasks           <-> pycocotools.mask.encode of every mask of a [n,h,w] block, on the GPU (restated format, unpinned; four launches)
    rle_decode                         <-> pycocotools.mask.decode on the host in numpy (for users and tests)
    solo_encode_results                <-> format_results + encode_mask_results for the SOLOv2-style heads: RLE dicts instead of masks cross to the host
    box2mask_encode_results            <-> MaskFormer.simple_test's formatting + encode_mask_results for Box2Mask, the same way
    box2mask_loss                      <-> Box2MaskHead.loss: the loss dict of all decoder layers in one call, no sync (csrc/box2mask_loss.hip)
    Box2MaskLossContext                : what loss_single recomputes per layer (resizes, both trees, edge weights, LCM affinity, box targets), once
    box2mask_mask_losses               <-> loss_project / loss_levelset of loss_single (:260-335) for the matched rows of all layers together
    parse_box2mask_head_cfg            : the panoptic_head block of configs/box2mask as box2mask_loss takes it
    discobox_loss                      <-> DiscoBoxSOLOv2Head.loss: the loss dict in one call, the only sync is solov2_targets' (csrc/discobox_loss.hip)
    discobox_pseudo_losses             <-> the mil / ts / ts_corr terms of loss (:1271-1306) and corr_loss (:1127-1137) for the rows of all levels: labels as bits
    live_means                         : the means over the rows whose target is not all zero, decided on the device
    parse_discobox_loss_cfg            : loss_ins / loss_ts / loss_corr of the bbox_head block of configs/discobox as discobox_loss reads them
    box_solov2_loss                    <-> BoxSOLOv2Head.loss: the loss dict in one call, the only sync is box_solov2_targets' (csrc/boxlevelset_loss.hip)
    BoxLevelSetLossContext             : what the level loop recomputes per level, image and set cell (resizes, both trees, orders, edge weights), once per size
    box_solov2_mask_losses             <-> loss_boxpro / loss_levelset of loss (:334-367) for the set cells of all levels together, rows of different sizes in one launch
    parse_box_solov2_loss_cfg          : loss_boxpro / loss_levelset / loss_cate of the bbox_head block of configs/boxlevelset as box_solov2_loss reads them
"""
from .pairwise import PairwiseNLog, pairwise_nlog, pairwise_nlog_backward, pairwise_nlog_forward
from .functional import BoxInstMaskLoss, box_bitmasks, boxinst_mask_loss, color_affinity
from .dynamic import DynamicMaskHead, dynamic_mask_forward, paste_masks, paste_masks_device
from .mask_head import CondInstMaskHead
from .discobox import MeanField, dice_loss, meanfield_forward, meanfield_kernel, mil_loss
from .levelset import LCM, BoxProjectionLoss, LevelsetLoss, LocalConsistencyModule, region_levelset
from .registry import ATTENTION, BBOX_ASSIGNERS, HEADS, LOSSES, MATCH_COST, build_assigner, build_attention, build_head, build_loss, build_match_cost
from .tree_filter import MinimumSpanningTree, TreeFilter2D, bfs, mst, refine
from .matrix_nms import box_solov2_get_seg_single, discobox_get_seg_single, mask_matrix_nms, seg_nms
from .seg_paste import seg_paste, solo_format_results, solo_get_seg
from .box_match import BoxMatchingCost, ClassificationCost, MaskHungarianAssigner, box2mask_get_targets
from .box_nms import batched_nms, condinst_get_bboxes, nms, nms_with_others
from .box_head_loss import condinst_box_loss, condinst_box_targets, parse_box_head_cfg
from .solo_targets import SoloTargets, box_solov2_targets, parse_solo_head_cfg, solo_cate_loss, solov2_targets
from .corr import ObjectBank, SemanticCorrSolver, corr_objects, parse_corr_cfg, superres_T
from .roi_align import RoIAlign, corr_level, relu_and_l2_norm_feat, roi_align, roi_feat_norm, sigmoid_roi_masks, target_boxes
from .msda import MultiScaleDeformableAttention, multi_scale_deformable_attn, multi_scale_deformable_attn_fused
from .solo_conv import solo_candidate_masks, solo_dynamic_masks, solo_dynamic_masks_pair
from .box_solo_masks import box_solov2_get_seg_single_kernels, box_solov2_ins_preds, box_solov2_set_cells
from .masked_attn import MultiheadAttention, PackedAttnMask, attn_mask_bits, box2mask_attn_mask, masked_attention, pack_attn_mask
from .inst_post import MaskFormerFusionHead, box2mask_format_results, box2mask_instances, instance_topk
from .mask_rle import EncodedMasks, box2mask_encode_results, rle_decode, rle_encode, solo_encode_results
from .box2mask_loss import Box2MaskLossContext, box2mask_loss, box2mask_mask_losses, parse_box2mask_head_cfg
from .discobox_loss import discobox_loss, discobox_pseudo_losses, live_means, parse_discobox_loss_cfg
from .boxlevelset_loss import BoxLevelSetLossContext, box_solov2_loss, box_solov2_mask_losses, parse_box_solov2_loss_cfg
from .config import load_config

__all__ = ['pairwise_nlog', 'pairwise_nlog_forward', 'pairwise_nlog_backward', 'PairwiseNLog',
           'boxinst_mask_loss', 'BoxInstMaskLoss', 'dynamic_mask_forward', 'DynamicMaskHead', 'paste_masks', 'paste_masks_device', 'color_affinity', 'box_bitmasks',
           'CondInstMaskHead', 'HEADS', 'build_head', 'load_config',
           'MeanField', 'meanfield_kernel', 'meanfield_forward', 'dice_loss', 'mil_loss',
           'BoxProjectionLoss', 'LevelsetLoss', 'region_levelset', 'LocalConsistencyModule', 'LCM', 'LOSSES', 'build_loss',
           'MinimumSpanningTree', 'TreeFilter2D', 'mst', 'bfs', 'refine',
           'mask_matrix_nms', 'seg_nms', 'box_solov2_get_seg_single', 'discobox_get_seg_single',
           'seg_paste', 'solo_get_seg', 'solo_format_results',
           'ClassificationCost', 'BoxMatchingCost', 'MaskHungarianAssigner', 'box2mask_get_targets', 'MATCH_COST', 'BBOX_ASSIGNERS',
           'build_match_cost', 'build_assigner', 'nms', 'batched_nms', 'nms_with_others', 'condinst_get_bboxes',
           'condinst_box_targets', 'condinst_box_loss', 'parse_box_head_cfg',
           'solov2_targets', 'box_solov2_targets', 'solo_cate_loss', 'parse_solo_head_cfg', 'SoloTargets',
           'ObjectBank', 'SemanticCorrSolver', 'superres_T', 'corr_objects', 'parse_corr_cfg',
           'roi_align', 'RoIAlign', 'relu_and_l2_norm_feat', 'roi_feat_norm', 'sigmoid_roi_masks', 'target_boxes', 'corr_level',
           'multi_scale_deformable_attn', 'multi_scale_deformable_attn_fused', 'MultiScaleDeformableAttention', 'ATTENTION', 'build_attention',
           'solo_dynamic_masks', 'solo_dynamic_masks_pair', 'solo_candidate_masks',
           'box_solov2_ins_preds', 'box_solov2_set_cells', 'box_solov2_get_seg_single_kernels',
           'PackedAttnMask', 'attn_mask_bits', 'box2mask_attn_mask', 'pack_attn_mask', 'masked_attention', 'MultiheadAttention',
           'instance_topk', 'box2mask_instances', 'MaskFormerFusionHead', 'box2mask_format_results',
           'rle_encode', 'rle_decode', 'EncodedMasks', 'solo_encode_results', 'box2mask_encode_results',
           'box2mask_loss', 'Box2MaskLossContext', 'box2mask_mask_losses', 'parse_box2mask_head_cfg',
           'discobox_loss', 'discobox_pseudo_losses', 'live_means', 'parse_discobox_loss_cfg',
           'box_solov2_loss', 'BoxLevelSetLossContext', 'box_solov2_mask_losses', 'parse_box_solov2_loss_cfg']
__version__ = '0.1.0'
