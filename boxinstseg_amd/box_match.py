"""Target assignment of one Box2Mask decoder layer: projection matching cost and Hungarian assignment on the GPU
(csrc/box_match.hip, include/boxinst/boxinst_hip_assign.h).

    ClassificationCost      <-> mmdet.core.bbox.match_costs.ClassificationCost (match_cost.py:153-193)
    BoxMatchingCost         <-> mmdet.core.bbox.match_costs.BoxMatchingCost (match_cost.py:365-425)
    MaskHungarianAssigner   <-> mmdet.core.bbox.assigners.MaskHungarianAssigner (mask_hungarian_assigner.py:16-132)
    box2mask_get_targets    <-> Box2MaskHead.get_targets + _get_target_single (box2mask_head.py:135-189), the whole batch at once

The reference up-samples the predictions to the ground-truth canvas, takes their sigmoid, projects them, copies the cost to the
host and solves the assignment with scipy.  Here the projections are taken from the logits as they are sampled (nothing of the
up-sampled size is ever stored), the cost of all images is one launch, the assignment of all images another, and nothing is read
back: the numbers the host needs (``min(Q, G_i)`` positives per image) follow from the shapes.

There is no CPU or PyTorch fallback: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _lib
from ._common import current_stream, need_cuda, ptr
from .registry import BBOX_ASSIGNERS, MATCH_COST, build_match_cost

__all__ = ['ClassificationCost', 'BoxMatchingCost', 'MaskHungarianAssigner', 'AssignResult', 'box2mask_get_targets',
           'project_pred', 'project_gt', 'match_cost', 'linear_sum_assignment']


def _offsets(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + int(c))
    return out


def _workspace(n, H, W, dev):
    nbytes = _lib.load().bxi_box_match_workspace_bytes(n, H, W)
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)


def _proj_outputs(n, H, W, dev):
    return (torch.empty((n, H), dtype=torch.float32, device=dev), torch.empty((n, W), dtype=torch.float32, device=dev),
            torch.empty((n, 2), dtype=torch.float32, device=dev))


def project_pred(logits: torch.Tensor, target_shape=None, act: bool = True):
    """``logits`` [n,h,w] fp32 -> (proj_rows [n,H], proj_cols [n,W], sumsq [n,2]) of the predictions bilinearly sampled at
    ``target_shape`` = (H, W) (``align_corners=False``; None: the logits' own size): the maximum of every row and of every column, after
    the sigmoid when ``act``, and the sum of squares of each projection.  Nothing of size n*H*W is allocated."""
    need_cuda(logits=logits)
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise RuntimeError(f'logits must be fp32 [n,h,w], got {logits.dtype} {tuple(logits.shape)}')
    dev = logits.device
    x = logits.detach().contiguous()
    n, h, w = x.shape
    H, W = (h, w) if target_shape is None else (int(target_shape[0]), int(target_shape[1]))
    rows, cols, sumsq = _proj_outputs(n, H, W, dev)
    ws = _workspace(n, H, W, dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_match_project_pred_f32', _lib.load().bxi_match_project_pred_f32(
            x.data_ptr(), n, h, w, H, W, 1 if act else 0, rows.data_ptr(), cols.data_ptr(), sumsq.data_ptr(), ws.data_ptr(), ws.numel() * 4,
            current_stream(dev)))
    return rows, cols, sumsq


def _project_gt_into(masks, rows, cols, sumsq, ws):
    dev = masks.device
    m = masks.detach().contiguous()
    g, H, W = m.shape
    lib = _lib.load()
    with torch.cuda.device(dev):
        if m.dtype in (torch.bool, torch.uint8):
            m = m.view(torch.uint8) if m.dtype == torch.bool else m
            _lib.check('bxi_match_project_gt_u8', lib.bxi_match_project_gt_u8(
                m.data_ptr(), g, H, W, rows.data_ptr(), cols.data_ptr(), sumsq.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))
        else:
            m = m.to(torch.float32)
            _lib.check('bxi_match_project_gt_f32', lib.bxi_match_project_gt_f32(
                m.data_ptr(), g, H, W, rows.data_ptr(), cols.data_ptr(), sumsq.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))


def project_gt(masks: torch.Tensor):
    """``masks`` [g,H,W] bool / uint8 / float -> (proj_rows [g,H], proj_cols [g,W], sumsq [g,2]) as fp32."""
    need_cuda(masks=masks)
    if masks.dim() != 3:
        raise RuntimeError(f'masks must be [g,H,W], got {tuple(masks.shape)}')
    g, H, W = masks.shape
    rows, cols, sumsq = _proj_outputs(g, H, W, masks.device)
    if g:
        _project_gt_into(masks, rows, cols, sumsq, _workspace(g, H, W, masks.device))
    return rows, cols, sumsq


def _project_gt_list(masks_list, H, W, dev):
    """One projection launch pair per image, written into the slices of one set of outputs: the masks are never concatenated."""
    counts = [int(m.shape[0]) for m in masks_list]
    total = sum(counts)
    rows, cols, sumsq = _proj_outputs(total, H, W, dev)
    if total:
        ws = _workspace(max(counts), H, W, dev)
        at = 0
        for m, g in zip(masks_list, counts):
            if g:
                _project_gt_into(m, rows[at:at + g], cols[at:at + g], sumsq[at:at + g], ws)
            at += g
    return rows, cols, sumsq


def match_cost(cls, gt_labels, pred_proj, gt_proj, Q, counts, w_cls, w_dice, eps):
    """The cost blocks of P problems in one launch: ``cls`` [P*Q, C] logits or None, ``gt_labels`` [sum(counts)] int64, ``pred_proj`` /
    ``gt_proj`` the triples of project_pred / project_gt (or None when ``w_dice`` is 0).  Returns (cost, status): ``cost`` is flat,
    problem p a row-major [Q, counts[p]] block at ``offsets[p] * Q``; ``status`` [P] int32 is non-zero where a label is outside [0, C)."""
    offsets = _offsets(counts)
    P, total = len(counts), offsets[-1]
    dev = (cls if cls is not None else pred_proj[0]).device
    cost = torch.empty(max(total * Q, 1), dtype=torch.float32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    C = 0
    if cls is not None:
        cls = cls.detach().to(torch.float32).contiguous()
        C = cls.shape[-1]
    labels = gt_labels.detach().to(torch.int64).contiguous()
    H = W = 1
    pp = gp = (None, None, None)
    if pred_proj is not None and gt_proj is not None:
        pp, gp = pred_proj, gt_proj
        H, W = pp[0].shape[-1], pp[1].shape[-1]
        if gp[0].shape[-1] != H or gp[1].shape[-1] != W:
            raise RuntimeError(f'projections of {H}x{W} predictions and {gp[0].shape[-1]}x{gp[1].shape[-1]} ground truths')
    with torch.cuda.device(dev):
        _lib.check('bxi_match_cost_f32', _lib.load().bxi_match_cost_f32(
            ptr(cls), C, labels.data_ptr(), ptr(pp[0]), ptr(pp[1]), ptr(pp[2]), ptr(gp[0]), ptr(gp[1]), ptr(gp[2]), P, Q,
            _lib.int_array(offsets), H, W, float(w_cls), float(w_dice), float(eps), cost.data_ptr(), status.data_ptr(), current_stream(dev)))
    return cost[:total * Q], status


def linear_sum_assignment(cost, gt_labels, Q, counts):
    """Exact assignment of P problems in one launch.  ``cost`` as match_cost returns it (for one problem: a contiguous [Q, G] fp32
    matrix), ``gt_labels`` [sum(counts)] int64.  Returns (assigned_gt_inds [P,Q], assigned_labels [P,Q], pos_inds, pos_assigned_gt_inds,
    status [P]): the compacted arrays hold ``min(Q, counts[p])`` entries per problem, one problem after the other."""
    need_cuda(cost=cost, gt_labels=gt_labels)
    offsets = _offsets(counts)
    P, total = len(counts), offsets[-1]
    dev = cost.device
    cost = cost.detach().to(torch.float32).contiguous()
    if cost.numel() != total * Q:
        raise RuntimeError(f'cost has {cost.numel()} elements for {Q} queries and {total} ground truths')
    labels = gt_labels.detach().to(torch.int64).contiguous()
    npos = sum(min(Q, int(c)) for c in counts)
    gt_inds = torch.empty((P, Q), dtype=torch.int64, device=dev)
    out_labels = torch.empty((P, Q), dtype=torch.int64, device=dev)
    pos = torch.empty(npos, dtype=torch.int64, device=dev)
    pos_gt = torch.empty(npos, dtype=torch.int64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_linear_sum_assignment_f32', _lib.load().bxi_linear_sum_assignment_f32(
            cost.data_ptr(), labels.data_ptr(), P, Q, _lib.int_array(offsets), gt_inds.data_ptr(), out_labels.data_ptr(), pos.data_ptr(),
            pos_gt.data_ptr(), status.data_ptr(), current_stream(dev)))
    return gt_inds, out_labels, pos, pos_gt, status


def _as_planes(t, name):
    """[n,H,W] from the reference's [n,1,H,W] (match_cost.py:400-425) or from [n,H,W]."""
    if t.dim() == 4 and t.shape[1] == 1:
        return t[:, 0]
    if t.dim() == 3:
        return t
    raise RuntimeError(f'{name} must be [n,1,H,W] or [n,H,W], got {tuple(t.shape)}')


@MATCH_COST.register_module()
class ClassificationCost:
    """``-softmax(cls_pred)[:, gt_labels] * weight`` (match_cost.py:153-193)."""

    def __init__(self, weight=1.):
        self.weight = weight

    def __call__(self, cls_pred, gt_labels):
        need_cuda(cls_pred=cls_pred, gt_labels=gt_labels)
        Q, G = cls_pred.shape[0], gt_labels.shape[0]
        if Q == 0 or G == 0:
            return cls_pred.new_zeros((Q, G), dtype=torch.float32)
        if self.weight == 0:
            return cls_pred.new_zeros((Q, G), dtype=torch.float32)
        cost, _ = match_cost(cls_pred, gt_labels, None, None, Q, [G], self.weight, 0.0, 0.0)
        return cost.view(Q, G)


@MATCH_COST.register_module()
class BoxMatchingCost:
    """Dice cost of the row and column projections of the predicted masks against those of the box masks (match_cost.py:365-425)."""

    def __init__(self, weight=1., pred_act=False, eps=1e-3):
        self.weight = weight
        self.pred_act = pred_act
        self.eps = eps

    def projections(self, mask_preds, target_shape=None):
        return project_pred(_as_planes(mask_preds, 'mask_preds').float(), target_shape, self.pred_act)

    def __call__(self, mask_preds, gt_box_masks, target_shape=None):
        """``mask_preds`` [n,1,H,W] / [n,H,W] logits at the ground truths' size -- or at their own size with ``target_shape`` = (H, W),
        then sampled as ``F.interpolate(..., mode='bilinear', align_corners=False)`` would without being stored;  ``gt_box_masks``
        [g,1,H,W] / [g,H,W].  Returns the [n, g] cost."""
        need_cuda(mask_preds=mask_preds, gt_box_masks=gt_box_masks)
        gt = _as_planes(gt_box_masks, 'gt_box_masks')
        n, g = mask_preds.shape[0], gt.shape[0]
        if n == 0 or g == 0:
            return mask_preds.new_zeros((n, g), dtype=torch.float32)
        cost, _ = match_cost(None, gt.new_zeros(g, dtype=torch.int64), self.projections(mask_preds, target_shape or gt.shape[-2:]),
                             project_gt(gt), n, [g], 0.0, self.weight, self.eps)
        return cost.view(n, g)


class _NoCost:
    """A cost of the reference this package does not compute, accepted at weight 0 (where the reference skips it too)."""

    def __init__(self, cfg):
        self.cfg, self.weight = dict(cfg), 0.0


class AssignResult:
    """The fields of mmdet's AssignResult that MaskHungarianAssigner fills, and the pseudo sampler's two index arrays."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None, pos_inds=None, pos_assigned_gt_inds=None, status=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels
        self.pos_inds, self.pos_assigned_gt_inds, self.status = pos_inds, pos_assigned_gt_inds, status

    @property
    def num_preds(self):
        return len(self.gt_inds)


@BBOX_ASSIGNERS.register_module()
class MaskHungarianAssigner:
    """One-to-one matching of queries and ground truths by classification and projection-dice cost
    (mask_hungarian_assigner.py:16-132).  ``dice_cost`` must be a BoxMatchingCost, ``mask_cost`` is accepted at weight 0 only (the
    default of the reference and what its Box2Mask configs use)."""

    def __init__(self, cls_cost=dict(type='ClassificationCost', weight=1.0),
                 mask_cost=dict(type='FocalLossCost', weight=0.0, binary_input=True),
                 dice_cost=dict(type='BoxMatchingCost', weight=1.0)):
        if dict(mask_cost).get('weight', 1.0) != 0:
            raise TypeError(f'mask_cost {dict(mask_cost).get("type")} at a non-zero weight is not supported: MaskHungarianAssigner '
                            'computes ClassificationCost and BoxMatchingCost only (mask_cost must have weight=0.0)')
        if dict(cls_cost).get('type') not in ('ClassificationCost', ClassificationCost) or \
                dict(dice_cost).get('type') not in ('BoxMatchingCost', BoxMatchingCost):
            raise TypeError(f'cls_cost {dict(cls_cost).get("type")} / dice_cost {dict(dice_cost).get("type")}: supported are '
                            "cls_cost=dict(type='ClassificationCost') and dice_cost=dict(type='BoxMatchingCost')")
        self.cls_cost = build_match_cost(cls_cost)
        self.mask_cost = _NoCost(mask_cost)
        self.dice_cost = build_match_cost(dice_cost)
        self.last_status = None

    def assign_batch(self, cls_scores, mask_preds, gt_labels_list, gt_masks_list, target_shape=None):
        """All images of a batch: ``cls_scores`` [B,Q,C] or None, ``mask_preds`` [B,Q,h,w], per image ``gt_labels`` [G_i] and ``gt_masks``
        [G_i,H,W] (one H x W for the batch).  Returns (gt_inds [B,Q], labels [B,Q], pos_inds, pos_assigned_gt_inds, counts): launches only,
        nothing is read back.  ``last_status`` keeps the two device status words per image (cost: bad label, solver: non-finite cost)."""
        need_cuda(cls_scores=cls_scores, mask_preds=mask_preds)
        need_cuda(**{f'gt_labels_list[{i}]': t for i, t in enumerate(gt_labels_list)})
        need_cuda(**{f'gt_masks_list[{i}]': t for i, t in enumerate(gt_masks_list)})
        B, Q = mask_preds.shape[:2]
        if len(gt_labels_list) != B or len(gt_masks_list) != B:
            raise RuntimeError(f'{B} images but {len(gt_labels_list)} label and {len(gt_masks_list)} mask entries')
        dev = mask_preds.device
        gt_masks_list = [_as_planes(m, 'gt_masks') for m in gt_masks_list]
        counts = [int(t.shape[0]) for t in gt_labels_list]
        if [int(m.shape[0]) for m in gt_masks_list] != counts:
            raise RuntimeError('gt_labels_list and gt_masks_list disagree on the number of ground truths')
        if target_shape is None:
            target_shape = tuple(gt_masks_list[0].shape[-2:])
        H, W = int(target_shape[0]), int(target_shape[1])
        if any(tuple(m.shape[-2:]) != (H, W) for m in gt_masks_list):
            raise RuntimeError(f'every image of the batch must carry its ground-truth masks on the same {H}x{W} canvas')
        labels_cat = torch.cat([t.to(torch.int64) for t in gt_labels_list]) if B else mask_preds.new_zeros(0, dtype=torch.int64)
        w_cls = self.cls_cost.weight if cls_scores is not None else 0.0
        w_dice = self.dice_cost.weight
        pred = gt = None
        if w_dice != 0 and sum(counts):
            pred = project_pred(mask_preds.detach().float().reshape(B * Q, *mask_preds.shape[-2:]), (H, W), self.dice_cost.pred_act)
            gt = _project_gt_list(gt_masks_list, H, W, dev)
        cls = None if (cls_scores is None or w_cls == 0) else cls_scores.reshape(B * Q, -1)
        if cls is None and pred is None:            # no cost at all: a zero matrix, as the reference's `cost = 0 + 0 + 0` would be
            cost, cost_status = torch.zeros(sum(counts) * Q, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        else:
            cost, cost_status = match_cost(cls, labels_cat, pred, gt, Q, counts, w_cls, w_dice if pred is not None else 0.0, self.dice_cost.eps)
        gt_inds, labels, pos, pos_gt, lsa_status = linear_sum_assignment(cost, labels_cat, Q, counts)
        self.last_status = (cost_status, lsa_status)
        return gt_inds, labels, pos, pos_gt, counts

    def assign(self, cls_pred, mask_pred, gt_labels, gt_mask, img_meta=None, gt_bboxes_ignore=None, eps=1e-7, target_shape=None):
        """``mask_pred`` [Q,H,W] / [Q,1,H,W] at the ground truths' size, as the reference passes it, or at the prediction size together
        with ``target_shape`` (nothing is up-sampled in memory then).  Returns an AssignResult: ``gt_inds`` 0 background / g + 1,
        ``labels`` -1 or the matched label, ``max_overlaps`` None."""
        assert gt_bboxes_ignore is None, 'Only case when gt_bboxes_ignore is None is supported.'
        need_cuda(cls_pred=cls_pred, mask_pred=mask_pred, gt_labels=gt_labels, gt_mask=gt_mask)
        num_gt, num_query = gt_labels.shape[0], mask_pred.shape[0]
        if num_query == 0:
            empty = mask_pred.new_full((0,), -1, dtype=torch.long)
            return AssignResult(num_gt, empty, None, labels=empty.clone())
        mask_pred = _as_planes(mask_pred, 'mask_pred')
        gt_mask = _as_planes(gt_mask, 'gt_mask')
        gt_inds, labels, pos, pos_gt, _ = self.assign_batch(None if cls_pred is None else cls_pred[None], mask_pred[None], [gt_labels], [gt_mask],
                                                             target_shape)
        return AssignResult(num_gt, gt_inds[0], None, labels=labels[0], pos_inds=pos, pos_assigned_gt_inds=pos_gt, status=self.last_status)


def box2mask_get_targets(cls_scores, mask_preds, gt_labels_list, gt_masks_list, assigner, num_classes):
    """``Box2MaskHead.get_targets`` (box2mask_head.py:135-189) for one decoder layer and the whole batch: ``cls_scores`` [B,Q,C+1],
    ``mask_preds`` [B,Q,h,w] logits at prediction size, per image ``gt_labels`` [G_i] and ``gt_masks`` [G_i,H,W].  One projection of the
    predictions, one per image of the ground truths, one cost launch, one assignment launch, then the gathers in torch; no ``.cpu()``,
    no ``.item()``, nothing of size Q*H*W.  Returns (labels_list, label_weights_list, mask_targets_list, mask_weights_list,
    num_total_pos, num_total_neg), the two totals Python ints from ``min(Q, G_i)``.  An image whose cost is not finite (the assigner's
    ``last_status``) comes back all background, and its ``mask_targets`` rows are those of its first ground truth."""
    need_cuda(cls_scores=cls_scores, mask_preds=mask_preds)
    B, Q = mask_preds.shape[:2]
    gt_inds, assigned, _, pos_gt, counts = assigner.assign_batch(cls_scores, mask_preds, gt_labels_list, gt_masks_list)
    labels_list, label_weights_list, mask_targets_list, mask_weights_list = [], [], [], []
    at = num_total_pos = 0
    for i in range(B):
        npos = min(Q, counts[i])
        matched = gt_inds[i] > 0
        labels_list.append(torch.where(matched, assigned[i], assigned[i].new_full((), num_classes)).to(gt_labels_list[i].dtype))
        label_weights_list.append(gt_labels_list[i].new_ones((Q,)))
        gt_masks = gt_masks_list[i] if gt_masks_list[i].dim() == 4 else gt_masks_list[i].unsqueeze(1)
        mask_targets_list.append(gt_masks[pos_gt[at:at + npos].clamp(min=0)])
        mask_weights_list.append(matched.to(mask_preds.dtype))
        at += npos
        num_total_pos += npos
    return labels_list, label_weights_list, mask_targets_list, mask_weights_list, num_total_pos, B * Q - num_total_pos
