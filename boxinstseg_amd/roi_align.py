"""RoIAlign and the front of one level of DiscoBox's ``corr_loss`` on the HIP kernels of ``csrc/roi_align.hip``
(include/boxinst/boxinst_hip_roi.h).

    roi_align / RoIAlign     <-> mmcv.ops.roi_align / RoIAlign, pool_mode='avg' (the reference builds two at discobox_head.py:740-742)
    relu_and_l2_norm_feat    <-> relu_and_l2_norm_feat (:16-20)
    target_boxes             <-> the boxes of the non-zero target masks and the label every object of the loop reads (:1025-1038)
    corr_level               <-> :1018-1127 for one level: the front on the device, then ``corr.corr_objects``; nothing is read back

mmcv's arithmetic is restated from its documented algorithm and is unpinned: mmcv never ran next to this library (INTEGRATION.md,
Level 3h).  Thin marshalling only: there is no CPU and no torch path for the pooling; everything is fp32 at the ABI.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import current_stream, need_cuda
from .corr import FEAT, MASK, ObjectBank, SemanticCorrSolver, corr_objects


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError('output_size must be an int or a pair')
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _check(input, rois, PH, PW, spatial_scale, sampling_ratio):
    if input.dim() != 4:
        raise RuntimeError(f'input must be [B,C,H,W], got {list(input.shape)}')
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError(f'rois must be [K,5] (batch index, x1, y1, x2, y2), got {list(rois.shape)}')
    if not 1 <= PH <= _lib.ROI_MAX_POOL or not 1 <= PW <= _lib.ROI_MAX_POOL:
        raise ValueError(f'output_size must be in 1..{_lib.ROI_MAX_POOL}')
    if not 0 <= int(sampling_ratio) <= _lib.ROI_MAX_SAMPLING:
        raise ValueError(f'sampling_ratio must be in 0..{_lib.ROI_MAX_SAMPLING} (0 = adaptive)')
    if math.isnan(float(spatial_scale)):
        raise ValueError('spatial_scale is NaN')
    need_cuda(input=input, rois=rois)
    if input.device != rois.device:
        raise RuntimeError('input and rois must be on the same device')


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _forward(x, rois, PH, PW, scale, sr, aligned, flags=0):
    B, C, H, W = (int(s) for s in x.shape)
    K = int(rois.shape[0])
    out = torch.empty((K, C, PH, PW), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check('bxi_roi_align_forward_f32', _lib.load().bxi_roi_align_forward_f32(
            x.data_ptr(), rois.data_ptr(), B, C, H, W, K, PH, PW, float(scale), int(sr), int(bool(aligned)), int(flags), out.data_ptr(),
            current_stream(x.device)))
    return out


class _RoIAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, rois, PH, PW, scale, sr, aligned):
        x, r = _f32c(input), _f32c(rois)
        ctx.save_for_backward(r)
        ctx.args = (tuple(int(s) for s in x.shape), PH, PW, float(scale), int(sr), bool(aligned), input.dtype)
        return _forward(x, r, PH, PW, scale, sr, aligned).to(input.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        (B, C, H, W), PH, PW, scale, sr, aligned, dtype = ctx.args
        g = g.to(torch.float32).contiguous()
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check('bxi_roi_align_backward_f32', _lib.load().bxi_roi_align_backward_f32(
                g.data_ptr(), r.data_ptr(), B, C, H, W, int(r.shape[0]), PH, PW, scale, sr, int(aligned), out.data_ptr(), current_stream(g.device)))
        return out.to(dtype), None, None, None, None, None, None


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    """mmcv's ``roi_align``: ``input [B,C,H,W]``, ``rois [K,5]`` (batch index, x1, y1, x2, y2) -> ``[K,C,PH,PW]`` in the input's dtype,
    differentiable w.r.t. ``input`` (half and bf16 are computed in fp32).  A roi with a batch index outside ``[0,B)`` or a non-finite
    coordinate gives a zero row.  ``pool_mode='max'`` is not built."""
    if pool_mode != 'avg':
        raise NotImplementedError(f"pool_mode={pool_mode!r} is not built: only 'avg'")
    PH, PW = _pair(output_size)
    _check(input, rois, PH, PW, spatial_scale, sampling_ratio)
    return _RoIAlign.apply(input, rois, PH, PW, float(spatial_scale), int(sampling_ratio), bool(aligned))


class RoIAlign(nn.Module):
    """mmcv's ``RoIAlign`` module, same constructor; ``use_torchvision`` is accepted and ignored."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True, use_torchvision=False):
        super().__init__()
        if pool_mode != 'avg':
            raise NotImplementedError(f"pool_mode={pool_mode!r} is not built: only 'avg'")
        self.output_size = _pair(output_size)
        self.spatial_scale, self.sampling_ratio, self.pool_mode, self.aligned = float(spatial_scale), int(sampling_ratio), pool_mode, bool(aligned)
        self.use_torchvision = use_torchvision

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.pool_mode, self.aligned)

    def __repr__(self):
        return (f'{self.__class__.__name__}(output_size={self.output_size}, spatial_scale={self.spatial_scale}, sampling_ratio={self.sampling_ratio}, '
                f'pool_mode={self.pool_mode}, aligned={self.aligned}, use_torchvision={self.use_torchvision})')


def relu_and_l2_norm_feat(feat, dim=1):
    """The reference's helper (:16-20) on a tensor the caller already has, out of place: relu, ``n = sqrt(sum f^2 + 1e-6)``, ``f / (n + 1e-6)``.
    Differentiable torch arithmetic; ``corr_level`` does not come through here, its feature path is the fused kernel."""
    need_cuda(feat=feat)
    feat = torch.relu(feat)
    return feat / (((feat ** 2).sum(dim=dim, keepdim=True) + 1e-6) ** 0.5 + 1e-6)


class _RoIFeatNorm(torch.autograd.Function):
    """relu_and_l2_norm_feat(RoIAlign 7 x 7) in one launch; the backward goes through the norm, the relu and the pooling."""

    @staticmethod
    def forward(ctx, feat, rois, scale, sr, aligned):
        x, r = _f32c(feat), _f32c(rois)
        B, C, H, W = (int(s) for s in x.shape)
        K, lib = int(r.shape[0]), _lib.load()
        nbytes = lib.bxi_roi_feat_norm_workspace_bytes(K, C)
        if nbytes == 0:
            raise RuntimeError(f'the fused feature path takes 1..{_lib.ROI_FUSED_MAX_C} channels, got {C}')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        out = torch.empty((K, C, FEAT, FEAT), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check('bxi_roi_feat_norm_forward_f32', lib.bxi_roi_feat_norm_forward_f32(
                x.data_ptr(), r.data_ptr(), B, C, H, W, K, float(scale), int(sr), int(bool(aligned)), out.data_ptr(), ws.data_ptr(), ws.numel(),
                current_stream(x.device)))
        ctx.save_for_backward(r, out, ws)
        ctx.args = ((B, C, H, W), float(scale), int(sr), bool(aligned), feat.dtype)
        return out.to(feat.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r, out, ws = ctx.saved_tensors
        (B, C, H, W), scale, sr, aligned, dtype = ctx.args
        g = g.to(torch.float32).contiguous()
        grad = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check('bxi_roi_feat_norm_backward_f32', _lib.load().bxi_roi_feat_norm_backward_f32(
                out.data_ptr(), g.data_ptr(), r.data_ptr(), B, C, H, W, int(r.shape[0]), scale, sr, int(aligned), grad.data_ptr(), ws.data_ptr(),
                ws.numel(), current_stream(g.device)))
        return grad.to(dtype), None, None, None, None


def roi_feat_norm(feat, rois, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    """``relu_and_l2_norm_feat(RoIAlign((7, 7))(feat, rois))`` fused (:1040-1044): ``[K,C,7,7]``, differentiable w.r.t. ``feat``.  Up to
    ``_lib.ROI_FUSED_MAX_C`` channels; compose ``roi_align`` and ``relu_and_l2_norm_feat`` beyond."""
    _check(feat, rois, FEAT, FEAT, spatial_scale, sampling_ratio)
    if not 1 <= int(feat.shape[1]) <= _lib.ROI_FUSED_MAX_C:
        raise RuntimeError(f'the fused feature path takes 1..{_lib.ROI_FUSED_MAX_C} channels, got {int(feat.shape[1])}')
    return _RoIFeatNorm.apply(feat, rois, float(spatial_scale), int(sampling_ratio), bool(aligned))


def sigmoid_roi_masks(logits, boxes):
    """``mask_roi_align(sigmoid(logits).unsqueeze(1), [arange(N), boxes])`` (:1018, :1050-1053): ``logits [N,H,W]``, ``boxes [N,4]`` ->
    ``[N,28,28]``; object i is pooled from its own plane, the sigmoid is taken of the taps.  No gradient (the reference detaches)."""
    if logits.dim() != 3 or tuple(boxes.shape) != (int(logits.shape[0]), 4):
        raise RuntimeError(f'logits must be [N,H,W] and boxes [N,4], got {list(logits.shape)} and {list(boxes.shape)}')
    need_cuda(logits=logits, boxes=boxes)
    N, H, W = (int(s) for s in logits.shape)
    x = _f32c(logits).view(N, 1, H, W)
    rois = torch.cat([torch.arange(N, dtype=torch.float32, device=x.device).unsqueeze(1), _f32c(boxes)], 1)
    return _forward(x, rois, MASK, MASK, 1.0, 0, True, _lib.ROI_SIGMOID).view(N, MASK, MASK)


def target_boxes(target, kernel_labels, own_labels=False):
    """``target [N,H,W]`` (uint8 or bool), ``kernel_labels [N]`` -> ``(boxes [N,4] fp32, keep [N] bool, labels [N] int64)``:
    ``(min_x, min_y, max_x + 1, max_y + 1)`` of the non-zero pixels (zeros for an all-zero target, which is dropped: ``keep`` False,
    label -1).  A kept object's label is ``kernel_labels[its rank among the kept]``, as the reference reads it after filtering the objects
    but not the labels (:1029, :1064); ``own_labels=True`` gives it ``kernel_labels[its own index]``."""
    if target.dim() != 3 or target.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError(f'target must be a uint8 or bool [N,H,W], got {target.dtype} {list(target.shape)}')
    N, H, W = (int(s) for s in target.shape)
    if tuple(kernel_labels.shape) != (N,):
        raise RuntimeError(f'kernel_labels must be [{N}], got {list(kernel_labels.shape)}')
    if H < 1 or W < 1:
        raise RuntimeError('target planes must not be empty')
    need_cuda(target=target, kernel_labels=kernel_labels)
    dev = target.device
    t = target.detach().contiguous()
    t = t.view(torch.uint8) if t.dtype == torch.bool else t
    lab = kernel_labels.detach().to(torch.int64).contiguous()
    boxes = torch.empty((N, 4), dtype=torch.float32, device=dev)
    keep = torch.empty((N,), dtype=torch.uint8, device=dev)
    labels = torch.empty((N,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_roi_target_boxes_u8', _lib.load().bxi_roi_target_boxes_u8(
            t.data_ptr(), lab.data_ptr(), N, H, W, int(bool(own_labels)), boxes.data_ptr(), keep.data_ptr(), labels.data_ptr(), current_stream(dev)))
    return boxes, keep.view(torch.bool), labels


def corr_level(s_input, t_input, target, img_inds, kernel_labels, s_feat, t_feat, bank: ObjectBank, solver: SemanticCorrSolver, min_size,
               min_objs=5, own_labels=False, details=None):
    """One level of ``DiscoBoxSOLOv2Head.corr_loss`` (:1018-1127) without a host synchronisation.  ``s_input`` / ``t_input [N,H,W]``: the raw
    mask predictions (``t_input`` may be ``s_input``: no independent teacher, the mask path then runs once); ``target [N,H,W]`` uint8;
    ``img_inds [N]`` (any dtype); ``kernel_labels [N]``; ``s_feat`` / ``t_feat [B,C,H,W]`` (the teacher's is detached).

    Returns ``(loss_sum, num_ins, iiu, keep)``: ``loss_sum`` differentiable w.r.t. ``s_feat``; ``iiu [N,2,H,W]`` with zero rows for the
    dropped (all-zero target) objects, where the reference has a shorter tensor; ``keep [N]`` bool.  Dropped objects go through
    ``corr_objects`` with label -1: they retrieve nothing and are never appended, the order of the rest is the loop's."""
    if s_input.dim() != 3 or tuple(t_input.shape) != tuple(s_input.shape) or tuple(target.shape) != tuple(s_input.shape):
        raise RuntimeError(f's_input, t_input and target must be the same [N,H,W], got {list(s_input.shape)}, {list(t_input.shape)}, {list(target.shape)}')
    N, H, W = (int(s) for s in s_input.shape)
    if tuple(img_inds.shape) != (N,):
        raise RuntimeError(f'img_inds must be [{N}], got {list(img_inds.shape)}')
    if s_feat.dim() != 4 or tuple(t_feat.shape) != tuple(s_feat.shape):
        raise RuntimeError(f's_feat and t_feat must be the same [B,C,H,W], got {list(s_feat.shape)} and {list(t_feat.shape)}')
    need_cuda(s_input=s_input, t_input=t_input, target=target, img_inds=img_inds, kernel_labels=kernel_labels, s_feat=s_feat, t_feat=t_feat)
    boxes, keep, labels = target_boxes(target, kernel_labels, own_labels)
    rois = torch.cat([img_inds.detach().to(torch.float32).view(N, 1), boxes], 1)
    roi_s_feat = roi_feat_norm(s_feat, rois)
    with torch.no_grad():
        roi_t_feat = roi_feat_norm(t_feat.detach(), rois)
        roi_s_mask = sigmoid_roi_masks(s_input, boxes)
        roi_t_mask = roi_s_mask if t_input is s_input else sigmoid_roi_masks(t_input, boxes)
    loss_sum, num_ins, iiu = corr_objects(roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, labels, bank, solver, (H, W), min_size, min_objs,
                                          details=details)
    if details is not None:
        details.update(boxes=boxes, labels=labels, keep=keep, roi_s_feat=roi_s_feat, roi_t_feat=roi_t_feat, roi_s_mask=roi_s_mask, roi_t_mask=roi_t_mask)
    return loss_sum, num_ins, iiu, keep
