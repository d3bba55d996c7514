"""The training step of CondInst's box head on the GPU: FCOS target assignment, sigmoid focal loss, IoU / GIoU loss and centerness
loss with their gradients (csrc/fcos_loss.hip, include/boxinst/boxinst_hip_fcos.h).

    condinst_box_targets  <-> CondInstBoxHead.get_targets / _get_target_single / centerness_target (condinst_head.py:478-633, :855-874)
    condinst_box_loss     <-> CondInstBoxHead.loss (condinst_head.py:365-476)
    parse_box_head_cfg    : the ``bbox_head=dict(type='CondInstBoxHead', ...)`` block of the reference's configs

The reference loops over the images, expands every quantity to [points, gts], copies all 15 maps into a flattened layout, calls
``nonzero`` and ``len(pos_inds)`` (a host synchronisation each), issues two scalar all-reduces and leaves a long autograd graph of small
ops.  Here the targets of all images and levels are one launch, the losses read the NCHW maps where they lie and write the finished
NCHW gradients in the same sweep (every averaging factor depends on the targets only), the two normalisers travel in ONE 2-word
all-reduce, and nothing synchronises with the host.

Order of the flattened outputs: the reference's training order -- level-major, then image, then y, then x.

Deviations, see the header: an image without ground truth gives background / zeros / -1 (the reference raises on such a batch);
among boxes of equal minimal area the lowest index wins (torch.min on the CPU; a device leaves it open); the focal loss restates
``py_sigmoid_focal_loss`` (mmcv's device op is not part of the reference: restated, unpinned).

There is no CPU or PyTorch fallback: CPU tensors raise.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import _lib
from . import dist as _dist
from ._common import cfg_get, cfg_only, current_stream, need_cuda

__all__ = ['condinst_box_targets', 'condinst_box_loss', 'parse_box_head_cfg', 'BoxTargets', 'INF', 'GT_CHUNK']

INF = 1e8
GT_CHUNK = _lib.FCOS_GT_CHUNK
DEFAULT_REGRESS_RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF))

BoxTargets = namedtuple('BoxTargets', ['labels', 'bbox_targets', 'gt_inds', 'points', 'level_inds', 'img_inds', 'ctr_targets', 'stats',
                                       'status'])


def parse_box_head_cfg(cfg):
    """``bbox_head=dict(type='CondInstBoxHead', ...)`` (dict or namespace) -> the flat settings ``condinst_box_loss`` takes:
    num_classes, strides, regress_ranges, center_sampling, center_sample_radius, norm_on_bbox, gamma, alpha, loss_weight_cls,
    bbox_loss_kind, eps, loss_weight_bbox, loss_weight_centerness.  Keys that only shape the network (in_channels, stacked_convs,
    feat_channels, ...) are accepted and ignored.  A loss type or option that is not built raises NotImplementedError naming the key."""
    kind = cfg_get(cfg, 'type', 'CondInstBoxHead')
    if kind != 'CondInstBoxHead':
        raise NotImplementedError(f"bbox_head.type {kind!r} is not supported: only 'CondInstBoxHead'")
    num_classes = cfg_get(cfg, 'num_classes')
    if num_classes is None:
        raise TypeError('bbox_head has no `num_classes`')
    strides = cfg_get(cfg, 'strides', (4, 8, 16, 32, 64))
    strides = [int(s[0] if isinstance(s, (tuple, list)) else s) for s in strides]
    ranges = cfg_get(cfg, 'regress_ranges', DEFAULT_REGRESS_RANGES)
    ranges = tuple((float(a), float(b)) for a, b in ranges)
    if len(ranges) != len(strides):
        raise TypeError(f'{len(strides)} strides but {len(ranges)} regress_ranges')

    lc = cfg_get(cfg, 'loss_cls', dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0))
    if cfg_get(lc, 'type') != 'FocalLoss':
        raise NotImplementedError(f"loss_cls.type {cfg_get(lc, 'type')!r} is not supported: only 'FocalLoss'")
    cfg_only(lc, 'loss_cls', ('type', 'use_sigmoid', 'gamma', 'alpha', 'loss_weight', 'reduction', 'activated'))
    if not cfg_get(lc, 'use_sigmoid', True):
        raise NotImplementedError('loss_cls.use_sigmoid=False is not supported')
    if cfg_get(lc, 'activated', False):
        raise NotImplementedError('loss_cls.activated=True is not supported')
    if cfg_get(lc, 'reduction', 'mean') != 'mean':
        raise NotImplementedError("loss_cls.reduction: only 'mean' is supported")

    lb = cfg_get(cfg, 'loss_bbox', dict(type='IoULoss', loss_weight=1.0))
    bt = cfg_get(lb, 'type')
    if bt == 'GIoULoss':
        cfg_only(lb, 'loss_bbox', ('type', 'eps', 'reduction', 'loss_weight'))
        bbox_kind = 'giou'
    elif bt == 'IoULoss':
        cfg_only(lb, 'loss_bbox', ('type', 'linear', 'eps', 'reduction', 'loss_weight', 'mode'))
        mode = 'linear' if cfg_get(lb, 'linear', False) else cfg_get(lb, 'mode', 'log')
        if mode not in ('log', 'linear', 'square'):
            raise NotImplementedError(f'loss_bbox.mode {mode!r} is not supported')
        bbox_kind = 'iou_' + mode
    else:
        raise NotImplementedError(f"loss_bbox.type {bt!r} is not supported: only 'GIoULoss' and 'IoULoss'")
    if cfg_get(lb, 'reduction', 'mean') != 'mean':
        raise NotImplementedError("loss_bbox.reduction: only 'mean' is supported")

    ln = cfg_get(cfg, 'loss_centerness', dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    if cfg_get(ln, 'type') != 'CrossEntropyLoss':
        raise NotImplementedError(f"loss_centerness.type {cfg_get(ln, 'type')!r} is not supported: only 'CrossEntropyLoss'")
    cfg_only(ln, 'loss_centerness', ('type', 'use_sigmoid', 'use_mask', 'reduction', 'class_weight', 'loss_weight'))
    if not cfg_get(ln, 'use_sigmoid', False) or cfg_get(ln, 'use_mask', False):
        raise NotImplementedError('loss_centerness: only use_sigmoid=True (binary cross entropy with logits) is supported')
    if cfg_get(ln, 'class_weight') is not None:
        raise NotImplementedError('loss_centerness.class_weight is not supported')
    if cfg_get(ln, 'reduction', 'mean') != 'mean':
        raise NotImplementedError("loss_centerness.reduction: only 'mean' is supported")

    return dict(num_classes=int(num_classes), strides=strides, regress_ranges=ranges,
                center_sampling=bool(cfg_get(cfg, 'center_sampling', True)), center_sample_radius=float(cfg_get(cfg, 'center_sample_radius', 1.5)),
                norm_on_bbox=bool(cfg_get(cfg, 'norm_on_bbox', True)),
                gamma=float(cfg_get(lc, 'gamma', 2.0)), alpha=float(cfg_get(lc, 'alpha', 0.25)), loss_weight_cls=float(cfg_get(lc, 'loss_weight', 1.0)),
                bbox_loss_kind=bbox_kind, eps=float(cfg_get(lb, 'eps', 1e-6)), loss_weight_bbox=float(cfg_get(lb, 'loss_weight', 1.0)),
                loss_weight_centerness=float(cfg_get(ln, 'loss_weight', 1.0)))


_FLAT_KEYS = ('num_classes', 'strides', 'regress_ranges', 'center_sampling', 'center_sample_radius', 'norm_on_bbox', 'gamma', 'alpha',
              'loss_weight_cls', 'bbox_loss_kind', 'eps', 'loss_weight_bbox', 'loss_weight_centerness')


def _settings(cfg):
    """The flat settings: ``cfg`` itself where it already is what :func:`parse_box_head_cfg` returns (checked), else parsed."""
    if not (isinstance(cfg, dict) and all(k in cfg for k in _FLAT_KEYS)):
        return parse_box_head_cfg(cfg)
    try:
        strides = [int(s) for s in cfg['strides']]
        ranges = tuple((float(a), float(b)) for a, b in cfg['regress_ranges'])
    except (TypeError, ValueError) as e:
        raise TypeError(f'settings: `strides` must be integers and `regress_ranges` (lo, hi) pairs: {e}') from None
    if len(ranges) != len(strides) or any(s < 1 for s in strides):
        raise TypeError(f'settings: {len(strides)} strides {strides} but {len(ranges)} regress_ranges')
    if cfg['bbox_loss_kind'] not in _lib.FCOS_BBOX_KINDS:
        raise NotImplementedError(f"bbox_loss_kind {cfg['bbox_loss_kind']!r} is not supported: one of {sorted(_lib.FCOS_BBOX_KINDS)}")
    out = dict(cfg, strides=strides, regress_ranges=ranges, num_classes=int(cfg['num_classes']))
    for k in ('center_sample_radius', 'gamma', 'alpha', 'loss_weight_cls', 'eps', 'loss_weight_bbox', 'loss_weight_centerness'):
        out[k] = float(cfg[k])
    return out


def _fcos_levels(featmap_sizes, strides):
    n = len(featmap_sizes)
    if not (1 <= n <= _lib.DET_MAX_LEVELS) or len(strides) != n:
        raise RuntimeError(f'1..{_lib.DET_MAX_LEVELS} levels with a size and a stride each, got {n} sizes and {len(strides)} strides')
    arr = (_lib.FcosLevel * n)()
    sizes = []
    for i, (hw, s) in enumerate(zip(featmap_sizes, strides)):
        H, W = int(hw[0]), int(hw[1])
        s = int(s[0] if isinstance(s, (tuple, list)) else s)
        if H < 1 or W < 1 or s < 1:
            raise RuntimeError(f'level {i}: size {H}x{W}, stride {s}')
        arr[i] = _lib.FcosLevel(H, W, s)
        sizes.append(H * W)
    return arr, sizes


def _workspace(arr, n, B, C, dev):
    nbytes = _lib.load().bxi_fcos_workspace_bytes(arr, n, B, C)
    if nbytes == 0:
        raise RuntimeError(f'bxi_fcos_workspace_bytes: bad shape (B={B}, C={C})')
    return torch.empty(nbytes // 4, dtype=torch.int32, device=dev)


def condinst_box_targets(featmap_sizes, strides, gt_bboxes, gt_labels, *, regress_ranges, center_sampling, center_sample_radius,
                         norm_on_bbox, num_classes, B, workspace=None):
    """``get_targets`` of all images and levels in one launch.  ``featmap_sizes``: (H, W) per level; ``gt_bboxes`` / ``gt_labels``: per
    image [G_i,4] / [G_i] on the GPU (an image may have none); ``B``: the number of images.  Returns :class:`BoxTargets` -- ``labels``,
    ``bbox_targets``, ``gt_inds`` (global, -1 = background), ``points``, ``level_inds``, ``img_inds``, ``ctr_targets`` over the
    ``N_all = B * sum(H * W)`` locations in training order, ``stats`` (number of positives, sum of ``ctr_targets``) and the ``status``
    word (``_lib.FCOS_STATUS_BAD_LABEL``), all on the device.  No host synchronisation."""
    B = int(B)
    if len(gt_bboxes) != B or len(gt_labels) != B:
        raise RuntimeError(f'{B} images but {len(gt_bboxes)} gt_bboxes and {len(gt_labels)} gt_labels')
    if not 1 <= B <= _lib.BXI_MAX_IMAGES:
        raise RuntimeError(f'B must be in 1..{_lib.BXI_MAX_IMAGES}, got {B}')
    need_cuda(**{f'gt_bboxes[{i}]': t for i, t in enumerate(gt_bboxes)}, **{f'gt_labels[{i}]': t for i, t in enumerate(gt_labels)})
    arr, sizes = _fcos_levels(featmap_sizes, strides)
    n = len(sizes)
    if len(regress_ranges) != n:
        raise RuntimeError(f'{n} levels but {len(regress_ranges)} regress_ranges')
    dev = gt_bboxes[0].device
    offsets = [0]
    for i, (bx, lb) in enumerate(zip(gt_bboxes, gt_labels)):
        if bx.dim() != 2 or bx.shape[1] != 4 or lb.dim() != 1 or lb.shape[0] != bx.shape[0]:
            raise RuntimeError(f'image {i}: gt_bboxes {tuple(bx.shape)} and gt_labels {tuple(lb.shape)} do not describe [G,4] and [G]')
        offsets.append(offsets[-1] + int(bx.shape[0]))
    G = offsets[-1]
    boxes = torch.cat([b.detach().to(torch.float32) for b in gt_bboxes]).contiguous() if G else None
    labs = torch.cat([t.detach().to(torch.int64) for t in gt_labels]).contiguous() if G else None
    N = B * sum(sizes)
    e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
    out = BoxTargets(e(N, dtype=torch.int64), e(N, 4), e(N, dtype=torch.int64), e(N, 2), e(N, dtype=torch.int64), e(N, dtype=torch.int64), e(N),
                     e(2), e(1, dtype=torch.int32))
    ws = _workspace(arr, n, B, 1, dev) if workspace is None else workspace
    ranges = _lib.float_array([v for r in regress_ranges for v in r])
    with torch.cuda.device(dev):
        _lib.check('bxi_fcos_targets_f32', _lib.load().bxi_fcos_targets_f32(
            arr, n, B, ranges, 1 if center_sampling else 0, float(center_sample_radius), 1 if norm_on_bbox else 0, int(num_classes),
            None if boxes is None else boxes.data_ptr(), None if labs is None else labs.data_ptr(), _lib.int_array(offsets),
            out.labels.data_ptr(), out.bbox_targets.data_ptr(), out.gt_inds.data_ptr(), out.points.data_ptr(), out.level_inds.data_ptr(),
            out.img_inds.data_ptr(), out.ctr_targets.data_ptr(), out.stats.data_ptr(), out.status.data_ptr(), ws.data_ptr(), ws.numel() * 4,
            current_stream(dev)))
    return out


def _grads_array(tensors):
    arr = (_lib.FcosGrads * len(tensors[0]))()
    for i, (a, b, c) in enumerate(zip(*tensors)):
        arr[i] = _lib.FcosGrads(a.data_ptr(), b.data_ptr(), c.data_ptr())
    return arr


class _BoxHeadLoss(torch.autograd.Function):
    """losses [3] = (loss_cls, loss_bbox, loss_centerness) of the 3 * n_levels maps; the unit gradients are made in the forward sweep."""

    @staticmethod
    def forward(ctx, s, tg, norm, n, *maps):
        cls, bbox, ctr = [m.contiguous() for m in maps[:n]], [m.contiguous() for m in maps[n:2 * n]], [m.contiguous() for m in maps[2 * n:]]
        dev = cls[0].device
        B, C = int(cls[0].shape[0]), int(cls[0].shape[1])
        lv = (_lib.DetLevel * n)()
        fl = (_lib.FcosLevel * n)()
        for i in range(n):
            H, W = int(cls[i].shape[2]), int(cls[i].shape[3])
            lv[i] = _lib.DetLevel(cls[i].data_ptr(), bbox[i].data_ptr(), ctr[i].data_ptr(), None, H, W, s['strides'][i])
            fl[i] = _lib.FcosLevel(H, W, s['strides'][i])
        unit = ([torch.empty_like(t) for t in cls], [torch.empty_like(t) for t in bbox], [torch.empty_like(t) for t in ctr])
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ws = _workspace(fl, n, B, C, dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_fcos_loss_f32', _lib.load().bxi_fcos_loss_f32(
                lv, n, B, C, tg.labels.data_ptr(), tg.bbox_targets.data_ptr(), tg.ctr_targets.data_ptr(), norm.data_ptr(), s['gamma'], s['alpha'],
                s['loss_weight_cls'], s['loss_weight_bbox'], s['loss_weight_centerness'], _lib.FCOS_BBOX_KINDS[s['bbox_loss_kind']], s['eps'],
                _grads_array(unit), losses.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))
        ctx.unit, ctx.fl, ctx.n, ctx.B, ctx.C = unit, fl, n, B, C
        return losses

    @staticmethod
    def backward(ctx, grad):
        unit, n = ctx.unit, ctx.n
        dev = unit[0][0].device
        up = grad.detach().to(torch.float32).contiguous()
        out = tuple([torch.empty_like(t) for t in part] for part in unit)
        with torch.cuda.device(dev):
            _lib.check('bxi_fcos_grad_rescale_f32', _lib.load().bxi_fcos_grad_rescale_f32(
                ctx.fl, n, ctx.B, ctx.C, _grads_array(unit), up.data_ptr(), _grads_array(out), current_stream(dev)))
        return (None, None, None, None, *out[0], *out[1], *out[2])


def condinst_box_loss(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, cfg):
    """``CondInstBoxHead.loss`` (condinst_head.py:365-476).  ``cls_scores`` / ``bbox_preds`` / ``centernesses``: per FPN level [B,C,H,W] /
    [B,4,H,W] / [B,1,H,W] on the GPU (half-precision maps are taken as ``.float()``: the reference's ``force_fp32``); ``gt_bboxes`` /
    ``gt_labels``: per image; ``img_metas`` is accepted for the signature's sake and not read (as in the reference); ``cfg``: the
    ``bbox_head`` block of the config (dict or namespace), or what :func:`parse_box_head_cfg` returned.

    Returns ``(losses, flatten_points, flatten_level_inds, flatten_img_inds, flatten_gt_inds)`` with ``losses`` =
    ``dict(loss_cls, loss_bbox, loss_centerness)``: what ``CondInstMaskHead.training_sample`` and the mask loss consume.

    Five launches forward, one backward, no host synchronisation; with an initialised process group of more than one rank, ONE
    all-reduce of the two normalisers (number of positives, centerness sum) between the targets and the losses.  A gt label outside
    [0, num_classes) makes its locations background; ``condinst_box_targets`` returns the status word that says so."""
    s = _settings(cfg)
    n = len(cls_scores)
    if not (1 <= n <= _lib.DET_MAX_LEVELS) or len(bbox_preds) != n or len(centernesses) != n:
        raise RuntimeError(f'1..{_lib.DET_MAX_LEVELS} levels with cls, bbox and centerness each, got {n}, {len(bbox_preds)}, {len(centernesses)}')
    if len(s['strides']) != n:
        raise RuntimeError(f"{n} levels but {len(s['strides'])} strides")
    need_cuda(**{f'cls_scores[{i}]': t for i, t in enumerate(cls_scores)}, **{f'bbox_preds[{i}]': t for i, t in enumerate(bbox_preds)},
               **{f'centernesses[{i}]': t for i, t in enumerate(centernesses)})
    for name, v in (('gamma', s['gamma']), ('alpha', s['alpha']), ('eps', s['eps'])):
        if math.isnan(v):
            raise RuntimeError(f'{name} is NaN')
    if s['bbox_loss_kind'] not in _lib.FCOS_BBOX_KINDS:
        raise NotImplementedError(f"bbox_loss_kind {s['bbox_loss_kind']!r} is not supported: one of {sorted(_lib.FCOS_BBOX_KINDS)}")
    if cls_scores[0].dim() != 4:
        raise RuntimeError(f'cls_scores[0] must be [B,C,H,W], got {tuple(cls_scores[0].shape)}')
    dev = cls_scores[0].device
    for name, ts in (('cls_scores', cls_scores), ('bbox_preds', bbox_preds), ('centernesses', centernesses), ('gt_bboxes', gt_bboxes),
                     ('gt_labels', gt_labels)):
        for i, t in enumerate(ts):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f'{name}[{i}] is not a tensor')
            if t.device != dev:
                raise RuntimeError(f'{name}[{i}] is on {t.device} but cls_scores[0] is on {dev}: everything must be on one device')
    B, C = int(cls_scores[0].shape[0]), int(cls_scores[0].shape[1])
    if len(gt_bboxes) != B or len(gt_labels) != B:
        raise RuntimeError(f'{B} images but {len(gt_bboxes)} gt_bboxes and {len(gt_labels)} gt_labels')
    if C != s['num_classes']:
        raise RuntimeError(f"cls_scores have {C} channels but num_classes is {s['num_classes']}")
    for i in range(n):
        if cls_scores[i].dim() != 4:
            raise RuntimeError(f'level {i}: cls_scores must be [B,C,H,W], got {tuple(cls_scores[i].shape)}')
        H, W = int(cls_scores[i].shape[2]), int(cls_scores[i].shape[3])
        if tuple(cls_scores[i].shape) != (B, C, H, W) or tuple(bbox_preds[i].shape) != (B, 4, H, W) or tuple(centernesses[i].shape) != (B, 1, H, W):
            raise RuntimeError(f'level {i}: cls {tuple(cls_scores[i].shape)}, bbox {tuple(bbox_preds[i].shape)}, centerness '
                               f'{tuple(centernesses[i].shape)} do not describe one [B,*,H,W] level')
    sizes = [tuple(t.shape[-2:]) for t in cls_scores]
    tg = condinst_box_targets(sizes, s['strides'], gt_bboxes, gt_labels, regress_ranges=s['regress_ranges'],
                              center_sampling=s['center_sampling'], center_sample_radius=s['center_sample_radius'],
                              norm_on_bbox=s['norm_on_bbox'], num_classes=s['num_classes'], B=B)
    norm = _dist.reduce_mean(tg.stats)
    maps = [t.float() for t in (*cls_scores, *bbox_preds, *centernesses)]
    losses = _BoxHeadLoss.apply(s, tg, norm, n, *maps)
    return (dict(loss_cls=losses[0], loss_bbox=losses[1], loss_centerness=losses[2]), tg.points, tg.level_inds, tg.img_inds, tg.gt_inds)
