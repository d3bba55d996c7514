"""Training targets of the two SOLOv2-style heads and their category loss on the GPU (csrc/solo_targets.hip,
include/boxinst/boxinst_hip_solo.h).

    solov2_targets      <-> DiscoBoxSOLOv2Head.solov2_target_single over the batch (discobox_head.py:1163-1196, :1442-1529)
    box_solov2_targets  <-> BoxSOLOv2Head.solo_target_single over the batch (box_solov2_head.py:284-297, :390-472), without the
                            F.interpolate of the image and the level-set features
    solo_cate_loss      <-> loss_cate of both heads (discobox_head.py:1341-1355, box_solov2_head.py:366-381)
    parse_solo_head_cfg : the ``bbox_head=dict(type='DiscoBoxSOLOv2Head' | 'BoxSOLOv2Head', ...)`` block of the reference's configs

The reference loops in Python over images x levels x instances x cells, resizes every mask on the host and uploads it, and calls
``nonzero`` / ``int()`` on device tensors in the inner loop.  Here the mask bytes of the batch are read ONCE (exact moments and the
rescaled masks at every factor in use), the assignment of all images and levels is ONE launch, and the host waits once per batch: for
the pair and cell counts that size the returned lists.

Deviations, see the header: ``mmcv.imrescale`` is restated from OpenCV's documented arithmetic (unpinned); the centre of mass comes
from the exact integer moments, rounded once; an image without boxes is all background.

There is no CPU or PyTorch fallback: CPU tensors raise.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._common import cfg_get, cfg_only, current_stream, need_cuda

__all__ = ['solov2_targets', 'box_solov2_targets', 'solo_cate_loss', 'parse_solo_head_cfg', 'SoloTargets', 'RESCALE_MIN_ONES']

RESCALE_MIN_ONES = _lib.SOLO_RESCALE_MIN_ONES
_HEADS = {'DiscoBoxSOLOv2Head': 'discobox', 'BoxSOLOv2Head': 'boxlevelset'}
_FLAT_KEYS = ('mode', 'num_classes', 'strides', 'scale_ranges', 'num_grids', 'sigma', 'gamma', 'alpha', 'loss_weight_cate')


def parse_solo_head_cfg(cfg):
    """``bbox_head=dict(type='DiscoBoxSOLOv2Head' | 'BoxSOLOv2Head', ...)`` (dict or namespace) -> the flat settings the functions here
    take: mode, num_classes, strides, scale_ranges, num_grids, sigma, gamma, alpha, loss_weight_cate.  Keys that shape the network or
    belong to the other losses are accepted and ignored.  A ``loss_cate`` that is not the sigmoid focal loss raises NotImplementedError."""
    kind = cfg_get(cfg, 'type')
    if kind not in _HEADS:
        raise NotImplementedError(f'bbox_head.type {kind!r} is not supported: one of {sorted(_HEADS)}')
    num_classes = cfg_get(cfg, 'num_classes')
    if num_classes is None:
        raise TypeError('bbox_head has no `num_classes`')
    num_grids = cfg_get(cfg, 'num_grids')
    if num_grids is None:
        raise TypeError('bbox_head has no `num_grids`')
    strides = [int(s) for s in cfg_get(cfg, 'strides', (4, 8, 16, 32, 64))]
    ranges = tuple((float(a), float(b)) for a, b in cfg_get(cfg, 'scale_ranges', ((8, 32), (16, 64), (32, 128), (64, 256), (128, 512))))
    num_grids = [int(s) for s in num_grids]
    if not len(strides) == len(ranges) == len(num_grids):
        raise TypeError(f'{len(strides)} strides, {len(ranges)} scale_ranges and {len(num_grids)} num_grids')
    lc = cfg_get(cfg, 'loss_cate')
    if lc is None:
        raise TypeError('bbox_head has no `loss_cate`')
    if cfg_get(lc, 'type') != 'FocalLoss':
        raise NotImplementedError(f"loss_cate.type {cfg_get(lc, 'type')!r} is not supported: only 'FocalLoss'")
    cfg_only(lc, 'loss_cate', ('type', 'use_sigmoid', 'gamma', 'alpha', 'loss_weight', 'reduction', 'activated'))
    if not cfg_get(lc, 'use_sigmoid', True):
        raise NotImplementedError('loss_cate.use_sigmoid=False is not supported')
    if cfg_get(lc, 'activated', False):
        raise NotImplementedError('loss_cate.activated=True is not supported')
    if cfg_get(lc, 'reduction', 'mean') != 'mean':
        raise NotImplementedError("loss_cate.reduction: only 'mean' is supported")
    return dict(mode=_HEADS[kind], num_classes=int(num_classes), strides=strides, scale_ranges=ranges, num_grids=num_grids,
                sigma=float(cfg_get(cfg, 'sigma', 0.2)), gamma=float(cfg_get(lc, 'gamma', 2.0)), alpha=float(cfg_get(lc, 'alpha', 0.25)),
                loss_weight_cate=float(cfg_get(lc, 'loss_weight', 1.0)))


class SoloTargets:
    """What one batch's targets are, on the device.  Per-level lists follow the reference's layout after its concatenation over the
    images (level l, then image b, then cell):

      cate_labels[l]     int64 [B * S_l^2]          ins_ind_labels[l]  bool [B * S_l^2]         cell_owner[l]  int32 [B * S_l^2]
      grid_order[l][b]   int64: the reference's grid_order of (level, image)
      pair_inst[l]       int64: the global instance index of every grid_order entry of the level, images concatenated
      sel_inst[l]        int64: the owner of every set cell of the level in ascending (image, cell) order
      masks[f]           uint8 [G, h, w]: every instance's mask rescaled by 1 / f -- the compact form
      level_factor[l]    the factor whose masks level l's planes come from
      moments            int64 [G, 3] (m00, m10, m01);  num_ins, status: int32 [1];  flat_cate_labels: int64 [sum_l B S_l^2]
      counts             host list [l][b] = (pairs, set cells)

    ``ins_labels()`` gathers the per-pair (DiscoBox) or per-set-cell (BoxLevelSet) planes, and ``kernel_labels()`` the labels of
    the pairs' cells; both only when asked for."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def ins_labels(self):
        idx = self.pair_inst if self.mode == 'discobox' else self.sel_inst
        return [self.masks[f].index_select(0, i) for f, i in zip(self.level_factor, idx)]

    def kernel_labels(self):
        out = []
        for l, S in enumerate(self.num_grids):
            lab = self.cate_labels[l].view(self.B, S * S)
            out.append(torch.cat([lab[b][self.grid_order[l][b]] for b in range(self.B)]))
        return out


def _as_mask_tensor(m, dev, i):
    if hasattr(m, 'to_ndarray'):
        m = torch.from_numpy(m.to_ndarray())
    if not isinstance(m, torch.Tensor):
        raise TypeError(f'gt_masks[{i}] is neither a tensor nor something with to_ndarray()')
    if m.dtype != torch.uint8 or m.dim() != 3:
        raise RuntimeError(f'gt_masks[{i}] must be uint8 [G,H,W], got {m.dtype} {tuple(m.shape)}')
    if not m.is_cuda:
        if dev is None or dev.type != 'cuda':
            raise RuntimeError(f'gt_masks[{i}] must be a CUDA (HIP) tensor: boxinstseg_amd has no CPU path')
        m = m.to(dev)                                  # host masks (BitmapMasks): uploaded once
    return m.contiguous()


def _targets(mode, gt_bboxes, gt_labels, gt_masks, level_sizes, canvas, *, scale_ranges, num_grids, strides, sigma, num_classes):
    B = len(gt_bboxes)
    if len(gt_labels) != B or len(gt_masks) != B:
        raise RuntimeError(f'{B} gt_bboxes but {len(gt_labels)} gt_labels and {len(gt_masks)} gt_masks')
    if not 1 <= B <= _lib.BXI_MAX_IMAGES:
        raise RuntimeError(f'B must be in 1..{_lib.BXI_MAX_IMAGES}, got {B}')
    L = len(num_grids)
    if not (1 <= L <= _lib.DET_MAX_LEVELS) or len(scale_ranges) != L or len(strides) != L or len(level_sizes) != L:
        raise RuntimeError(f'1..{_lib.DET_MAX_LEVELS} levels with a num_grid, a scale range, a stride and a size each, got {L}, '
                           f'{len(scale_ranges)}, {len(strides)}, {len(level_sizes)}')
    num_grids = [int(s) for s in num_grids]
    if any(not 1 <= s <= _lib.SOLO_MAX_GRID for s in num_grids):
        raise RuntimeError(f'num_grids must be in 1..{_lib.SOLO_MAX_GRID}, got {num_grids}')
    if int(num_classes) < 1 or math.isnan(float(sigma)):
        raise RuntimeError(f'num_classes {num_classes}, sigma {sigma}')
    for i, (bx, lb) in enumerate(zip(gt_bboxes, gt_labels)):
        if not isinstance(bx, torch.Tensor) or not isinstance(lb, torch.Tensor):
            raise TypeError(f'gt_bboxes[{i}] / gt_labels[{i}] is not a tensor')
    need_cuda(**{f'gt_bboxes[{i}]': t for i, t in enumerate(gt_bboxes)}, **{f'gt_labels[{i}]': t for i, t in enumerate(gt_labels)})
    dev = gt_bboxes[0].device
    masks = [_as_mask_tensor(m, dev, i) for i, m in enumerate(gt_masks)]
    # the factor of every level and the plane size of every factor
    if mode == 'discobox':
        level_factor = [4] * L
    else:
        level_factor = []
        for s in strides:
            if int(s) != s or int(s) % 4:
                raise NotImplementedError(f'stride {s}: output_stride = stride / 2 must be an even integer')
            level_factor.append(int(s) // 2)
    planes = {}
    for f, hw in zip(level_factor, level_sizes):
        hw = (int(hw[0]), int(hw[1]))
        if planes.setdefault(f, hw) != hw:
            raise RuntimeError(f'levels of output stride {f} have different sizes: {planes[f]} and {hw}')
    factors = sorted(planes)
    fmax = factors[-1]
    if len(factors) > _lib.SOLO_MAX_FACTORS or any(f < 2 or f > _lib.SOLO_MAX_FACTOR or fmax % f for f in factors):
        raise NotImplementedError(f'rescale factors {factors}: at most {_lib.SOLO_MAX_FACTORS}, even, each dividing the largest')
    offsets = [0]
    for i, (bx, lb, m) in enumerate(zip(gt_bboxes, gt_labels, masks)):
        if bx.dim() != 2 or bx.shape[1] != 4 or lb.dim() != 1 or lb.shape[0] != bx.shape[0] or m.shape[0] != bx.shape[0]:
            raise RuntimeError(f'image {i}: gt_bboxes {tuple(bx.shape)}, gt_labels {tuple(lb.shape)} and gt_masks {tuple(m.shape)} do not '
                               'describe [G,4], [G] and [G,H,W]')
        if bx.device != dev or lb.device != dev or m.device != dev:
            raise RuntimeError(f'image {i}: everything must be on one device ({dev})')
        if m.shape[0]:
            H, W = int(m.shape[1]), int(m.shape[2])
            if H < 1 or W < 1 or H % fmax or W % fmax:
                raise NotImplementedError(f'image {i}: masks of {H}x{W} are not a multiple of the largest rescale factor {fmax} '
                                          '(the configs pad to a multiple of 32)')
            for f in factors:
                if planes[f][0] < H // f or planes[f][1] < W // f:
                    raise RuntimeError(f'image {i}: masks of {H}x{W} do not fit the {planes[f]} plane of factor {f}')
        offsets.append(offsets[-1] + int(bx.shape[0]))
    G = offsets[-1]
    boxes = torch.cat([b.detach().to(torch.float32) for b in gt_bboxes]).contiguous() if G else None
    labs = torch.cat([t.detach().to(torch.int64) for t in gt_labels]).contiguous() if G else None
    e = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
    moments = e(G, 3, dtype=torch.int64)
    rescaled = {f: e(G, planes[f][0], planes[f][1], dtype=torch.uint8) for f in factors}
    cells = [s * s for s in num_grids]
    N = B * sum(cells)
    cate, ind, owner, sel = e(N, dtype=torch.int64), e(N, dtype=torch.uint8), e(N), e(N)
    P = _lib.SOLO_PAIRS_PER_INSTANCE
    pair_cell, pair_inst = e(P * L * G), e(P * L * G)
    counts, tail = e(L * B * 2), e(2)
    num_ins, status = tail[0:1], tail[1:2]
    lib = _lib.load()
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()                  # noqa: E731
    with torch.cuda.device(dev):
        st = current_stream(dev)
        _lib.check('bxi_solo_mask_pass_u8', lib.bxi_solo_mask_pass_u8(
            _lib.ptr_array([ptr(m) or 0 for m in masks]), _lib.int_array(offsets), _lib.int_array([m.shape[1] for m in masks]),
            _lib.int_array([m.shape[2] for m in masks]), B, _lib.int_array(factors), _lib.int_array([planes[f][0] for f in factors]),
            _lib.int_array([planes[f][1] for f in factors]), len(factors), _lib.ptr_array([ptr(rescaled[f]) or 0 for f in factors]),
            ptr(moments), st))
        _lib.check('bxi_solo_assign_f32', lib.bxi_solo_assign_f32(
            _lib.SOLO_MODES[mode], B, L, _lib.int_array(num_grids), _lib.float_array([v for r in scale_ranges for v in r]), float(sigma),
            int(num_classes), int(canvas[0]), int(canvas[1]), ptr(boxes), ptr(labs), ptr(moments), _lib.int_array(offsets), cate.data_ptr(),
            ind.data_ptr(), owner.data_ptr(), sel.data_ptr(), ptr(pair_cell), ptr(pair_inst), counts.data_ptr(), num_ins.data_ptr(),
            status.data_ptr(), st))
    host_counts = counts.view(L, B, 2).cpu().tolist()          # THE host synchronisation of the batch
    cate_l, ind_l, owner_l, order_l, pinst_l, sel_l = [], [], [], [], [], []
    at = 0
    for l in range(L):
        n = B * cells[l]
        cate_l.append(cate[at:at + n])
        ind_l.append(ind[at:at + n].view(torch.bool))
        owner_l.append(owner[at:at + n])
        orders, pi, si = [], [], []
        for b in range(B):
            p0 = P * (l * G + offsets[b])
            np_, ns = host_counts[l][b]
            orders.append(pair_cell[p0:p0 + np_].long())
            pi.append(pair_inst[p0:p0 + np_])
            si.append(sel[at + b * cells[l]:at + b * cells[l] + ns])
        order_l.append(orders)
        pinst_l.append(torch.cat(pi).long())
        sel_l.append(torch.cat(si).long())
        at += n
    return SoloTargets(mode=mode, B=B, G=G, num_grids=num_grids, gt_offsets=offsets, cate_labels=cate_l, ins_ind_labels=ind_l,
                       cell_owner=owner_l, grid_order=order_l, pair_inst=pinst_l, sel_inst=sel_l, masks=rescaled, level_factor=level_factor,
                       moments=moments, num_ins=num_ins, status=status, flat_cate_labels=cate, counts=host_counts)


def _split(cfg, where):
    cfg = dict(cfg)
    mode = cfg.pop('mode', None)
    for k in ('gamma', 'alpha', 'loss_weight_cate'):
        cfg.pop(k, None)
    missing = [k for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes') if k not in cfg]
    if missing:
        raise TypeError(f'{where}: missing settings {missing}')
    extra = sorted(set(cfg) - {'scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes'})
    if extra:
        raise TypeError(f'{where}: unknown settings {extra}')
    return mode, cfg


def solov2_targets(gt_bboxes, gt_labels, gt_masks, mask_feat_size, **cfg):
    """``multi_apply(solov2_target_single, ...)`` of DiscoBoxSOLOv2Head for the whole batch.  ``gt_bboxes`` / ``gt_labels``: per image
    [G_i,4] / [G_i] on the GPU; ``gt_masks``: per image uint8 [G_i,H_i,W_i] (device tensors, or anything with ``to_ndarray()``, which is
    uploaded once); ``mask_feat_size``: (h, w) of the mask feature map, the canvas being 4x that; ``cfg``: scale_ranges, num_grids,
    strides, sigma, num_classes (what :func:`parse_solo_head_cfg` returns may be passed as it is).  Returns :class:`SoloTargets`."""
    mode, cfg = _split(cfg, 'solov2_targets')
    if mode not in (None, 'discobox'):
        raise RuntimeError(f'solov2_targets is the DiscoBox head; the settings say {mode!r}')
    h, w = int(mask_feat_size[0]), int(mask_feat_size[1])
    if h < 1 or w < 1:
        raise RuntimeError(f'mask_feat_size {h}x{w}')
    return _targets('discobox', gt_bboxes, gt_labels, gt_masks, [(h, w)] * len(cfg['num_grids']), (4 * h, 4 * w), **cfg)


def box_solov2_targets(gt_bboxes, gt_labels, gt_masks, featmap_sizes, **cfg):
    """``multi_apply(solo_target_single, ...)`` of BoxSOLOv2Head for the whole batch (without its two ``F.interpolate``).
    ``featmap_sizes``: (h, w) of every level's mask prediction; level l's masks are rescaled by 2 / stride_l and the canvas is 4x
    ``featmap_sizes[0]``.  Everything else as :func:`solov2_targets`.  ``ins_labels()`` of the result holds, per level, the planes the
    reference's ``ins_label[ins_ind_label]`` selects: ascending cell order, each the mask of the cell's last writer."""
    mode, cfg = _split(cfg, 'box_solov2_targets')
    if mode not in (None, 'boxlevelset'):
        raise RuntimeError(f'box_solov2_targets is the BoxLevelSet head; the settings say {mode!r}')
    sizes = [(int(s[0]), int(s[1])) for s in featmap_sizes]
    if not sizes or any(h < 1 or w < 1 for h, w in sizes):
        raise RuntimeError(f'featmap_sizes {sizes}')
    return _targets('boxlevelset', gt_bboxes, gt_labels, gt_masks, sizes, (4 * sizes[0][0], 4 * sizes[0][1]), **cfg)


class _CateLoss(torch.autograd.Function):
    """loss_cate of the n_levels maps; the unit gradients are made in the forward sweep."""

    @staticmethod
    def forward(ctx, labels, num_ins, gamma, alpha, loss_weight, *maps):
        maps = [m.contiguous() for m in maps]
        dev = maps[0].device
        n, B, C = len(maps), int(maps[0].shape[0]), int(maps[0].shape[1])
        grids = _lib.int_array([m.shape[2] for m in maps])
        lib = _lib.load()
        nbytes = lib.bxi_solo_cate_workspace_bytes(grids, n, B, C)
        if nbytes == 0:
            raise RuntimeError(f'bxi_solo_cate_workspace_bytes: bad shape (B={B}, C={C})')
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        unit = [torch.empty_like(m) for m in maps]
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_solo_cate_loss_f32', lib.bxi_solo_cate_loss_f32(
                _lib.ptr_array([m.data_ptr() for m in maps]), grids, n, B, C, labels.data_ptr(), num_ins.data_ptr(), gamma, alpha, loss_weight,
                _lib.ptr_array([u.data_ptr() for u in unit]), loss.data_ptr(), ws.data_ptr(), nbytes, current_stream(dev)))
        ctx.unit, ctx.grids, ctx.shape = unit, grids, (n, B, C)
        return loss[0]

    @staticmethod
    def backward(ctx, grad):
        unit = ctx.unit
        n, B, C = ctx.shape
        dev = unit[0].device
        up = grad.detach().to(torch.float32).reshape(1).contiguous()
        out = [torch.empty_like(u) for u in unit]
        with torch.cuda.device(dev):
            _lib.check('bxi_solo_cate_grad_rescale_f32', _lib.load().bxi_solo_cate_grad_rescale_f32(
                ctx.grids, n, B, C, _lib.ptr_array([u.data_ptr() for u in unit]), up.data_ptr(), _lib.ptr_array([o.data_ptr() for o in out]),
                current_stream(dev)))
        return (None, None, None, None, None, *out)


def solo_cate_loss(cate_preds, cate_labels, num_ins, gamma=2.0, alpha=0.25, loss_weight=1.0):
    """``loss_cate(flatten_cate_preds, flatten_cate_labels, avg_factor=num_ins + 1)``.  ``cate_preds``: per level [B,C,S,S] on the GPU,
    read where they lie; ``cate_labels``: int64 in the flatten order (``SoloTargets.flat_cate_labels``) or the per-level list;
    ``num_ins``: int32 [1] on the device (``SoloTargets.num_ins``) -- it is not read on the host.  Two launches forward, one backward."""
    n = len(cate_preds)
    if not 1 <= n <= _lib.DET_MAX_LEVELS:
        raise RuntimeError(f'1..{_lib.DET_MAX_LEVELS} levels, got {n}')
    for i, t in enumerate(cate_preds):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'cate_preds[{i}] is not a tensor')
    if isinstance(cate_labels, (list, tuple)):
        cate_labels = torch.cat([t.reshape(-1) for t in cate_labels])
    if not isinstance(cate_labels, torch.Tensor) or not isinstance(num_ins, torch.Tensor):
        raise TypeError('cate_labels and num_ins must be tensors')
    need_cuda(**{f'cate_preds[{i}]': t for i, t in enumerate(cate_preds)}, cate_labels=cate_labels, num_ins=num_ins)
    for name, v in (('gamma', gamma), ('alpha', alpha), ('loss_weight', loss_weight)):
        if math.isnan(float(v)):
            raise RuntimeError(f'{name} is NaN')
    if float(gamma) < 0:
        raise RuntimeError(f'gamma must be >= 0, got {gamma}')
    if cate_preds[0].dim() != 4:
        raise RuntimeError(f'cate_preds[0] must be [B,C,S,S], got {tuple(cate_preds[0].shape)}')
    B, C = int(cate_preds[0].shape[0]), int(cate_preds[0].shape[1])
    dev = cate_preds[0].device
    total = 0
    for i, t in enumerate(cate_preds):
        if t.dim() != 4 or t.shape[0] != B or t.shape[1] != C or t.shape[2] != t.shape[3] or not 1 <= t.shape[2] <= _lib.SOLO_MAX_GRID:
            raise RuntimeError(f'cate_preds[{i}] must be [{B},{C},S,S] with S in 1..{_lib.SOLO_MAX_GRID}, got {tuple(t.shape)}')
        if t.device != dev:
            raise RuntimeError(f'cate_preds[{i}] is on {t.device} but cate_preds[0] is on {dev}')
        total += B * int(t.shape[2]) ** 2
    if B < 1 or C < 1:
        raise RuntimeError(f'cate_preds of B={B}, C={C}')
    if cate_labels.dtype != torch.int64 or cate_labels.numel() != total or cate_labels.device != dev:
        raise RuntimeError(f'cate_labels must be {total} int64 on {dev}, got {cate_labels.numel()} {cate_labels.dtype} on {cate_labels.device}')
    if num_ins.dtype != torch.int32 or num_ins.numel() != 1 or num_ins.device != dev:
        raise RuntimeError(f'num_ins must be one int32 on {dev}, got {num_ins.numel()} {num_ins.dtype} on {num_ins.device}')
    return _CateLoss.apply(cate_labels.contiguous().view(-1), num_ins.contiguous(), float(gamma), float(alpha), float(loss_weight),
                           *[t.float() for t in cate_preds])
