"""``BoxSOLOv2Head.loss`` (``mmdet/models/dense_heads/box_solov2_head.py:259-388``) as one call for all levels, on the kernels of
``csrc/boxlevelset_loss.hip`` (``include/boxinst/boxinst_hip_bls.h``).

The reference resizes the image and the level-set feature once per (level, image) -- five levels, three distinct sizes --, copies both
once per set cell (:300-314) and builds one minimum spanning tree, one breadth-first order and one set of edge weights per copy
(:353-357).  ``BoxLevelSetLossContext`` keeps, per distinct size, the resized image and feature, both trees of every image, one
breadth-first order per tree and the edge weights.  A ROW is one set cell; ``box_solov2_mask_losses`` evaluates the rows of all levels
together: one pass over each row's logits gives the scores, the projection term, ``pixel_num`` and the image level-set energy; the two
tree filters run once per (size, image) over that image's rows as channels of one tree -- the reference's batch of per-row copies of one
tree, and its weight gradient summed over the copies --; a second pair of kernels takes the level-set energy on the rows' own filter
outputs, and one backward launch writes every level's gradient.  The one host synchronisation of ``box_solov2_loss`` is the targets'.

DEVIATIONS.  Zero rows give two zeros that are connected to the graph; the reference's ``torch.cat([])`` raises there.  A row whose
``tgt_of`` / ``img_of`` is -1 is inert and leaves the denominators of both means (counted on the device).  The level-set feature is
resized by two matrix products (``_resize_det``), whose backward adds in a fixed order.  The projection gradient goes to the first
index of the largest logit of a line or column (the project's arg-max rule).  fp32 only, as the reference's ``feats.float()`` makes it.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import cfg_get, cfg_only, current_stream, need_cuda
from .box2mask_loss import _EdgeWeight, _need_fp32, _resize, _resize_det
from .tree_filter import MinimumSpanningTree, TreeFilter2D, _bfs_levels, _Refine

__all__ = ['BoxLevelSetLossContext', 'box_solov2_mask_losses', 'parse_box_solov2_loss_cfg', 'box_solov2_loss']

_HEADER = 'boxinst_hip_bls.h'
W_IMG, W_FEAT = 0.05, 5.0                             # box_solov2_head.py:351, :360


class BoxLevelSetLossContext:
    """What ``solo_target_single`` (:412-416) and the level loop (:353-357) recompute per level, image and set cell, once per iteration.

    ``norm_img`` [B,3,H,W], ``levelset_feats`` [B,Cf,hf,wf] (differentiable), ``level_sizes`` the (h, w) of every level's mask
    prediction.  Levels of one size form a size group, in order of first appearance: ``sizes[g]``, ``group_of_level[l]``.
    ``trees[g]`` = (img_tree, lst_tree), each [B,V_g-1,2] int32, replaces the two ``MinimumSpanningTree`` calls of group g.

    Keeps per group: ``img[g]`` [B,3,h,w], ``feat[g]`` [B,Cf,h,w] (through ``_resize_det``), both trees, one breadth-first order per
    tree, ``w_img[g]`` (low tree, sigma 0.02, no gradient) and ``w_lst[g]`` (differentiable), both [B,V_g]."""

    def __init__(self, norm_img, levelset_feats, level_sizes, trees=None):
        need_cuda(norm_img=norm_img, levelset_feats=levelset_feats)
        _need_fp32(norm_img=norm_img, levelset_feats=levelset_feats)
        if norm_img.dim() != 4 or levelset_feats.dim() != 4 or levelset_feats.shape[0] != norm_img.shape[0]:
            raise RuntimeError(f'norm_img [B,3,H,W] and levelset_feats [B,C,h,w], got {tuple(norm_img.shape)} and {tuple(levelset_feats.shape)}')
        self.device, self.B = norm_img.device, int(norm_img.shape[0])
        self.level_sizes = [(int(s[0]), int(s[1])) for s in level_sizes]
        if not 1 <= len(self.level_sizes) <= _lib.BLS_MAX_LEVELS:
            raise NotImplementedError(f'{len(self.level_sizes)} levels: 1 .. {_lib.BLS_MAX_LEVELS} per call (include/boxinst/{_HEADER})')
        self.sizes = list(dict.fromkeys(self.level_sizes))
        if len(self.sizes) > _lib.BLS_MAX_GROUPS:
            raise NotImplementedError(f'{len(self.sizes)} distinct level sizes: at most {_lib.BLS_MAX_GROUPS} (include/boxinst/{_HEADER})')
        for h, w in self.sizes:
            if h < 2 or w < 2:
                raise NotImplementedError(f'level size {(h, w)}: a tree needs at least 2 pixels per axis')
            if w > _lib.BLS_MAX_W:
                raise NotImplementedError(f'level size {(h, w)}: at most {_lib.BLS_MAX_W} columns (include/boxinst/{_HEADER})')
        self.group_of_level = [self.sizes.index(s) for s in self.level_sizes]
        if trees is not None and len(trees) != len(self.sizes):
            raise RuntimeError(f'trees must hold one (img_tree, lst_tree) per distinct size: {len(self.sizes)}, got {len(trees)}')
        self.lst_feat = levelset_feats
        self.img, self.feat, self.img_tree, self.lst_tree, self.img_order, self.lst_order, self.w_img, self.w_lst = [], [], [], [], [], [], [], []
        mst, tf = MinimumSpanningTree(TreeFilter2D.norm2_distance), TreeFilter2D()
        for g, size in enumerate(self.sizes):
            img = _resize(norm_img.detach(), size).contiguous()
            feat = _resize_det(levelset_feats, size)
            it, lt = (mst(img), mst(feat)) if trees is None else trees[g]
            io, lo = _bfs_levels(it, 4), _bfs_levels(lt, 4)          # (sorted_index, sorted_parent, sorted_child, levels)
            self.img.append(img)
            self.feat.append(feat)
            self.img_tree.append(it)
            self.lst_tree.append(lt)
            self.img_order.append(io)
            self.lst_order.append(lo)
            self.w_img.append(tf.build_edge_weight(img, io[0], io[1], True).contiguous())
            self.w_lst.append(_EdgeWeight.apply(feat, lo[0], lo[1], lo[2]))


class _Plan:
    """The host side of one call: the group and level tables of the C ABI and the segments of the ragged row order."""

    def __init__(self, ctx, levels, masks, counts):
        L, B = len(ctx.level_sizes), ctx.B
        self.L, self.B, self.n_groups = L, B, len(ctx.sizes)
        self.counts = [[int(c[1]) if isinstance(c, (tuple, list)) else int(c) for c in per] for per in counts]
        if len(self.counts) != L or any(len(per) != B for per in self.counts):
            raise RuntimeError(f'counts must be [level][image] = [{L}][{B}]')
        self.level_rows = [sum(per) for per in self.counts]
        for l, t in enumerate(levels):
            if tuple(t.shape) != (self.level_rows[l],) + ctx.level_sizes[l]:
                raise RuntimeError(f'ins_pred_rows[{l}] must be {[self.level_rows[l], *ctx.level_sizes[l]]}, got {list(t.shape)}')
        # ragged order (group, image, level, cell): segment = (level, first plane, planes, image); blocks = per (group, image) (first row, rows)
        self.segments, self.blocks, self.group_rows = [], [], []
        m = 0
        for g in range(self.n_groups):
            first = m
            for b in range(B):
                at = m
                for l in range(L):
                    if ctx.group_of_level[l] == g and self.counts[l][b]:
                        self.segments.append((l, sum(self.counts[l][:b]), self.counts[l][b], b))
                        m += self.counts[l][b]
                if m > at:
                    self.blocks.append((g, b, at, m - at))
            self.group_rows.append(m - first)
        self.M = m
        if m > 65535 or any(n >= _lib.BLS_LEVEL_ROWS for n in self.level_rows):
            raise NotImplementedError(f'{m} rows: at most 65535 per call (include/boxinst/{_HEADER})')
        self.group_masks = []
        for g, (h, w) in enumerate(ctx.sizes):
            mk = next(masks[l] for l in range(L) if ctx.group_of_level[l] == g)
            if mk.dtype != torch.uint8 or mk.dim() != 3 or tuple(mk.shape[1:]) != (h, w):
                raise RuntimeError(f'the masks of size group {g} must be uint8 [G,{h},{w}], got {mk.dtype} {list(mk.shape)}')
            self.group_masks.append(mk.contiguous())
        self.pix_first = [0]
        for g, (h, w) in enumerate(ctx.sizes):
            self.pix_first.append(self.pix_first[-1] + self.group_rows[g] * h * w)
        self.pixels = self.pix_first[-1]
        self.ctx = ctx
        self.groups = (_lib.BlsGroup * self.n_groups)(*[
            _lib.BlsGroup(ctx.img[g].data_ptr(), self.group_masks[g].data_ptr() if self.group_masks[g].numel() else None, h, w, self.group_rows[g],
                          int(self.group_masks[g].shape[0])) for g, (h, w) in enumerate(ctx.sizes)])
        self.level_rows_c, self.level_group_c = _lib.int_array(self.level_rows), _lib.int_array(ctx.group_of_level)

    def row_pixels(self, g, first_row, rows):
        """[lo, hi) of rows first_row .. first_row + rows of group g in a ragged per-pixel buffer."""
        h, w = self.ctx.sizes[g]
        lo = self.pix_first[g] + (first_row - sum(self.group_rows[:g])) * h * w
        return lo, lo + rows * h * w


def _ptrs(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() if t.numel() else None for t in tensors])


class _Front(torch.autograd.Function):
    """(p [ragged], loss_proj [M], loss_img [M], pixel_num [M], live [M]) of the rows from the L level tensors read in place; the backward
    is the ONE launch that writes each level's whole gradient."""

    @staticmethod
    def forward(ctx, plan, row_src, tgt_of, img_of, w_proj, w_img, *levels):
        lib = _lib.load()
        dev = row_src.device
        flat = [t.detach().contiguous() for t in levels]
        M = plan.M
        p = torch.empty((plan.pixels,), dtype=torch.float32, device=dev)
        out = [torch.empty((M,), dtype=torch.float32, device=dev) for _ in range(4)]      # loss_proj, loss_img, pixel_num, live
        nbytes = lib.bxi_bls_state_bytes(plan.groups, plan.n_groups)
        if nbytes == 0:
            raise NotImplementedError(f'bxi_bls_front_f32: outside the support set of include/boxinst/{_HEADER}')
        state = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_bls_front_f32', lib.bxi_bls_front_f32(
                plan.groups, plan.n_groups, _ptrs(flat), plan.level_rows_c, plan.level_group_c, plan.L, row_src.data_ptr(), tgt_of.data_ptr(),
                img_of.data_ptr(), M, plan.B, w_proj, w_img, p.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                out[3].data_ptr(), state.data_ptr(), state.numel() * 8, current_stream(dev)), _HEADER)
        ctx.save_for_backward(p, state, row_src, tgt_of, img_of)
        ctx.meta = (plan, w_proj, w_img, [tuple(t.shape) for t in levels])
        ctx.mark_non_differentiable(out[2], out[3])
        return p, out[0], out[1], out[2], out[3]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_p, g_proj, g_img, _g_pn, _g_live):
        p, state, row_src, tgt_of, img_of = ctx.saved_tensors
        plan, w_proj, w_img, shapes = ctx.meta
        dev = p.device
        g_p, g_proj, g_img = (t.to(torch.float32).contiguous() for t in (g_p, g_proj, g_img))
        grads = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_bls_backward_f32', _lib.load().bxi_bls_backward_f32(
                plan.groups, plan.n_groups, _ptrs(grads), plan.level_rows_c, plan.level_group_c, plan.L, row_src.data_ptr(), tgt_of.data_ptr(),
                img_of.data_ptr(), plan.M, plan.B, w_proj, w_img, p.data_ptr(), g_p.data_ptr(), g_proj.data_ptr(), g_img.data_ptr(),
                state.data_ptr(), state.numel() * 8, current_stream(dev)), _HEADER)
        return (None, None, None, None, None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[6:])])


class _High(torch.autograd.Function):
    """``LevelsetLoss`` on (p T, (1 - p) T) against (y_img T, y_lst T) per row, everything ragged, T read as bytes."""

    @staticmethod
    def forward(ctx, plan, weight, p, y_img, y_lst, tgt_of, live, pixel_num):
        lib = _lib.load()
        dev = p.device
        p, y_img, y_lst = (t.detach().contiguous() for t in (p, y_img, y_lst))
        loss = torch.empty((plan.M,), dtype=torch.float32, device=dev)
        nbytes = lib.bxi_bls_high_state_bytes(plan.groups, plan.n_groups)
        if nbytes == 0:
            raise NotImplementedError(f'bxi_bls_high_forward_f32: outside the support set of include/boxinst/{_HEADER}')
        state = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_bls_high_forward_f32', lib.bxi_bls_high_forward_f32(
                plan.groups, plan.n_groups, p.data_ptr(), y_img.data_ptr(), y_lst.data_ptr(), tgt_of.data_ptr(), live.data_ptr(),
                pixel_num.data_ptr(), plan.M, weight, loss.data_ptr(), state.data_ptr(), nbytes, current_stream(dev)), _HEADER)
        ctx.save_for_backward(p, y_img, y_lst, tgt_of, live, pixel_num, state)
        ctx.meta = (plan, weight, nbytes)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, y_img, y_lst, tgt_of, live, pixel_num, state = ctx.saved_tensors
        plan, weight, nbytes = ctx.meta
        dev = p.device
        g = g.to(torch.float32).contiguous()
        g_p, g_yi, g_yl = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_bls_high_backward_f32', _lib.load().bxi_bls_high_backward_f32(
                plan.groups, plan.n_groups, p.data_ptr(), y_img.data_ptr(), y_lst.data_ptr(), tgt_of.data_ptr(), live.data_ptr(),
                pixel_num.data_ptr(), plan.M, weight, state.data_ptr(), nbytes, g.data_ptr(), g_p.data_ptr(), g_yi.data_ptr(), g_yl.data_ptr(),
                current_stream(dev)), _HEADER)
        return None, None, g_p, g_yi, g_yl, None, None, None


class _Blocks(torch.autograd.Function):
    """The rows of every (size, image) block of the ragged scores as [1,C,V] views; the backward is ONE concatenation of the blocks'
    gradients, not a zero-padded add per block."""

    @staticmethod
    def forward(ctx, p, bounds):
        ctx.n = p.numel()
        return tuple(p[lo:hi].view(1, c, v) for lo, hi, c, v in bounds)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return torch.cat([g.reshape(-1) for g in grads]), None


def _zero(levels):
    return torch.stack([t[:0].sum() for t in levels]).sum()


def box_solov2_mask_losses(ctx, ins_pred_rows, masks, tgt_of, img_of, counts, loss_boxpro_weight=1.0, loss_levelset_weight=1.0):
    """``loss_boxpro`` and ``loss_levelset`` of :334-367 -- the means over the rows of all levels -- and the per-row values.

    ``ins_pred_rows``: the L tensors [N_l, oh_l, ow_l] of ``box_solov2_ins_preds`` (logits; separate allocations, read in place).
    ``masks``: per level the uint8 [G,oh_l,ow_l] planes the level's targets come from (``[t.masks[f] for f in t.level_factor]`` of a
    ``SoloTargets`` t, or t itself); the levels of one size share one tensor.  ``tgt_of``: per level an integer tensor [N_l], the
    ground truth of every row (``SoloTargets.sel_inst``).  ``img_of``: per level an integer tensor [N_l], or None for what ``counts``
    says.  ``counts[l][b]``: the rows of (level, image) -- host values since the targets' synchronisation (``SoloTargets.counts``
    entries ``(pairs, set cells)`` are accepted).  An index of -1 (or out of range) makes the row inert: zero loss, zero gradient, and
    it leaves the denominators of the means.

    Returns ``(loss_boxpro, loss_levelset, rows)``; ``rows`` holds ``proj`` and ``levelset`` [M] in the ragged order (size group,
    image, level, cell), ``live`` [M] and ``segments``: the host list of (level, first plane, planes, image) in that order.  Autograd
    reaches every ``ins_pred_rows[l]`` and ``ctx.lst_feat``.  No host synchronisation.  Zero rows give two zeros connected to the graph
    (the reference raises there)."""
    levels = list(ins_pred_rows)
    if len(levels) != len(ctx.level_sizes):
        raise RuntimeError(f'{len(levels)} levels of ins_pred_rows for the context\'s {len(ctx.level_sizes)}')
    need_cuda(**{f'ins_pred_rows[{l}]': t for l, t in enumerate(levels)})
    _need_fp32(**{f'ins_pred_rows[{l}]': t for l, t in enumerate(levels)})
    if hasattr(masks, 'level_factor'):
        masks = [masks.masks[f] for f in masks.level_factor]
    masks, tgt_of = list(masks), list(tgt_of)
    L = len(levels)
    if len(masks) != L or len(tgt_of) != L or (img_of is not None and len(img_of) != L):
        raise RuntimeError(f'{L} levels, {len(masks)} of masks and {len(tgt_of)} of tgt_of')
    need_cuda(**{f'masks[{l}]': t for l, t in enumerate(masks)}, **{f'tgt_of[{l}]': t for l, t in enumerate(tgt_of)})
    plan = _Plan(ctx, levels, masks, counts)
    for l in range(L):
        if tgt_of[l].numel() != plan.level_rows[l] or (img_of is not None and img_of[l].numel() != plan.level_rows[l]):
            raise RuntimeError(f'tgt_of[{l}] / img_of[{l}] must hold {plan.level_rows[l]} rows')
    dev = levels[0].device
    if plan.M == 0:
        z = _zero(levels)
        e = torch.zeros((0,), dtype=torch.float32, device=dev)
        return z, z.clone(), dict(proj=e, levelset=e.clone(), live=e.clone(), segments=[])
    i32 = dict(dtype=torch.int32, device=dev)
    row_src = torch.cat([torch.arange(l * _lib.BLS_LEVEL_ROWS + a, l * _lib.BLS_LEVEL_ROWS + a + c, **i32) for l, a, c, _ in plan.segments])
    tgt = torch.cat([tgt_of[l][a:a + c] for l, a, c, _ in plan.segments]).to(torch.int32)
    if img_of is None:
        img = torch.cat([torch.full((c,), b, **i32) for _, b, _, c in plan.blocks])
    else:
        img = torch.cat([img_of[l][a:a + c] for l, a, c, _ in plan.segments]).to(torch.int32)
    w_proj, w_ls = float(loss_boxpro_weight), float(loss_levelset_weight)
    p, per_proj, per_img, pixel_num, live = _Front.apply(plan, row_src, tgt, img, w_proj, w_ls * W_IMG, *levels)
    # :353-358: per (size, image) one tree of each kind with the image's rows of the size group as channels
    bounds = []
    for g, b, first, rows in plan.blocks:
        lo, hi = plan.row_pixels(g, first, rows)
        bounds.append((lo, hi, rows, (hi - lo) // rows))
    y_img, y_lst = [], []
    for (g, b, _, _), x in zip(plan.blocks, _Blocks.apply(p, tuple(bounds))):
        si, sp, sc, lv = (t[b:b + 1] for t in ctx.img_order[g])
        y = _Refine.apply(x, ctx.w_img[g][b:b + 1], si, sp, sc, True, lv)
        si, sp, sc, lv = (t[b:b + 1] for t in ctx.lst_order[g])
        z = _Refine.apply(y, ctx.w_lst[g][b:b + 1], si, sp, sc, False, lv)
        y_img.append(y.reshape(-1))
        y_lst.append(z.reshape(-1))
    per_feat = _High.apply(plan, w_ls * W_FEAT, p, torch.cat(y_img), torch.cat(y_lst), tgt, live, pixel_num)      # :358-360
    per_levelset = per_img + per_feat                                                                             # :363
    count = live.sum().clamp(min=1)
    return per_proj.sum() / count, per_levelset.sum() / count, dict(proj=per_proj, levelset=per_levelset, live=live, segments=list(plan.segments))


def parse_box_solov2_loss_cfg(bbox_head_cfg):
    """``bbox_head=dict(type='BoxSOLOv2Head', loss_cate=..., loss_boxpro=..., loss_levelset=...)`` of ``configs/boxlevelset/*`` (dict or
    namespace) -> what ``parse_solo_head_cfg`` returns plus ``loss_boxpro`` and ``loss_levelset``, the two loss weights."""
    from .solo_targets import parse_solo_head_cfg
    head = parse_solo_head_cfg(bbox_head_cfg)
    if head['mode'] != 'boxlevelset':
        raise NotImplementedError(f"bbox_head.type {cfg_get(bbox_head_cfg, 'type')!r} is not supported here: only 'BoxSOLOv2Head'")
    for name, kind in (('loss_boxpro', 'BoxProjectionLoss'), ('loss_levelset', 'LevelsetLoss')):
        blk = cfg_get(bbox_head_cfg, name)
        if blk is None:
            raise TypeError(f'bbox_head has no `{name}`')
        if cfg_get(blk, 'type') != kind:
            raise NotImplementedError(f"bbox_head.{name}.type {cfg_get(blk, 'type')!r} is not supported: only {kind!r}")
        cfg_only(blk, f'bbox_head.{name}', ('type', 'loss_weight'))
        head[name] = float(cfg_get(blk, 'loss_weight', 1.0))
    return head


def box_solov2_loss(kernel_preds, cate_preds, feature_pred, levelset_feats, gt_bbox_list, gt_label_list, gt_mask_list, img, img_metas,
                    head_cfg, *, level_sizes=None, trees=None):
    """``BoxSOLOv2Head.loss`` (:259-388) from the head's raw outputs: ``kernel_preds`` the L maps [B,E,S_l,S_l], ``cate_preds`` the L
    maps [B,classes,S_l,S_l], ``feature_pred`` [B,E,h,w], ``levelset_feats`` [B,Cf,hf,wf], ``img`` the normalised image [B,3,H,W];
    ``head_cfg`` the ``bbox_head`` block of the config (dict or namespace).  ``level_sizes``: the (oh, ow) of every level's mask
    prediction (the reference's ``2 x featmap_size``); by default ``(8 h / stride_l, 8 w / stride_l)`` of ``feature_pred``'s (h, w),
    which must divide.  ``img_metas`` is accepted for the signature and not read.  Returns ``dict(loss_boxpro, loss_levelset,
    loss_cate)``, all 0-dim.  The steps: ``box_solov2_targets`` (the one host synchronisation) -> ``box_solov2_set_cells`` ->
    ``box_solov2_ins_preds`` -> ``box_solov2_mask_losses`` -> ``solo_cate_loss``."""
    from .box_solo_masks import box_solov2_ins_preds, box_solov2_set_cells
    from .solo_targets import box_solov2_targets, solo_cate_loss
    head = parse_box_solov2_loss_cfg(head_cfg)
    kernel_preds, cate_preds = list(kernel_preds), list(cate_preds)
    h, w = int(feature_pred.shape[-2]), int(feature_pred.shape[-1])
    if level_sizes is None:
        if any((8 * h) % s or (8 * w) % s for s in head['strides']):
            raise RuntimeError(f'feature_pred of {h}x{w} does not divide by the strides {head["strides"]}: pass level_sizes')
        level_sizes = [(8 * h // s, 8 * w // s) for s in head['strides']]
    level_sizes = [(int(s[0]), int(s[1])) for s in level_sizes]
    targets = box_solov2_targets(gt_bbox_list, gt_label_list, gt_mask_list, level_sizes,
                                 **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')})
    loss_cate = solo_cate_loss(cate_preds, targets.flat_cate_labels, targets.num_ins, head['gamma'], head['alpha'], head['loss_weight_cate'])
    cells = box_solov2_set_cells(targets)
    rows = box_solov2_ins_preds(kernel_preds, feature_pred, cells, level_sizes)
    ctx = BoxLevelSetLossContext(img.to(torch.float32), levelset_feats.float(), level_sizes, trees)
    counts = [[int(targets.counts[l][b][1]) for b in range(targets.B)] for l in range(len(level_sizes))]
    loss_boxpro, loss_levelset, _ = box_solov2_mask_losses(ctx, rows, targets, targets.sel_inst, None, counts, head['loss_boxpro'], head['loss_levelset'])
    return dict(loss_boxpro=loss_boxpro, loss_levelset=loss_levelset, loss_cate=loss_cate)
