"""``Box2MaskHead.loss`` / ``loss_single`` (``mmdet/models/dense_heads/box2mask_head.py:192-335``) as one call for all decoder layers,
on the kernels of ``csrc/box2mask_loss.hip`` (``include/boxinst/boxinst_hip_b2m.h``).

The reference runs ``loss_single`` once per decoder layer.  Most of a call does not depend on the layer: the image and the level-set
feature resized to the prediction and to 96x96, both minimum spanning trees with their breadth-first orders and edge weights, the LCM
affinity (per image), the resized box targets and ``pixel_num`` (per ground truth).  ``Box2MaskLossContext`` computes those once per
iteration.  Only the matched rows of ``mask_preds`` depend on the layer; ``box2mask_mask_losses`` evaluates the rows of ALL layers
together, reading image, targets and affinity through index arrays instead of the reference's per-instance copies (:280-297).  Both
tree filters run once per image over that image's rows of all layers as channels of one tree -- the reference's batch of per-instance
copies of one tree, and its weight gradient summed over the copies.  No host synchronisation; no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import cfg_get, cfg_only, current_stream, need_cuda
from .levelset import BoxProjectionLoss, LocalConsistencyModule
from .tree_filter import MinimumSpanningTree, TreeFilter2D, _bfs_levels, _Refine

_HEADER = 'boxinst_hip_b2m.h'
W_IMG, W_FEAT, W_LCM = 0.05, 5.0, 0.2                # box2mask_head.py:312, :327, :331
LCM_ITERS, LCM_DILATION = 10, 2                      # levelset_loss.py:55


def _resize(x, size):
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False)


def _axis_matrix(n_in, n_out, dev):
    """[n_out, n_in]: one axis of ``_resize`` as a matrix -- torch's source index scale * (o + 0.5) - 0.5 clamped at 0, its two taps and weights."""
    o = torch.arange(n_out, device=dev, dtype=torch.float64)           # the index in double, as csrc/box2mask_loss.hip takes it (b2m_axis)
    src = ((o + 0.5) * (float(n_in) / float(n_out)) - 0.5).clamp(min=0)
    i0 = src.floor().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = (src - i0).to(torch.float32)
    m = torch.zeros((n_out, n_in), dtype=torch.float32, device=dev)
    m.scatter_add_(1, i0.long()[:, None], (1 - l1)[:, None])           # at most two terms per element, onto zero: the order cannot matter
    m.scatter_add_(1, i1.long()[:, None], l1[:, None])
    return m


def _resize_det(x, size):
    """``_resize`` for a tensor that carries a gradient: rows, then columns, as two matrix products.  The backward of F.interpolate adds
    with float atomics, so two runs of it differ in the last bits; a matrix product's backward is a matrix product."""
    h, w = int(size[0]), int(size[1])
    if tuple(x.shape[-2:]) == (h, w):
        return x
    return torch.matmul(torch.matmul(x, _axis_matrix(x.shape[-1], w, x.device).t()).transpose(-1, -2),
                        _axis_matrix(x.shape[-2], h, x.device).t()).transpose(-1, -2)


class _EdgeWeight(torch.autograd.Function):
    """``TreeFilter2D.build_edge_weight(fm, si, sp, low_tree=False)`` (tree_filter.py:90-108, one group) with a backward made of gathers:
    position i receives its own edge's term and, with the opposite sign, the terms of its children (``sorted_child``, 0 = none, in slot
    order).  The autograd of the module's two ``torch.gather`` calls scatters with float atomics instead: up to five adds per vertex in
    whatever order they land."""

    @staticmethod
    def forward(ctx, fm, si, sp, sc):
        B, C = fm.shape[:2]
        x = fm.reshape(B, C, -1)
        src = TreeFilter2D.batch_index_opr(x, si)
        diff = src - TreeFilter2D.batch_index_opr(src, sp)
        w = torch.exp(-(diff * diff).sum(dim=1))
        ctx.save_for_backward(diff, w, si, sc)
        ctx.shape = fm.shape
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, gw):
        diff, w, si, sc = ctx.saved_tensors
        t = (gw * w * -2.0).unsqueeze(1) * diff
        t[:, :, 0] = 0                                                     # the root has no edge
        r = t
        for k in range(sc.shape[2]):
            r = r - TreeFilter2D.batch_index_opr(t, sc[:, :, k])           # slot 0 = no child reads the root's zero
        out = torch.empty_like(r)
        out.scatter_(2, si.long().unsqueeze(1).expand(-1, r.shape[1], -1), r)      # a permutation: every element written once
        return out.view(ctx.shape), None, None, None


class _Take(torch.autograd.Function):
    """v[idx] for a bijection idx between rows and (layer, slot) cells, its inverse given: the backward is the gather g[inv], not a scatter-add."""

    @staticmethod
    def forward(ctx, v, idx, inv):
        ctx.save_for_backward(inv)
        return v[idx]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        return g.reshape(-1)[inv], None, None


def _need_fp32(**tensors):
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise RuntimeError(f'{name} must be float32, got {t.dtype}: Box2MaskHead.loss is force_fp32 in the reference')


class Box2MaskLossContext:
    """What ``loss_single`` recomputes in every decoder layer, once per iteration.

    ``norm_img`` [B,3,H,W], ``lst_feat`` [B,Cf,hf,wf] (differentiable), ``pred_shape`` (h, w), per image ``gt_masks`` [G_i,H,W].
    ``trees`` = (img_tree, lst_tree), each [B,V-1,2] int32 over the ``scaled_size`` grid, replaces the two ``MinimumSpanningTree`` calls.

    Keeps: ``img`` [B,3,h,w], ``feat`` [B,Cf,h,w] (:232-233); ``img_s``, ``feat_s`` at ``scaled_size`` (:269-270); both trees, one
    breadth-first order per tree, the edge weights ``w_img`` (low_tree, sigma 0.02, no gradient) and ``w_lst`` (differentiable) [B,V];
    ``aff`` [B,8,sh,sw]; per ground truth ``T`` [G,h,w] (:300), ``T_small`` [G,sh,sw] (:329, the resize of the resize) and
    ``pixel_num`` [G] (:309-310, clamped); ``counts`` and ``gt_offsets`` as Python ints."""

    def __init__(self, norm_img, lst_feat, pred_shape, gt_masks_list, scaled_size=(96, 96), trees=None):
        need_cuda(norm_img=norm_img, lst_feat=lst_feat)
        need_cuda(**{f'gt_masks_list[{i}]': m for i, m in enumerate(gt_masks_list)})
        _need_fp32(norm_img=norm_img, lst_feat=lst_feat)
        B = norm_img.shape[0]
        if lst_feat.shape[0] != B or len(gt_masks_list) != B:
            raise RuntimeError(f'{B} images, {lst_feat.shape[0]} feature maps and {len(gt_masks_list)} ground-truth entries')
        self.device = norm_img.device
        self.B, self.pred_shape, self.scaled_size = B, (int(pred_shape[0]), int(pred_shape[1])), (int(scaled_size[0]), int(scaled_size[1]))
        self.lst_feat = lst_feat
        self.img = _resize(norm_img.detach(), self.pred_shape).contiguous()
        self.feat = _resize_det(lst_feat, self.pred_shape)
        self.img_s = _resize(self.img, self.scaled_size).contiguous()
        self.feat_s = _resize_det(self.feat, self.scaled_size)
        if trees is None:
            mst = MinimumSpanningTree(TreeFilter2D.norm2_distance)
            trees = (mst(self.img_s), mst(self.feat_s))
        self.img_tree, self.lst_tree = trees
        self.img_order = _bfs_levels(self.img_tree, 4)            # (sorted_index, sorted_parent, sorted_child, levels)
        self.lst_order = _bfs_levels(self.lst_tree, 4)
        tf = TreeFilter2D()
        self.w_img = tf.build_edge_weight(self.img_s, self.img_order[0], self.img_order[1], True).contiguous()
        self.w_lst = _EdgeWeight.apply(self.feat_s, self.lst_order[0], self.lst_order[1], self.lst_order[2])
        self.aff = LocalConsistencyModule(num_iter=LCM_ITERS, dilations=[LCM_DILATION]).affinity(self.img_s)
        masks = [m[:, 0] if m.dim() == 4 else m for m in gt_masks_list]
        self.counts = [int(m.shape[0]) for m in masks]
        self.gt_offsets = [sum(self.counts[:i]) for i in range(B + 1)]
        self.G = self.gt_offsets[-1]
        if self.G:
            self.T = _resize(torch.cat(masks, 0).to(torch.float32).unsqueeze(1), self.pred_shape)[:, 0].contiguous()
            self.T_small = _resize(self.T.unsqueeze(1), self.scaled_size)[:, 0].contiguous()
        else:
            self.T = norm_img.new_zeros((0,) + self.pred_shape)
            self.T_small = norm_img.new_zeros((0,) + self.scaled_size)
        self.pixel_num = self.T.sum((1, 2)).clamp(min=1)


def build_row_table(pos_inds, pos_assigned_gt_inds, counts, B, Q, gt_offsets):
    """The rows of all layers, on the device: (row_plane, tgt_of, img_of, layer_of) int32 [M], row_of int64 [L,S] and cell_of int64 [M].

    Layer l's arrays hold S = sum_i min(Q, G_i) slots, image i's from sum_{k<i} min(Q, G_k) on.  Row m = L * off_i + l * n_i + k is slot
    off_i + k of layer l: the rows are ordered by (image, layer), so one image's rows of all layers are contiguous.  ``row_of[l, s]`` is
    the row of slot s of layer l and ``cell_of[m]`` = l * S + s its inverse.  A slot holding -1 gives an inert row: row_plane = tgt_of = img_of = -1.  Only ``counts``, B, Q and
    ``gt_offsets`` are host values; nothing is read back."""
    L = len(pos_inds)
    dev = pos_inds[0].device
    n = [min(int(Q), int(c)) for c in counts]
    off = [sum(n[:i]) for i in range(B + 1)]
    S = off[-1]
    lay, slot, img, gto, row_of = [], [], [], [], []
    for i in range(B):
        if n[i] == 0:
            continue
        r = torch.arange(L * n[i], device=dev)
        lay.append(r // n[i])
        slot.append(off[i] + r % n[i])
        img.append(torch.full_like(r, i))
        gto.append(torch.full_like(r, int(gt_offsets[i])))
        row_of.append(L * off[i] + torch.arange(L, device=dev)[:, None] * n[i] + torch.arange(n[i], device=dev)[None, :])
    if S == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return e, e.clone(), e.clone(), e.clone(), torch.empty((L, 0), dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    lay, slot, img, gto = torch.cat(lay), torch.cat(slot), torch.cat(img), torch.cat(gto)
    q = torch.stack([p.to(torch.int64) for p in pos_inds])[lay, slot]
    g = torch.stack([p.to(torch.int64) for p in pos_assigned_gt_inds])[lay, slot]
    live = (q >= 0) & (g >= 0)
    minus = torch.full_like(q, -1)
    row_plane = torch.where(live, lay * (B * Q) + img * Q + q, minus).to(torch.int32)
    tgt_of = torch.where(live, gto + g, minus).to(torch.int32)
    img_of = torch.where(live, img, minus).to(torch.int32)
    return row_plane, tgt_of, img_of, lay.to(torch.int32), torch.cat(row_of, 1), lay * S + slot


class _Scores(torch.autograd.Function):
    """(p [M,h,w], p_small [M,sh,sw]) of the rows from the L layer tensors read in place; the backward writes each layer's whole gradient."""

    @staticmethod
    def forward(ctx, row_plane, plane_row, small, *layers):
        lib = _lib.load()
        dev = layers[0].device
        L = len(layers)
        Bn, Q, h, w = layers[0].shape
        M = row_plane.numel()
        sh, sw = small
        flat = [t.detach().contiguous() for t in layers]
        p = torch.empty((M, h, w), dtype=torch.float32, device=dev)
        ps = torch.empty((M, sh, sw), dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in flat])
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_b2m_scores_f32', lib.bxi_b2m_scores_f32(
                ptrs, L, Bn * Q, h, w, row_plane.data_ptr(), M, sh, sw, p.data_ptr(), ps.data_ptr(), current_stream(dev)), _HEADER)
        ctx.save_for_backward(p, plane_row)
        ctx.meta = (L, Bn, Q, h, w, sh, sw, M)
        return p, ps

    @staticmethod
    @once_differentiable
    def backward(ctx, g_p, g_ps):
        p, plane_row = ctx.saved_tensors
        L, Bn, Q, h, w, sh, sw, M = ctx.meta
        dev = p.device
        lib = _lib.load()
        g_p, g_ps = g_p.contiguous(), g_ps.contiguous()
        grads = []
        with torch.cuda.device(dev):
            for l in range(L):
                if not ctx.needs_input_grad[3 + l]:
                    grads.append(None)
                    continue
                g = torch.empty((Bn, Q, h, w), dtype=torch.float32, device=dev)
                _lib.check_supported('bxi_b2m_scores_backward_f32', lib.bxi_b2m_scores_backward_f32(
                    g_p.data_ptr(), g_ps.data_ptr(), p.data_ptr(), plane_row[l].data_ptr(), Bn * Q, M, h, w, sh, sw, g.data_ptr(),
                    current_stream(dev)), _HEADER)
                grads.append(g)
        return (None, None, None, *grads)


class _RowLevelset(torch.autograd.Function):
    """``LevelsetLoss`` on (p T, (1 - p) T) against target * T per row, T = T_all[tgt_of]; ``target`` shared per image or the row's own."""

    @staticmethod
    def forward(ctx, p, target, T_all, pixel_num, tgt_of, img_of, shared, n_img, weight):
        lib = _lib.load()
        dev = p.device
        M, h, w = p.shape
        Cc, G = target.shape[1], T_all.shape[0]
        pc, tc = p.detach().contiguous(), target.detach().contiguous()
        loss = torch.empty((M,), dtype=torch.float32, device=dev)
        nbytes = lib.bxi_b2m_levelset_state_bytes(M, Cc)
        if nbytes == 0:
            raise NotImplementedError(f'bxi_b2m_levelset_forward_f32: outside the support set of include/boxinst/{_HEADER}')
        state = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_b2m_levelset_forward_f32', lib.bxi_b2m_levelset_forward_f32(
                pc.data_ptr(), T_all.data_ptr(), tc.data_ptr(), int(shared), tgt_of.data_ptr(), img_of.data_ptr(), pixel_num.data_ptr(), M, G,
                n_img, Cc, h, w, float(weight), loss.data_ptr(), state.data_ptr(), current_stream(dev)), _HEADER)
        ctx.save_for_backward(pc, tc, T_all, pixel_num, tgt_of, img_of, state)
        ctx.meta = (bool(shared), n_img, float(weight))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pc, tc, T_all, pixel_num, tgt_of, img_of, state = ctx.saved_tensors
        shared, n_img, weight = ctx.meta
        dev = pc.device
        M, h, w = pc.shape
        Cc, G = tc.shape[1], T_all.shape[0]
        g = g.to(torch.float32).contiguous()
        g_p = torch.empty_like(pc)
        g_t = None if shared or not ctx.needs_input_grad[1] else torch.empty_like(tc)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_b2m_levelset_backward_f32', _lib.load().bxi_b2m_levelset_backward_f32(
                pc.data_ptr(), T_all.data_ptr(), tc.data_ptr(), int(shared), tgt_of.data_ptr(), img_of.data_ptr(), pixel_num.data_ptr(), M, G,
                n_img, Cc, h, w, weight, state.data_ptr(), g.data_ptr(), g_p.data_ptr(), None if g_t is None else g_t.data_ptr(),
                current_stream(dev)), _HEADER)
        return g_p, g_t, None, None, None, None, None, None, None


def _row_lcm(aff, phi, img_of, transpose):
    lib = _lib.load()
    dev = phi.device
    M, h, w = phi.shape
    out = torch.empty_like(phi)
    ws = torch.empty(max(lib.bxi_lcm_workspace_bytes(M, h, w), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_b2m_lcm_refine_f32', lib.bxi_b2m_lcm_refine_f32(
            aff.data_ptr(), phi.data_ptr(), img_of.data_ptr(), aff.shape[0], M, h, w, LCM_DILATION, LCM_ITERS, int(transpose), out.data_ptr(),
            ws.data_ptr(), ws.numel(), current_stream(dev)))
    return out


class _RowLcm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, aff, phi, img_of):
        ctx.save_for_backward(aff, img_of)
        return _row_lcm(aff, phi.detach().contiguous(), img_of, 0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        aff, img_of = ctx.saved_tensors
        return None, _row_lcm(aff, g.contiguous(), img_of, 1), None


def _zero_match(all_mask_preds):
    """:262-267: ``mask_preds[mask_weights > 0].sum()`` of an empty selection, per layer -- zero, with a zero gradient."""
    z = torch.stack([mp[:0].sum() for mp in all_mask_preds])
    return z, z.clone()


def box2mask_mask_losses(ctx, all_mask_preds, pos_inds, pos_assigned_gt_inds, counts, loss_box_weight=1.0, loss_mask_weight=1.0):
    """``loss_project`` [L] and ``loss_levelset`` [L] of :260-335 for all decoder layers.

    ``all_mask_preds``: L tensors [B,Q,h,w] fp32, separate allocations, read in place.  ``pos_inds`` / ``pos_assigned_gt_inds``: per
    layer the compacted arrays of ``MaskHungarianAssigner.assign_batch``; ``counts``: the ground truths per image.  Autograd reaches
    every ``all_mask_preds[l]`` and ``ctx.lst_feat``.  A slot holding -1 is an inert row: no loss, no gradient, and it leaves the
    denominators of its layer's means (counted on the device); a layer without live rows returns zero losses and zero gradients."""
    all_mask_preds = list(all_mask_preds)
    L = len(all_mask_preds)
    if L == 0 or len(pos_inds) != L or len(pos_assigned_gt_inds) != L:
        raise RuntimeError(f'{L} layers of mask_preds, {len(pos_inds)} of pos_inds and {len(pos_assigned_gt_inds)} of pos_assigned_gt_inds')
    need_cuda(**{f'all_mask_preds[{l}]': t for l, t in enumerate(all_mask_preds)})
    _need_fp32(**{f'all_mask_preds[{l}]': t for l, t in enumerate(all_mask_preds)})
    if L > _lib.B2M_MAX_LAYERS:
        raise NotImplementedError(f'{L} layers: at most {_lib.B2M_MAX_LAYERS} per call (include/boxinst/{_HEADER})')
    B, Q, h, w = all_mask_preds[0].shape
    if any(tuple(t.shape) != (B, Q, h, w) for t in all_mask_preds) or (h, w) != ctx.pred_shape or B != ctx.B:
        raise RuntimeError(f'every layer must be [{ctx.B},Q,{ctx.pred_shape[0]},{ctx.pred_shape[1]}]')
    if [int(c) for c in counts] != ctx.counts:
        raise RuntimeError(f'counts {list(counts)} differ from the context\'s ground truths {ctx.counts}')
    dev = all_mask_preds[0].device
    row_plane, tgt_of, img_of, layer_of, row_of, cell_of = build_row_table(pos_inds, pos_assigned_gt_inds, counts, B, Q, ctx.gt_offsets)
    M = row_plane.numel()
    if M == 0:
        return _zero_match(all_mask_preds)
    sh, sw = ctx.scaled_size
    rows = torch.arange(M, device=dev, dtype=torch.int32)
    live = row_plane >= 0
    # plane_row[l, b * Q + q]: the row of every plane, -1 where none; inert rows land in one spare slot behind the table
    plane_row = torch.full((L * B * Q + 1,), -1, dtype=torch.int32, device=dev)
    plane_row.scatter_(0, torch.where(live, row_plane, torch.full_like(row_plane, L * B * Q)).to(torch.int64), rows)
    plane_row = plane_row[:L * B * Q].view(L, B * Q)

    p, p_small = _Scores.apply(row_plane, plane_row, (sh, sw), *all_mask_preds)
    tsel = tgt_of.clamp(min=0).to(torch.int64)
    # :303 (the existing projection kernel on the rows' targets; an inert row's value is dropped below)
    per_project = BoxProjectionLoss(loss_box_weight)(p.unsqueeze(1), ctx.T.index_select(0, tsel).unsqueeze(1))
    per_img = _RowLevelset.apply(p, ctx.img, ctx.T, ctx.pixel_num, tgt_of, img_of, True, B, loss_mask_weight)             # :312
    # :319-322: per image one tree with its rows of all layers as channels
    n = [min(Q, c) for c in ctx.counts]
    f_img, f_lst, at = [], [], 0
    for b in range(B):
        cb = L * n[b]
        if cb == 0:
            continue
        x = p_small[at:at + cb].reshape(1, cb, sh * sw)
        si, sp, sc, lv = (t[b:b + 1] for t in ctx.img_order)
        y = _Refine.apply(x, ctx.w_img[b:b + 1], si, sp, sc, True, lv)
        si, sp, sc, lv = (t[b:b + 1] for t in ctx.lst_order)
        z = _Refine.apply(y, ctx.w_lst[b:b + 1], si, sp, sc, False, lv)
        f_img.append(y.view(cb, sh, sw))
        f_lst.append(z.view(cb, sh, sw))
        at += cb
    deep = _resize_det(torch.stack([torch.cat(f_img), torch.cat(f_lst)], 1), (h, w))                                          # :323-325
    per_feat = _RowLevelset.apply(p, deep, ctx.T, ctx.pixel_num, tgt_of, img_of, False, B, loss_mask_weight)              # :327
    # :329-331
    refined = _RowLcm.apply(ctx.aff, p_small, img_of)
    t_small = ctx.T_small.index_select(0, tsel)
    per_consist = ((refined - p_small).abs() * t_small).sum((1, 2))
    per_region = t_small.sum((1, 2))

    # per-layer means in a fixed order: the rows of layer l gathered to [L,S] through row_of and summed along the slots
    keep = live.to(torch.float32)[row_of]
    count = keep.sum(1).clamp(min=1)

    def per_layer(v):
        return (_Take.apply(v, row_of, cell_of) * keep).sum(1)

    loss_project = per_layer(per_project) / count
    loss_lcm = W_LCM * per_layer(per_consist) / per_layer(per_region).clamp(min=1)
    loss_levelset = W_IMG * per_layer(per_img) / count + W_FEAT * per_layer(per_feat) / count + loss_lcm
    return loss_project, loss_levelset


def parse_box2mask_head_cfg(cfg):
    """The ``panoptic_head=dict(type='Box2MaskHead', ...)`` block of ``configs/box2mask/*`` (dict or namespace) -> the keyword
    arguments of ``box2mask_loss`` that come from it: class_weight, loss_cls_weight, loss_box, loss_mask, num_classes.  Keys that shape
    the network are accepted and ignored; a loss the functions here do not compute raises NotImplementedError naming the field."""
    if cfg_get(cfg, 'type') != 'Box2MaskHead':
        raise NotImplementedError(f"panoptic_head.type {cfg_get(cfg, 'type')!r} is not supported: only 'Box2MaskHead'")
    num_classes = int(cfg_get(cfg, 'num_things_classes', 80)) + int(cfg_get(cfg, 'num_stuff_classes', 53))
    lc, lb, lm = cfg_get(cfg, 'loss_cls'), cfg_get(cfg, 'loss_box'), cfg_get(cfg, 'loss_mask')
    for name, blk in (('loss_cls', lc), ('loss_box', lb), ('loss_mask', lm)):
        if blk is None:
            raise TypeError(f'panoptic_head has no `{name}`')
    if cfg_get(lc, 'type') != 'CrossEntropyLoss':
        raise NotImplementedError(f"panoptic_head.loss_cls.type {cfg_get(lc, 'type')!r} is not supported: only 'CrossEntropyLoss'")
    cfg_only(lc, 'panoptic_head.loss_cls', ('type', 'use_sigmoid', 'loss_weight', 'reduction', 'class_weight'))
    if cfg_get(lc, 'use_sigmoid', False):
        raise NotImplementedError('panoptic_head.loss_cls.use_sigmoid=True is not supported')
    if cfg_get(lc, 'reduction', 'mean') != 'mean':
        raise NotImplementedError("panoptic_head.loss_cls.reduction: only 'mean' is supported")
    class_weight = cfg_get(lc, 'class_weight')
    if class_weight is None or len(class_weight) != num_classes + 1:
        raise NotImplementedError(f'panoptic_head.loss_cls.class_weight must list {num_classes + 1} weights')
    if cfg_get(lb, 'type') != 'BoxProjectionLoss':
        raise NotImplementedError(f"panoptic_head.loss_box.type {cfg_get(lb, 'type')!r} is not supported: only 'BoxProjectionLoss'")
    cfg_only(lb, 'panoptic_head.loss_box', ('type', 'loss_weight'))
    if cfg_get(lm, 'type') != 'LevelsetLoss':
        raise NotImplementedError(f"panoptic_head.loss_mask.type {cfg_get(lm, 'type')!r} is not supported: only 'LevelsetLoss'")
    cfg_only(lm, 'panoptic_head.loss_mask', ('type', 'loss_weight'))
    return dict(class_weight=[float(v) for v in class_weight], loss_cls_weight=float(cfg_get(lc, 'loss_weight', 1.0)),
                loss_box=float(cfg_get(lb, 'loss_weight', 1.0)), loss_mask=float(cfg_get(lm, 'loss_weight', 1.0)), num_classes=num_classes)


_CLASS_WEIGHTS = {}


def _class_weight(class_weight, like):
    """``cls_scores.new_tensor(self.class_weight)`` (:253), copied to the device once per (weights, device): the copy of a host list is the
    one synchronising call the reference's statement would leave in every iteration."""
    if torch.is_tensor(class_weight):
        return class_weight.to(like)
    key = (tuple(float(v) for v in class_weight), like.device)
    if key not in _CLASS_WEIGHTS:
        _CLASS_WEIGHTS[key] = like.new_tensor(key[0])
    return _CLASS_WEIGHTS[key]


def _weight_of(loss):
    return float(loss.loss_weight) if hasattr(loss, 'loss_weight') else float(loss)


def box2mask_loss(all_cls_scores, all_mask_preds, all_lst_feats, gt_labels_list, gt_masks_list, img_metas, norm_img, *, assigner,
                  class_weight, loss_cls_weight, loss_box, loss_mask, num_classes, scaled_size=(96, 96), trees=None):
    """``Box2MaskHead.loss`` (:192-221): the reference's loss dict (``loss_cls``, ``loss_project``, ``loss_levelset`` of the last layer,
    ``d{i}.*`` of the others) for L layers of ``all_cls_scores`` [B,Q,C+1] and ``all_mask_preds`` [B,Q,h,w].

    ``all_lst_feats`` is one tensor, or a list of L whose entries are the same object (what the reference passes: ``levelset_bottom``
    of one ``mask_feature``); distinct tensors get one ``Box2MaskLossContext`` each.  ``loss_box`` / ``loss_mask`` are the two
    loss_weights (or modules that carry one); ``class_weight`` is a list (copied to the device on its first use) or a
    device tensor.  ``loss_cls`` is mmdet's class-weighted cross entropy with
    ``avg_factor = class_weight[labels].sum()`` as torch ops over the stacked scores.  ``img_metas`` is unused, as in the reference's
    assigner.  No host synchronisation."""
    all_cls_scores, all_mask_preds = list(all_cls_scores), list(all_mask_preds)
    L = len(all_mask_preds)
    if L == 0 or len(all_cls_scores) != L:
        raise RuntimeError(f'{len(all_cls_scores)} layers of cls_scores and {L} of mask_preds')
    need_cuda(norm_img=norm_img, **{f'all_cls_scores[{l}]': t for l, t in enumerate(all_cls_scores)})
    need_cuda(**{f'all_mask_preds[{l}]': t for l, t in enumerate(all_mask_preds)})
    _need_fp32(**{f'all_cls_scores[{l}]': t for l, t in enumerate(all_cls_scores)}, **{f'all_mask_preds[{l}]': t for l, t in enumerate(all_mask_preds)})
    feats = [all_lst_feats] * L if torch.is_tensor(all_lst_feats) else list(all_lst_feats)
    if len(feats) != L:
        raise RuntimeError(f'{len(feats)} entries of all_lst_feats for {L} layers')
    B, Q = all_mask_preds[0].shape[:2]
    pred_shape = tuple(all_mask_preds[0].shape[-2:])
    labels, pos, pos_gt, counts = [], [], [], None
    for l in range(L):                                                         # get_targets (:135-189), launches only
        gt_inds, assigned, p_l, g_l, counts = assigner.assign_batch(all_cls_scores[l], all_mask_preds[l], gt_labels_list, gt_masks_list)
        labels.append(torch.where(gt_inds > 0, assigned, assigned.new_full((), num_classes)))
        pos.append(p_l)
        pos_gt.append(g_l)
    # :249-258 for all layers: F.cross_entropy(weight=class_weight, reduction='none') summed per layer over avg_factor + eps
    cw = _class_weight(class_weight, all_cls_scores[0])
    flat_labels = torch.stack(labels).reshape(-1)
    ce = F.cross_entropy(torch.stack(all_cls_scores).reshape(L * B * Q, -1), flat_labels, weight=cw, reduction='none')
    avg = cw[flat_labels].view(L, -1).sum(1)
    loss_cls = float(loss_cls_weight) * ce.view(L, -1).sum(1) / (avg + torch.finfo(torch.float32).eps)
    loss_project, loss_levelset = [None] * L, [None] * L
    groups = {}
    for l, f in enumerate(feats):
        groups.setdefault(id(f), []).append(l)
    for ls in groups.values():
        ctx = Box2MaskLossContext(norm_img, feats[ls[0]], pred_shape, gt_masks_list, scaled_size, trees)
        lp, lv = box2mask_mask_losses(ctx, [all_mask_preds[l] for l in ls], [pos[l] for l in ls], [pos_gt[l] for l in ls], counts,
                                      _weight_of(loss_box), _weight_of(loss_mask))
        for k, l in enumerate(ls):
            loss_project[l], loss_levelset[l] = lp[k], lv[k]
    out = {'loss_cls': loss_cls[L - 1], 'loss_project': loss_project[L - 1], 'loss_levelset': loss_levelset[L - 1]}
    for l in range(L - 1):
        out[f'd{l}.loss_cls'], out[f'd{l}.loss_project'], out[f'd{l}.loss_levelset'] = loss_cls[l], loss_project[l], loss_levelset[l]
    return out
