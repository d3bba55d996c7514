"""BoxLevelSet's mask predictions (csrc/solo_dconv_level.hip, include/boxinst/boxinst_hip_dconvl.h): the step between the training
targets and ``BoxProjectionLoss`` / ``LevelsetLoss``, and test time from the kernels instead of from every cell's mask.

    box_solov2_ins_preds               <-> BoxSOLOv2Head.forward, box_solov2_head.py:205-216 (``F.conv2d(feature_pred, kernel, groups=N)``
                                           over all cells of a level and ``F.interpolate(..., mode='bilinear')`` of the whole result) and
                                           ``loss`` :317-320 (``ins_preds_level_img[ins_ind_labels_level_img]``): the rows of the set cells only
    box_solov2_set_cells               the ``cells`` argument from a ``SoloTargets`` of ``box_solov2_targets``, without a host synchronisation
    box_solov2_get_seg_single_kernels  <-> BoxSOLOv2Head.get_seg_single from the mask feature and the kernels: only the candidates' masks exist

There is no CPU or PyTorch fallback: CPU tensors raise.  fp32 only: the reference runs ``feat.float()`` here and no BoxLevelSet config sets
fp16, so half-precision tensors raise.  DEVIATION: the feature is resized once per size group and the product is taken on the resized
feature -- the two act on different axes and commute in real arithmetic, so the results equal the reference's to rounding, not in
operation order.  Nothing of the size (cells of a level) x h x w is ever formed."""
from __future__ import annotations

import types

import torch

from . import _lib
from ._common import cfg_require, current_stream, need_cuda
from .solo_conv import _backward

__all__ = ['box_solov2_ins_preds', 'box_solov2_set_cells', 'box_solov2_get_seg_single_kernels']

HEADER = 'boxinst_hip_dconvl.h'


def _sizes_flat(plan):
    return _lib.int_array([v for hw in plan.sizes for v in hw])


def _call_forward(plan, feat, maps):
    lib = _lib.load()
    dev = feat.device
    B, E, H, W = feat.shape
    out = torch.empty((plan.total,), dtype=torch.float32, device=dev)
    if plan.N == 0:
        return out
    sizes, counts = _sizes_flat(plan), _lib.int_array(plan.counts)
    ws_bytes = lib.bxi_solo_dconvl_forward_workspace_bytes(B, E, H, W, sizes, counts, plan.L)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check_supported('bxi_solo_dconvl_forward_f32', lib.bxi_solo_dconvl_forward_f32(
            feat.data_ptr(), B, E, H, W, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), sizes, plan.L,
            plan.cells.data_ptr(), counts, plan.N, out.data_ptr(), plan.status.data_ptr(), ws.data_ptr(), ws_bytes, current_stream(dev)), HEADER)
    return out


class _InsPreds(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, feat, *maps):
        out = _call_forward(plan, feat, maps)
        ctx.plan = plan
        ctx.save_for_backward(feat, *maps)
        return out

    @staticmethod
    def backward(ctx, g_out):
        plan = ctx.plan
        feat, *maps = ctx.saved_tensors
        B, E, H, W = feat.shape
        sizes, counts = _sizes_flat(plan), _lib.int_array(plan.counts)

        def call(lib, g, g_feat, g_maps, ws, ws_bytes, stream):
            _lib.check_supported('bxi_solo_dconvl_backward_f32', lib.bxi_solo_dconvl_backward_f32(
                feat.data_ptr(), B, E, H, W, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), sizes, plan.L,
                None if plan.cells is None else plan.cells.data_ptr(), counts, plan.N, g, g_feat, g_maps, plan.status.data_ptr(), ws,
                ws_bytes, stream), HEADER)

        return _backward(ctx, g_out, torch.float32, feat, maps,
                         lambda lib: lib.bxi_solo_dconvl_backward_workspace_bytes(B, E, H, W, sizes, counts, plan.L), call)


def _supported(H, W, sizes):
    for l, (oh, ow) in enumerate(sizes):
        for name, n_in, n_out in (('height', H, oh), ('width', W, ow)):
            if n_in > _lib.DCONVL_MAX_DOWN * n_out or n_out > _lib.DCONVL_MAX_UP * n_in:
                raise NotImplementedError(f'level_sizes[{l}] = {(oh, ow)} of a {H} x {W} feature: {name} {n_in} -> {n_out} is outside the '
                                          f'support set of include/boxinst/{HEADER} (in <= {_lib.DCONVL_MAX_DOWN} * out, out <= '
                                          f'{_lib.DCONVL_MAX_UP} * in per axis)')


def _plan(kernel_preds, feature_pred, cells, level_sizes, status):
    maps = list(kernel_preds)
    tensors = dict(feature_pred=feature_pred, **{f'kernel_preds[{l}]': m for l, m in enumerate(maps)})
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise RuntimeError(f'{name} is {t.dtype}: BoxLevelSet masks are fp32 only (include/boxinst/{HEADER}); half precision is not cast here')
    if feature_pred.dim() != 4:
        raise RuntimeError(f'feature_pred must be [B,E,h,w], got {tuple(feature_pred.shape)}')
    B, E, H, W = (int(v) for v in feature_pred.shape)
    L = len(maps)
    if not 1 <= L <= _lib.DCONV_MAX_LEVELS:
        raise RuntimeError(f'{L} levels: 1 .. {_lib.DCONV_MAX_LEVELS} are supported')
    if not 1 <= B <= _lib.BXI_MAX_IMAGES or not 1 <= E <= _lib.DCONV_MAX_E:
        raise RuntimeError(f'B = {B}, E = {E}: 1 .. {_lib.BXI_MAX_IMAGES} images and 1 .. {_lib.DCONV_MAX_E} channels are supported')
    if len(cells) != L or any(len(c) != B for c in cells):
        raise RuntimeError(f'cells must be [level][image] = [{L}][{B}]')
    if len(level_sizes) != L or any(len(hw) != 2 for hw in level_sizes):
        raise RuntimeError(f'level_sizes must be {L} pairs (oh, ow), got {level_sizes!r}')
    sizes = [(int(oh), int(ow)) for oh, ow in level_sizes]
    if any(oh < 1 or ow < 1 for oh, ow in sizes):
        raise RuntimeError(f'level_sizes must be positive, got {sizes!r}')
    for l, m in enumerate(maps):
        if m.dim() != 4 or m.shape[0] != B or m.shape[1] != E or m.shape[2] != m.shape[3] or m.device != feature_pred.device:
            raise RuntimeError(f'kernel_preds[{l}] must be [{B},{E},S,S] on {feature_pred.device}, got {tuple(m.shape)} on {m.device}')
    flat = [cells[l][b] for l in range(L) for b in range(B)]
    for i, c in enumerate(flat):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.int64 or c.dim() != 1:
            raise RuntimeError(f'cells[{i // B}][{i % B}] must be an int64 vector')
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1 or status.device != feature_pred.device):
        raise RuntimeError(f'status must be int32 [1] on {feature_pred.device}')
    _supported(H, W, sizes)
    need_cuda(**tensors, **{f'cells[{i // B}][{i % B}]': c for i, c in enumerate(flat)})               # shapes first: they are said without a device
    counts = [int(c.numel()) for c in flat]
    per_level = [sum(counts[l * B:(l + 1) * B]) for l in range(L)]
    N = sum(counts)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=feature_pred.device)
    return types.SimpleNamespace(grids=[int(m.shape[2]) for m in maps], sizes=sizes, counts=counts, per_level=per_level, N=N, L=L, B=B,
                                 total=sum(n * oh * ow for n, (oh, ow) in zip(per_level, sizes)),
                                 cells=torch.cat(flat).contiguous() if N else None, status=status)


def box_solov2_ins_preds(kernel_preds, feature_pred, cells, level_sizes, status=None):
    """The mask logits of the set cells, as ``BoxSOLOv2Head.loss`` sees ``ins_preds`` after box_solov2_head.py:317-320.

    ``kernel_preds``: the L maps [B,E,S_l,S_l] of ``forward_single``; ``feature_pred`` [B,E,h,w]; ``cells[l][b]``: int64 device vector
    of the set cells of (level, image), ascending (``box_solov2_set_cells``; the sizes are host values); ``level_sizes[l] = (oh_l, ow_l)``,
    the reference's ``2 x featmap_size``.  Returns a list of L fp32 tensors [N_l, oh_l, ow_l] (logits: the sigmoid is the loss's), images
    concatenated in order, [0, oh_l, ow_l] for a level without rows; all are views of one buffer.  Differentiable with respect to every
    ``kernel_preds[l]`` and ``feature_pred`` through one autograd function: every element of every gradient is written, zero for a cell no
    row names.  A cell outside its map gives the row of an all-zero kernel and sets ``status[0]`` (int32 [1] on the device, a fresh zero
    when not given) to 1; nothing reads it back here.  A level size outside the support set of include/boxinst/boxinst_hip_dconvl.h raises
    ``NotImplementedError`` before any launch."""
    plan = _plan(kernel_preds, feature_pred, cells, level_sizes, status)
    out = _InsPreds.apply(plan, feature_pred.contiguous(), *[m.contiguous() for m in kernel_preds])
    res, at = [], 0
    for n, (oh, ow) in zip(plan.per_level, plan.sizes):
        res.append(out[at:at + n * oh * ow].view(n, oh, ow))
        at += n * oh * ow
    return res


def box_solov2_set_cells(targets):
    """``cells[l][b]`` of ``box_solov2_ins_preds`` from the ``SoloTargets`` of ``box_solov2_targets``: the set cells of every (level,
    image) in ascending order, i.e. ``ins_ind_labels_level_img.nonzero()`` with the count taken from ``targets.counts`` (host values since
    the targets' own synchronisation) -- a stable argsort of the cleared cells cut to the known count, so nothing waits for the device."""
    if getattr(targets, 'mode', None) != 'boxlevelset':
        raise RuntimeError(f"box_solov2_set_cells takes the SoloTargets of box_solov2_targets (mode 'boxlevelset'), got "
                           f"{getattr(targets, 'mode', type(targets).__name__)!r}")
    out = []
    for l, S in enumerate(targets.num_grids):
        order = torch.argsort((~targets.ins_ind_labels[l].view(targets.B, S * S)).to(torch.uint8), dim=1, stable=True)
        out.append([order[b, :int(targets.counts[l][b][1])].contiguous() for b in range(targets.B)])
    return out


def box_solov2_get_seg_single_kernels(cate_preds, mask_feat, kernel_preds, featmap_size, img_meta, cfg, seg_num_grids, strides):
    """``BoxSOLOv2Head.get_seg_single`` (box_solov2_head.py:503-590) from the kernels instead of from every cell's mask: ``cate_preds``
    [sum(grid^2), classes], ``mask_feat`` [1,E,h,w] the mask feature, ``kernel_preds`` [sum(grid^2), E] the dynamic kernels cell by cell
    (as ``get_seg`` builds them for DiscoBox).  The candidates' probabilities come from ``solo_candidate_masks(mask_feat, kernel_preds,
    rows)`` -- a row's bits do not depend on the other rows, so the result equals ``box_solov2_get_seg_single`` on the masks of all cells
    bit for bit -- and everything after them is the same tail.  Returns what ``box_solov2_get_seg_single`` returns."""
    from .matrix_nms import _empty_results, _level_strides, _seg_tail
    from .solo_conv import solo_candidate_masks
    if cate_preds.dim() != 2 or kernel_preds.dim() != 2 or len(cate_preds) != len(kernel_preds):
        raise RuntimeError(f'cate_preds must be [cells, classes] and kernel_preds [cells, E], got {tuple(cate_preds.shape)} and '
                           f'{tuple(kernel_preds.shape)}')
    if mask_feat.dim() != 4 or mask_feat.shape[0] != 1 or mask_feat.shape[1] != kernel_preds.shape[1]:
        raise RuntimeError(f'mask_feat must be [1,{int(kernel_preds.shape[1])},h,w], got {tuple(mask_feat.shape)}')
    if len(seg_num_grids) != len(strides) or sum(int(g) ** 2 for g in seg_num_grids) != len(cate_preds):
        raise RuntimeError(f'seg_num_grids {list(seg_num_grids)} / strides {list(strides)} do not describe {len(cate_preds)} cells')
    need_cuda(cate_preds=cate_preds, mask_feat=mask_feat, kernel_preds=kernel_preds)
    inds = cate_preds > cfg_require(cfg, 'score_thr')
    cate_scores = cate_preds[inds]
    if len(cate_scores) == 0:
        return _empty_results(img_meta, cate_scores)
    inds = inds.nonzero()
    cate_labels = inds[:, 1]
    level = _level_strides(cate_scores, cate_labels, seg_num_grids, strides)[inds[:, 0]]
    probs = solo_candidate_masks(mask_feat, kernel_preds, inds[:, 0].contiguous())
    return _seg_tail(probs, cate_labels, cate_scores, level, featmap_size, img_meta, cfg)
