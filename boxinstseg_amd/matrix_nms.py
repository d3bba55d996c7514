"""Test-time end of the two SOLOv2-style heads (BoxLevelSet's ``BoxSOLOv2Head`` and ``DiscoBoxSOLOv2Head``): mask thresholding,
area, mask scoring and Matrix NMS on bit-packed masks (csrc/matrix_nms.hip, include/boxinst/boxinst_hip_post.h).

    mask_matrix_nms            <-> mmdet.core.post_processing.matrix_nms.mask_matrix_nms (matrix_nms.py:5-121)
    seg_nms                    <-> the block box_solov2_head.py:546-574 / discobox_head.py:1610-1639, fused
    box_solov2_get_seg_single  <-> BoxSOLOv2Head.get_seg_single (box_solov2_head.py:503-590)
    discobox_get_seg_single    <-> DiscoBoxSOLOv2Head.get_seg_single (discobox_head.py:1560-1660)

There is no CPU or PyTorch fallback: CPU tensors raise.  What stays in torch is what has data-dependent sizes in the reference
too (``nonzero``, the sorts, ``filter_thr`` / ``max_num``).  The resizes and the final threshold of the kept masks are one more kernel
(seg_paste.py, csrc/seg_paste.hip).
"""
from __future__ import annotations

import types

import torch
import torch.nn.functional as F

from . import _lib
from ._common import cfg_require, current_stream, need_cuda
from .seg_paste import paste_results

__all__ = ['mask_matrix_nms', 'seg_nms', 'pack_probs', 'pack_masks', 'matrix_nms_decay', 'matrix_nms_scores',
           'box_solov2_get_seg_single', 'discobox_get_seg_single']


def _words(h: int, w: int) -> int:
    return (h * w + 63) // 64


def pack_probs(seg_preds: torch.Tensor, mask_thr: float):
    """``seg_preds`` [n,h,w] fp32 -> (bits [n, ceil(hw/64)] int64, area [n] int32, psum [n] fp32): ``seg_preds > mask_thr`` as bits,
    its pixel count, and the sum of the probabilities over the set pixels -- one pass, no boolean or fp32 mask tensor."""
    need_cuda(seg_preds=seg_preds)
    if seg_preds.dim() != 3 or seg_preds.dtype != torch.float32:
        raise RuntimeError(f'seg_preds must be fp32 [n,h,w], got {seg_preds.dtype} {tuple(seg_preds.shape)}')
    dev = seg_preds.device
    p = seg_preds.detach().contiguous()
    n, h, w = p.shape
    bits = torch.empty((n, _words(h, w)), dtype=torch.int64, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    psum = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_mask_pack_f32', _lib.load().bxi_mask_pack_f32(p.data_ptr(), n, h, w, float(mask_thr), bits.data_ptr(),
                                                                      area.data_ptr(), psum.data_ptr(), current_stream(dev)))
    return bits, area, psum


def pack_masks(masks: torch.Tensor):
    """``masks`` [n,h,w] bool / uint8 (non-zero = set) -> (bits, area)."""
    need_cuda(masks=masks)
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f'masks must be bool or uint8 [n,h,w], got {masks.dtype} {tuple(masks.shape)}')
    dev = masks.device
    m = masks.detach().contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    n, h, w = m.shape
    bits = torch.empty((n, _words(h, w)), dtype=torch.int64, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_mask_pack_u8', _lib.load().bxi_mask_pack_u8(m.data_ptr(), n, h, w, bits.data_ptr(), area.data_ptr(), current_stream(dev)))
    return bits, area


def _kernel_id(kernel) -> int:
    if kernel not in _lib.NMS_KERNELS:
        raise NotImplementedError(f'{kernel} kernel is not supported in matrix nms!')
    return _lib.NMS_KERNELS[kernel]


def matrix_nms_decay(bits, area, labels, order, scores_sorted, hw, kernel='gaussian', sigma=2.0):
    """The kernels of matrix_nms.py:60-99 on packed masks: ``order`` [n] indexes the candidates of ``bits`` / ``area`` / ``labels``
    by descending score, ``scores_sorted`` [n] are their scores, ``hw`` = (h, w).  Returns (decayed [n], decay_iou [n,n],
    compensate [n]); ``compensate`` is a view of the call's workspace."""
    need_cuda(bits=bits, area=area, labels=labels, order=order, scores_sorted=scores_sorted)
    kid = _kernel_id(kernel)
    dev = bits.device
    n_all, n = bits.size(0), order.numel()
    h, w = int(hw[0]), int(hw[1])
    if bits.dim() != 2 or bits.dtype != torch.int64 or bits.size(1) != _words(h, w) or not bits.is_contiguous():
        raise RuntimeError(f'bits must be contiguous int64 [n_all, {_words(h, w)}] for {h}x{w} masks, got {bits.dtype} {tuple(bits.shape)}')
    if area.numel() != n_all or labels.numel() != n_all or scores_sorted.numel() != n:
        raise RuntimeError(f'area / labels must have {n_all} entries and scores_sorted {n}')
    if n > _lib.NMS_MAX_CANDIDATES:              # said here, before the n x n allocation; the entry point refuses the same with BXI_ERR_UNSUPPORTED
        raise NotImplementedError(f'{n} candidates would enter the n x n stage of Matrix NMS: at most BXI_NMS_MAX_CANDIDATES = '
                                  f'{_lib.NMS_MAX_CANDIDATES} are supported (include/boxinst/boxinst_hip_post.h); cut them with '
                                  f'nms_pre <= {_lib.NMS_MAX_CANDIDATES}')
    area = area.to(torch.int32).contiguous()
    labels = labels.to(torch.int64).contiguous()
    order = order.to(torch.int64).contiguous()
    scores_sorted = scores_sorted.to(torch.float32).contiguous()
    lib = _lib.load()
    ws_bytes = lib.bxi_matrix_nms_workspace_bytes(n)
    decayed = torch.empty(n, dtype=torch.float32, device=dev)
    decay_iou = torch.empty((n, n), dtype=torch.float32, device=dev)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_matrix_nms_f32', lib.bxi_matrix_nms_f32(
            bits.data_ptr(), area.data_ptr(), labels.data_ptr(), order.data_ptr(), scores_sorted.data_ptr(), n_all, n, h, w, kid,
            float(sigma), decayed.data_ptr(), decay_iou.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))
    return decayed, decay_iou, ws[:n]


def matrix_nms_scores(bits, area, labels, scores, hw, nms_pre=-1, kernel='gaussian', sigma=2.0):
    """Sort, cut to ``nms_pre`` and decay (matrix_nms.py:53-99) with no data-dependent size, so it can be captured in a graph:
    returns (decayed [n], order [n]) with n = min(len(scores), nms_pre)."""
    sorted_scores, order = torch.sort(scores, descending=True, stable=True)
    if nms_pre > 0 and order.numel() > nms_pre:
        order, sorted_scores = order[:nms_pre], sorted_scores[:nms_pre]
    decayed, _, _ = matrix_nms_decay(bits, area, labels, order, sorted_scores, hw, kernel, sigma)
    return decayed, order


def _finish(decayed, order, filter_thr, max_num):
    """matrix_nms.py:101-117: ``filter_thr``, the second sort and ``max_num``.  None when nothing survives."""
    keep_inds = order
    if filter_thr > 0:
        keep = decayed >= filter_thr
        keep_inds = keep_inds[keep]
        if keep_inds.numel() == 0:
            return None
        decayed = decayed[keep]
    scores, sort_inds = torch.sort(decayed, descending=True, stable=True)
    keep_inds = keep_inds[sort_inds]
    if max_num > 0 and keep_inds.numel() > max_num:
        keep_inds, scores = keep_inds[:max_num], scores[:max_num]
    return scores, keep_inds


def mask_matrix_nms(masks, labels, scores, filter_thr=-1, nms_pre=-1, max_num=-1, kernel='gaussian', sigma=2.0, mask_area=None):
    """Matrix NMS for multi-class masks: the signature and the results ``(scores, labels, masks, keep_inds)`` of the reference's
    ``mask_matrix_nms`` (matrix_nms.py:5-121).  ``masks`` [n,h,w] bool / uint8, ``labels`` [n], ``scores`` [n], on the GPU.

    The masks are packed to bits once, intersections are popcounts (the integers the reference's fp32 matrix product computes) and
    the n x n stage is two launches.  Both sorts are ``torch.sort(descending=True, stable=True)``: among equal scores the lower
    index goes first, which is one of the orders the reference's unstable sort may produce.  At most 2048 candidates enter the
    n x n stage (after ``nms_pre``)."""
    _kernel_id(kernel)
    need_cuda(masks=masks, labels=labels, scores=scores, mask_area=mask_area)
    assert len(labels) == len(masks) == len(scores)
    if len(labels) == 0:
        return scores.new_zeros(0), labels.new_zeros(0), masks.new_zeros(0, *masks.shape[-2:]), labels.new_zeros(0)
    bits, area = pack_masks(masks)
    if mask_area is not None:
        assert len(masks) == len(mask_area)
        area = mask_area.to(torch.int32)
    decayed, order = matrix_nms_scores(bits, area, labels, scores.to(torch.float32), masks.shape[-2:], nms_pre, kernel, sigma)
    done = _finish(decayed, order, filter_thr, max_num)
    if done is None:
        return scores.new_zeros(0), labels.new_zeros(0), masks.new_zeros(0, *masks.shape[-2:]), labels.new_zeros(0)
    out_scores, keep_inds = done
    return out_scores.to(scores.dtype), labels[keep_inds], masks[keep_inds], keep_inds


def seg_nms(seg_preds, cate_labels, cate_scores, strides, cfg):
    """The block ``seg_masks = seg_preds > cfg.mask_thr`` ... ``mask_matrix_nms(...)`` of the SOLOv2-style heads
    (box_solov2_head.py:546-574), fused: threshold, bits, area and the mask-score numerator in one pass over ``seg_preds`` [n,h,w];
    ``sum_masks > strides``; ``cate_scores * psum / area``; Matrix NMS through the surviving rows.  Returns
    ``(scores, labels, keep_inds)`` with ``keep_inds`` indexing the n input candidates; empty tensors when nothing survives.
    ``cfg`` holds mask_thr, filter_thr, nms_pre, max_per_img, kernel, sigma (attributes or keys)."""
    kernel, sigma = cfg_require(cfg, 'kernel'), cfg_require(cfg, 'sigma')
    _kernel_id(kernel)
    need_cuda(seg_preds=seg_preds, cate_labels=cate_labels, cate_scores=cate_scores, strides=strides)
    n = seg_preds.size(0)
    assert len(cate_labels) == len(cate_scores) == len(strides) == n
    empty = (cate_scores.new_zeros(0), cate_labels.new_zeros(0), cate_labels.new_zeros(0))
    if n == 0:
        return empty
    bits, area, psum = pack_probs(seg_preds, cfg_require(cfg, 'mask_thr'))
    sum_masks = area.float()
    kept = (sum_masks > strides).nonzero(as_tuple=True)[0]
    if kept.numel() == 0:
        return empty
    scores = cate_scores[kept].float() * (psum[kept] / sum_masks[kept])
    sorted_scores, sort_inds = torch.sort(scores, descending=True, stable=True)
    nms_pre = cfg_require(cfg, 'nms_pre')
    if nms_pre > 0 and sort_inds.numel() > nms_pre:
        sort_inds, sorted_scores = sort_inds[:nms_pre], sorted_scores[:nms_pre]
    order = kept[sort_inds]
    decayed, _, _ = matrix_nms_decay(bits, area, cate_labels, order, sorted_scores, seg_preds.shape[-2:], kernel, sigma)
    done = _finish(decayed, order, cfg_require(cfg, 'filter_thr'), cfg_require(cfg, 'max_per_img'))
    if done is None:
        return empty
    out_scores, keep_inds = done
    return out_scores.to(cate_scores.dtype), cate_labels[keep_inds], keep_inds


def _level_strides(cate_scores, cate_labels, seg_num_grids, strides):
    """box_solov2_head.py:537-542: the stride of the FPN level of every grid cell."""
    size_trans = cate_labels.new_tensor(seg_num_grids).pow(2).cumsum(0)
    out = cate_scores.new_ones(int(size_trans[-1]))
    out[:size_trans[0]] *= strides[0]
    for k in range(1, len(seg_num_grids)):
        out[size_trans[k - 1]:size_trans[k]] *= strides[k]
    return out


def _results(img_meta, scores, labels, masks):
    meta = dict(img_meta)
    return types.SimpleNamespace(scores=scores, labels=labels, masks=masks, img_shape=meta['img_shape'], ori_shape=meta['ori_shape'],
                                 mask_stats=None)


def _empty_results(img_meta, cls_scores):
    ori = dict(img_meta)['ori_shape']
    r = _results(img_meta, cls_scores.new_ones(0), cls_scores.new_ones(0), cls_scores.new_zeros(0, *ori[:2]))
    r.mask_stats = cls_scores.new_zeros((0, 5), dtype=torch.int32)
    return r


def _seg_tail(seg_preds, cate_labels, cate_scores, strides, featmap_size, img_meta, cfg):
    """box_solov2_head.py:546-590 from the candidates' probabilities on: the block through ``seg_nms``, then the two bilinear resizes
    and the final threshold of the kept masks in one kernel (``seg_paste``), which also leaves the area and the box of every mask in
    ``mask_stats``."""
    scores, labels, keep_inds = seg_nms(seg_preds, cate_labels, cate_scores, strides, cfg)
    if keep_inds.numel() == 0:
        return _empty_results(img_meta, cate_scores)
    return paste_results(_results(img_meta, scores, labels, None), seg_preds, keep_inds, featmap_size, img_meta, cfg_require(cfg, 'mask_thr'))


def box_solov2_get_seg_single(cate_preds, seg_preds, featmap_size, img_meta, cfg, seg_num_grids, strides):
    """``BoxSOLOv2Head.get_seg_single`` (box_solov2_head.py:503-590).  ``cate_preds`` [sum(grid^2), classes], ``seg_preds``
    [sum(grid^2), h, w] probabilities, ``seg_num_grids`` / ``strides`` the head's per-level settings.  Returns an object with
    ``scores``, ``labels``, ``masks`` (bool [n, ori_h, ori_w]), ``mask_stats`` (int32 [n,5]: area and box of every mask, see ``seg_paste``)
    and the image's ``img_shape`` / ``ori_shape``."""
    need_cuda(cate_preds=cate_preds, seg_preds=seg_preds)
    assert len(cate_preds) == len(seg_preds)
    inds = cate_preds > cfg_require(cfg, 'score_thr')
    cate_scores = cate_preds[inds]
    if len(cate_scores) == 0:
        return _empty_results(img_meta, cate_scores)
    inds = inds.nonzero()
    cate_labels = inds[:, 1]
    level = _level_strides(cate_scores, cate_labels, seg_num_grids, strides)[inds[:, 0]]
    return _seg_tail(seg_preds[inds[:, 0]].float(), cate_labels, cate_scores, level, featmap_size, img_meta, cfg)


def discobox_get_seg_single(cate_preds, seg_preds, kernel_preds, featmap_size, img_meta, cfg, seg_num_grids, strides, conv='torch'):
    """``DiscoBoxSOLOv2Head.get_seg_single`` (discobox_head.py:1560-1660).  ``seg_preds`` [1, C, h, w] is the mask feature and
    ``kernel_preds`` [sum(grid^2), C] the dynamic 1x1 kernels; with ``conv='torch'`` the convolution and the sigmoid run in torch in the
    tensors' own precision (the reference runs this method under autocast), with ``conv='hip'`` in ``solo_candidate_masks`` (fp32, the
    candidates' kernel rows read in place), with ``conv='hip_half'`` in ``solo_candidate_masks(compute='half', out_dtype=torch.float32)``
    on fp16 or bf16 ``seg_preds`` / ``kernel_preds`` (read in place, fp32 accumulation, fp32 probabilities); the block after them through
    ``seg_nms`` in fp32."""
    need_cuda(cate_preds=cate_preds, seg_preds=seg_preds, kernel_preds=kernel_preds)
    assert len(cate_preds) == len(kernel_preds)
    if conv not in ('torch', 'hip', 'hip_half'):
        raise ValueError(f"conv must be 'torch', 'hip' or 'hip_half', got {conv!r}")
    inds = cate_preds > cfg_require(cfg, 'score_thr')
    cate_scores = cate_preds[inds]
    if len(cate_scores) == 0:
        return _empty_results(img_meta, cate_scores)
    inds = inds.nonzero()
    cate_labels = inds[:, 1]
    if conv != 'torch':
        from .solo_conv import solo_candidate_masks
        level = _level_strides(kernel_preds, cate_labels, seg_num_grids, strides)[inds[:, 0]]
        half = dict(compute='half', out_dtype=torch.float32) if conv == 'hip_half' else {}
        probs = solo_candidate_masks(seg_preds, kernel_preds, inds[:, 0], **half)
        return _seg_tail(probs, cate_labels, cate_scores, level.float(), featmap_size, img_meta, cfg)
    kernel_preds = kernel_preds[inds[:, 0]]
    level = _level_strides(kernel_preds, cate_labels, seg_num_grids, strides)[inds[:, 0]]
    I, N = kernel_preds.shape
    probs = F.conv2d(seg_preds, kernel_preds.view(I, N, 1, 1), stride=1).squeeze(0).sigmoid()
    return _seg_tail(probs.float(), cate_labels, cate_scores, level.float(), featmap_size, img_meta, cfg)
