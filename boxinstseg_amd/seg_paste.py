"""The final masks of the two SOLOv2-style heads (``BoxSOLOv2Head``, ``DiscoBoxSOLOv2Head``) and what the detector makes of them
(csrc/seg_paste.hip, include/boxinst/boxinst_hip_seg.h).

    seg_paste            <-> the two ``F.interpolate`` and ``> cfg.mask_thr`` that end get_seg_single (box_solov2_head.py:576-588,
                             discobox_head.py:1641-1655), plus the area and the tight box of every final mask
    solo_get_seg         <-> BoxSOLOv2Head.get_seg (box_solov2_head.py:475-500) / DiscoBoxSOLOv2Head.get_seg (discobox_head.py:1531-1557)
    solo_format_results  <-> SingleStageTSDetector.format_results (single_stage_ts.py:88-103, single_stage_boxseg.py:75-90)

There is no CPU or PyTorch fallback: CPU tensors raise.  The kept candidates are read in place through ``keep_inds`` (no gathered copy, no
fp32 canvas), and the results of one image -- labels, statistics, scores, masks -- live in ONE device buffer, so ``solo_format_results``
brings them to the host in one copy into pinned memory with one synchronisation; the reference synchronises about eight times per mask.
"""
from __future__ import annotations

import torch

from . import _lib
from ._common import cfg_require, current_stream, need_cuda

__all__ = ['seg_paste', 'solo_get_seg', 'solo_format_results']

_HEAD = 32          # bytes per mask in front of the mask bytes: label int64, stats 5 x int32, score fp32


def _block_views(block, n, oh, ow):
    """One uint8 buffer -> (labels int64 [n], stats int32 [n,5], scores fp32 [n], masks uint8 [n,oh,ow]): views, nothing is copied."""
    return (block[:8 * n].view(torch.int64), block[8 * n:28 * n].view(torch.int32).view(n, 5), block[28 * n:32 * n].view(torch.float32),
            block[_HEAD * n:].view(n, oh, ow))


def _paste(seg_preds, keep_inds, featmap_size, img_meta, mask_thr):
    need_cuda(seg_preds=seg_preds, keep_inds=keep_inds)
    if seg_preds.dim() != 3 or seg_preds.dtype != torch.float32:
        raise RuntimeError(f'seg_preds must be fp32 [n_all,h,w], got {seg_preds.dtype} {tuple(seg_preds.shape)}')
    if keep_inds.dim() != 1 or keep_inds.dtype != torch.int64:
        raise RuntimeError(f'keep_inds must be int64 [n], got {keep_inds.dtype} {tuple(keep_inds.shape)}')
    if tuple(featmap_size) != tuple(seg_preds.shape[-2:]):
        raise RuntimeError(f'featmap_size {tuple(featmap_size)} is not the size of seg_preds {tuple(seg_preds.shape[-2:])}')
    meta = dict(img_meta)
    ch, cw = (int(v) for v in meta['img_shape'][:2])
    oh, ow = (int(v) for v in meta['ori_shape'][:2])
    dev = seg_preds.device
    p, keep = seg_preds.detach().contiguous(), keep_inds.contiguous()
    n_all, h, w = p.shape
    n = keep.numel()
    lib = _lib.load()
    block = torch.empty(n * (_HEAD + oh * ow), dtype=torch.uint8, device=dev)
    _, stats, _, masks = _block_views(block, n, oh, ow)
    ws_bytes = lib.bxi_seg_paste_workspace_bytes(n, oh, ow)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_seg_paste_u8', lib.bxi_seg_paste_u8(p.data_ptr(), n_all, h, w, keep.data_ptr(), n, 4 * h, 4 * w, ch, cw, oh, ow,
                                                            float(mask_thr), masks.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes,
                                                            current_stream(dev)))
    return block, masks.view(torch.bool), stats


def seg_paste(seg_preds, keep_inds, featmap_size, img_meta, mask_thr):
    """``F.interpolate(F.interpolate(seg_preds[keep_inds], size=4 * featmap_size, mode='bilinear')[:, :, :h, :w], size=ori_shape[:2],
    mode='bilinear') > mask_thr`` with ``h, w = img_shape[:2]``, in one kernel: ``seg_preds`` [n_all,h,w] fp32 probabilities and
    ``keep_inds`` [n] int64 on the GPU.  Returns ``(masks, stats)``: ``masks`` bool [n, ori_h, ori_w] (a view of the kernel's uint8 bytes)
    and ``stats`` int32 [n,5] = area, x_min, y_min, x_max, y_max of every mask, (0, -1, -1, -1, -1) for an empty one; both stay on the device.
    A ``keep_inds`` entry outside ``[0, n_all)`` gives an all-zero mask.  Mask bits may differ from the torch composition only where the
    resized probability lies within ~1e-6 of ``mask_thr`` (the products of the two stages are regrouped)."""
    _, masks, stats = _paste(seg_preds, keep_inds, featmap_size, img_meta, mask_thr)
    return masks, stats


def paste_results(results, seg_preds, keep_inds, featmap_size, img_meta, mask_thr):
    """``seg_paste`` for ``_seg_tail``: fills ``results.masks`` / ``results.mask_stats`` and puts the labels and scores next to them in the
    same buffer (``results.host_block``), so that ``solo_format_results`` needs one copy."""
    block, masks, stats = _paste(seg_preds, keep_inds, featmap_size, img_meta, mask_thr)
    n = keep_inds.numel()
    labels, _, scores, _ = _block_views(block, n, *masks.shape[-2:])
    labels.copy_(results.labels)
    scores.copy_(results.scores)
    results.masks, results.mask_stats, results.host_block = masks, stats, block
    return results


def solo_get_seg(cate_preds, kernel_preds, seg_pred, img_metas, cfg, seg_num_grids, strides, cate_out_channels, kernel_out_channels=None):
    """``get_seg`` of both heads: the per-image views and the concatenation over the levels, then the matching ``*_get_seg_single``.
    ``cate_preds`` is a list over levels of [B, grid, grid, classes].  With ``kernel_preds`` (a list over levels of [B, C, grid, grid]) and
    ``seg_pred`` the mask feature [B, C, h, w] it is DiscoBoxSOLOv2Head.get_seg (discobox_head.py:1531-1557); with ``kernel_preds=None`` and
    ``seg_pred`` a list over levels of [B, grid^2, h, w] probabilities it is BoxSOLOv2Head.get_seg (box_solov2_head.py:475-500).  Returns
    one results object per image."""
    from .matrix_nms import box_solov2_get_seg_single, discobox_get_seg_single
    num_levels = len(cate_preds)
    out = []
    for img_id in range(len(img_metas)):
        cate = torch.cat([cate_preds[i][img_id].view(-1, cate_out_channels).detach() for i in range(num_levels)], dim=0)
        if kernel_preds is None:
            assert len(seg_pred) == num_levels
            featmap_size = tuple(seg_pred[0].shape[-2:])
            seg = torch.cat([seg_pred[i][img_id].detach() for i in range(num_levels)], dim=0)
            out.append(box_solov2_get_seg_single(cate, seg, featmap_size, img_metas[img_id], cfg, seg_num_grids, strides))
        else:
            if kernel_out_channels is None:
                raise RuntimeError('kernel_out_channels is required with kernel_preds')
            featmap_size = tuple(seg_pred.shape[-2:])
            kernels = torch.cat([kernel_preds[i][img_id].permute(1, 2, 0).reshape(-1, kernel_out_channels).detach() for i in range(num_levels)], dim=0)
            out.append(discobox_get_seg_single(cate, seg_pred[img_id].unsqueeze(0), kernels, featmap_size, img_metas[img_id], cfg, seg_num_grids,
                                               strides))
    return out


def solo_format_results(results, num_classes):
    """``format_results`` of the reference's detectors on a results object of ``*_get_seg_single``: returns ``(bbox_results, (mask_results,
    score_results))`` -- per class, in result order, the masks whose area is non-zero (CPU bool tensors), their scores (CPU 0-d tensors) and
    the float64 rows ``[x_min, y_min, x_max + 1, y_max + 1, score]``; ``np.zeros((0, 5))`` for a class without masks.

    The area and the box come from ``results.mask_stats`` (the kernel that wrote the masks counted them) instead of ``sum`` / ``where`` /
    ``min`` / ``max`` per mask, and labels, statistics, scores and masks reach the host in one copy into pinned memory with one
    synchronisation; the per-class masks are views of that buffer, which they keep alive."""
    import numpy as np
    bbox_results = [[] for _ in range(num_classes)]
    mask_results = [[] for _ in range(num_classes)]
    score_results = [[] for _ in range(num_classes)]
    masks = results.masks
    n = int(masks.shape[0])
    if n:
        need_cuda(masks=masks)
        stats = getattr(results, 'mask_stats', None)
        if stats is None:
            raise RuntimeError('results.mask_stats is missing: solo_format_results reads the area and the box of a mask from the statistics '
                               'of seg_paste (there is no fallback)')
        oh, ow = (int(v) for v in masks.shape[-2:])
        block = getattr(results, 'host_block', None)
        if block is None or block.numel() != n * (_HEAD + oh * ow):
            block = torch.cat([results.labels.to(torch.int64).contiguous().view(torch.uint8), stats.contiguous().view(torch.uint8).view(-1),
                               results.scores.float().contiguous().view(torch.uint8), masks.contiguous().view(torch.uint8).view(-1)])
        host = torch.empty(block.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(block, non_blocking=True)
        torch.cuda.current_stream(block.device).synchronize()
        labels, stats_h, scores, masks_h = _block_views(host, n, oh, ow)
        masks_h = masks_h.view(torch.bool)
        scores_t = scores if results.scores.dtype == torch.float32 else scores.to(results.scores.dtype)
        lab, st, sc = labels.numpy(), stats_h.numpy(), scores.numpy()
        for i in range(n):
            if st[i, 0] > 0:
                c = int(lab[i])
                mask_results[c].append(masks_h[i])
                score_results[c].append(scores_t[i])
                bbox_results[c].append([st[i, 1], st[i, 2], st[i, 3] + 1, st[i, 4] + 1, sc[i]])
    bbox_results = [np.array(b, dtype=np.float64) if len(b) > 0 else np.zeros((0, 5)) for b in bbox_results]
    return bbox_results, (mask_results, score_results)
