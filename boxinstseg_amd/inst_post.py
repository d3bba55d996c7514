"""Box2Mask at test time: everything the reference does after the decoder (csrc/inst_post.hip, include/boxinst/boxinst_hip_inst.h).

    instance_topk            <-> the softmax, label table, ``topk`` and ``is_thing`` filter of MaskFormerFusionHead.instance_postprocess
                                 (maskformer_fusion_head.py:133-151), one launch for the batch
    box2mask_instances       <-> Box2MaskHead.simple_test's F.interpolate (box2mask_head.py:452-457), the crop and the second
                                 F.interpolate of MaskFormerFusionHead.simple_test (:211-221), and the rest of instance_postprocess
                                 (:145-160: ``> 0``, the mask score, ``mask2bbox``, the det score), two launches per image
    MaskFormerFusionHead     <-> mmdet's class of the same name (``panoptic_fusion_head`` of configs/box2mask), instance results only
    box2mask_format_results  <-> MaskFormer.simple_test's formatting (maskformer.py:155-175: ``bbox2result`` and the per-mask ``.cpu()``)

There is no CPU or PyTorch fallback: CPU tensors raise.  The logits of the selected queries are read in place through the query indices
(no gathered copy, no full-size fp32 canvas), and the results of one image -- labels, boxes, statistics, mask scores, count, masks -- live
in ONE device buffer, so ``box2mask_format_results`` brings them to the host in one copy into pinned memory with one synchronisation.
"""
from __future__ import annotations

import types

import torch

from . import _lib
from ._common import cfg_get, current_stream, need_cuda
from .registry import HEADS

__all__ = ['instance_topk', 'box2mask_instances', 'MaskFormerFusionHead', 'box2mask_format_results']

_HEADER = 'boxinst_hip_inst.h'
_ROW = 52           # bytes per detection in front of the mask bytes: label int64, box 5 x fp32, stats 5 x int32, mask score fp32
_TAIL = 4           # bytes behind the rows: count int32 (no padding anywhere: every byte of the buffer is written by every call)


def _block_views(block, n, oh, ow):
    """One uint8 buffer -> (labels int64 [n], bboxes fp32 [n,5], stats int32 [n,5], mask_scores fp32 [n], count int32 [1], masks uint8
    [n,oh,ow]): views, nothing is copied."""
    a, b, c, d = 8 * n, 28 * n, 48 * n, 52 * n
    return (block[:a].view(torch.int64), block[a:b].view(torch.float32).view(n, 5), block[b:c].view(torch.int32).view(n, 5),
            block[c:d].view(torch.float32), block[_ROW * n:_ROW * n + 4].view(torch.int32), block[_ROW * n + _TAIL:].view(n, oh, ow))


def instance_topk(mask_cls, num_things_classes, num_stuff_classes, max_per_image):
    """``F.softmax(mask_cls, dim=-1)[..., :-1]`` -> the ``max_per_image`` largest of the Q x C scores of every image -> the ``is_thing``
    filter, in one launch.  ``mask_cls`` is [B,Q,C+1] or [Q,C+1] fp32 on the GPU with C = things + stuff.  Returns ``(scores fp32 [B,k],
    labels int64 [B,k], query int64 [B,k], count int32 [B])`` (without the batch axis for a 2-d input); everything stays on the device.
    The order is defined: descending score, equal scores by ascending ``q * C + c``, NaN last; rows at and behind ``count`` hold score 0,
    label -1, query -1."""
    need_cuda(mask_cls=mask_cls)
    if mask_cls.dim() not in (2, 3) or mask_cls.dtype != torch.float32:
        raise RuntimeError(f'mask_cls must be fp32 [B,Q,C+1] or [Q,C+1], got {mask_cls.dtype} {tuple(mask_cls.shape)}')
    things, stuff, k = int(num_things_classes), int(num_stuff_classes), int(max_per_image)
    batched = mask_cls.dim() == 3
    x = (mask_cls if batched else mask_cls.unsqueeze(0)).detach().contiguous()
    B, Q, C1 = x.shape
    if C1 != things + stuff + 1:
        raise RuntimeError(f'mask_cls has {C1} columns, expected num_things_classes + num_stuff_classes + 1 = {things + stuff + 1}')
    dev = x.device
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    query = torch.empty((B, k), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check_supported('bxi_inst_topk_f32', lib.bxi_inst_topk_f32(x.data_ptr(), B, Q, C1 - 1, things, k, scores.data_ptr(), labels.data_ptr(),
                                                                       query.data_ptr(), count.data_ptr(), current_stream(dev)), _HEADER)
    if not batched:
        return scores[0], labels[0], query[0], count[0]
    return scores, labels, query, count


def _paste_image(logits, query, cls_scores, labels, count, up, crop, out):
    """One image: [n_all,h,w] logits, [n] query / cls_scores / labels, 0-d count -> its results object."""
    dev = logits.device
    n_all, h, w = logits.shape
    n = query.numel()
    oh, ow = out
    lib = _lib.load()
    block = torch.empty(n * (_ROW + oh * ow) + _TAIL, dtype=torch.uint8, device=dev)
    lab, boxes, stats, mscores, cnt, masks = _block_views(block, n, oh, ow)
    ws_bytes = lib.bxi_inst_paste_workspace_bytes(n, oh, ow)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check_supported('bxi_inst_paste_u8', lib.bxi_inst_paste_u8(
            logits.data_ptr(), n_all, h, w, query.data_ptr(), cls_scores.data_ptr(), n, up[0], up[1], crop[0], crop[1], oh, ow, masks.data_ptr(),
            stats.data_ptr(), mscores.data_ptr(), boxes.data_ptr(), ws.data_ptr(), ws_bytes, current_stream(dev)), _HEADER)
    lab.copy_(labels)
    cnt.copy_(count.reshape(1))
    return types.SimpleNamespace(labels=lab, bboxes=boxes, masks=masks.view(torch.bool), mask_stats=stats, mask_scores=mscores, count=cnt[0],
                                 scores=cls_scores, query=query, host_block=block)


def box2mask_instances(mask_cls_results, mask_pred_results, img_metas, test_cfg, num_things_classes, num_stuff_classes, rescale=False):
    """The instance results of a batch: ``mask_cls_results`` [B,Q,C+1] and ``mask_pred_results`` [B,Q,h,w], fp32 on the GPU, the last
    decoder layer's outputs.  ``mask_pred_results`` may be the raw prediction -- stage 1 then resizes it to
    ``img_metas[0]['batch_input_shape']`` as Box2MaskHead.simple_test does -- or already at that size (stage 1 is the identity).  Every
    image is cropped to its ``img_shape`` and, with ``rescale``, resized to its ``ori_shape``.

    Returns one results object per image with ``labels`` int64 [k], ``bboxes`` fp32 [k,5] (x_min, y_min, x_max + 1, y_max + 1, class score
    x mask score; zeros for an empty mask), ``masks`` bool [k,H,W] (a view of the kernel's bytes), ``mask_stats`` int32 [k,5] (area, x_min,
    y_min, x_max, y_max; -1 for an empty mask), ``mask_scores`` fp32 [k], ``count`` (0-d int32, on the device: the rows in front of it are
    the detections, the rows behind it have label -1, a zero box and an empty mask; with ``num_stuff_classes == 0`` it equals k) and
    ``host_block``, the one device buffer that holds all of it.  k = ``test_cfg.max_per_image``.  Nothing synchronises."""
    need_cuda(mask_cls_results=mask_cls_results, mask_pred_results=mask_pred_results)
    if mask_cls_results.dim() != 3 or mask_cls_results.dtype != torch.float32:
        raise RuntimeError(f'mask_cls_results must be fp32 [B,Q,C+1], got {mask_cls_results.dtype} {tuple(mask_cls_results.shape)}')
    if mask_pred_results.dim() != 4 or mask_pred_results.dtype != torch.float32:
        raise RuntimeError(f'mask_pred_results must be fp32 [B,Q,h,w], got {mask_pred_results.dtype} {tuple(mask_pred_results.shape)}')
    B, Q = mask_cls_results.shape[:2]
    if tuple(mask_pred_results.shape[:2]) != (B, Q) or len(img_metas) != B:
        raise RuntimeError(f'mask_pred_results {tuple(mask_pred_results.shape)} and {len(img_metas)} img_metas do not belong to mask_cls_results '
                           f'{tuple(mask_cls_results.shape)}')
    if B == 0:
        return []
    k = int(cfg_get(test_cfg, 'max_per_image', 100))
    scores, labels, query, count = instance_topk(mask_cls_results, num_things_classes, num_stuff_classes, k)
    pred = mask_pred_results.detach().contiguous()
    up = tuple(int(v) for v in dict(img_metas[0])['batch_input_shape'][:2])
    results = []
    for b in range(B):
        meta = dict(img_metas[b])
        crop = tuple(int(v) for v in meta['img_shape'][:2])
        if crop[0] > up[0] or crop[1] > up[1]:
            raise RuntimeError(f'img_shape {crop} of image {b} is larger than batch_input_shape {up}')
        out = tuple(int(v) for v in meta['ori_shape'][:2]) if rescale else crop
        results.append(_paste_image(pred[b], query[b], scores[b], labels[b], count[b], up, crop, out))
    return results


@HEADS.register_module()
class MaskFormerFusionHead:
    """mmdet's MaskFormerFusionHead for instance results (every configs/box2mask file: ``panoptic_on=False``, ``instance_on=True``,
    ``num_stuff_classes=0``): built from the ``panoptic_fusion_head`` block plus ``test_cfg`` as the detector passes them.
    ``panoptic_on`` or ``semantic_on`` raise NotImplementedError when ``simple_test`` is called."""

    def __init__(self, num_things_classes=80, num_stuff_classes=53, test_cfg=None, loss_panoptic=None, init_cfg=None, **kwargs):
        if loss_panoptic is not None:
            raise NotImplementedError('MaskFormerFusionHead.loss_panoptic is not supported')
        self.num_things_classes, self.num_stuff_classes = int(num_things_classes), int(num_stuff_classes)
        self.num_classes = self.num_things_classes + self.num_stuff_classes
        self.test_cfg = test_cfg if test_cfg is not None else {}
        self.init_cfg = init_cfg

    def forward_train(self, **kwargs):
        """MaskFormerFusionHead has no training loss."""
        return dict()

    def instance_results(self, mask_cls_results, mask_pred_results, img_metas, rescale=False):
        """``box2mask_instances`` with the head's classes and ``test_cfg``: the results objects ``box2mask_format_results`` takes."""
        return box2mask_instances(mask_cls_results, mask_pred_results, img_metas, self.test_cfg, self.num_things_classes, self.num_stuff_classes,
                                  rescale)

    def simple_test(self, mask_cls_results, mask_pred_results, img_metas, rescale=False, **kwargs):
        """-> ``[{'ins_results': (labels, bboxes, masks)}]`` per image, on the device.  With ``num_stuff_classes == 0`` every selected entry
        is a thing and nothing synchronises; otherwise the rows are cut at the image's count, which costs one synchronisation per image."""
        if cfg_get(self.test_cfg, 'panoptic_on', True):
            raise NotImplementedError('MaskFormerFusionHead: panoptic_on=True (panoptic_postprocess) is not supported')
        if cfg_get(self.test_cfg, 'semantic_on', False):
            raise NotImplementedError('MaskFormerFusionHead: semantic_on=True is not supported (nor by the reference)')
        if not cfg_get(self.test_cfg, 'instance_on', False):
            return [dict() for _ in img_metas]
        out = []
        for r in self.instance_results(mask_cls_results, mask_pred_results, img_metas, rescale):
            n = r.labels.numel() if self.num_stuff_classes == 0 else int(r.count)
            out.append({'ins_results': (r.labels[:n], r.bboxes[:n], r.masks[:n])})
        return out


def box2mask_format_results(results, num_things_classes):
    """MaskFormer.simple_test's formatting of one image's results object (of ``box2mask_instances``): returns ``(bbox_results,
    mask_results)`` -- per class, in result order, the float32 rows [x1, y1, x2, y2, score] as ``bbox2result`` gives them (``np.zeros((0,
    5), float32)`` for a class without detections) and the masks as numpy bool arrays.  All ``count`` detections are kept, empty masks
    included, as the reference does.  One copy into pinned memory and one synchronisation; the arrays are views of that buffer."""
    import numpy as np
    masks = results.masks
    need_cuda(masks=masks)
    n = int(masks.shape[0])
    oh, ow = (int(v) for v in masks.shape[-2:])
    block = getattr(results, 'host_block', None)
    if block is None or block.numel() != n * (_ROW + oh * ow) + _TAIL:
        raise RuntimeError('results.host_block is missing or not the buffer of these masks: box2mask_format_results copies the one buffer '
                           'box2mask_instances filled (there is no fallback)')
    host = torch.empty(block.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(block, non_blocking=True)
    torch.cuda.current_stream(block.device).synchronize()
    labels, boxes, _, _, count, masks_h = _block_views(host, n, oh, ow)
    lab, bx, mk = labels.numpy(), boxes.numpy(), masks_h.numpy().view(np.bool_)
    cnt = int(count.numpy()[0])
    things = int(num_things_classes)
    lab = lab[:cnt]
    bbox_results = [bx[:cnt][lab == c, :] for c in range(things)]
    mask_results = [[] for _ in range(things)]
    for j in range(cnt):
        mask_results[int(lab[j])].append(mk[j])
    return bbox_results, mask_results
