"""CondInst's test-time detections on the GPU: the decode of the box head, the score filter and greedy box NMS
(csrc/box_nms.hip, include/boxinst/boxinst_hip_det.h).

    nms, batched_nms      <-> mmcv.ops.nms.nms / batched_nms (restated, unpinned: mmcv's source is not part of the reference)
    nms_with_others       <-> mmdet.models.dense_heads.condinst_head.nms_with_others (condinst_head.py:18-83)
    condinst_get_bboxes   <-> CondInstBoxHead.get_bboxes / _get_bboxes (condinst_head.py:640-853), the whole batch at once

The reference runs per level (permute, sigmoid, a [B,HW,C] product, max, topk, five gathers), then per image (nonzero, the class
offset copy, an NMS whose greedy scan mmcv runs after a device-to-host copy).  Here the location scores of all levels and images
are one launch, the per-level top-k stays ``torch.topk`` on slices of that buffer, the decode / filter of all images is two
launches that write the candidates in the reference's ``nonzero`` order together with their count ON THE DEVICE, the NMS of all
images is one workgroup per image, and the kept detections' params / points / level indices are fetched straight from the NCHW
maps.  One host synchronisation at the very end reads the counts.

Two deviations from mmcv, see the header: the IoU test is ``inter > thr * (Sa + Sb - inter)`` in fp32, and classes are kept apart
by comparing labels instead of adding ``label * (max coordinate + 1)`` to the boxes.  Ties between equal scores are resolved by
ascending index (mmcv and torch's device sort leave them open).

There is no CPU or PyTorch fallback: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _lib
from ._common import cfg_get, current_stream, need_cuda, ptr

__all__ = ['nms', 'batched_nms', 'nms_with_others', 'condinst_get_bboxes', 'location_scores', 'det_candidates', 'box_nms', 'det_gather',
           'SORT_MAX', 'NMS_ROUND', 'KEEP_TILE']

SORT_MAX, NMS_ROUND, KEEP_TILE = _lib.DET_SORT_MAX, _lib.DET_NMS_ROUND, _lib.DET_KEEP_TILE


def parse_test_cfg(cfg):
    """``test_cfg`` (dict or namespace) -> dict(nms_pre, score_thr, iou_threshold, max_per_img, class_agnostic, nms_max_num)."""
    nms_cfg = cfg_get(cfg, 'nms')
    if nms_cfg is None:
        raise TypeError('test_cfg has no `nms` entry')
    kind = cfg_get(nms_cfg, 'type', 'nms')
    if kind != 'nms':
        raise NotImplementedError(f"nms type {kind!r} is not supported: only dict(type='nms', iou_threshold=...)")
    score_thr = cfg_get(cfg, 'score_thr')
    if score_thr is None:
        raise TypeError('test_cfg has no `score_thr`')
    max_per_img = cfg_get(cfg, 'max_per_img', -1)
    return dict(nms_pre=int(cfg_get(cfg, 'nms_pre', -1)), score_thr=float(score_thr), iou_threshold=float(cfg_get(nms_cfg, 'iou_threshold')),
                max_per_img=int(-1 if max_per_img is None else max_per_img), class_agnostic=bool(cfg_get(nms_cfg, 'class_agnostic', False)),
                nms_max_num=int(cfg_get(nms_cfg, 'max_num', -1)))


# ---- the four entry points ------------------------------------------------------------------------------------------------
class _Levels:
    """The NCHW maps of the FPN levels as the array of ``bxi_det_level`` the entry points take (keeps the tensors alive)."""

    def __init__(self, cls_scores, bbox_preds, centernesses, param_preds, strides):
        n = len(cls_scores)
        if not (1 <= n <= _lib.DET_MAX_LEVELS) or len(bbox_preds) != n or len(centernesses) != n or len(strides) != n or \
                (param_preds is not None and len(param_preds) != n):
            raise RuntimeError(f'1..{_lib.DET_MAX_LEVELS} levels with cls, bbox, centerness (and params) and a stride each, got {n}')
        need_cuda(**{f'cls_scores[{i}]': t for i, t in enumerate(cls_scores)}, **{f'bbox_preds[{i}]': t for i, t in enumerate(bbox_preds)},
                   **{f'centernesses[{i}]': t for i, t in enumerate(centernesses)},
                   **({} if param_preds is None else {f'param_preds[{i}]': t for i, t in enumerate(param_preds)}))
        f = lambda t: t.detach().to(torch.float32).contiguous()            # noqa: E731
        self.cls, self.bbox, self.ctr = [f(t) for t in cls_scores], [f(t) for t in bbox_preds], [f(t) for t in centernesses]
        self.params = None if param_preds is None else [f(t) for t in param_preds]
        self.B, self.C = int(self.cls[0].shape[0]), int(self.cls[0].shape[1])
        self.P = 0 if self.params is None else int(self.params[0].shape[1])
        self.dev = self.cls[0].device
        self.sizes, self.strides = [], []
        arr = (_lib.DetLevel * n)()
        for i in range(n):
            H, W = int(self.cls[i].shape[2]), int(self.cls[i].shape[3])
            s = strides[i][0] if isinstance(strides[i], (tuple, list)) else strides[i]
            if tuple(self.cls[i].shape) != (self.B, self.C, H, W) or tuple(self.bbox[i].shape) != (self.B, 4, H, W) or \
                    tuple(self.ctr[i].shape) != (self.B, 1, H, W) or (self.params is not None and tuple(self.params[i].shape) != (self.B, self.P, H, W)):
                raise RuntimeError(f'level {i}: cls {tuple(self.cls[i].shape)}, bbox {tuple(self.bbox[i].shape)}, centerness '
                                   f'{tuple(self.ctr[i].shape)} do not describe one [B,*,H,W] level')
            arr[i] = _lib.DetLevel(self.cls[i].data_ptr(), self.bbox[i].data_ptr(), self.ctr[i].data_ptr(),
                                   None if self.params is None else self.params[i].data_ptr(), H, W, int(s))
            self.sizes.append(H * W)
            self.strides.append(int(s))
        self.arr, self.n, self.M_all = arr, n, sum(self.sizes)


def location_scores(levels: _Levels) -> torch.Tensor:
    """[B, M_all] fp32: ``sigmoid(max_c cls) * sigmoid(centerness)`` of every location, levels concatenated (condinst_head.py:781)."""
    out = torch.empty((levels.B, levels.M_all), dtype=torch.float32, device=levels.dev)
    with torch.cuda.device(levels.dev):
        _lib.check('bxi_det_location_score_f32', _lib.load().bxi_det_location_score_f32(
            levels.arr, levels.n, levels.B, levels.C, out.data_ptr(), current_stream(levels.dev)))
    return out


def det_candidates(levels: _Levels, sel, img_dims, rescale, score_thr, cap, fill_scores=None):
    """Decode and filter (condinst_head.py:796-823, :25-62).  ``sel`` [B,M] int64 or None, ``img_dims`` B rows of (clamp_h, clamp_w,
    four scale factors).  Returns (cand_boxes [B,cap,4], cand_scores [B,cap], cand_labels [B,cap], cand_pos [B,cap], count [B]); rows
    from ``count[b]`` on are not written (``fill_scores``: what cand_scores holds there)."""
    B, dev = levels.B, levels.dev
    M = levels.M_all if sel is None else int(sel.shape[1])
    if sel is not None:
        need_cuda(sel=sel)
        if sel.dtype != torch.int64 or tuple(sel.shape) != (B, M) or not sel.is_contiguous():
            raise RuntimeError(f'sel must be contiguous int64 [{B}, M], got {sel.dtype} {tuple(sel.shape)}')
    rows = max(cap, 1)
    boxes = torch.empty((B, rows, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, rows), dtype=torch.float32, device=dev) if fill_scores is None else \
        torch.full((B, rows), fill_scores, dtype=torch.float32, device=dev)
    labels = torch.empty((B, rows), dtype=torch.int64, device=dev)
    pos = torch.empty((B, rows), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = lib.bxi_det_candidates_workspace_bytes(B, M)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
    dims = _lib.float_array([v for row in img_dims for v in row])
    with torch.cuda.device(dev):
        _lib.check('bxi_det_candidates_f32', lib.bxi_det_candidates_f32(
            levels.arr, levels.n, B, levels.C, ptr(sel), M, dims, 1 if rescale else 0, float(score_thr), int(cap), boxes.data_ptr(),
            scores.data_ptr(), labels.data_ptr(), pos.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))
    return boxes, scores, labels, pos, count


def box_nms(boxes, scores, labels, count, iou_threshold, offset=0, max_num=-1, order=None):
    """Greedy NMS of P segments: ``boxes`` [P,cap,4], ``scores`` [P,cap], ``labels`` [P,cap] int64 or None (class-agnostic), ``count`` [P]
    int32 on the device, ``order`` [P,cap] int32 or None (the library sorts; needs count <= SORT_MAX).  Returns (keep [P,max_keep] int32,
    n_keep [P] int32, status [P] int32), all on the device; max_keep = max_num when max_num > 0, else cap (the rule of the header)."""
    need_cuda(boxes=boxes, scores=scores, labels=labels, count=count, order=order)
    if boxes.dim() != 3 or boxes.shape[-1] != 4 or boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise RuntimeError(f'boxes must be contiguous fp32 [P,cap,4], got {boxes.dtype} {tuple(boxes.shape)}')
    P, cap = int(boxes.shape[0]), int(boxes.shape[1])
    for name, t, dt in (('scores', scores, torch.float32), ('labels', labels, torch.int64), ('order', order, torch.int32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (P, cap) or not t.is_contiguous()):
            raise RuntimeError(f'{name} must be contiguous {dt} [{P}, {cap}], got {t.dtype} {tuple(t.shape)}')
    if count.dtype != torch.int32 or tuple(count.shape) != (P,) or not count.is_contiguous():
        raise RuntimeError(f'count must be int32 [{P}], got {count.dtype} {tuple(count.shape)}')
    if cap < 1:
        raise RuntimeError('cap must be at least 1')
    dev = boxes.device
    max_keep = max_num if max_num > 0 else cap
    keep = torch.empty((P, max_keep), dtype=torch.int32, device=dev)
    n_keep = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return keep, n_keep, status
    lib = _lib.load()
    nbytes = lib.bxi_box_nms_workspace_bytes(P, cap, max_keep)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_box_nms_f32', lib.bxi_box_nms_f32(
            boxes.data_ptr(), scores.data_ptr(), ptr(labels), count.data_ptr(), ptr(order), P, cap, float(iou_threshold), int(offset),
            int(max_num), keep.data_ptr(), n_keep.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 4, current_stream(dev)))
    return keep, n_keep, status


def det_gather(levels: _Levels, sel, cand, keep, n_keep):
    """The kept detections of every image (condinst_head.py:72-83): (dets [B,max_keep,5], det_labels [B,max_keep], det_params
    [B,max_keep,P], det_coors [B,max_keep,2], det_level_inds [B,max_keep]); rows from n_keep[b] on are zeros."""
    boxes, scores, labels, pos, _ = cand
    B, dev, P = levels.B, levels.dev, levels.P
    cap, max_keep = int(boxes.shape[1]), int(keep.shape[1])
    M = levels.M_all if sel is None else int(sel.shape[1])
    dets = torch.empty((B, max_keep, 5), dtype=torch.float32, device=dev)
    det_labels = torch.empty((B, max_keep), dtype=torch.int64, device=dev)
    det_params = torch.empty((B, max_keep, P), dtype=torch.float32, device=dev)
    det_coors = torch.empty((B, max_keep, 2), dtype=torch.float32, device=dev)
    det_level_inds = torch.empty((B, max_keep), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_det_gather_f32', _lib.load().bxi_det_gather_f32(
            levels.arr, levels.n, B, levels.C, P, ptr(sel), M, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), pos.data_ptr(), cap,
            keep.data_ptr(), n_keep.data_ptr(), max_keep, dets.data_ptr(), det_labels.data_ptr(), det_params.data_ptr() if P else None,
            det_coors.data_ptr(), det_level_inds.data_ptr(), current_stream(dev)))
    return dets, det_labels, det_params, det_coors, det_level_inds


def _stable_order(scores):
    """[P,cap] int32: descending score, ties by ascending index, NaN first (the rule of bxi_box_nms_f32), by torch's stable sort."""
    return torch.sort(scores, dim=1, descending=True, stable=True)[1].to(torch.int32).contiguous()


# ---- mmcv's names -----------------------------------------------------------------------------------------------------------
def _nms_single(boxes, scores, labels, iou_threshold, offset, max_num):
    """Keep indices (int64, score order) of one set of boxes; one host synchronisation for their number."""
    n = int(boxes.shape[0])
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    b = boxes.detach().to(torch.float32).contiguous().view(1, n, 4)
    s = scores.detach().to(torch.float32).contiguous().view(1, n)
    lab = None if labels is None else labels.detach().to(torch.int64).contiguous().view(1, n)
    count = torch.full((1,), n, dtype=torch.int32, device=boxes.device)
    order = _stable_order(s) if n > SORT_MAX else None
    keep, n_keep, status = box_nms(b, s, lab, count, iou_threshold, offset, min(max_num, n), order)    # no rows beyond n
    k, st = torch.stack([n_keep[0], status[0]]).tolist()
    if st != 0 or k < 0:
        raise RuntimeError(f'bxi_box_nms_f32: status word {st}')
    return keep[0, :k].to(torch.int64)


def nms(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1):
    """``mmcv.ops.nms.nms``: ``boxes`` [n,4], ``scores`` [n] on the GPU -> (dets [k,5], inds [k] int64), in descending score order."""
    need_cuda(boxes=boxes, scores=scores)
    assert boxes.dim() == 2 and boxes.size(1) == 4 and boxes.size(0) == scores.size(0)
    assert offset in (0, 1)
    src = None
    if score_threshold > 0:
        src = (scores > score_threshold).nonzero(as_tuple=False).squeeze(1)
        boxes, scores = boxes[src], scores[src]
    inds = _nms_single(boxes, scores, None, iou_threshold, offset, max_num)
    dets = torch.cat((boxes[inds], scores[inds].reshape(-1, 1)), dim=1)
    return dets, (inds if src is None else src[inds])


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """``mmcv.ops.nms.batched_nms``: NMS among boxes of the same ``idxs`` -> (dets [k,5], keep [k]).  ``nms_cfg`` keys: ``type`` ('nms'
    only), ``iou_threshold``, ``class_agnostic``, ``max_num``; ``split_thr`` is accepted and ignored (mmcv's threshold above which it
    loops over the classes; the result is the same).  Any other key raises."""
    need_cuda(boxes=boxes, scores=scores, idxs=idxs)
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    kind = cfg.pop('type', 'nms')
    if kind != 'nms':
        raise NotImplementedError(f"nms type {kind!r} is not supported: only 'nms'")
    cfg.pop('split_thr', None)
    max_num = cfg.pop('max_num', -1)
    iou_threshold = cfg.pop('iou_threshold')
    if cfg:
        raise TypeError(f'unknown nms_cfg keys {sorted(cfg)}')
    keep = _nms_single(boxes, scores, None if class_agnostic else idxs, iou_threshold, 0, max_num)
    return torch.cat([boxes[keep], scores[keep].reshape(-1, 1)], -1), keep


def nms_with_others(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, others=None):
    """``nms_with_others`` of the reference (condinst_head.py:18-83): ``multi_bboxes`` [n,4] or [n,C*4], ``multi_scores`` [n,C+1] with
    the background column last.  A (row, class) pair is a candidate where its class score is above ``score_thr``; its score is the class
    score times the row's ``score_factors``.  Returns (dets [k,5], labels [k], the rows of every ``others`` item that belong to the kept
    detections); the labels are on the boxes' device (the reference leaves them on the CPU)."""
    need_cuda(multi_bboxes=multi_bboxes, multi_scores=multi_scores, score_factors=score_factors)
    n, C = multi_scores.size(0), multi_scores.size(1) - 1
    if others is not None and any(item.size(0) != n for item in others):
        raise RuntimeError(f'every item of `others` needs {n} rows')
    m, c = (multi_scores[:, :C] > score_thr).nonzero(as_tuple=True)        # ascending (row, class)
    scores = multi_scores[m, c]
    if score_factors is not None:
        scores = scores * score_factors.reshape(-1)[m]
    boxes = multi_bboxes.view(n, -1, 4)[m, c] if multi_bboxes.shape[1] > 4 else multi_bboxes[m]
    if m.numel() == 0:
        dets, keep = torch.cat([boxes, scores[:, None]], -1), m
    else:
        dets, keep = batched_nms(boxes, scores, c, nms_cfg)
        if max_num > 0:
            dets, keep = dets[:max_num], keep[:max_num]
    rows = m[keep]
    return dets, c[keep], None if others is None else [item[rows] for item in others]


# ---- the box head's test path ---------------------------------------------------------------------------------------------
def _img_dims(img_metas, B):
    rows = []
    for i in range(B):
        meta = dict(img_metas[i])
        h, w = meta['img_shape'][:2]
        sf = meta.get('scale_factor', (1.0, 1.0, 1.0, 1.0))
        sf = [float(v) for v in (sf.tolist() if hasattr(sf, 'tolist') else sf)] if not isinstance(sf, (int, float)) else [float(sf)] * 4
        if len(sf) != 4:
            raise RuntimeError(f'scale_factor of image {i} must have four entries (w, h, w, h), got {sf}')
        rows.append([float(h), float(w)] + sf)
    return rows


def _select(levels, loc_score, nms_pre):
    """The per-level top-k of condinst_head.py:779-794 as indices into M_all, or None when no level is cut."""
    if nms_pre <= 0 or all(hw <= nms_pre for hw in levels.sizes):
        return None
    parts, at = [], 0
    for hw in levels.sizes:
        if hw > nms_pre:
            parts.append(loc_score[:, at:at + hw].topk(nms_pre, dim=1)[1] + at)
        else:
            parts.append(torch.arange(at, at + hw, device=levels.dev, dtype=torch.int64).expand(levels.B, hw))
        at += hw
    return torch.cat(parts, dim=1).contiguous()


def _det_pipeline(levels, sel, dims, rescale, cfg, cap, max_num, own_sort):
    cand = det_candidates(levels, sel, dims, rescale, cfg['score_thr'], cap, fill_scores=None if own_sort else float('-inf'))
    order = None if own_sort else _stable_order(cand[1])
    keep, n_keep, status = box_nms(cand[0], cand[1], None if cfg['class_agnostic'] else cand[2], cand[4], cfg['iou_threshold'], 0, min(max_num, cap), order)    # no rows beyond cap
    return cand, keep, n_keep, status, det_gather(levels, sel, cand, keep, n_keep)


def condinst_get_bboxes(cls_scores, bbox_preds, centernesses, param_preds, img_metas, cfg, strides, rescale=False,
                        max_candidates=SORT_MAX):
    """``CondInstBoxHead.get_bboxes`` (condinst_head.py:640-853) for the whole batch.  ``cls_scores`` / ``bbox_preds`` / ``centernesses``
    / ``param_preds``: per FPN level [B,C,H,W] / [B,4,H,W] / [B,1,H,W] / [B,P,H,W];  ``img_metas``: per image ``img_shape`` and
    ``scale_factor``;  ``cfg``: the ``test_cfg`` (dict or namespace: nms_pre, score_thr, nms=dict(type='nms', iou_threshold=...),
    max_per_img);  ``strides``: the head's per-level strides.

    Returns a list per image of ``(det_bboxes [n,5], det_labels [n], det_params [n,P], det_coors [n,2], det_level_inds [n])``: what
    ``CondInst.simple_test`` unzips and ``CondInstMaskHead.simple_test`` takes.  An image without detections gets empty tensors.

    A handful of launches for the batch and ONE host synchronisation, at the end, for the counts.  The first attempt holds
    ``cap = min(M * C, max_candidates)`` candidates per image, sorted by the library.  If the counts show an image with more
    (``score_thr`` passed by more than ``max_candidates`` (location, class) pairs), the batch is redone with ``cap = max(count)``,
    ``torch.sort(stable=True, descending=True)`` for the order and the same NMS kernel: the same result, one more synchronisation
    and one more pass.  ``with_nms=False`` of the reference is not offered (its callers never pass it)."""
    t = parse_test_cfg(cfg)
    levels = _Levels(cls_scores, bbox_preds, centernesses, param_preds, strides)
    B = levels.B
    if len(img_metas) < B:
        raise RuntimeError(f'{B} images but {len(img_metas)} img_metas')
    if max_candidates < 1 or max_candidates > SORT_MAX:
        raise RuntimeError(f'max_candidates must be in 1..{SORT_MAX}')
    if B == 0:
        return []
    dims = _img_dims(img_metas, B)
    sel = _select(levels, location_scores(levels), t['nms_pre']) if t['nms_pre'] > 0 and any(hw > t['nms_pre'] for hw in levels.sizes) else None
    M = levels.M_all if sel is None else int(sel.shape[1])
    max_num = min(v for v in (t['max_per_img'], t['nms_max_num'], 1 << 30) if v > 0)
    max_num = -1 if max_num == 1 << 30 else max_num
    cap = max(1, min(M * levels.C, int(max_candidates)))
    cand, keep, n_keep, status, out = _det_pipeline(levels, sel, dims, rescale, t, cap, max_num, True)
    host = torch.stack([n_keep, cand[4], status]).tolist()                     # the one synchronisation
    if max(host[1]) > cap:
        cap = max(host[1])
        cand, keep, n_keep, status, out = _det_pipeline(levels, sel, dims, rescale, t, cap, max_num, False)
        host = torch.stack([n_keep, cand[4], status]).tolist()
    if any(host[2]) or min(host[0]) < 0:
        raise RuntimeError(f'bxi_box_nms_f32: status words {host[2]} for counts {host[1]} at cap {cap}')
    dets, det_labels, det_params, det_coors, det_level_inds = out
    return [(dets[b, :n], det_labels[b, :n], det_params[b, :n], det_coors[b, :n], det_level_inds[b, :n]) for b, n in enumerate(host[0])]
