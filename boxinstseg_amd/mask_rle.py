"""The test-time masks as COCO run-length encodings, encoded on the GPU (csrc/mask_rle.hip, include/boxinst/boxinst_hip_rle.h).

    rle_encode               <-> ``mask_util.encode`` once per mask (mmdet/core/mask/utils.py:55-61), for a whole [n,h,w] block in four launches
    EncodedMasks.to_coco     : the ``{'size': [h, w], 'counts': bytes}`` dicts, one pinned copy and one synchronisation
    rle_decode               <-> ``mask_util.decode``, on the host in numpy (rleFrString + rleDecode): for users and tests
    solo_encode_results      <-> ``format_results`` followed by ``encode_mask_results`` (mmdet/apis/test.py:65,72,112,119) for the SOLOv2-style heads
    box2mask_encode_results  <-> MaskFormer.simple_test's formatting followed by ``encode_mask_results`` for Box2Mask

There is no CPU or PyTorch fallback: CPU tensors raise.  The format is restated from the published algorithm of cocoapi's maskApi.c and
UNPINNED (pycocotools never ran next to it); any non-zero byte counts as a set pixel.

Capacities.  The counts and characters of a block are packed mask after mask into buffers whose size has to be chosen before the masks
are looked at.  The default rule is ``cap_runs = n * (2 * w + 2)`` (two transitions per column and mask: a blob without holes never needs
more), at most the worst case ``n * (h * w + 1)``, and ``cap_chars = 2 * cap_runs``.  Running out is never silent: the kernels still write
every offset and the true totals, the status word says which capacity ran out, and ``EncodedMasks.host()`` (which ``to_coco`` and both
``*_encode_results`` go through) then encodes ONCE more with exactly the totals it has just read -- one more synchronisation.
"""
from __future__ import annotations

import torch

from . import _lib
from ._common import current_stream, need_cuda, ptr

__all__ = ['rle_encode', 'rle_decode', 'EncodedMasks', 'solo_encode_results', 'box2mask_encode_results']

_HEADER = 'boxinst_hip_rle.h'


def default_capacities(n, h, w):
    """The documented rule: (cap_runs, cap_chars) for n masks of h x w."""
    cap_runs = min(n * (2 * w + 2), n * (h * w + 1))
    return cap_runs, 2 * cap_runs


def check_shape(n, h, w):
    """What bxi_mask_rle_u8 refuses, before anything is allocated or launched."""
    if n < 0 or h < 1 or w < 1:
        raise RuntimeError(f'masks must be [n,h,w] with h, w >= 1, got {(n, h, w)}')
    if h * w >= _lib.RLE_MAX_PIXELS or n * (h * w + 1) * _lib.RLE_MAX_CHARS_PER_COUNT > 0x7fffffff:
        raise NotImplementedError(f'rle_encode: {n} masks of {h} x {w} are outside the support set of include/boxinst/{_HEADER} '
                                  '(h * w < 2^29 and n * (h * w + 1) * 6 < 2^31)')


class EncodedMasks:
    """The device buffers of one ``rle_encode`` call.  ``block`` is ONE uint8 buffer: ``extra`` bytes of the caller's (what a
    ``*_encode_results`` wants on the host next to the strings), then status int32 [1], run_offsets int32 [n+1], char_offsets int32 [n+1]
    and chars uint8 [cap_chars]; ``counts`` uint32 [cap_runs] is a buffer of its own (the strings are what COCO consumes).  Nothing
    has been synchronised: ``status`` is a device value."""

    def __init__(self, masks, stats, cap_runs, cap_chars, extra=0):
        self.masks, self.stats, self.extra = masks, stats, int(extra)
        self.n, self.h, self.w = (int(v) for v in masks.shape)
        self.retried = False
        self._run(int(cap_runs), int(cap_chars), None)

    def _run(self, cap_runs, cap_chars, head):
        n, dev = self.n, self.masks.device
        self.cap_runs, self.cap_chars = cap_runs, cap_chars
        pad = (self.extra + 7) // 8 * 8
        self.block = torch.empty(pad + 4 + 8 * (n + 1) + cap_chars, dtype=torch.uint8, device=dev)
        self.counts = torch.empty(cap_runs, dtype=torch.int32, device=dev)          # uint32 values below 2^29
        self.head = self.block[:self.extra]
        if head is not None:
            self.head.copy_(head)
        self.status, self.run_offsets, self.char_offsets, self.chars = self._views(self.block)
        lib = _lib.load()
        ws_bytes = lib.bxi_mask_rle_workspace_bytes(n, self.h, self.w)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_mask_rle_u8', lib.bxi_mask_rle_u8(
                self.masks.data_ptr() if n else None, n, self.h, self.w, ptr(self.stats), cap_runs, cap_chars, self.run_offsets.data_ptr(),
                self.counts.data_ptr() if cap_runs else None, self.char_offsets.data_ptr(), self.chars.data_ptr() if cap_chars else None,
                self.status.data_ptr(), ws.data_ptr(), ws_bytes, current_stream(dev)), _HEADER)

    def _views(self, block):
        n = self.n
        a = (self.extra + 7) // 8 * 8
        b, c, d = a + 4, a + 4 + 4 * (n + 1), a + 4 + 8 * (n + 1)
        return block[a:b].view(torch.int32), block[b:c].view(torch.int32), block[c:d].view(torch.int32), block[d:]

    def host(self):
        """-> ``(head, char_offsets, chars)`` on the host (numpy views of one pinned buffer): one copy and one synchronisation.  When the
        status says a capacity ran out, the encoding runs once more with the exact totals just read and is copied again."""
        for attempt in (0, 1):
            host = torch.empty(self.block.numel(), dtype=torch.uint8, pin_memory=True)
            host.copy_(self.block, non_blocking=True)
            torch.cuda.current_stream(self.block.device).synchronize()
            status, run_offsets, char_offsets, chars = self._views(host)
            if int(status[0]) == 0:
                return host[:self.extra], char_offsets.numpy(), chars.numpy()
            if attempt:
                raise RuntimeError(f'rle_encode: status {int(status[0])} with the exact capacities {self.cap_runs}, {self.cap_chars}')
            self.retried = True
            self._run(int(run_offsets[self.n]), int(char_offsets[self.n]), self.head.clone())

    def to_coco(self):
        """``[{'size': [h, w], 'counts': bytes}, ...]``: what ``mask_util.encode(...)[0]`` returns for every mask."""
        _, off, chars = self.host()
        return _rles(off, chars, self.h, self.w, range(self.n))


def _rles(off, chars, h, w, which):
    buf = chars.tobytes()
    return [{'size': [h, w], 'counts': buf[off[i]:off[i + 1]]} for i in which]


def _encode(masks, stats, cap_runs, cap_chars, extra=0):
    need_cuda(masks=masks, stats=stats)
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f'masks must be bool or uint8 [n,h,w], got {masks.dtype} {tuple(masks.shape)}')
    n, h, w = (int(v) for v in masks.shape)
    check_shape(n, h, w)
    if stats is not None:
        if stats.dtype != torch.int32 or tuple(stats.shape) != (n, 5):
            raise RuntimeError(f'stats must be int32 [{n},5], got {stats.dtype} {tuple(stats.shape)}')
        stats = stats.contiguous()
    m = masks.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    rule = default_capacities(n, h, w)
    cap_runs = rule[0] if cap_runs is None else int(cap_runs)
    cap_chars = rule[1] if cap_chars is None else int(cap_chars)
    if cap_runs < 0 or cap_chars < 0:
        raise RuntimeError(f'negative capacity: {cap_runs}, {cap_chars}')
    return EncodedMasks(m, stats, cap_runs, cap_chars, extra)


def rle_encode(masks, stats=None, cap_runs=None, cap_chars=None):
    """COCO's run-length encoding of ``masks``, bool or uint8 [n,h,w] on the GPU (any contiguous view, at any byte address; a non-zero
    byte is a set pixel), in four launches and without a synchronisation.  ``stats`` int32 [n,5] = area, x_min, y_min, x_max, y_max as
    ``seg_paste`` / ``box2mask_instances`` leave them lets the kernels read the masks' boxes only (everything outside must be zero).
    ``cap_runs`` / ``cap_chars`` default to the module's rule.  Returns an ``EncodedMasks``; its ``to_coco()`` gives the dicts."""
    return _encode(masks, stats, cap_runs, cap_chars)


def rle_decode(rles):
    """rleFrString + rleDecode on the host: a list of ``{'size': [h, w], 'counts': bytes or str}`` of ONE size -> numpy bool [n,h,w]."""
    import numpy as np
    rles = list(rles)
    if not rles:
        return np.zeros((0, 0, 0), dtype=bool)
    h, w = (int(v) for v in rles[0]['size'])
    out = np.zeros((len(rles), w, h), dtype=bool)                             # column-major planes
    for i, rle in enumerate(rles):
        if [int(v) for v in rle['size']] != [h, w]:
            raise RuntimeError(f'rle_decode: sizes differ: {rle["size"]} and {[h, w]}')
        s = rle['counts']
        s = s.encode('ascii') if isinstance(s, str) else bytes(s)
        cnts, p = [], 0
        while p < len(s):
            x, k, more = 0, 0, True
            while more:
                c = s[p] - 48
                x |= (c & 0x1f) << (5 * k)
                more = bool(c & 0x20)
                p += 1
                k += 1
                if not more and (c & 0x10):
                    x |= -1 << (5 * k)
            if len(cnts) > 2:
                x += cnts[-2]
            cnts.append(x)
        if sum(cnts) != h * w or any(c < 0 for c in cnts):
            raise RuntimeError(f'rle_decode: the counts of mask {i} do not tile {h} x {w}')
        flat, at = out[i].reshape(-1), 0
        for j, c in enumerate(cnts):
            if j & 1:
                flat[at:at + c] = True
            at += c
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def solo_encode_results(results, num_classes):
    """``format_results`` of the reference's detectors followed by ``encode_mask_results`` (the mask-scoring tuple form) on a results object
    of ``*_get_seg_single``: returns ``(bbox_results, (encoded_masks, score_results))``.  The selection (area > 0), the order, the boxes
    and the scores are those of ``solo_format_results``; a mask is its ``{'size', 'counts'}`` dict instead of a bool tensor.  The masks and
    their statistics are read in place on the device; labels, statistics, scores, offsets and characters reach the host in one copy
    into pinned memory with one synchronisation (one more if the default capacities ran out)."""
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
            raise RuntimeError('results.mask_stats is missing: solo_encode_results reads the area and the box of a mask from the statistics '
                               'of seg_paste (there is no fallback)')
        oh, ow = (int(v) for v in masks.shape[-2:])
        enc = _encode(masks, stats, None, None, extra=32 * n)
        block = getattr(results, 'host_block', None)
        if block is not None and block.numel() == n * (32 + oh * ow):
            enc.head.copy_(block[:32 * n])                                    # labels, statistics, scores as paste_results laid them out
        else:
            enc.head[:8 * n].copy_(results.labels.to(torch.int64).contiguous().view(torch.uint8))
            enc.head[8 * n:28 * n].copy_(enc.stats.view(torch.uint8).view(-1))
            enc.head[28 * n:].copy_(results.scores.float().contiguous().view(torch.uint8))
        head, off, chars = enc.host()
        labels, stats_h, scores = head[:8 * n].view(torch.int64), head[8 * n:28 * n].view(torch.int32).view(n, 5), head[28 * n:].view(torch.float32)
        scores_t = scores if results.scores.dtype == torch.float32 else scores.to(results.scores.dtype)
        lab, st, sc = labels.numpy(), stats_h.numpy(), scores.numpy()
        rles = _rles(off, chars, oh, ow, range(n))
        for i in range(n):
            if st[i, 0] > 0:
                c = int(lab[i])
                mask_results[c].append(rles[i])
                score_results[c].append(scores_t[i])
                bbox_results[c].append([st[i, 1], st[i, 2], st[i, 3] + 1, st[i, 4] + 1, sc[i]])
    bbox_results = [np.array(b, dtype=np.float64) if len(b) > 0 else np.zeros((0, 5)) for b in bbox_results]
    return bbox_results, (mask_results, score_results)


def box2mask_encode_results(results, num_things_classes):
    """MaskFormer.simple_test's formatting followed by ``encode_mask_results`` on one image's results object of ``box2mask_instances``:
    returns ``(bbox_results, encoded_masks)``.  The rows and their order are those of ``box2mask_format_results`` -- all ``count``
    detections, empty masks included (an empty mask is the single count h * w).  The masks and their statistics are read in place on the
    device; labels, boxes, statistics, mask scores, the count, offsets and characters reach the host in one copy into pinned memory with
    one synchronisation (one more if the default capacities ran out)."""
    masks = results.masks
    need_cuda(masks=masks)
    n = int(masks.shape[0])
    oh, ow = (int(v) for v in masks.shape[-2:])
    block = getattr(results, 'host_block', None)
    if block is None or block.numel() != n * (52 + oh * ow) + 4:
        raise RuntimeError('results.host_block is missing or not the buffer of these masks: box2mask_encode_results copies the rows '
                           'box2mask_instances filled (there is no fallback)')
    enc = _encode(masks, results.mask_stats, None, None, extra=52 * n + 4)
    enc.head.copy_(block[:52 * n + 4])                                        # labels, boxes, statistics, mask scores, count
    head, off, chars = enc.host()
    lab = head[:8 * n].view(torch.int64).numpy()
    bx = head[8 * n:28 * n].view(torch.float32).view(n, 5).numpy()
    cnt = int(head[52 * n:52 * n + 4].view(torch.int32).numpy()[0])
    things = int(num_things_classes)
    lab = lab[:cnt]
    bbox_results = [bx[:cnt][lab == c, :] for c in range(things)]
    rles = _rles(off, chars, oh, ow, range(cnt))
    mask_results = [[] for _ in range(things)]
    for j in range(cnt):
        mask_results[int(lab[j])].append(rles[j])
    return bbox_results, mask_results
