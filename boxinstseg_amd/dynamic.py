"""The producer of ``mask_logits``: ``CondInstMaskHead.forward`` of the reference
(``mmdet/models/dense_heads/condinst_head.py:1139-1164``) as one HIP kernel forward and two backward
(SURVEY 8(f-2)): relative coordinates, the three per-instance dynamic 1x1 convolutions with ReLU,
``aligned_bilinear`` -- see ``csrc/dynamic_head.hip``.  Thin marshalling only; no CPU path.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import current_stream


class DynamicMaskHead(torch.autograd.Function):
    """logits[N,1,fH,fW] = f(feat[B,C,H,W], params[N,P]); differentiable w.r.t. feat and params."""

    @staticmethod
    def forward(ctx, feat, params, coors, level_inds, img_inds, sizes_of_interest, in_stride, factor,
                disable_rel_coors):
        for name, t in (('feat', feat), ('params', params), ('coors', coors), ('level_inds', level_inds),
                        ('img_inds', img_inds), ('sizes_of_interest', sizes_of_interest)):
            if not t.is_cuda:
                raise RuntimeError(f'{name} must be a CUDA (HIP) tensor: boxinstseg_amd has no CPU path')
        dev = feat.device
        B, C, H, W = feat.shape
        N = params.size(0)
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        i64 = lambda t: t.detach().to(device=dev, dtype=torch.int64).contiguous()
        feat_c, params_c, coors_c = f32(feat), f32(params), f32(coors).view(-1, 2)
        lvl, img, soi = i64(level_inds), i64(img_inds), f32(sizes_of_interest)
        expect = (C + (0 if disable_rel_coors else 2)) * 8 + 64 + 8 + 8 + 8 + 1
        if params_c.dim() != 2 or (N > 0 and params_c.size(1) != expect):
            raise RuntimeError(f'params must be [N,{expect}] for {C} feature channels, got {tuple(params.shape)}')
        out = torch.empty((N, 1, H * factor, W * factor), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_dynamic_mask_forward_f32', _lib.load().bxi_dynamic_mask_forward_f32(
                feat_c.data_ptr(), B, C, H, W, params_c.data_ptr(), N, coors_c.data_ptr(), lvl.data_ptr(),
                img.data_ptr(), soi.data_ptr(), soi.numel(), int(in_stride), int(factor), int(bool(disable_rel_coors)),
                out.data_ptr(), current_stream(dev)))
        ctx.save_for_backward(feat_c, params_c, coors_c, lvl, img, soi)
        ctx.cfg = (int(in_stride), int(factor), int(bool(disable_rel_coors)))
        ctx.dtypes = (feat.dtype, params.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        feat, params, coors, lvl, img, soi = ctx.saved_tensors
        in_stride, factor, no_rel = ctx.cfg
        dev = feat.device
        B, C, H, W = feat.shape
        N = params.size(0)
        g = g.to(torch.float32).contiguous()
        g_feat = torch.empty_like(feat)
        g_params = torch.empty_like(params)
        lib = _lib.load()
        ws = torch.empty(max(lib.bxi_dynamic_mask_backward_workspace_bytes(B, C, H, W, N, no_rel), 256),
                         dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_dynamic_mask_backward_f32', lib.bxi_dynamic_mask_backward_f32(
                feat.data_ptr(), B, C, H, W, params.data_ptr(), N, coors.data_ptr(), lvl.data_ptr(), img.data_ptr(),
                soi.data_ptr(), soi.numel(), in_stride, factor, no_rel, g.data_ptr(), g_feat.data_ptr(),
                g_params.data_ptr(), ws.data_ptr(), ws.numel(), current_stream(dev)))
        return (g_feat.to(ctx.dtypes[0]), g_params.to(ctx.dtypes[1]), None, None, None, None, None, None, None)


def generic_supported(dynamic_convs: int, dynamic_channels: int, in_channels: int, disable_rel_coors: bool) -> bool:
    """The shapes ``csrc/dynamic_head_generic.hip`` is built for."""
    return 1 <= dynamic_convs <= 4 and 1 <= dynamic_channels <= 16 and 1 <= in_channels and in_channels + (0 if disable_rel_coors else 2) <= 34


class GenericDynamicMaskHead(torch.autograd.Function):
    """``DynamicMaskHead`` for every head shape the reference's constructor admits (condinst_head.py:1079-1089): ``layers``
    dynamic convolutions of ``channels`` channels -- HIP forward and backward (``csrc/dynamic_head_generic.hip``)."""

    @staticmethod
    def forward(ctx, feat, params, coors, level_inds, img_inds, sizes_of_interest, in_stride, factor, disable_rel_coors, layers,
                channels):
        for name, t in (('feat', feat), ('params', params), ('coors', coors), ('level_inds', level_inds),
                        ('img_inds', img_inds), ('sizes_of_interest', sizes_of_interest)):
            if not t.is_cuda:
                raise RuntimeError(f'{name} must be a CUDA (HIP) tensor: boxinstseg_amd has no CPU path')
        dev = feat.device
        B, C, H, W = feat.shape
        N = params.size(0)
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        i64 = lambda t: t.detach().to(device=dev, dtype=torch.int64).contiguous()
        feat_c, params_c, coors_c = f32(feat), f32(params), f32(coors).view(-1, 2)
        lvl, img, soi = i64(level_inds), i64(img_inds), f32(sizes_of_interest)
        cin = C + (0 if disable_rel_coors else 2)
        expect = (cin + 1) if layers == 1 else (cin * channels + (layers - 2) * channels * channels + channels +
                                                  (layers - 1) * channels + 1)
        if params_c.dim() != 2 or (N > 0 and params_c.size(1) != expect):
            raise RuntimeError(f'params must be [N,{expect}] for {layers} layers x {channels} channels on {C} feature channels, '
                               f'got {tuple(params.shape)}')
        for name, t in (('coors', coors_c), ('level_inds', lvl), ('img_inds', img)):
            if t.size(0) != N:
                raise RuntimeError(f'{name} has {t.size(0)} entries for {N} instances')
        out = torch.empty((N, 1, H * factor, W * factor), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_dynamic_mask_generic_forward_f32', _lib.load().bxi_dynamic_mask_generic_forward_f32(
                feat_c.data_ptr(), B, C, H, W, params_c.data_ptr(), N, int(layers), int(channels), coors_c.data_ptr(), lvl.data_ptr(),
                img.data_ptr(), soi.data_ptr(), soi.numel(), int(in_stride), int(factor), int(bool(disable_rel_coors)),
                out.data_ptr(), current_stream(dev)))
        ctx.save_for_backward(feat_c, params_c, coors_c, lvl, img, soi)
        ctx.cfg = (int(in_stride), int(factor), int(bool(disable_rel_coors)), int(layers), int(channels))
        ctx.dtypes = (feat.dtype, params.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        feat, params, coors, lvl, img, soi = ctx.saved_tensors
        in_stride, factor, no_rel, layers, channels = ctx.cfg
        dev = feat.device
        B, C, H, W = feat.shape
        N = params.size(0)
        g = g.to(torch.float32).contiguous()
        g_feat = torch.empty_like(feat)
        g_params = torch.empty_like(params)
        lib = _lib.load()
        ws = torch.empty(max(lib.bxi_dynamic_mask_generic_backward_workspace_bytes(B, C, H, W, N, layers, channels, no_rel), 256),
                         dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_dynamic_mask_generic_backward_f32', lib.bxi_dynamic_mask_generic_backward_f32(
                feat.data_ptr(), B, C, H, W, params.data_ptr(), N, layers, channels, coors.data_ptr(), lvl.data_ptr(), img.data_ptr(),
                soi.data_ptr(), soi.numel(), in_stride, factor, no_rel, g.data_ptr(), g_feat.data_ptr(), g_params.data_ptr(),
                ws.data_ptr(), ws.numel(), current_stream(dev)))
        return (g_feat.to(ctx.dtypes[0]), g_params.to(ctx.dtypes[1])) + (None,) * 9


def dynamic_mask_forward_generic(feat, params, coors, level_inds, img_inds, sizes_of_interest, dynamic_convs, dynamic_channels,
                                 in_stride=8, out_stride=4, disable_rel_coors=False):
    """``CondInstMaskHead.forward`` for a head of ``dynamic_convs`` layers x ``dynamic_channels`` channels -> ``[N,1,H*f,W*f]``."""
    if in_stride % out_stride:
        raise RuntimeError('in_stride must be a multiple of out_stride')
    return GenericDynamicMaskHead.apply(feat, params, coors, level_inds, img_inds, sizes_of_interest, in_stride,
                                        in_stride // out_stride, disable_rel_coors, dynamic_convs, dynamic_channels)


def dynamic_mask_forward(feat, params, coors, level_inds, img_inds, sizes_of_interest, in_stride=8, out_stride=4,
                         disable_rel_coors=False):
    """``CondInstMaskHead.forward(feat, params, coors, level_inds, img_inds)`` -> ``[N,1,H*f,W*f]``."""
    if in_stride % out_stride:
        raise RuntimeError('in_stride must be a multiple of out_stride')
    return DynamicMaskHead.apply(feat, params, coors, level_inds, img_inds, sizes_of_interest, in_stride,
                                 in_stride // out_stride, disable_rel_coors)


def aligned_bilinear(tensor, factor):
    """The module-level ``aligned_bilinear(tensor, factor)`` of condinst_head.py:146-167 for the test-time path
    (``simple_test`` up-samples the mask probabilities to the input resolution): output sample ``(y, x)`` sits at source
    coordinate ``((y - factor // 2) / factor, (x - factor // 2) / factor)``, clamped to the map.  Composed of torch ops on
    whatever device the tensor lives on; the training-time ``x factor`` step is fused into ``dyn_fwd_kernel`` instead."""
    import torch.nn.functional as F
    assert tensor.dim() == 4 and factor >= 1 and int(factor) == factor
    if factor == 1:
        return tensor
    h, w = tensor.shape[2:]
    x = F.pad(tensor, (0, 1, 0, 1), mode='replicate')
    x = F.interpolate(x, size=(factor * h + 1, factor * w + 1), mode='bilinear', align_corners=True)
    x = F.pad(x, (factor // 2, 0, factor // 2, 0), mode='replicate')
    return x[:, :, :factor * h, :factor * w]


def _paste_dims(img_metas, rescale: bool):
    """Per image (crop_h, crop_w, out_h, out_w): the crop is ``img_shape``, the output ``ori_shape`` when rescaling."""
    dims = []
    for meta in img_metas:
        ih, iw = (int(v) for v in meta['img_shape'][:2])
        oh, ow = (int(v) for v in meta['ori_shape'][:2]) if rescale else (ih, iw)
        dims.append((ih, iw, oh, ow))
    return dims


def paste_order(img_inds, labels, counts, hw, num_classes=None):
    """Byte offsets of every instance's mask in one buffer that holds, image after image, the masks of each image.

    ``counts[i]`` / ``hw[i]``: detections and mask bytes (``out_h * out_w``) of image ``i`` (host ints).  With ``num_classes``
    an image's masks are grouped by class, each class in detection order -- the order of the reference's ``masks[labels == c]``
    for ``c`` in ``range(num_classes)``; labels outside ``0..num_classes-1`` go last and belong to no class.  Without it they stay
    in detection order.  Returns ``(offsets [N] int64, key [N] int64)``, ``key = img * (num_classes + 1) + class`` (the class
    count table of the host side), on the tensors' device; torch ops only, no host synchronisation."""
    dev = img_inds.device
    img = img_inds.to(torch.int64)
    n = img.numel()
    if num_classes is None:
        key = img
    else:
        lab = labels.to(device=dev, dtype=torch.int64)
        lab = torch.where((lab >= 0) & (lab < num_classes), lab, torch.full_like(lab, num_classes))
        key = img * (num_classes + 1) + lab
    order = torch.argsort(key, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n, dtype=torch.int64, device=dev)
    counts_t = torch.tensor(list(counts), dtype=torch.int64)
    hw_t = torch.tensor(list(hw), dtype=torch.int64)
    start = (torch.cumsum(counts_t, 0) - counts_t).to(dev)
    base = (torch.cumsum(counts_t * hw_t, 0) - counts_t * hw_t).to(dev)
    hw_d = hw_t.to(dev)
    return base[img] + (rank - start[img]) * hw_d[img], key


def _paste(logits, img_inds, offsets, dims, total, out_stride, threshold):
    """One bxi_mask_paste_u8 launch into a new device buffer of ``total`` bytes."""
    import ctypes as C
    dev = logits.device
    if logits.dim() != 4 or logits.size(1) != 1:
        raise RuntimeError(f'logits must be [N,1,h,w], got {tuple(logits.shape)}')
    N, _, h, w = logits.shape
    lg = logits.detach().to(torch.float32).contiguous()
    img = img_inds.to(device=dev, dtype=torch.int64).contiguous()
    off = offsets.contiguous()
    masks = torch.empty(total, dtype=torch.uint8, device=dev)
    flat = [int(v) for d in dims for v in d]
    dims_host = (C.c_int32 * max(len(flat), 1))(*flat)
    with torch.cuda.device(dev):
        _lib.check('bxi_mask_paste_u8', _lib.load().bxi_mask_paste_u8(
            lg.data_ptr(), N, h, w, int(out_stride), img.data_ptr(), off.data_ptr(), len(dims), dims_host, float(threshold),
            masks.data_ptr(), current_stream(dev)))
    return masks


def _check_paste_inputs(logits, img_inds, labels):
    for name, t in (('logits', logits), ('img_inds', img_inds), ('labels', labels)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'{name} must be a CUDA (HIP) tensor: boxinstseg_amd has no CPU path')


def _counts(img_inds, B, counts):
    if counts is not None:
        return [int(c) for c in counts]
    return torch.bincount(img_inds.to(torch.int64), minlength=B).tolist()[:B]      # one small copy when the caller has no counts


def paste_masks(logits, img_inds, labels, img_metas, num_classes, *, out_stride=4, rescale=False, threshold=0.5, counts=None):
    """The mask post-processing of ``CondInstMaskHead.simple_test`` (condinst_head.py:1259-1285) after ``forward``:
    ``sigmoid`` -> ``aligned_bilinear(., out_stride)`` -> crop to ``img_shape`` -> bilinear to ``ori_shape`` when ``rescale`` ->
    ``> threshold`` -> per image, per class ``uint8`` arrays ``[n_c, H, W]`` (``masks[labels == c]`` of the reference).

    ``logits`` ``[N,1,h,w]`` (the head's output at ``out_stride``), ``img_inds`` / ``labels`` ``[N]`` on the same device.
    ``counts`` (optional): detections per image, if the caller knows them -- else they are counted from ``img_inds`` with one
    small device-to-host copy.  One kernel (``csrc/mask_paste.hip``) writes every image's masks, class-grouped, into one device
    buffer, which comes to the host in one copy (into pinned memory); the per-class arrays are non-overlapping, C-contiguous
    slices of it (an empty class gives ``(0, H, W)``)."""
    import numpy as np
    _check_paste_inputs(logits, img_inds, labels)
    dims = _paste_dims(img_metas, rescale)
    B = len(dims)
    counts = _counts(img_inds, B, counts)
    hw = [d[2] * d[3] for d in dims]
    total = sum(c * s for c, s in zip(counts, hw))
    offsets, key = paste_order(img_inds, labels, counts, hw, num_classes)
    masks = _paste(logits, img_inds, offsets, dims, total, out_stride, threshold)
    # pinned host memory (torch's caching host allocator): the copy runs at DMA speed, 10.8 against 60.7 ms into pageable memory
    # for 614 MB (tools/bench_mask_paste.py).  The arrays below keep their block alive, so a later call never reuses it under them.
    host_t = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    key_t = torch.empty(key.numel(), dtype=torch.int64, pin_memory=True)
    host_t.copy_(masks, non_blocking=True)
    key_t.copy_(key, non_blocking=True)
    torch.cuda.current_stream(logits.device).synchronize()
    host, key_host = host_t.numpy(), key_t.numpy()
    per_class = np.bincount(key_host, minlength=B * (num_classes + 1)).reshape(B, num_classes + 1)
    results, pos = [], 0
    for i, (_, _, oh, ow) in enumerate(dims):
        cls = []
        for c in range(num_classes):
            n = int(per_class[i, c])
            cls.append(host[pos:pos + n * oh * ow].reshape(n, oh, ow))
            pos += n * oh * ow
        pos += int(per_class[i, num_classes]) * oh * ow
        results.append(cls)
    return results


def paste_masks_device(logits, img_inds, img_metas, *, out_stride=4, rescale=False, threshold=0.5, counts=None):
    """``paste_masks`` for callers that post-process on the GPU: the same launch, masks in detection order, per image a device
    ``uint8`` tensor ``[n_i, H_i, W_i]`` (views of one buffer)."""
    _check_paste_inputs(logits, img_inds, None)
    dims = _paste_dims(img_metas, rescale)
    counts = _counts(img_inds, len(dims), counts)
    hw = [d[2] * d[3] for d in dims]
    total = sum(c * s for c, s in zip(counts, hw))
    offsets, _ = paste_order(img_inds, None, counts, hw)
    masks = _paste(logits, img_inds, offsets, dims, total, out_stride, threshold)
    out, pos = [], 0
    for c, (_, _, oh, ow) in zip(counts, dims):
        out.append(masks[pos:pos + c * oh * ow].view(c, oh, ow))
        pos += c * oh * ow
    return out
