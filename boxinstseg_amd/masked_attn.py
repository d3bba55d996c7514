"""The masked cross-attention of Box2Mask's transformer decoder on the HIP kernels of ``csrc/masked_attn.hip``
(include/boxinst/boxinst_hip_attn.h).

    attn_mask_bits       : ``mask_pred [B,Q,H,W]`` resized bilinearly to ``size``, thresholded and packed to one bit per (query, key)
    box2mask_attn_mask   <-> Box2MaskHead.forward_head, box2mask_head.py:346-355, and the repair of forward, :397, as ONE launch
    pack_attn_mask       : an existing bool mask ``[B*M,Q,S]`` or ``[Q,S]`` packed to bits on the device
    masked_attention     : softmax((q * scale) k^T, masked) v per head, forward and backward, the [Q,S] scores never stored
    MultiheadAttention   <-> mmcv.cnn.bricks.transformer.MultiheadAttention over torch.nn.MultiheadAttention (the cross- and self-attention of
                             every layer of Box2Mask's DetrTransformerDecoder); ATTENTION, build_attention

mmcv's wrapper is restated from its documented behaviour and is unpinned: mmcv never ran next to this library (Level 3l).
The arithmetic under it is torch.nn.MultiheadAttention's and is pinned against it.  DEVIATIONS: the mask is one bit per (image, query, key)
and is NOT repeated over the heads; a key is masked where the resized logit is ``< 0`` (the reference's ``sigmoid() < 0.5`` is false for
logits in about (-1.2e-7, 0), where the fp32 sigmoid rounds to 0.5).  There is no CPU and no torch path: fp32 CUDA tensors only; a float mask,
a key_padding_mask, attention dropout in training mode, half precision and CPU tensors raise ``NotImplementedError``.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import current_stream
from .registry import ATTENTION

__all__ = ['PackedAttnMask', 'attn_mask_bits', 'box2mask_attn_mask', 'pack_attn_mask', 'masked_attention', 'MultiheadAttention']


class PackedAttnMask:
    """A bool attention mask as bits: ``bits`` int32 ``[R,Q,ceil(S/32)]`` on the device, bit ``s & 31`` of word ``s >> 5`` set where key ``s``
    is masked; ``S`` keys; ``per_head``: R = B*M, row ``b*M + m`` (torch's layout), else R = B, one mask per image for all its heads (R = 1:
    one mask for every image)."""
    __slots__ = ('bits', 'S', 'per_head')

    def __init__(self, bits: torch.Tensor, S: int, per_head: bool):
        self.bits, self.S, self.per_head = bits, int(S), bool(per_head)

    def __repr__(self):
        return f'PackedAttnMask(bits={tuple(self.bits.shape)}, S={self.S}, per_head={self.per_head})'


_status = functools.partial(_lib.check_supported, header='boxinst_hip_attn.h')


def _need_fp32_cuda(**tensors):
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise NotImplementedError(f'{name} must be float32, got {t.dtype}: half precision is not built')
        if not t.is_cuda:
            raise NotImplementedError(f'{name} must be a CUDA (HIP) tensor: the masked attention has no CPU path')


def _unsupported(embed_dims, num_heads):
    if num_heads < 1 or embed_dims % num_heads != 0:
        raise ValueError(f'embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}')
    if embed_dims // num_heads not in _lib.ATTN_HEAD_DIMS:
        raise NotImplementedError(f'the masked attention is built for a head dimension in {_lib.ATTN_HEAD_DIMS}, got {embed_dims // num_heads}')


def attn_mask_bits(mask_pred, size):
    """``mask_pred [B,Q,H,W]`` (fp32 logits) -> the ``PackedAttnMask`` of ``F.interpolate(mask_pred, size, mode='bilinear',
    align_corners=False).flatten(2) < 0`` with every all-masked row cleared, one launch, no synchronisation.  Not differentiable (the
    reference detaches the mask)."""
    _need_fp32_cuda(mask_pred=mask_pred)
    if mask_pred.dim() != 4:
        raise RuntimeError(f'mask_pred must be [B,Q,H,W], got {list(mask_pred.shape)}')
    h, w = (int(s) for s in size)
    B, Q, H, W = (int(s) for s in mask_pred.shape)
    if h < 1 or w < 1 or h * w > _lib.ATTN_MAX_S:
        raise RuntimeError(f'size must be positive with at most {_lib.ATTN_MAX_S} positions, got {(h, w)}')
    pred = mask_pred.detach().contiguous()
    bits = torch.empty((B, Q, (h * w + 31) // 32), dtype=torch.int32, device=pred.device)
    with torch.cuda.device(pred.device):
        _status('bxi_attn_mask_bits_f32', _lib.load().bxi_attn_mask_bits_f32(pred.data_ptr(), B, Q, H, W, h, w, bits.data_ptr(),
                                                                             current_stream(pred.device)))
    return PackedAttnMask(bits, h * w, False)


def box2mask_attn_mask(mask_pred, attn_mask_target_size):
    """The attention mask of ``Box2MaskHead.forward_head`` (box2mask_head.py:346-355) with the repair of ``forward`` (:397) already applied."""
    return attn_mask_bits(mask_pred, attn_mask_target_size)


def pack_attn_mask(bool_mask, num_heads):
    """A bool mask ``[B*num_heads,Q,S]`` (torch's 3-D ``attn_mask``) or ``[Q,S]`` as a ``PackedAttnMask``, packed on the device.  All-masked
    rows stay as they are: they give NaN, as in torch."""
    if not isinstance(bool_mask, torch.Tensor) or bool_mask.dtype != torch.bool:
        raise NotImplementedError(f'only bool attention masks are built, got {getattr(bool_mask, "dtype", type(bool_mask))}')
    if not bool_mask.is_cuda:
        raise NotImplementedError('attn_mask must be a CUDA (HIP) tensor: the masked attention has no CPU path')
    if bool_mask.dim() == 2:
        rows, per_head = 1, False
    elif bool_mask.dim() == 3 and int(bool_mask.shape[0]) % int(num_heads) == 0:
        rows, per_head = int(bool_mask.shape[0]), True
    else:
        raise RuntimeError(f'attn_mask must be [B*{num_heads},Q,S] or [Q,S], got {list(bool_mask.shape)}')
    Q, S = int(bool_mask.shape[-2]), int(bool_mask.shape[-1])
    if Q < 1 or S < 1:
        raise RuntimeError(f'attn_mask must not be empty, got {list(bool_mask.shape)}')
    src = bool_mask.contiguous().view(torch.uint8)
    bits = torch.empty((rows, Q, (S + 31) // 32), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _status('bxi_attn_pack_mask_u8', _lib.load().bxi_attn_pack_mask_u8(src.data_ptr(), rows * Q, S, bits.data_ptr(), current_stream(src.device)))
    return PackedAttnMask(bits, S, per_head)


class _MaskedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bits, per_head, M, scale):
        lib, dev = _lib.load(), q.device
        q_, k_, v_ = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        Q, B, E = (int(s) for s in q_.shape)
        S, D = int(k_.shape[0]), E // M
        out = torch.empty((Q, B, E), dtype=torch.float32, device=dev)
        lse = torch.empty((B, M, Q), dtype=torch.float32, device=dev)
        nbytes = lib.bxi_masked_attn_forward_workspace_bytes(B, M, Q, S, D)
        if nbytes == 0:
            raise NotImplementedError(f'masked attention: B*M={B * M}, Q={Q}, S={S}, D={D} is outside include/boxinst/boxinst_hip_attn.h')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _status('bxi_masked_attn_forward_f32', lib.bxi_masked_attn_forward_f32(
                q_.data_ptr(), k_.data_ptr(), v_.data_ptr(), None if bits is None else bits.data_ptr(), int(per_head), B, M, Q, S, D, scale,
                out.data_ptr(), lse.data_ptr(), ws.data_ptr(), nbytes, current_stream(dev)))
        ctx.save_for_backward(q_, k_, v_, bits, out, lse)
        ctx.args = (per_head, M, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, k, v, bits, out, lse = ctx.saved_tensors
        per_head, M, scale = ctx.args
        lib, dev = _lib.load(), q.device
        Q, B, E = (int(s) for s in q.shape)
        S, D = int(k.shape[0]), E // M
        g = g.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        nbytes = lib.bxi_masked_attn_backward_workspace_bytes(B, M, Q, S, D)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _status('bxi_masked_attn_backward_f32', lib.bxi_masked_attn_backward_f32(
                g.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), None if bits is None else bits.data_ptr(), int(per_head), out.data_ptr(),
                lse.data_ptr(), B, M, Q, S, D, scale, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), nbytes, current_stream(dev)))
        return dq, dk, dv, None, None, None, None


def masked_attention(q, k, v, mask, num_heads):
    """``q [Q,B,E]``, ``k`` and ``v [S,B,E]`` as ``F.linear`` leaves the in-projection with ``batch_first=False`` (E = num_heads * D, head m in
    columns m*D .. m*D+D-1), ``mask`` a ``PackedAttnMask`` or None -> ``[Q,B,E]``: per (image, head) ``softmax((q / sqrt(D)) k^T, -inf where
    masked) v``, torch.nn.MultiheadAttention's core.  Differentiable w.r.t. q, k and v; bit-identical from run to run.  A row with every key
    masked gives NaN, as in torch."""
    _need_fp32_cuda(q=q, k=k, v=v)
    if q.dim() != 3 or k.dim() != 3 or tuple(k.shape) != tuple(v.shape) or tuple(k.shape[1:]) != tuple(q.shape[1:]):
        raise RuntimeError(f'q must be [Q,B,E] and k, v [S,B,E], got {list(q.shape)}, {list(k.shape)}, {list(v.shape)}')
    Q, B, E = (int(s) for s in q.shape)
    S, M = int(k.shape[0]), int(num_heads)
    _unsupported(E, M)
    if Q < 1 or S < 1 or B < 1:
        raise RuntimeError(f'masked_attention takes at least one query, key and image, got Q={Q}, S={S}, B={B}')
    bits, per_head = None, False
    if mask is not None:
        if not isinstance(mask, PackedAttnMask):
            raise NotImplementedError('mask must be a PackedAttnMask (attn_mask_bits / pack_attn_mask) or None')
        rows = B * M if mask.per_head else B
        bits, per_head = mask.bits, mask.per_head
        if not per_head and int(bits.shape[0]) == 1 and B > 1:
            bits = bits.expand(B, -1, -1)
        if mask.S != S or tuple(bits.shape) != (rows, Q, (S + 31) // 32) or bits.dtype != torch.int32 or bits.device != q.device:
            raise RuntimeError(f'the mask is {mask} for {mask.S} keys; q, k give rows={rows}, Q={Q}, S={S} on {q.device}')
        bits = bits.contiguous()
    return _MaskedAttention.apply(q, k, v, bits, per_head, M, math.sqrt(1.0 / (E // M)))


@ATTENTION.register_module()
class MultiheadAttention(nn.Module):
    """mmcv's ``MultiheadAttention``: same constructor, state-dict keys (``attn.in_proj_weight``, ``attn.in_proj_bias``,
    ``attn.out_proj.weight``, ``attn.out_proj.bias``) and ``forward``.  ``self.attn`` is a ``torch.nn.MultiheadAttention`` that holds the
    parameters and their initialisation and is never called: the projections are ``F.linear``, the core is the HIP kernel."""

    def __init__(self, embed_dims, num_heads, attn_drop=0., proj_drop=0., dropout_layer=dict(type='Dropout', drop_prob=0.), init_cfg=None,
                 batch_first=False, **kwargs):
        super().__init__()
        _unsupported(embed_dims, num_heads)
        if kwargs.get('kdim', embed_dims) != embed_dims or kwargs.get('vdim', embed_dims) != embed_dims or kwargs.get('add_bias_kv') or \
                kwargs.get('add_zero_attn') or not kwargs.get('bias', True):
            raise NotImplementedError(f'kdim / vdim / add_bias_kv / add_zero_attn / bias=False are not built, got {kwargs}')
        self.embed_dims, self.num_heads, self.batch_first, self.init_cfg = embed_dims, num_heads, batch_first, init_cfg
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
        self.proj_drop = nn.Dropout(proj_drop)
        if dropout_layer:
            cfg = dict(dropout_layer)
            if cfg.pop('type', None) != 'Dropout':
                raise NotImplementedError(f'dropout_layer {dropout_layer}: only type="Dropout" is built')
            self.dropout_layer = nn.Dropout(cfg.pop('drop_prob', 0.5), **cfg)
        else:
            self.dropout_layer = nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None, key_padding_mask=None, **kwargs):
        """``query [Q,B,C]``, ``key`` and ``value [S,B,C]`` (``[B,.,C]`` with batch_first); ``attn_mask`` a ``PackedAttnMask``, a bool tensor
        ``[B*num_heads,Q,S]`` or ``[Q,S]`` (True = masked), or None.  Returns ``identity + dropout_layer(proj_drop(attention))``."""
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
            key_pos = query_pos
        if key_padding_mask is not None:
            raise NotImplementedError('key_padding_mask is not built')
        if self.training and self.attn.dropout > 0:
            raise NotImplementedError('attention dropout (attn_drop > 0 in training mode) is not built')
        if attn_mask is not None and not isinstance(attn_mask, PackedAttnMask) and \
                (not isinstance(attn_mask, torch.Tensor) or attn_mask.dtype != torch.bool):
            raise NotImplementedError(f'only bool attention masks are built, got {getattr(attn_mask, "dtype", type(attn_mask))}')
        _need_fp32_cuda(query=query, key=key, value=value, query_pos=query_pos, key_pos=key_pos)
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
        E = self.embed_dims
        w, b = self.attn.in_proj_weight, self.attn.in_proj_bias
        q = F.linear(query, w[:E], b[:E])
        k = F.linear(key, w[E:2 * E], b[E:2 * E])
        v = F.linear(value, w[2 * E:], b[2 * E:])
        if isinstance(attn_mask, torch.Tensor):
            attn_mask = pack_attn_mask(attn_mask, self.num_heads)
        out = masked_attention(q, k, v, attn_mask, self.num_heads)
        out = F.linear(out, self.attn.out_proj.weight, self.attn.out_proj.bias)
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))
