"""Multi-scale deformable attention on the HIP kernels of ``csrc/msda.hip`` (include/boxinst/boxinst_hip_msda.h).

    multi_scale_deformable_attn        <-> mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttnFunction.apply (the plain form)
    multi_scale_deformable_attn_fused  : reference points, raw offsets and raw logits; the normaliser and the softmax run in the kernel
    MultiScaleDeformableAttention      <-> mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttention, the self-attention of every
                                           layer of Box2Mask's MSDeformAttnPixelDecoder (msdeformattn_pixel_decoder.py:48-67)

mmcv's arithmetic is restated from its documented algorithm and is unpinned: mmcv never ran next to this library (INTEGRATION.md,
Level 3i).  Thin marshalling only: there is no CPU and no torch path for the sampling; everything is fp32 at the ABI, half precision raises.
"""
from __future__ import annotations

import functools
import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import current_stream, need_cuda
from .registry import ATTENTION


def _levels(spatial_shapes, level_start_index, S, device):
    """The two level tensors as the ABI takes them: int64, contiguous, on the device.  Given on the host they are checked against S here;
    given on the device they are NOT read back (no synchronisation): the kernels bound every index by S themselves."""
    ss, ls = torch.as_tensor(spatial_shapes), torch.as_tensor(level_start_index)
    if ss.dim() != 2 or ss.shape[1] != 2 or ss.dtype.is_floating_point:
        raise RuntimeError(f'spatial_shapes must be an integer [L,2] as (H, W), got {ss.dtype} {list(ss.shape)}')
    L = int(ss.shape[0])
    if tuple(ls.shape) != (L,) or ls.dtype.is_floating_point:
        raise RuntimeError(f'level_start_index must be an integer [{L}], got {ls.dtype} {list(ls.shape)}')
    if not ss.is_cuda:
        hw = [(int(h), int(w)) for h, w in ss.tolist()]
        if any(h < 1 or w < 1 for h, w in hw):
            raise RuntimeError(f'spatial_shapes must be positive, got {hw}')
        if sum(h * w for h, w in hw) != S:
            raise RuntimeError(f'value has {S} positions, spatial_shapes {hw} add up to {sum(h * w for h, w in hw)}')
    if not ls.is_cuda and not ss.is_cuda:
        starts, at = [int(v) for v in ls.tolist()], 0
        for (h, w), st in zip(hw, starts):
            if st != at:
                raise RuntimeError(f'level_start_index {starts} is not the running sum of spatial_shapes {hw}')
            at += h * w
    return ss.to(device=device, dtype=torch.int64).contiguous(), ls.to(device=device, dtype=torch.int64).contiguous(), L


def _check(value, a, offsets, w, fused):
    tensors = dict(value=value, reference_points=a, sampling_offsets=offsets, attention_logits=w) if fused else \
        dict(value=value, sampling_locations=a, attention_weights=w)
    need_cuda(**tensors)
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise RuntimeError(f'{name} must be float32, got {t.dtype}: half precision is not built')
        if t.device != value.device:
            raise RuntimeError(f'{name} must be on the device of value')
    if value.dim() != 4:
        raise RuntimeError(f'value must be [B,S,M,D], got {list(value.shape)}')
    B, S, M, D = (int(s) for s in value.shape)
    return B, S, M, D


def _unsupported(M, D, L, P):
    if D < _lib.MSDA_MIN_HEAD_DIM or D > _lib.MSDA_MAX_HEAD_DIM or D & (D - 1) or not 1 <= L <= _lib.MSDA_MAX_LEVELS or \
            not 1 <= P <= _lib.MSDA_MAX_POINTS:
        raise NotImplementedError(
            f'multi-scale deformable attention is built for a head dimension that is a power of two in {_lib.MSDA_MIN_HEAD_DIM}..'
            f'{_lib.MSDA_MAX_HEAD_DIM}, 1..{_lib.MSDA_MAX_LEVELS} levels and 1..{_lib.MSDA_MAX_POINTS} points; got D={D}, L={L}, P={P}')


_status = functools.partial(_lib.check_supported, header='boxinst_hip_msda.h')


class _MSDA(torch.autograd.Function):
    """flags = 0: (value, shapes, starts, sampling_locations, None, attention_weights); flags = MSDA_FUSED: (value, shapes, starts,
    reference_points, sampling_offsets, attention_logits)."""

    @staticmethod
    def forward(ctx, value, shapes, starts, a, offsets, w, dims, flags):
        B, S, M, D, Q, L, P = dims
        v, a_, w_ = value.detach().contiguous(), a.detach().contiguous(), w.detach().contiguous()
        o_ = offsets.detach().contiguous() if offsets is not None else None
        out = torch.empty((B, Q, M * D), dtype=torch.float32, device=value.device)
        with torch.cuda.device(value.device):
            _status('bxi_msda_forward_f32', _lib.load().bxi_msda_forward_f32(
                v.data_ptr(), shapes.data_ptr(), starts.data_ptr(), a_.data_ptr(), o_.data_ptr() if o_ is not None else None, w_.data_ptr(),
                B, S, M, D, Q, L, P, flags, out.data_ptr(), current_stream(value.device)))
        ctx.save_for_backward(v, shapes, starts, a_, o_, w_)
        ctx.dims, ctx.flags = dims, flags
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        v, shapes, starts, a, o, w = ctx.saved_tensors
        B, S, M, D, Q, L, P = ctx.dims
        lib, dev = _lib.load(), v.device
        g = g.contiguous()
        nbytes = lib.bxi_msda_backward_workspace_bytes(B, S, M, D, Q, L, P)
        if nbytes == 0:
            raise NotImplementedError(f'the backward takes Q * L * P < {_lib.MSDA_MAX_CELL_SAMPLES}, got {Q * L * P}')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        g_value = torch.empty((B, S, M, D), dtype=torch.float32, device=dev)
        g_a = torch.empty((B, Q, M, L, P, 2), dtype=torch.float32, device=dev)
        g_w = torch.empty(tuple(w.shape), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _status('bxi_msda_backward_f32', lib.bxi_msda_backward_f32(
                g.data_ptr(), v.data_ptr(), shapes.data_ptr(), starts.data_ptr(), a.data_ptr(), o.data_ptr() if o is not None else None, w.data_ptr(),
                B, S, M, D, Q, L, P, ctx.flags, g_value.data_ptr(), g_a.data_ptr(), g_w.data_ptr(), ws.data_ptr(), ws.numel(), current_stream(dev)))
        if ctx.flags & _lib.MSDA_FUSED:
            # loc = ref + off / (W, H): the reference point of (b, q, l) takes the location gradients of its M * P samples, which the kernel
            # wrote divided by (W, H)
            g_ref = None
            if ctx.needs_input_grad[3]:
                wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(torch.float32)
                g_ref = (g_a * wh[None, None, None, :, None, :]).sum(dim=(2, 4))
            return g_value, None, None, g_ref, g_a, g_w, None, None
        return g_value, None, None, g_a, None, g_w, None, None


def multi_scale_deformable_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
    """mmcv's ``MultiScaleDeformableAttnFunction.apply``, same argument order: ``value [B,S,M,D]``, ``spatial_shapes [L,2]`` as (H, W),
    ``level_start_index [L]``, ``sampling_locations [B,Q,M,L,P,2]`` as (x, y) in [0, 1], ``attention_weights [B,Q,M,L,P]`` ->
    ``[B,Q,M*D]``; differentiable w.r.t. value, locations and weights, bit-identical from run to run.  ``im2col_step`` is accepted and
    ignored.  fp32 only; a head dimension, level or point count outside the support set raises ``NotImplementedError``."""
    B, S, M, D = _check(value, sampling_locations, None, attention_weights, False)
    if sampling_locations.dim() != 6 or sampling_locations.shape[-1] != 2 or int(sampling_locations.shape[0]) != B or int(sampling_locations.shape[2]) != M:
        raise RuntimeError(f'sampling_locations must be [{B},Q,{M},L,P,2], got {list(sampling_locations.shape)}')
    Q, L, P = int(sampling_locations.shape[1]), int(sampling_locations.shape[3]), int(sampling_locations.shape[4])
    if tuple(attention_weights.shape) != (B, Q, M, L, P):
        raise RuntimeError(f'attention_weights must be [{B},{Q},{M},{L},{P}], got {list(attention_weights.shape)}')
    shapes, starts, nl = _levels(spatial_shapes, level_start_index, S, value.device)
    if nl != L:
        raise RuntimeError(f'spatial_shapes has {nl} levels, sampling_locations {L}')
    _unsupported(M, D, L, P)
    return _MSDA.apply(value, shapes, starts, sampling_locations, None, attention_weights, (B, S, M, D, Q, L, P), 0)


def multi_scale_deformable_attn_fused(value, spatial_shapes, level_start_index, reference_points, sampling_offsets, attention_logits):
    """The same attention from what the module's linear layers give: ``reference_points [B,Q,L,2]``, raw ``sampling_offsets
    [B,Q,M,L,P,2]``, raw ``attention_logits [B,Q,M,L*P]``.  The kernel forms ``ref + off / (W_l, H_l)`` and the softmax over the L*P logits
    itself; neither the locations nor the weights are stored.  Differentiable w.r.t. value, offsets, logits and reference points."""
    B, S, M, D = _check(value, reference_points, sampling_offsets, attention_logits, True)
    if sampling_offsets.dim() != 6 or sampling_offsets.shape[-1] != 2 or int(sampling_offsets.shape[0]) != B or int(sampling_offsets.shape[2]) != M:
        raise RuntimeError(f'sampling_offsets must be [{B},Q,{M},L,P,2], got {list(sampling_offsets.shape)}')
    Q, L, P = int(sampling_offsets.shape[1]), int(sampling_offsets.shape[3]), int(sampling_offsets.shape[4])
    if tuple(reference_points.shape) != (B, Q, L, 2):
        raise RuntimeError(f'reference_points must be [{B},{Q},{L},2], got {list(reference_points.shape)}')
    if tuple(attention_logits.shape) != (B, Q, M, L * P):
        raise RuntimeError(f'attention_logits must be [{B},{Q},{M},{L * P}], got {list(attention_logits.shape)}')
    shapes, starts, nl = _levels(spatial_shapes, level_start_index, S, value.device)
    if nl != L:
        raise RuntimeError(f'spatial_shapes has {nl} levels, sampling_offsets {L}')
    _unsupported(M, D, L, P)
    return _MSDA.apply(value, shapes, starts, reference_points, sampling_offsets, attention_logits, (B, S, M, D, Q, L, P), _lib.MSDA_FUSED)


@ATTENTION.register_module()
class MultiScaleDeformableAttention(nn.Module):
    """mmcv's ``MultiScaleDeformableAttention``: same constructor, state-dict keys (``sampling_offsets``, ``attention_weights``,
    ``value_proj``, ``output_proj``), ``init_weights`` and ``forward``.  The four linear layers, the padding mask, the dropout and the
    residual are torch ops; the sampling is the HIP kernel.  ``reference_points[..., 2]`` takes the fused path, ``[..., 4]`` (boxes) forms
    the locations with torch ops and takes the plain path.  ``norm_cfg`` and ``init_cfg`` are kept and unused, as in mmcv."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False, norm_cfg=None,
                 init_cfg=None):
        super().__init__()
        if embed_dims % num_heads != 0:
            raise ValueError(f'embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}')
        _unsupported(num_heads, embed_dims // num_heads, num_levels, num_points)
        self.norm_cfg, self.init_cfg = norm_cfg, init_cfg
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.im2col_step, self.embed_dims, self.num_levels, self.num_heads, self.num_points = im2col_step, embed_dims, num_levels, num_heads, num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.init_weights()

    def init_weights(self):
        """mmcv's: zero offset weights with the directional grid in the bias (head h looks along angle 2 pi h / M, point i at distance
        i + 1), zero attention weights and bias, xavier-uniform projections with zero bias."""
        with torch.no_grad():
            self.sampling_offsets.weight.zero_()
            thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
            grid = torch.stack([thetas.cos(), thetas.sin()], -1)
            grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(self.num_heads, 1, 1, 2).repeat(1, self.num_levels, self.num_points, 1)
            for i in range(self.num_points):
                grid[:, :, i, :] *= i + 1
            self.sampling_offsets.bias.copy_(grid.view(-1))
            self.attention_weights.weight.zero_()
            self.attention_weights.bias.zero_()
            for proj in (self.value_proj, self.output_proj):
                nn.init.xavier_uniform_(proj.weight, gain=1)
                proj.bias.zero_()
        self._is_init = True

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None, reference_points=None,
                spatial_shapes=None, level_start_index=None, **kwargs):
        """``query [Q,B,C]`` (``[B,Q,C]`` with batch_first), ``value`` likewise with S positions (the query when None), ``reference_points
        [B,Q,L,2]`` in [0, 1] or ``[B,Q,L,4]`` boxes, ``key_padding_mask [B,S]``.  ``key`` and further keyword arguments (key_pos, attn_mask,
        valid_radios of BaseTransformerLayer) are ignored."""
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if reference_points is None or spatial_shapes is None or level_start_index is None:
            raise RuntimeError('reference_points, spatial_shapes and level_start_index are required')
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        bs, num_query, _ = query.shape
        num_value = int(value.shape[1])
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        value = value.view(bs, num_value, self.num_heads, -1)
        offsets = self.sampling_offsets(query).view(bs, num_query, self.num_heads, self.num_levels, self.num_points, 2)
        logits = self.attention_weights(query).view(bs, num_query, self.num_heads, self.num_levels * self.num_points)
        if reference_points.shape[-1] == 2:
            output = multi_scale_deformable_attn_fused(value, spatial_shapes, level_start_index, reference_points, offsets, logits)
        elif reference_points.shape[-1] == 4:
            weights = logits.softmax(-1).view(bs, num_query, self.num_heads, self.num_levels, self.num_points)
            locations = reference_points[:, :, None, :, None, :2] + offsets / self.num_points * reference_points[:, :, None, :, None, 2:] * 0.5
            output = multi_scale_deformable_attn(value, spatial_shapes, level_start_index, locations, weights, self.im2col_step)
        else:
            raise ValueError(f'Last dim of reference_points must be 2 or 4, but get {reference_points.shape[-1]} instead.')
        output = self.output_proj(output)
        if not self.batch_first:
            output = output.permute(1, 0, 2)
        return self.dropout(output) + identity
