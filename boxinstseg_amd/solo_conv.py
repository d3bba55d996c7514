"""The dynamic 1x1 mask convolution of the SOLOv2-style heads (csrc/solo_dconv.hip, include/boxinst/boxinst_hip_dconv.h): the step between
the training targets and the mask losses, and between the candidates and Matrix NMS.

    solo_dynamic_masks       <-> DiscoBoxSOLOv2Head.loss, discobox_head.py:1180-1246 and the sigmoid at :1275-1279 (corr_loss :936-1022 is the
                                 same block): kernel_pred.view(E, -1)[:, grid_order], one F.conv2d per (level, image), the cats, the sigmoid
    solo_dynamic_masks_pair  the student's and the teacher's maps with one grid_order (use_ind_teacher=True), the teacher without a backward
    solo_candidate_masks     <-> get_seg_single, discobox_head.py:1607-1608: F.conv2d(seg_preds, kernel_preds[rows]).sigmoid()

There is no CPU or PyTorch fallback: CPU tensors raise.  The kernel values are gathered by the library (torch makes no [N,E] copy), the feature of
an image is read once per call, and all levels and images are one call forward (a small gather of the kernel values into scratch and ONE
launch for the product) and one call backward (the gather, the main kernel, the reduction of grad_kernel's per-tile sums and the pass that
writes every element of every gradient map).  Around the call torch concatenates the grid_order entries into one int64 vector and zeroes
the status word.  Two precisions, chosen with ``compute``:

    compute='fp32' (default)  every operand fp32 -- half-precision tensors are upcast here and the masks are fp32; every logit is one
                              fp32 fmaf chain over e ascending.  DEVIATION from the reference, which runs these statements under fp16
                              autocast: its own precision is ``compute='half'``.
    compute='half'            csrc/solo_dconv16.hip, include/boxinst/boxinst_hip_dconv16.h: fp16 or bf16 tensors read in place (no upcast
                              copy, no cast of the gradients), fp32 accumulation on v_mfma_f32_32x32x16_{f16,bf16}, masks in the inputs'
                              dtype as autocast gives them (or fp32 with ``out_dtype=torch.float32``), gradients in the inputs' dtype.
                              fp32 or mixed input raises: there is no silent cast.
"""
from __future__ import annotations

import types

import torch

from . import _lib
from ._common import current_stream, need_cuda

__all__ = ['solo_dynamic_masks', 'solo_dynamic_masks_pair', 'solo_candidate_masks']


_HALF = {torch.float16: _lib.DCONV16_F16, torch.bfloat16: _lib.DCONV16_BF16}


def _family(plan, feat):
    """The entry points of the feature's precision: their common prefix, the suffix of the two calls, and what the half family's calls
    take beyond the fp32 family's -- the dtype code after ``feat`` and the masks' dtype code after ``out`` / ``grad_out``."""
    if feat.dtype in _HALF:
        code = _HALF[feat.dtype]
        return 'bxi_solo_dconv16', '', (code,), (_lib.DCONV16_OUT_F32 if plan.out_dtype == torch.float32 else code,)
    return 'bxi_solo_dconv', '_f32', (), ()


def _call_forward(plan, feat, maps):
    lib = _lib.load()
    dev = feat.device
    B, E, H, W = feat.shape
    fam, suffix, dtype_code, out_code = _family(plan, feat)
    out = torch.empty((plan.N, H, W), dtype=plan.out_dtype, device=dev)
    img = torch.empty((plan.N,), dtype=torch.int64, device=dev)
    ws_bytes = getattr(lib, fam + '_forward_workspace_bytes')(plan.N, B, E)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    name = fam + '_forward' + suffix
    with torch.cuda.device(dev):
        _lib.check(name, getattr(lib, name)(
            feat.data_ptr(), *dtype_code, B, E, H, W, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), len(maps),
            plan.layout, None if plan.cells is None else plan.cells.data_ptr(), _lib.int_array(plan.counts), plan.N, plan.act, out.data_ptr(),
            *out_code, img.data_ptr(), plan.status.data_ptr(), ws.data_ptr(), ws_bytes, current_stream(dev)))
    return out, img


def _backward(ctx, g_out, g_dtype, feat, maps, ws_bytes, call):
    """The backward of an autograd function over ``(plan, feat, *maps)``: which gradients are wanted, their buffers, the workspace of
    ``ws_bytes(lib)`` bytes and the tuple autograd expects.  ``call(lib, g, g_feat, g_maps, ws, ws_bytes, stream)`` runs the library on
    the pointers (None for a gradient nobody wants); box_solo_masks uses it too."""
    need_feat, need_maps = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
    if not (need_feat or need_maps):
        return (None, None) + (None,) * len(maps)
    lib = _lib.load()
    dev = feat.device
    g = g_out.detach().to(g_dtype).contiguous()                            # autograd hands it over in the masks' dtype: no copy
    g_feat = torch.empty_like(feat) if need_feat else None
    g_maps = [torch.empty_like(m) for m in maps] if need_maps else None
    nbytes = ws_bytes(lib)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        call(lib, g.data_ptr(), None if g_feat is None else g_feat.data_ptr(),
             None if g_maps is None else _lib.ptr_array([m.data_ptr() for m in g_maps]), ws.data_ptr(), nbytes, current_stream(dev))
    grads = [gm if need else None for gm, need in zip(g_maps, ctx.needs_input_grad[2:])] if need_maps else [None] * len(maps)
    return (None, g_feat, *grads)


class _DynamicMasks(torch.autograd.Function):
    """Both precisions: fp32 tensors, or (``compute='half'``) the half tensors as they are, the masks in ``plan.out_dtype``, the gradients
    in the inputs' dtype."""

    @staticmethod
    def forward(ctx, plan, feat, *maps):
        out, img = _call_forward(plan, feat, maps)
        ctx.plan = plan
        ctx.save_for_backward(feat, out, *maps)
        ctx.mark_non_differentiable(img)
        return out, img

    @staticmethod
    def backward(ctx, g_out, _g_img):
        plan = ctx.plan
        feat, out, *maps = ctx.saved_tensors
        B, E, H, W = feat.shape
        fam, suffix, dtype_code, out_code = _family(plan, feat)
        name = fam + '_backward' + suffix

        def call(lib, g, g_feat, g_maps, ws, ws_bytes, stream):
            _lib.check(name, getattr(lib, name)(
                feat.data_ptr(), *dtype_code, B, E, H, W, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), len(maps),
                plan.layout, None if plan.cells is None else plan.cells.data_ptr(), _lib.int_array(plan.counts), plan.N, plan.act,
                out.data_ptr(), g, *out_code, g_feat, g_maps, plan.status.data_ptr(), ws, ws_bytes, stream))

        return _backward(ctx, g_out, out.dtype, feat, maps,
                         lambda lib: getattr(lib, fam + '_backward_workspace_bytes')(plan.N, B, E, H, W), call)


def _fp32(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def _plan(kernel_preds_raw, grid_order, ins_pred, sigmoid, status):
    """The segment table of one grid_order: counts on the host, the cells as one int64 vector on the device, level-major."""
    grid_order = getattr(grid_order, 'grid_order', grid_order)
    maps = list(kernel_preds_raw)
    need_cuda(ins_pred=ins_pred, **{f'kernel_preds_raw[{l}]': m for l, m in enumerate(maps)})
    if ins_pred.dim() != 4:
        raise RuntimeError(f'ins_pred must be [B,E,H,W], got {tuple(ins_pred.shape)}')
    B, E = int(ins_pred.shape[0]), int(ins_pred.shape[1])
    L = len(maps)
    if not 1 <= L <= _lib.DCONV_MAX_LEVELS:
        raise RuntimeError(f'{L} levels: 1 .. {_lib.DCONV_MAX_LEVELS} are supported')
    if len(grid_order) != L or any(len(g) != B for g in grid_order):
        raise RuntimeError(f'grid_order must be [level][image] = [{L}][{B}]')
    for l, m in enumerate(maps):
        if m.dim() != 4 or m.shape[0] != B or m.shape[1] != E or m.shape[2] != m.shape[3] or m.device != ins_pred.device:
            raise RuntimeError(f'kernel_preds_raw[{l}] must be [{B},{E},S,S] on {ins_pred.device}, got {tuple(m.shape)} on {m.device}')
    flat = [grid_order[l][b].reshape(-1) for l in range(L) for b in range(B)]
    need_cuda(**{f'grid_order[{i // B}][{i % B}]': g for i, g in enumerate(flat)})
    counts = [int(g.numel()) for g in flat]
    N = sum(counts)
    cells = torch.cat(flat).to(torch.int64).contiguous() if N else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=ins_pred.device)
    return types.SimpleNamespace(layout=_lib.DCONV_MAPS, grids=[int(m.shape[2]) for m in maps], counts=counts, cells=cells, N=N,
                                 act=_lib.DCONV_SIGMOID if sigmoid else _lib.DCONV_NONE, status=status, L=L, B=B, out_dtype=torch.float32)


def _lists(plan, out, img):
    """The reference's two lists: per level the masks of its images concatenated and their image indices, None for a level without rows."""
    masks, inds, at = [], [], 0
    for l in range(plan.L):
        n = sum(plan.counts[l * plan.B:(l + 1) * plan.B])
        masks.append(out[at:at + n] if n else None)
        inds.append(img[at:at + n] if n else None)
        at += n
    return masks, inds


def _run(plan, kernel_preds_raw, ins_pred, compute='fp32', out_dtype=None):
    if compute == 'half':                                                  # the tensors as they are; fp32 plans keep their fp32 masks
        plan.out_dtype = out_dtype or ins_pred.dtype
        out, img = _DynamicMasks.apply(plan, ins_pred.contiguous(), *[m.contiguous() for m in kernel_preds_raw])
    else:
        out, img = _DynamicMasks.apply(plan, _fp32(ins_pred), *[_fp32(m) for m in kernel_preds_raw])
    return _lists(plan, out, img)


def _dynamic_rows(kernel_preds_raw, grid_order, ins_pred, sigmoid=True, status=None, cells=None):
    """The fp32 row buffer itself, for callers inside the package (discobox_loss): ``(rows [N,H,W], img_inds [N], rows per level, cells)``, level-major --
    what ``solo_dynamic_masks`` slices into its per-level views.  ``cells``: the cell vector of an earlier call with the same ``grid_order``."""
    kernel_preds_raw = list(kernel_preds_raw)
    plan = _plan(kernel_preds_raw, grid_order, ins_pred, sigmoid, status)
    if cells is not None:
        plan.cells = cells
    out, img = _DynamicMasks.apply(plan, _fp32(ins_pred), *[_fp32(m) for m in kernel_preds_raw])
    return out, img, [sum(plan.counts[l * plan.B:(l + 1) * plan.B]) for l in range(plan.L)], plan.cells


def _check_compute(compute, out_dtype, **tensors):
    """``compute`` is 'fp32' or 'half'; with 'half' every tensor is of ONE half dtype (checked before anything else, so that it is said
    without a device) and ``out_dtype`` is None, that dtype or torch.float32; with 'fp32' the masks are fp32."""
    if compute not in ('fp32', 'half'):
        raise ValueError(f"compute must be 'fp32' or 'half', got {compute!r}")
    if compute == 'fp32':
        if out_dtype not in (None, torch.float32):
            raise RuntimeError(f"compute='fp32' returns fp32 masks, got out_dtype={out_dtype}")
        return
    dtypes = {name: t.dtype for name, t in tensors.items() if t is not None}
    first = next(iter(dtypes.values()))
    if first not in _HALF or any(d != first for d in dtypes.values()):
        raise RuntimeError("compute='half' takes tensors of one half dtype, torch.float16 or torch.bfloat16, and casts nothing: got "
                           + ', '.join(f'{n} {d}' for n, d in dtypes.items()))
    if out_dtype not in (None, first, torch.float32):
        raise RuntimeError(f"compute='half' returns masks in the inputs' dtype {first} or in torch.float32, got out_dtype={out_dtype}")


def solo_dynamic_masks(kernel_preds_raw, grid_order, ins_pred, sigmoid=True, status=None, compute='fp32', out_dtype=None):
    """The masks of the assigned grid cells.  ``kernel_preds_raw``: a list over levels of [B,E,S,S]; ``grid_order``: ``SoloTargets.grid_order``
    ([level][image] int64 on the device, sizes known on the host) or the ``SoloTargets`` object; ``ins_pred`` [B,E,H,W].  Returns
    ``(masks, img_inds)``: per level the fp32 masks [N_l,H,W] of its images concatenated in order (``sigmoid`` of the logits, or the logits) and
    the int64 image index of every mask on the device, as ``meanfield_forward`` takes it; ``None`` for a level without instances.  All masks are
    views of one [N,H,W] buffer.  Gradients reach the kernel maps and ``ins_pred`` where they require them: every element of a map gets one,
    zero for a cell nobody selected and the sum of its rows' for a cell ``grid_order`` names more than once.  A cell outside its map gives the
    masks of an all-zero kernel and sets ``status[0]`` (int32 [1] on the device, a fresh zero when not given) to 1; nothing reads it back
    here.  ``compute='half'``: fp16 or bf16 tensors read in place (the module's docstring); the masks are then of the inputs' dtype, or fp32
    with ``out_dtype=torch.float32``."""
    kernel_preds_raw = list(kernel_preds_raw)
    _check_compute(compute, out_dtype, ins_pred=ins_pred, **{f'kernel_preds_raw[{l}]': m for l, m in enumerate(kernel_preds_raw)})
    plan = _plan(kernel_preds_raw, grid_order, ins_pred, sigmoid, status)
    return _run(plan, kernel_preds_raw, ins_pred, compute, out_dtype)


def solo_dynamic_masks_pair(s_kernel_preds_raw, t_kernel_preds_raw, grid_order, s_ins_pred, t_ins_pred, sigmoid=True, status=None,
                            compute='fp32', out_dtype=None):
    """``solo_dynamic_masks`` for the student and for the independent teacher with one ``grid_order``: the call ``loss`` and ``corr_loss``
    make.  The teacher runs without a backward (its tensors are detached).  Returns ``(s_masks, t_masks, img_inds)``.  Nothing is kept from
    one call to the next.  ``compute`` and ``out_dtype`` as in ``solo_dynamic_masks``, for both legs: all tensors of one half dtype."""
    s_kernel_preds_raw, t_kernel_preds_raw = list(s_kernel_preds_raw), list(t_kernel_preds_raw)
    _check_compute(compute, out_dtype, s_ins_pred=s_ins_pred, t_ins_pred=t_ins_pred,
                   **{f's_kernel_preds_raw[{l}]': m for l, m in enumerate(s_kernel_preds_raw)},
                   **{f't_kernel_preds_raw[{l}]': m for l, m in enumerate(t_kernel_preds_raw)})
    plan = _plan(s_kernel_preds_raw, grid_order, s_ins_pred, sigmoid, status)
    t_plan = _plan(t_kernel_preds_raw, grid_order, t_ins_pred, sigmoid, plan.status)
    t_plan.cells = plan.cells
    s_masks, inds = _run(plan, s_kernel_preds_raw, s_ins_pred, compute, out_dtype)
    with torch.no_grad():
        t_masks, _ = _run(t_plan, [m.detach() for m in t_kernel_preds_raw], t_ins_pred.detach(), compute, out_dtype)
    return s_masks, t_masks, inds


def solo_candidate_masks(seg_pred, kernel_preds, rows=None, sigmoid=True, status=None, compute='fp32', out_dtype=None):
    """``F.conv2d(seg_pred, kernel_preds[rows].view(I, E, 1, 1)).squeeze(0).sigmoid()`` of get_seg_single: ``seg_pred`` [1,E,h,w] the mask
    feature, ``kernel_preds`` [sum(grid^2),E] read in place through ``rows`` (int64 [I] on the device, any order, repeats allowed; every row
    when None).  Returns [I,h,w] fp32 probabilities (logits with ``sigmoid=False``), ready for ``seg_nms``.  No gradient.
    ``compute='half'``: fp16 or bf16 ``seg_pred`` and ``kernel_preds`` read in place, fp32 accumulation, the result in their dtype or, with
    ``out_dtype=torch.float32``, in fp32."""
    _check_compute(compute, out_dtype, seg_pred=seg_pred, kernel_preds=kernel_preds)
    need_cuda(seg_pred=seg_pred, kernel_preds=kernel_preds, rows=rows)
    if seg_pred.dim() != 4 or seg_pred.shape[0] != 1 or kernel_preds.dim() != 2 or kernel_preds.shape[1] != seg_pred.shape[1]:
        raise RuntimeError(f'seg_pred must be [1,E,h,w] and kernel_preds [rows,E], got {tuple(seg_pred.shape)} and {tuple(kernel_preds.shape)}')
    if rows is not None and (rows.dim() != 1 or rows.dtype != torch.int64):
        raise RuntimeError(f'rows must be int64 [I], got {rows.dtype} {tuple(rows.shape)}')
    n = int(kernel_preds.shape[0]) if rows is None else int(rows.numel())
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=seg_pred.device)
    plan = types.SimpleNamespace(layout=_lib.DCONV_ROWS, grids=[max(int(kernel_preds.shape[0]), 1)], counts=[n], N=n,
                                 cells=None if rows is None else rows.contiguous(), act=_lib.DCONV_SIGMOID if sigmoid else _lib.DCONV_NONE,
                                 status=status, L=1, B=1, out_dtype=torch.float32)
    if compute == 'half':
        plan.out_dtype = out_dtype or seg_pred.dtype
        return _call_forward(plan, seg_pred.detach().contiguous(), [kernel_preds.detach().contiguous()])[0]
    return _call_forward(plan, _fp32(seg_pred.detach()), [_fp32(kernel_preds.detach())])[0]
