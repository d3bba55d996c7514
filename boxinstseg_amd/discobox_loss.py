"""``DiscoBoxSOLOv2Head.loss`` as one call (reference: ``mmdet/models/dense_heads/discobox_head.py`` :1143-1361, with the tail of
``corr_loss`` :1127-1137), on the kernels of ``csrc/discobox_loss.hip`` and the modules the package already has.

The reference loops over levels, and inside a level over images, twice: once in ``loss`` (mil term, mean field without
``inter_img_mask``, dice) and once in ``corr_loss`` (mean field with it, dice on the gamma-mixed student).  Each pass reads a row's
target on the host (``torch.tensor([t.sum() for t in target])``), indexes with boolean masks and runs one ``MeanField.forward`` per
(level, image).  Here the rows of all levels -- one row per assigned (level, image, cell), level-major, as
``solo_dynamic_masks_pair`` returns them -- go through ONE prepare launch, ONE launch per mean-field iteration for both legs, and the
dice terms read the labels as bits.  A row whose target is all zero stays in place and is not *live*: the means skip it.

Public:
  ``discobox_pseudo_losses``   per-row mil / ts / ts_corr terms, ``live`` and ``n_live`` of a row buffer; autograd w.r.t. ``s_rows``.
  ``discobox_loss``            the reference's dict: ``loss_ins``, ``loss_ts``, ``loss_cate``, ``loss_corr``.
  ``parse_discobox_loss_cfg``  ``bbox_head=dict(...)`` -> the settings of ``loss_ins`` / ``loss_ts`` / ``loss_corr`` read here.

Deviations from the reference, on purpose: all four losses are 0-dim (the reference returns shape ``[1]`` zeros when nothing is live);
no live row with ``use_corr`` gives zeros (the reference's ``torch.cat([])`` raises); the statement is fp32 (the reference runs under
autocast).  No CPU path; a shape outside the support set of ``include/boxinst/boxinst_hip_dbx.h`` raises ``NotImplementedError``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import cfg_get, cfg_require, current_stream, need_cuda
from .discobox import dice_loss, meanfield_kernel, mil_loss

_HEADER = 'boxinst_hip_dbx.h'


def _f32c(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def _unpack(ws, which, iters, R, H, W, legs):
    out = torch.empty((R, H, W), dtype=torch.uint8, device=ws.device)
    with torch.cuda.device(ws.device):
        _lib.check_supported('bxi_dbx_unpack_u8', _lib.load().bxi_dbx_unpack_u8(
            ws.data_ptr(), ws.numel(), which, iters, R, H, W, legs, out.data_ptr(), current_stream(ws.device)), _HEADER)
    return out


class _PseudoDice(torch.autograd.Function):
    """prepare + steps + dice forward; the backward is one launch over ``s_rows``."""

    @staticmethod
    def forward(ctx, s_rows, t_rows, target_rows, img_inds, kernel, meta, *iiu):
        iters, base, gamma, legs, level_rows, details = meta
        dev = s_rows.device
        R, H, W = (int(v) for v in s_rows.shape)
        B, K2 = int(kernel.shape[0]), int(kernel.shape[1])
        ks = int(round(K2 ** 0.5))
        lib = _lib.load()
        nbytes = lib.bxi_dbx_workspace_bytes(R, H, W, legs)
        if nbytes == 0:
            raise NotImplementedError(f'discobox_pseudo_losses: rows [{R},{H},{W}] are outside the support set of include/boxinst/{_HEADER}')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        live = torch.empty((max(R, 1),), dtype=torch.int32, device=dev)
        n_live = torch.empty((1,), dtype=torch.int32, device=dev)
        loss = torch.empty((legs, R), dtype=torch.float32, device=dev)
        sums = torch.empty((legs, max(R, 1), 2), dtype=torch.float64, device=dev)
        st = current_stream(dev)
        ptrs = _lib.ptr_array([0 if t is None else t.data_ptr() for t in iiu])
        firsts, at = [], 0
        for n in level_rows:
            firsts.append(at)
            at += int(n)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_dbx_prepare_f32', lib.bxi_dbx_prepare_f32(
                s_rows.data_ptr(), t_rows.data_ptr(), target_rows.data_ptr(), R, H, W, legs, live.data_ptr(), n_live.data_ptr(), ws.data_ptr(),
                ws.numel(), st), _HEADER)
            _lib.check_supported('bxi_dbx_steps_f32', lib.bxi_dbx_steps_f32(
                kernel.data_ptr(), B, H, W, ks, img_inds.data_ptr(), R, iters, base, gamma, legs, ptrs, _lib.int_array(firsts),
                len(firsts) if legs == 2 else 0, ws.data_ptr(), ws.numel(), st), _HEADER)
            _lib.check_supported('bxi_dbx_dice_forward_f32', lib.bxi_dbx_dice_forward_f32(
                s_rows.data_ptr(), R, H, W, legs, iters, gamma, ws.data_ptr(), ws.numel(), loss.data_ptr(), sums.data_ptr(), st), _HEADER)
        if details is not None:
            details.update(target=_unpack(ws, _lib.DBX_TARGET, iters, R, H, W, legs), enlarged=_unpack(ws, _lib.DBX_ENLARGED, iters, R, H, W, legs),
                           pseudo=_unpack(ws, _lib.DBX_LABEL, iters, R, H, W, legs),
                           pseudo_corr=_unpack(ws, _lib.DBX_LABEL + 1, iters, R, H, W, legs) if legs == 2 else None)
        ctx.save_for_backward(s_rows, ws, sums)
        ctx.meta = (R, H, W, legs, iters, gamma)
        live = live[:R]
        ctx.mark_non_differentiable(live, n_live)
        return loss, live, n_live

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_live, _g_n):
        s_rows, ws, sums = ctx.saved_tensors
        R, H, W, legs, iters, gamma = ctx.meta
        g_rows = _f32c(g_loss)
        g_s = torch.empty_like(s_rows)
        with torch.cuda.device(s_rows.device):
            _lib.check_supported('bxi_dbx_dice_backward_f32', _lib.load().bxi_dbx_dice_backward_f32(
                s_rows.data_ptr(), R, H, W, legs, iters, gamma, ws.data_ptr(), ws.numel(), sums.data_ptr(), g_rows.data_ptr(), g_s.data_ptr(),
                current_stream(s_rows.device)), _HEADER)
        return (g_s, None, None, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 6)


def discobox_pseudo_losses(s_rows, t_rows, target_rows, img_inds, kernel, iiu_levels=None, level_rows=None, *, iters, base, gamma=0.01,
                           details=None):
    """The per-row terms of the pseudo-label block for a row buffer.  ``s_rows`` / ``t_rows [R,H,W]`` fp32: the student's and the
    teacher's sigmoid masks (``t_rows`` may be ``s_rows``); ``target_rows [R,H,W]`` uint8; ``img_inds [R]``; ``kernel [B,k*k,H,W]``
    (``meanfield_kernel`` of the batch, k 3 or 5).  ``iiu_levels``: per level the ``[N_l,2,H,W]`` tensor ``corr_level`` returned, or
    ``None`` for a level without rows, with ``level_rows`` the rows per level (host ints, summing to R); ``None`` runs leg 0 alone.

    Returns ``(mil_rows, ts_rows, ts_corr_rows | None, live, n_live)``: ``mil_loss(dice_loss, s, s, target)`` (:1289),
    ``dice_loss(s * enlarged, pseudo)`` (:1300) and ``dice_loss(s e gamma + (s e).detach() (1 - gamma), pseudo_corr)`` (:1135-1137) per
    row, ``live [R]`` int32 (the row's target is not all zero, :1281-1286) and ``n_live [1]`` int32, both on the device.  Differentiable
    w.r.t. ``s_rows``.  ``details``: a dict that receives ``target``, ``enlarged``, ``pseudo``, ``pseudo_corr`` as uint8 ``[R,H,W]``."""
    need_cuda(s_rows=s_rows, t_rows=t_rows, target_rows=target_rows, img_inds=img_inds, kernel=kernel)
    if s_rows.dim() != 3 or tuple(t_rows.shape) != tuple(s_rows.shape) or tuple(target_rows.shape) != tuple(s_rows.shape):
        raise RuntimeError(f's_rows, t_rows and target_rows must be the same [R,H,W], got {list(s_rows.shape)}, {list(t_rows.shape)}, '
                           f'{list(target_rows.shape)}')
    for name, t in (('s_rows', s_rows), ('t_rows', t_rows), ('kernel', kernel)):
        if t.dtype != torch.float32:
            raise NotImplementedError(f'{name} is {t.dtype}: the rows are fp32 only (include/boxinst/{_HEADER})')
    if target_rows.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError(f'target_rows must be uint8, got {target_rows.dtype}')
    R, H, W = (int(v) for v in s_rows.shape)
    if kernel.dim() != 4 or tuple(kernel.shape[2:]) != (H, W) or int(kernel.shape[1]) not in (9, 25):
        raise NotImplementedError(f'kernel must be [B,9 or 25,{H},{W}], got {list(kernel.shape)}')
    if tuple(img_inds.shape) != (R,):
        raise RuntimeError(f'img_inds must be [{R}], got {list(img_inds.shape)}')
    if R > 65535:
        raise NotImplementedError(f'{R} rows: at most 65535 (include/boxinst/{_HEADER})')
    legs = 1 if iiu_levels is None else 2
    iiu, rows = [], []
    if legs == 2:
        iiu, rows = list(iiu_levels), [int(n) for n in (level_rows or [])]
        if len(iiu) != len(rows) or sum(rows) != R or not 1 <= len(rows) <= _lib.DBX_MAX_LEVELS:
            raise RuntimeError(f'iiu_levels ({len(iiu)}) and level_rows {rows} must name 1..{_lib.DBX_MAX_LEVELS} levels with {R} rows in all')
        for l, (t, n) in enumerate(zip(iiu, rows)):
            if t is None:
                continue
            need_cuda(**{f'iiu_levels[{l}]': t})
            if t.dtype != torch.float32 or tuple(t.shape) != (n, 2, H, W):
                raise RuntimeError(f'iiu_levels[{l}] must be fp32 [{n},2,{H},{W}], got {t.dtype} {list(t.shape)}')
        iiu = [None if t is None or t.numel() == 0 else t.detach().contiguous() for t in iiu]
    sc = s_rows.contiguous()
    tc = sc if t_rows is s_rows else t_rows.detach().contiguous()
    tg = target_rows.detach().contiguous().view(torch.uint8)
    img = img_inds.detach().to(torch.int64).contiguous()
    mil_rows = mil_loss(dice_loss, sc, sc, tg)
    ts, live, n_live = _PseudoDice.apply(sc, tc.detach(), tg, img, kernel.detach().contiguous(), (int(iters), float(base), float(gamma), legs, rows, details),
                                         *iiu)
    return mil_rows, ts[0], (ts[1] if legs == 2 else None), live, n_live


class _LiveMeans(torch.autograd.Function):
    """means[k] = sum_r live[r] rows_k[r] / max(n_live, 1); the backward is a per-row scale."""

    @staticmethod
    def forward(ctx, live, n_live, *rows):
        dev = live.device
        R, K = int(live.numel()), len(rows)
        rows = [_f32c(r.detach()) for r in rows]
        means = torch.empty((K,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check_supported('bxi_dbx_means_f32', _lib.load().bxi_dbx_means_f32(
                _lib.ptr_array([r.data_ptr() for r in rows]), K, live.data_ptr(), n_live.data_ptr(), R, means.data_ptr(), current_stream(dev)), _HEADER)
        ctx.save_for_backward(live, n_live)
        ctx.K = K
        return means

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        live, n_live = ctx.saved_tensors
        R, K = int(live.numel()), ctx.K
        g = _f32c(g)
        out = torch.empty((K, R), dtype=torch.float32, device=live.device)
        with torch.cuda.device(live.device):
            _lib.check_supported('bxi_dbx_means_backward_f32', _lib.load().bxi_dbx_means_backward_f32(
                g.data_ptr(), K, live.data_ptr(), n_live.data_ptr(), R, out.data_ptr(), current_stream(live.device)), _HEADER)
        return (None, None) + tuple(out[k] for k in range(K))


def live_means(live, n_live, *rows):
    """``sum_r live[r] rows_k[r] / max(n_live, 1)`` of every per-row array, as one fp32 ``[K]`` tensor (fp64 sums, a fixed order)."""
    if not 1 <= len(rows) <= _lib.DBX_MAX_MEANS:
        raise RuntimeError(f'1..{_lib.DBX_MAX_MEANS} per-row arrays, got {len(rows)}')
    need_cuda(live=live, n_live=n_live, **{f'rows[{k}]': r for k, r in enumerate(rows)})
    for k, r in enumerate(rows):
        if tuple(r.shape) != tuple(live.shape):
            raise RuntimeError(f'rows[{k}] must be {list(live.shape)}, got {list(r.shape)}')
    return _LiveMeans.apply(live.contiguous(), n_live.contiguous(), *rows)


def parse_discobox_loss_cfg(bbox_head_cfg):
    """``bbox_head=dict(type='DiscoBoxSOLOv2Head', loss_ins=..., loss_ts=..., loss_corr=...)`` (dict or namespace) -> ``dict(w_ins, w_ts,
    w_corr, kernel, max_iter, alpha0, theta0, theta1, theta2, base)``: what ``DiscoBoxSOLOv2Head.__init__`` (:700-713) reads for
    ``loss``.  The other keys of ``loss_ts`` (crf_height / crf_width / momentum / use_ind_teacher: the detector's) are ignored."""
    li, lt = cfg_get(bbox_head_cfg, 'loss_ins'), cfg_get(bbox_head_cfg, 'loss_ts')
    if li is None or lt is None:
        raise TypeError('bbox_head needs `loss_ins` and `loss_ts`')
    lc = cfg_get(bbox_head_cfg, 'loss_corr')
    kernel = int(cfg_require(lt, 'kernel'))
    if kernel not in (3, 5):
        raise NotImplementedError(f'loss_ts.kernel {kernel} is not supported: 3 or 5')
    base = float(cfg_require(lt, 'base'))
    if not 0.0 < base < 0.5:
        raise RuntimeError(f'loss_ts.base must be in (0, 0.5), got {base}')
    return dict(w_ins=float(cfg_require(li, 'loss_weight')), w_ts=float(cfg_require(lt, 'loss_weight')),
                w_corr=float(cfg_get(lc, 'loss_weight', 1.0)) if lc is not None else 1.0, kernel=kernel, max_iter=int(cfg_require(lt, 'max_iter')),
                alpha0=float(cfg_require(lt, 'alpha0')), theta0=float(cfg_require(lt, 'theta0')), theta1=float(cfg_require(lt, 'theta1')),
                theta2=float(cfg_require(lt, 'theta2')), base=base)


def discobox_loss(cate_preds, s_kernel_preds_raw, t_kernel_preds_raw, s_ins_pred, t_ins_pred, gt_bbox_list, gt_label_list, gt_mask_list,
                  img_metas, cfg, img, *, use_loss_ts, use_ind_teacher, use_corr, s_feat=None, t_feat=None, bank=None, solver=None, head_cfg,
                  details=None):
    """``DiscoBoxSOLOv2Head.loss`` (:1143-1361).  The tensors are the reference's; ``head_cfg`` is the ``bbox_head`` block of the config
    (dict or namespace); ``bank`` / ``solver``: the ``ObjectBank`` and ``SemanticCorrSolver`` of ``parse_corr_cfg`` (needed with
    ``use_corr``; the bank is updated in the reference's order); ``s_feat`` / ``t_feat``: the reference's lists, ``[0]`` is read.
    ``img_metas`` and ``cfg`` are accepted for the signature and not read.  Returns ``dict(loss_ins, loss_ts, loss_cate, loss_corr)``, all
    0-dim.  The only host synchronisation is the one inside ``solov2_targets``."""
    from .corr import parse_corr_cfg
    from .roi_align import corr_level
    from .solo_conv import _dynamic_rows
    from .solo_targets import parse_solo_head_cfg, solo_cate_loss, solov2_targets
    head = parse_solo_head_cfg(head_cfg)
    lcfg = parse_discobox_loss_cfg(head_cfg)
    dev = s_ins_pred.device
    use_corr = bool(use_loss_ts and use_corr)
    H, W = int(s_ins_pred.shape[-2]), int(s_ins_pred.shape[-1])
    targets = solov2_targets(gt_bbox_list, gt_label_list, gt_mask_list, (H, W),
                             **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')})
    loss_cate = solo_cate_loss(list(cate_preds), targets.flat_cate_labels, targets.num_ins, head['gamma'], head['alpha'], head['loss_weight_cate'])
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    # the rows of all levels as ONE [R,H,W] buffer, level-major (what solo_dynamic_masks_pair slices into per-level views)
    s_raw, img_inds, level_rows, cells = _dynamic_rows(s_kernel_preds_raw, targets, s_ins_pred, sigmoid=False)
    R = sum(level_rows)
    if R == 0:
        return dict(loss_ins=zero, loss_ts=zero.clone(), loss_cate=loss_cate, loss_corr=zero.clone())
    t_raw = s_raw
    if use_ind_teacher:
        with torch.no_grad():
            t_raw = _dynamic_rows([m.detach() for m in t_kernel_preds_raw], targets, t_ins_pred.detach(), sigmoid=False, cells=cells)[0]
    s_rows = torch.sigmoid(s_raw)
    t_rows = s_rows if not use_ind_teacher else torch.sigmoid(t_raw.detach())
    # ins_labels of every level in ONE gather (the levels of DiscoBox share one compact mask set: level_factor is the same for all)
    factors = set(targets.level_factor)
    if len(factors) != 1:
        raise RuntimeError(f'the levels read masks of different factors {sorted(factors)}')
    target_rows = targets.masks[factors.pop()].index_select(0, torch.cat(targets.pair_inst))
    with torch.no_grad():
        color = F.interpolate(img.to(torch.float32), (H, W), mode='bilinear', align_corners=True)
        kernel = meanfield_kernel(color, lcfg['kernel'], lcfg['alpha0'], lcfg['theta0'], lcfg['theta1'])
    iiu_levels, loss_corr = None, zero.clone()
    if use_corr:
        if bank is None or solver is None or s_feat is None or t_feat is None:
            raise RuntimeError('use_corr needs bank, solver, s_feat and t_feat')
        ccfg = parse_corr_cfg(head_cfg)
        sf, tf = s_feat[0], t_feat[0]
        kernel_labels = targets.kernel_labels()
        iiu_levels, at, loss_sum, num = [], 0, zero.clone(), torch.zeros((), dtype=torch.float32, device=dev)
        for l, n in enumerate(level_rows):
            if n == 0:
                iiu_levels.append(None)
                continue
            ls, ni, iiu, _ = corr_level(s_raw[at:at + n], t_raw[at:at + n] if use_ind_teacher else s_raw[at:at + n], target_rows[at:at + n],
                                        img_inds[at:at + n], kernel_labels[l], sf, tf, bank, solver, ccfg['min_size'], ccfg['min_objs'], own_labels=False)
            loss_sum, num = loss_sum + ls, num + ni.to(torch.float32)
            iiu_levels.append(iiu)
            at += n
        loss_corr = loss_sum / (num + 1e-4) * lcfg['w_corr']
    if not use_loss_ts:
        mil_rows = mil_loss(dice_loss, s_rows, s_rows, target_rows)
        live = target_rows.flatten(1).any(1).to(torch.int32)
        n_live = live.sum(dtype=torch.int32).view(1)
        return dict(loss_ins=live_means(live, n_live, mil_rows)[0] * lcfg['w_ins'], loss_ts=zero.clone(), loss_cate=loss_cate, loss_corr=loss_corr)
    mil_rows, ts_rows, ts_corr_rows, live, n_live = discobox_pseudo_losses(
        s_rows, t_rows, target_rows, img_inds, kernel, iiu_levels, level_rows if use_corr else None, iters=lcfg['max_iter'], base=lcfg['base'],
        details=details)
    means = live_means(live, n_live, mil_rows, ts_rows, *((ts_corr_rows,) if use_corr else ()))
    loss_ts = (means[1] + (means[2] if use_corr else 0.0)) * lcfg['w_ts']
    return dict(loss_ins=means[0] * lcfg['w_ins'], loss_ts=loss_ts, loss_cate=loss_cate, loss_corr=loss_corr)
