"""Shared helpers for the parity tests: run the CPU oracle / the HIP path on a synthetic batch."""
from __future__ import annotations

import numpy as np
import torch

from boxinstseg_amd import functional as F_hip
from boxinstseg_amd.functional import rows_removed
from oracle import c_oracle


def oracle_path(d, warmup=1.0, g_prj=1.0, g_pw=1.0, bottom_pixels_removed=10, size=3, dil=2, thresh=0.3,
                want_targets=True):
    hw = np.array([[m['img_shape'][0], m['img_shape'][1]] for m in d['img_metas']], np.int32).reshape(-1, 2)
    rr = np.array([rows_removed(bottom_pixels_removed, m['img_shape'], m['ori_shape']) for m in d['img_metas']],
                  np.int32)
    boxes = np.concatenate(d['gt_bboxes'], axis=0) if len(d['gt_bboxes']) else np.zeros((0, 4), np.float32)
    cfg = d['img_metas'][0]['img_norm_cfg'] if d['img_metas'] else dict(mean=d['mean'], std=d['std'], to_rgb=True)
    return c_oracle.boxinst_path(d['imgs'], hw, rr, cfg['mean'], cfg['std'], cfg['to_rgb'], boxes,
                                 np.array([len(b) for b in d['gt_bboxes']], np.int32), d['gt_inds'],
                                 d['mask_logits'][:, 0], stride=d['stride'], size=size, dil=dil,
                                 color_thresh=thresh, warmup=warmup, g_prj=g_prj, g_pw=g_pw,
                                 want_targets=want_targets)


def oracle_path_f64(d, warmup=1.0, g_prj=1.0, g_pw=1.0, bottom_pixels_removed=10, size=3, dil=2, thresh=0.3):
    hw = np.array([[m['img_shape'][0], m['img_shape'][1]] for m in d['img_metas']], np.int32).reshape(-1, 2)
    rr = np.array([rows_removed(bottom_pixels_removed, m['img_shape'], m['ori_shape']) for m in d['img_metas']], np.int32)
    boxes = np.concatenate(d['gt_bboxes'], axis=0)
    cfg = d['img_metas'][0]['img_norm_cfg']
    return c_oracle.boxinst_path_f64(d['imgs'], hw, rr, cfg['mean'], cfg['std'], cfg['to_rgb'], boxes,
                                     np.array([len(b) for b in d['gt_bboxes']], np.int32), d['gt_inds'], d['mask_logits'][:, 0],
                                     stride=d['stride'], size=size, dil=dil, color_thresh=thresh, warmup=warmup, g_prj=g_prj,
                                     g_pw=g_pw)


def to_dev(d, dev):
    return dict(imgs=torch.from_numpy(d['imgs']).to(dev),
                logits=torch.from_numpy(d['mask_logits']).to(dev),
                gt_inds=torch.from_numpy(d['gt_inds']).to(dev),
                gt_bboxes=[torch.from_numpy(b).to(dev) for b in d['gt_bboxes']])


def hip_loss(d, dev, warmup=1.0, up=None, **kw):
    """-> (loss_prj, loss_pairwise, grad[N,h,w] numpy)."""
    F_hip.DEBUG_KEEP_LAST = True
    t = to_dev(d, dev)
    logits = t['logits'].clone().requires_grad_(True)
    out = F_hip.boxinst_mask_loss(logits, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'],
                                  out_stride=d['stride'], warmup_factor=warmup, **kw)
    if up is None:
        (out['loss_prj'] + out['loss_pairwise']).backward()
    else:
        (up[0] * out['loss_prj'] + up[1] * out['loss_pairwise']).backward()
    torch.cuda.synchronize()
    if kw.get('pairwise_dilation', 2) <= 4 and logits.size(0) > 0:
        status, rows = F_hip.last_eval_status()
        assert status == 0 and rows in (4, 8), f'in-kernel wait timed out: status {status}'
    return float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), logits.grad.cpu().numpy()[:, 0]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def grad_report(got, want, logits=None, tie_eps=2.5e-7):
    """max-abs error relative to max|want|; positions where the arg-max of the projection term is
    ambiguous in fp32 (top-2 sigmoid values of a row/column within a few ulp) are excluded and counted."""
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want)
    n_tie = 0
    if logits is not None:
        s = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
        mask = np.zeros_like(err, dtype=bool)
        for axis in (1, 2):
            top2 = np.sort(s, axis=axis)
            gap = (np.take(top2, -1, axis=axis) - np.take(top2, -2, axis=axis))
            amb = gap <= tie_eps * np.take(top2, -1, axis=axis)          # [N, other]
            if amb.any():
                idx = np.argwhere(amb)
                for n, o in idx:
                    if axis == 1:
                        mask[n, :, o] = True
                    else:
                        mask[n, o, :] = True
                n_tie += len(idx)
        err = np.where(mask, 0.0, err)
    return float(err.max() / scale), n_tie


# ---------------------------------------------------------------------------------------------
# the projection term with its arg-max rule stated, for inputs with tied lines (nothing excluded)
# ---------------------------------------------------------------------------------------------
def _first_argmax(a, axis):
    return np.argmax(a, axis=axis)


def _last_argmax(a, axis):
    n = a.shape[axis]
    return n - 1 - np.argmax(np.flip(a, axis=axis), axis=axis)


def project_term_f64(logits, bitmask, rule='logit_first', g_out=1.0):
    """Float64 restatement of oracle/loss_terms.inc:109-154 on fp32 `logits` [N,h,w] and `bitmask` [N,h,w]: dice over the column
    and row maxima of sigmoid(logits), gradient du * s(1-s) * g_out / N sent to ONE pixel per line, chosen by `rule`:
      'logit_first'  first index of the largest fp32 logit along the line (what the kernels document);
      'logit_last'   last index of it (what a merge with the wrong tie order would do; for checking the checks);
      'sigma_first'  first index of the largest fp32 sigmoid, 1 / (1 + exp(-x)) evaluated in fp32 by numpy.
    -> (loss [N], grad [N,h,w] float64, (col_arg [N,w] = row index per column, row_arg [N,h] = column index per row))."""
    x32 = np.ascontiguousarray(logits, dtype=np.float32)
    N, h, w = x32.shape
    t = np.asarray(bitmask, np.float64)
    s = 1.0 / (1.0 + np.exp(-x32.astype(np.float64)))
    if rule == 'logit_first':
        key, pick = x32, _first_argmax
    elif rule == 'logit_last':
        key, pick = x32, _last_argmax
    elif rule == 'sigma_first':
        with np.errstate(over='ignore'):
            key, pick = (np.float32(1) / (np.float32(1) + np.exp(-x32))).astype(np.float32), _first_argmax
    else:
        raise ValueError(rule)
    col_arg = pick(key, 1) if N else np.zeros((0, w), np.int64)        # [N,w]
    row_arg = pick(key, 2) if N else np.zeros((0, h), np.int64)        # [N,h]
    loss = np.zeros(N)
    grad = np.zeros((N, h, w))
    nn = np.arange(N)[:, None]
    for axis, arg in ((1, col_arg), (2, row_arg)):
        if N == 0:
            break
        u = np.take_along_axis(s, np.expand_dims(arg, axis), axis).squeeze(axis)      # [N, line]
        tm = t.max(axis)
        inter = (u * tm).sum(1, keepdims=True)
        uni = (u * u).sum(1, keepdims=True) + (tm * tm).sum(1, keepdims=True) + 1e-5
        loss += 1.0 - 2.0 * inter[:, 0] / uni[:, 0]
        g = (-2.0 * tm * uni + 4.0 * inter * u) / (uni * uni) * u * (1.0 - u) * (float(g_out) / N)
        line = np.arange(arg.shape[1])[None, :]
        if axis == 1:
            np.add.at(grad, (nn, arg, line), g)
        else:
            np.add.at(grad, (nn, line, arg), g)
    return loss, grad, (col_arg, row_arg)


def instance_bitmasks(d):
    """Per-instance box masks [N,h,w] f32 of a synthetic batch: c_oracle.box_bitmask of every GT box, indexed by gt_inds."""
    allb = np.concatenate(d['gt_bboxes'], axis=0) if len(d['gt_bboxes']) else np.zeros((0, 4), np.float32)
    gi = np.asarray(d['gt_inds'], np.int64).reshape(-1)
    if gi.size == 0:
        return np.zeros((0, d['h'], d['w']), np.float32)
    bm = np.stack([c_oracle.box_bitmask(b, d['H'], d['W'], d['stride']) for b in allb])
    return bm[gi]


def expected_grad_logit_first(d, ref, g_prj=1.0, logits=None):
    """The gradient the library documents for the batch `d`: the C oracle's (`ref['grad']`, from oracle_path with the same
    parameters and the same `g_prj`) with the projection part moved from the oracle's arg-max pixels (first maximum of ITS fp32
    sigmoid) to the first index of the largest logit:  ref['grad'] - P_oracle + P_logit_first.  Where no line is tied the two
    parts cancel to rounding; on a tied line the line's mass moves to the documented pixel.  The oracle's sigmoid is not
    re-derived: P_oracle is what c_oracle.project_term itself returns for these logits and masks.  -> [N,h,w] float64."""
    x = np.ascontiguousarray(d['mask_logits'][:, 0] if logits is None else logits, dtype=np.float32)
    if x.shape[0] == 0:
        return np.asarray(ref['grad'], np.float64)
    bm = instance_bitmasks(d)
    _, p_oracle = c_oracle.project_term(x, bm, g_out=float(g_prj))
    _, p_first, _ = project_term_f64(x, bm, 'logit_first', g_out=float(g_prj))
    return np.asarray(ref['grad'], np.float64) - p_oracle.astype(np.float64) + p_first


def grad_check_all_lines(got, expected):
    """max-abs error over max|expected|: every pixel, no line excluded."""
    if np.size(expected) == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - expected).max() / (np.abs(expected).max() + 1e-30))
