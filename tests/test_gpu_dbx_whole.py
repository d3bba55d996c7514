"""GPU: ``discobox_loss`` against tests/dbx_compose.py -- the reference's loops over the package's existing modules, what a user wrote
before -- at B = 2, E = 8, mask feature 24 x 40: grids [6, 4] and once the configs' five grids, use_corr and use_ind_teacher on and off,
one image without boxes.  Three calls in a row on each side's own bank.  The inputs are ``make_inputs(sharp=True)``: masks and RoI features
that pass the bank's four retrieval thresholds, so with use_corr the solver runs, ``iiu`` is not zero, ``loss_corr > 0``, the legs' labels
differ and ``s_feat`` gets a gradient -- all asserted.

Both sides run the same kernels up to the row buffer, the same mil rows and the same ``corr_level``; they differ in where sums are rounded.
* labels: equal;
* a loss: 4 x the largest tol_mean_* / tol_mil_rows of tests/golden/discobox_loss.npz (the reference's own fp32-against-fp64 difference of
  such means: the project's rule), plus what the composition's fp32 ``.mean()`` over at most MAX_ROWS rows may add, MAX_ROWS * 2^-24;
* a gradient: the row gradients of the two sides agree within 4 x tol_grad of the fixture; the shared backward kernels then accumulate at
  most H * W = 960 fp32 products per element on each side, 960 * 2^-24, relative to the tensor's largest gradient magnitude."""
import numpy as np
import pytest
import torch

from tests import dbx_compose as C
from tests import dbx_loss_ref as R

pytestmark = pytest.mark.gpu

FIVE = dict(num_grids=[40, 36, 24, 16, 12], strides=[8, 8, 16, 32, 32], scale_ranges=((1, 96), (48, 192), (96, 384), (192, 768), (384, 2048)))
TWO = dict(num_grids=[6, 4], strides=[8, 16], scale_ranges=((1, 64), (32, 512)))
MAX_ROWS, PIXELS = 128, 24 * 40
_FIX = [R.fixture(n) for n in R.FIXTURE_CASES]
TOL_LOSS = R.TOL_FACTOR * max(float(f[k]) for f in _FIX for k in ('tol_mean_ts', 'tol_mean_ts_corr', 'tol_mil_rows')) + MAX_ROWS * 2.0 ** -24
TOL_GRAD = R.TOL_FACTOR * max(float(f['tol_grad']) for f in _FIX) + PIXELS * 2.0 ** -24


def _side(fn, grids, dev, use_corr, use_ind_teacher, empty_image, calls=3, use_loss_ts=True):
    import boxinstseg_amd as B
    block = C.head_block(**grids)
    ccfg = B.parse_corr_cfg(block)
    bank, solver = B.ObjectBank(**ccfg['bank']), B.SemanticCorrSolver(**ccfg['solver'])
    out = []
    for call in range(calls):
        d = C.make_inputs(grids['num_grids'], empty_image=empty_image, seed=call, sharp=True)
        t = lambda a, g=False: torch.from_numpy(a).to(dev).requires_grad_(g)
        leaves = dict(s_kern=[t(a, True) for a in d['s_kern']], s_ins=t(d['s_ins'], True), s_feat=t(d['s_feat'], True), cate=[t(a, True) for a in d['cate']])
        details = {}
        args = (leaves['cate'], leaves['s_kern'], [t(a) for a in d['t_kern']], leaves['s_ins'], t(d['t_ins']), [t(b) for b in d['boxes']],
                [t(l) for l in d['labels']], [t(m) for m in d['masks']])
        kw = dict(use_loss_ts=use_loss_ts, use_ind_teacher=use_ind_teacher, use_corr=use_corr, s_feat=[leaves['s_feat']], t_feat=[t(d['t_feat'])], bank=bank,
                  solver=solver, head_cfg=block, details=details)
        losses = fn(*args, None, None, t(d['img']), **kw) if fn is B.discobox_loss else fn(*args, t(d['img']), **kw)
        total = losses['loss_ins'] + 0.7 * losses['loss_ts'] + 1.3 * losses['loss_corr'] + 0.9 * losses['loss_cate']
        flat = leaves['s_kern'] + [leaves['s_ins'], leaves['s_feat']] + leaves['cate']
        grads = torch.autograd.grad(total, flat, allow_unused=True)
        out.append(dict(losses={k: v.detach() for k, v in losses.items()}, grads=grads, details=details, n_kern=len(leaves['s_kern'])))
    return out


@pytest.mark.parametrize('grids,use_corr,use_ind_teacher,empty_image', [
    (TWO, True, True, None), (TWO, False, True, None), (TWO, True, False, None), (TWO, False, False, 1), (TWO, True, True, 0), (FIVE, True, True, None)],
    ids=['corr_teacher', 'teacher', 'corr', 'plain_empty1', 'corr_teacher_empty0', 'five_grids'])
def test_discobox_loss_against_the_composition(dev, grids, use_corr, use_ind_teacher, empty_image):
    import boxinstseg_amd as B
    got = _side(B.discobox_loss, grids, dev, use_corr, use_ind_teacher, empty_image)
    want = _side(C.compose_loss, grids, dev, use_corr, use_ind_teacher, empty_image)
    rows_seen = 0
    for call, (g, w) in enumerate(zip(got, want)):
        # labels
        pseudo = g['details'].get('pseudo')
        if pseudo is not None:
            rows_seen += pseudo.shape[0]
            assert pseudo.shape[0] <= MAX_ROWS
            seen = torch.zeros(pseudo.shape[0], dtype=torch.bool, device=dev)
            for k, (rows, lab) in enumerate(w['details']['labels']):
                assert torch.equal(pseudo[rows], lab.to(torch.uint8)), (call, k)
                seen[rows] = True
                if use_corr:
                    assert torch.equal(g['details']['pseudo_corr'][rows], w['details']['labels_corr'][k].to(torch.uint8)), (call, k)
            assert torch.equal(seen, (g['details']['target'] != 0).flatten(1).any(1))          # the composition ran exactly the live rows
            assert not bool(pseudo[~seen].any())
        # losses: 0-dim, close
        for k in ('loss_ins', 'loss_ts', 'loss_cate', 'loss_corr'):
            a, b = g['losses'][k], w['losses'][k]
            assert a.dim() == 0 and a.dtype == torch.float32, k
            err = abs(float(a) - float(b))
            print(f'call {call} {k}: {float(a):.7g} against {float(b):.7g}')
            assert err <= TOL_LOSS * max(abs(float(a)), abs(float(b)), 1e-30), (call, k, float(a), float(b))
        # gradients: every kernel map, s_ins_pred, s_feat (and the category maps), every element present
        for i, (a, b) in enumerate(zip(g['grads'], w['grads'])):
            if b is None:
                assert a is None or not bool(a.any()), i
                continue
            assert a is not None and a.shape == b.shape and bool(torch.isfinite(a).all()), i
            scale = max(float(b.abs().max()), 1e-30)
            print(f'call {call} gradient {i}: differs by {float((a - b).abs().max()) / scale:.3e} of the maximum (bound {TOL_GRAD:.3e})')
            assert float((a - b).abs().max()) <= TOL_GRAD * scale, (call, i, float((a - b).abs().max()), scale)
        for a in g['grads'][:g['n_kern'] + 1]:
            assert a is not None
    assert rows_seen > 0
    if use_corr and empty_image is None:                                   # the correspondence path ran with a result, on both sides (three
        # objects of one image alone do not reach five matches in three calls)
        last, n_kern = got[-1], got[-1]['n_kern']
        assert float(last['losses']['loss_corr']) > 0 and float(want[-1]['losses']['loss_corr']) > 0
        assert not torch.equal(last['details']['pseudo'], last['details']['pseudo_corr'])
        assert last['grads'][n_kern + 1] is not None and bool(last['grads'][n_kern + 1].any())          # s_feat
    if empty_image is None:
        assert float(got[-1]['losses']['loss_ts']) > 0 and float(got[-1]['losses']['loss_ins']) > 0


def test_without_loss_ts(dev):
    """use_loss_ts=False: the mil term alone, loss_ts and loss_corr zero (:1293, :1310), the same gradients as the composition."""
    import boxinstseg_amd as B
    got = _side(B.discobox_loss, TWO, dev, True, False, None, calls=1, use_loss_ts=False)[0]
    want = _side(C.compose_loss, TWO, dev, True, False, None, calls=1, use_loss_ts=False)[0]
    assert float(got['losses']['loss_ts']) == 0 and float(got['losses']['loss_corr']) == 0 and float(got['losses']['loss_ins']) > 0
    for k in got['losses']:
        a, b = float(got['losses'][k]), float(want['losses'][k])
        assert got['losses'][k].dim() == 0 and abs(a - b) <= TOL_LOSS * max(abs(a), abs(b), 1e-30), (k, a, b)
    for i, (a, b) in enumerate(zip(got['grads'], want['grads'])):
        if b is None:
            assert a is None or not bool(a.any()), i
        else:
            assert float((a - b).abs().max()) <= TOL_GRAD * max(float(b.abs().max()), 1e-30), i


def test_nothing_assigned_gives_zeros(dev):
    """No box in any image: four 0-dim losses, zeros but for loss_cate, where the reference's torch.cat([]) raises with use_corr."""
    import boxinstseg_amd as B
    block = C.head_block(**TWO)
    ccfg = B.parse_corr_cfg(block)
    d = C.make_inputs(TWO['num_grids'], boxes_per_image=0)
    t = lambda a: torch.from_numpy(a).to(dev)
    losses = B.discobox_loss([t(a) for a in d['cate']], [t(a) for a in d['s_kern']], [t(a) for a in d['t_kern']], t(d['s_ins']), t(d['t_ins']),
                             [t(b) for b in d['boxes']], [t(l) for l in d['labels']], [t(m) for m in d['masks']], None, None, t(d['img']),
                             use_loss_ts=True, use_ind_teacher=True, use_corr=True, s_feat=[t(d['s_feat'])], t_feat=[t(d['t_feat'])],
                             bank=B.ObjectBank(**ccfg['bank']), solver=B.SemanticCorrSolver(**ccfg['solver']), head_cfg=block)
    assert all(v.dim() == 0 for v in losses.values())
    assert float(losses['loss_ins']) == 0 and float(losses['loss_ts']) == 0 and float(losses['loss_corr']) == 0 and float(losses['loss_cate']) > 0
