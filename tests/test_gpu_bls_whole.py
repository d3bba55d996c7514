"""GPU: ``box_solov2_loss`` end to end against tests/bls_compose.py -- the level loop a user wrote before from the package's existing
modules, with the reference's per-row repeats and one tree per row -- at B = 2, E = 8, mask feature 24 x 40, level sizes (24,40), (24,40),
(12,20), (6,10), (6,10), grids [6, 5, 4, 3, 2].

The project's rule, elementwise: the three losses and the gradients of kernel_preds, feature_pred, levelset_feats and cate_preds lie
within max(4 |ref32 - ref64|, floor) of ref64, with the composition's own fp32 result as ref32 and its restatement in fp64 on the CPU
(tests/bls_compose.restate under the same assignment, tests/solo_ref.cate_loss) as ref64; the floor is 1e-4 of the tensor's largest
magnitude, for ``levelset_feats.grad`` tests/test_gpu_bls_loss.py's bound through the resizes.  And the call waits for the device once."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bls_compose as C
from tests.test_gpu_tree_filter import EMB_GRAD_TOL

pytestmark = pytest.mark.gpu
TOL = 1e-4
SIZES = [(24, 40), (24, 40), (12, 20), (6, 10), (6, 10)]
HEAD = dict(type='BoxSOLOv2Head', num_classes=3, strides=[8, 8, 16, 32, 32], scale_ranges=((1, 24), (12, 48), (24, 96), (48, 192), (96, 512)), sigma=0.2,
            num_grids=[6, 5, 4, 3, 2], loss_cate=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_boxpro=dict(type='BoxProjectionLoss', loss_weight=3.0), loss_levelset=dict(type='LevelsetLoss', loss_weight=1.0))
NB, E, CF, CANVAS = 2, 8, 3, (96, 160)


def make_inputs(seed=0):
    rng = np.random.default_rng(seed)
    H, W = CANVAS
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([np.stack([np.sin(yy / (9.0 + ch + b)) + np.cos(xx / (11.0 + ch)) for ch in range(3)]) for b in range(NB)])
    img = (img + 0.3 * rng.standard_normal(img.shape)).astype(np.float32)
    boxes, labels, masks = [], [], []
    for b in range(NB):
        bx, mk = [], []
        for side in (10, 20, 34, 60, 90)[:4 + b]:                         # sqrt(area) across the scale ranges
            bh, bw = min(side, H - 2), min(int(side * 1.2), W - 2)
            y, x = int(rng.integers(0, H - bh)), int(rng.integers(0, W - bw))
            bx.append([x, y, x + bw, y + bh])
            m = np.zeros((H, W), np.uint8)
            m[y:y + bh, x:x + bw] = 1
            mk.append(m)
        boxes.append(np.array(bx, np.float32))
        labels.append(rng.integers(0, HEAD['num_classes'], len(bx)).astype(np.int64))
        masks.append(np.stack(mk))
    kern = [(0.3 * rng.standard_normal((NB, E, s, s))).astype(np.float32) for s in HEAD['num_grids']]
    cate = [(rng.standard_normal((NB, HEAD['num_classes'], s, s)) * 2.0 - 2.0).astype(np.float32) for s in HEAD['num_grids']]
    feat = rng.standard_normal((NB, E) + SIZES[0]).astype(np.float32)
    lst = rng.standard_normal((NB, CF) + SIZES[0]).astype(np.float32)
    return dict(img=img, boxes=boxes, labels=labels, masks=masks, kern=kern, cate=cate, feat=feat, lst=lst)


def _leaves(d, dev):
    t = lambda a, g=False: torch.from_numpy(a).to(dev).requires_grad_(g)
    return dict(kern=[t(a, True) for a in d['kern']], cate=[t(a, True) for a in d['cate']], feat=t(d['feat'], True), lst=t(d['lst'], True), img=t(d['img']),
                boxes=[t(a) for a in d['boxes']], labels=[t(a) for a in d['labels']], masks=[t(a) for a in d['masks']])


def _evaluate(fn, v):
    out = fn(v)
    flat = v['kern'] + [v['feat'], v['lst']] + v['cate']
    grads = torch.autograd.grad(out['loss_boxpro'] + out['loss_levelset'] + out['loss_cate'], flat)
    return {k: x.detach() for k, x in out.items()}, grads


def test_box_solov2_loss_against_the_composition(dev):
    import boxinstseg_amd as B
    from tests import guarded as G
    from tests import solo_ref
    d = make_inputs()
    new = lambda v: B.box_solov2_loss(v['kern'], v['cate'], v['feat'], v['lst'], v['boxes'], v['labels'], v['masks'], v['img'], None, HEAD)
    a, b = _evaluate(new, _leaves(d, dev)), _evaluate(new, _leaves(d, dev))
    assert all(G.same(a[0][k], b[0][k]) for k in a[0]) and all(G.same(x, y) for x, y in zip(a[1], b[1])), 'two runs differ'
    assert sorted(a[0]) == ['loss_boxpro', 'loss_cate', 'loss_levelset'] and all(x.dim() == 0 and x.dtype == torch.float32 for x in a[0].values())
    keep = {}
    def comp(v):
        out, keep['targets'] = C.compose_loss(v['kern'], v['cate'], v['feat'], v['lst'], v['boxes'], v['labels'], v['masks'], v['img'], HEAD, SIZES)
        return out
    c = _evaluate(comp, _leaves(d, dev))
    tg = keep['targets']
    rows = [[int(tg.counts[l][i][1]) for i in range(NB)] for l in range(len(SIZES))]
    assert sum(map(sum, rows)) >= 6 and sum(1 for r in rows if sum(r)) >= 3, rows                  # several levels and sizes carry rows
    cells = [[x.cpu().numpy() for x in per] for per in B.box_solov2_set_cells(tg)]
    sel = [s.cpu().numpy() for s in tg.sel_inst]
    masks = [tg.masks[f].cpu().numpy() for f in tg.level_factor]
    r64, gk, gf, gl = C.restate(d['kern'], d['feat'], d['lst'], d['img'], cells, sel, masks, SIZES, torch.float64, 3.0, 1.0)
    cate64, gcate = solo_ref.cate_loss(d['cate'], tg.flat_cate_labels.cpu().numpy(), int(tg.num_ins.cpu()), 2.0, 0.25, 1.0)
    # the floor of levelset_feats.grad: EMB_GRAD_TOL * max(gw, 1) per embedding element of every size through the adjoint of the resize
    sizes = list(dict.fromkeys(SIZES))
    floor = np.zeros((NB, 1) + SIZES[0])
    for g, size in enumerate(sizes):
        x = torch.ones(floor.shape, dtype=torch.float64, requires_grad=True)
        F.interpolate(x, size=size, mode='bilinear', align_corners=False).sum().backward()
        floor += x.grad.numpy() * (EMB_GRAD_TOL * np.maximum(r64['gw_sum'][g], 1.0))[:, None, None, None]
    one = lambda v: np.array([float(v)], np.float64)
    L = len(SIZES)
    items = [(k, a[0][k], c[0][k], one(w), None) for k, w in (('loss_boxpro', r64['loss_boxpro']), ('loss_levelset', r64['loss_levelset']), ('loss_cate', cate64))]
    items += [(f'kernel_preds[{l}].grad', a[1][l], c[1][l], gk[l], None) for l in range(L)]
    items += [('feature_pred.grad', a[1][L], c[1][L], gf, None), ('levelset_feats.grad', a[1][L + 1], c[1][L + 1], gl, floor)]
    items += [(f'cate_preds[{l}].grad', a[1][L + 2 + l], c[1][L + 2 + l], gcate[l].numpy().astype(np.float64), None) for l in range(L)]
    for what, got, ref32, ref64, fl in items:
        got, ref32 = got.cpu().numpy().astype(np.float64).reshape(ref64.shape), ref32.cpu().numpy().astype(np.float64).reshape(ref64.shape)
        assert np.isfinite(got).all(), what
        if fl is None:
            fl = TOL * max(np.abs(ref64).max(), 1e-12)
        tol = np.maximum(4.0 * np.abs(ref32 - ref64), fl)
        share = float((np.abs(got - ref64) / tol).max())
        print(f'{what}: max |want| {np.abs(ref64).max():.4g}, largest share of the bound {share:.3g}')
        assert share <= 1.0, f'{what}: {share:.3g} of the bound'
    assert float(a[0]['loss_boxpro']) > 0 and float(a[0]['loss_levelset']) > 0 and bool(a[1][L + 1].any())


def test_exactly_one_host_synchronisation(dev):
    import boxinstseg_amd as B
    v = _leaves(make_inputs(1), dev)
    run = lambda: sum(B.box_solov2_loss(v['kern'], v['cate'], v['feat'], v['lst'], v['boxes'], v['labels'], v['masks'], v['img'], None, HEAD).values()).backward()
    run()                                                                  # (the first call loads the library)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    syncs = [str(w.message) for w in seen if 'synchroniz' in str(w.message).lower() and 'prototype' not in str(w.message).lower()]
    assert len(syncs) == 1, syncs                                          # box_solov2_targets' read of the counts
