"""GPU: the mask losses of BoxSOLOv2Head.loss for all levels (boxinstseg_amd/boxlevelset_loss.py on csrc/boxlevelset_loss.hip) against the
per-row restatement of tests/bls_loss_ref.py, on the cases of tests/bls_cases.py (tests/test_host_bls_loss.py takes their census).

TOLERANCE, the project's rule, elementwise, nothing skipped: both losses, every per-row value and every element of every level's logit
gradient lie within max(4 |ref32 - ref64|, 1e-4 max|ref64|) of the fp64 restatement, ref32 being the same restatement in float32.  For
``levelset_feats.grad`` the floor is tests/test_gpu_tree_filter.py's bound on the embedding gradient, EMB_GRAD_TOL * max(|gw|max, 1) per
element of a size's embedding, carried through the adjoint of the resize to that size and summed over the sizes (gw: the restatement's
weight gradient, summed as the shared tree sums it).  The largest share of the bound reached on an MI355X is in profiles/NOTES.md (R31-1).

In every case: two runs are bit-identical, ``box_solov2_mask_losses`` runs under torch.cuda.set_sync_debug_mode('error'), and inert rows
give exact zeros.  On ``three_groups`` the result also holds against tests/golden/box_solov2_loss.npz (the reference's own statements in
float32) by the same rule."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bls_cases as K
from tests.test_gpu_tree_filter import EMB_GRAD_TOL

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _run(name, dev, d=None):
    from boxinstseg_amd import BoxLevelSetLossContext, box_solov2_mask_losses
    d = d or K.inputs(name)
    preds = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in d['ins_preds']]
    lst = torch.from_numpy(d['lst_feat']).to(dev).requires_grad_(True)
    img = torch.from_numpy(d['norm_img']).to(dev)
    on_dev = {}
    masks = [on_dev.setdefault(id(m), torch.from_numpy(m).to(dev)) for m in d['masks']]
    tgt = [torch.from_numpy(t).to(dev) for t in d['tgt_of']]
    img_of = [torch.from_numpy(t).to(dev) for t in d['img_of']]
    trees = None if d['trees'] is None else [tuple(torch.from_numpy(t).to(dev) for t in pair) for pair in d['trees']]
    ctx = BoxLevelSetLossContext(img, lst, d['level_sizes'], trees)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lb, ll, rows = box_solov2_mask_losses(ctx, preds, masks, tgt, img_of, d['counts'], K.LOSS_BOXPRO_WEIGHT, K.LOSS_LEVELSET_WEIGHT)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    (lb + ll).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    # the per-row values back in the levels' own order
    proj = [torch.zeros(len(p), device=dev) for p in preds]
    levelset = [torch.zeros(len(p), device=dev) for p in preds]
    live = [torch.zeros(len(p), device=dev) for p in preds]
    m = 0
    for l, a, c, _ in rows['segments']:
        proj[l][a:a + c], levelset[l][a:a + c], live[l][a:a + c] = rows['proj'][m:m + c].detach(), rows['levelset'][m:m + c].detach(), rows['live'][m:m + c]
        m += c
    assert m == rows['proj'].numel() == sum(len(p) for p in preds)
    return dict(loss_boxpro=lb.detach().reshape(1), loss_levelset=ll.detach().reshape(1), proj=proj, levelset=levelset, live=live,
                grads=[zero(p) for p in preds], lst_grad=zero(lst), ctx=ctx)


def _flat(run):
    return [run['loss_boxpro'], run['loss_levelset'], *run['proj'], *run['levelset'], *run['grads'], run['lst_grad']]


def _lst_floor(name, r64):
    """EMB_GRAD_TOL * max(gw, 1) per embedding element of every size, through the adjoint of lst_feat -> that size: the column sums."""
    d = K.inputs(name)
    sizes, _ = K.groups_of(d['level_sizes'])
    total = np.zeros((d['B'], 1) + tuple(d['lst_feat'].shape[-2:]))
    for g, size in enumerate(sizes):
        x = torch.ones(total.shape, dtype=torch.float64, requires_grad=True)
        F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False).sum().backward()
        total += x.grad.numpy() * (EMB_GRAD_TOL * np.maximum(r64['gw_sum'][g], 1.0))[:, None, None, None]
    return total


def _items(name, run, r32, r64):
    L = len(r64['grads'])
    one = lambda v: np.array([v], np.float64)
    items = [('loss_boxpro', run['loss_boxpro'], one(r32['loss_boxpro']), one(r64['loss_boxpro']), None),
             ('loss_levelset', run['loss_levelset'], one(r32['loss_levelset']), one(r64['loss_levelset']), None)]
    items += [(f'proj[{l}]', run['proj'][l], r32['proj'][l], r64['proj'][l], None) for l in range(L)]
    items += [(f'levelset[{l}]', run['levelset'][l], r32['levelset'][l], r64['levelset'][l], None) for l in range(L)]
    items += [(f'grad[{l}]', run['grads'][l], r32['grads'][l], r64['grads'][l], None) for l in range(L)]
    items.append(('lst_grad', run['lst_grad'], r32['lst_grad'], r64['lst_grad'], _lst_floor(name, r64)))
    return items


def _hold(name, run, refs=None):
    r32, r64 = refs or (K.reference(name, 'float32'), K.reference(name, 'float64'))
    worst = 0.0
    for what, got, a32, a64, floor in _items(name, run, r32, r64):
        got = got.cpu().numpy().astype(np.float64)
        a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
        assert got.shape == a64.shape, (what, got.shape, a64.shape)
        if got.size == 0:
            continue
        assert np.isfinite(got).all(), what
        if floor is None:
            floor = TOL * max(np.abs(a64).max(), 1e-12)
        tol = np.maximum(4.0 * np.abs(a32 - a64), floor)
        err = np.abs(got - a64)
        assert (err[tol == 0] == 0).all(), f'{name}: {what}: an element with a zero bound is off'
        share = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
        print(f'{name}: {what}: max |want| {np.abs(a64).max():.4g}, largest share of the bound {share:.3g}')
        worst = max(worst, share)
        assert share <= 1.0, f'{name}: {what}: {share:.3g} of the bound'
    print(f'{name}: largest share of the bound {worst:.3g}')
    return worst


@pytest.mark.parametrize('name', [n for n in K.CASES if n != 'no_rows'])
def test_case_against_the_restatement(dev, name):
    from tests import guarded as G
    a = _run(name, dev)
    b = _run(name, dev)
    for x, y in zip(_flat(a), _flat(b)):
        assert G.same(x, y), 'two runs differ'
    _hold(name, a)
    d = K.inputs(name)
    inert = [(l, r) for l in range(len(d['tgt_of'])) for r in range(len(d['tgt_of'][l])) if d['tgt_of'][l][r] < 0 or d['img_of'][l][r] < 0]
    assert bool(inert) == (name == 'inert')
    for l in range(len(d['tgt_of'])):
        dead = [r for ll, r in inert if ll == l]
        want = torch.ones(len(d['tgt_of'][l]), device=dev)
        want[dead] = 0
        assert torch.equal(a['live'][l], want)
        for r in dead:                                                    # exact zeros
            assert float(a['proj'][l][r]) == 0.0 and float(a['levelset'][l][r]) == 0.0 and not bool(a['grads'][l][r].any())
    if K.CASES[name].get('own_trees'):
        from tests import b2m_loss_ref as R
        sizes, _ = K.groups_of(d['level_sizes'])
        r = lambda t, s: F.interpolate(t, size=tuple(s), mode='bilinear', align_corners=False)
        edges = lambda t: [set((int(min(u, v)), int(max(u, v))) for u, v in e.tolist()) for e in np.asarray(t)]
        for g, size in enumerate(sizes):
            want = (R.mst_trees(r(torch.from_numpy(d['norm_img']), size)), R.mst_trees(r(torch.from_numpy(d['lst_feat']), size)))
            for got, w in zip((a['ctx'].img_tree[g], a['ctx'].lst_tree[g]), want):
                assert edges(got.cpu().numpy()) == edges(w), f'size {size}: the context built another tree than the restatement'


def test_three_groups_against_the_reference_fixture(dev):
    """tests/golden/box_solov2_loss.npz: the reference's own statements :334-367 in float32 take the place of ref32."""
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'box_solov2_loss.npz'))
    r64 = K.reference('three_groups', 'float64')
    L = len(r64['grads'])
    fix = dict(loss_boxpro=float(g['loss_boxpro']), loss_levelset=float(g['loss_levelset']), proj=[g[f'proj_{l}'] for l in range(L)],
               levelset=[g[f'levelset_{l}'] for l in range(L)], grads=[g[f'grad_{l}'] for l in range(L)], lst_grad=g['lst_grad'])
    _hold('three_groups', _run('three_groups', dev), refs=(fix, r64))


def test_inert_rows_read_nothing(dev):
    """With the inert rows' logits replaced by NaN, every loss and every gradient is bit-identical and the inert planes get exact zeros."""
    from tests import guarded as G
    a = _run('inert', dev)
    d = K.inputs('inert')
    poisoned = [p.copy() for p in d['ins_preds']]
    for l, r, _ in K.CASES['inert']['inert']:
        poisoned[l][r] = np.nan
    b = _run('inert', dev, dict(d, ins_preds=poisoned))
    for x, y in zip(_flat(a), _flat(b)):
        assert G.same(x, y), 'an inert row read something'


def test_no_rows_gives_two_zeros_connected_to_the_graph(dev):
    a = _run('no_rows', dev)
    assert float(a['loss_boxpro']) == 0.0 and float(a['loss_levelset']) == 0.0
    assert all(g.numel() == 0 for g in a['grads']) and not bool(a['lst_grad'].any())
    from boxinstseg_amd import BoxLevelSetLossContext, box_solov2_mask_losses
    d = K.inputs('no_rows')
    preds = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in d['ins_preds']]
    ctx = BoxLevelSetLossContext(torch.from_numpy(d['norm_img']).to(dev), torch.from_numpy(d['lst_feat']).to(dev), d['level_sizes'])
    lb, ll, _ = box_solov2_mask_losses(ctx, preds, [torch.from_numpy(m).to(dev) for m in d['masks']], [torch.from_numpy(t).to(dev) for t in d['tgt_of']],
                                       None, d['counts'])
    assert lb.requires_grad and ll.requires_grad and lb.dim() == 0


def test_refusals(dev):
    from boxinstseg_amd import BoxLevelSetLossContext, box_solov2_mask_losses
    d = K.inputs('odd')
    img, lst = torch.from_numpy(d['norm_img']).to(dev), torch.from_numpy(d['lst_feat']).to(dev)
    with pytest.raises(RuntimeError, match='CUDA'):
        BoxLevelSetLossContext(img.cpu(), lst.cpu(), d['level_sizes'])
    with pytest.raises(RuntimeError, match='float32'):
        BoxLevelSetLossContext(img.half(), lst.half(), d['level_sizes'])
    with pytest.raises(NotImplementedError, match='2 pixels'):
        BoxLevelSetLossContext(img, lst, [(1, 8)])
    with pytest.raises(NotImplementedError, match='distinct level sizes'):
        BoxLevelSetLossContext(img, lst, [(4, 4), (5, 5), (6, 6), (7, 7), (8, 8)])
    trees = [tuple(torch.from_numpy(t).to(dev) for t in pair) for pair in d['trees']]
    ctx = BoxLevelSetLossContext(img, lst, d['level_sizes'], trees)
    preds = [torch.from_numpy(p).to(dev) for p in d['ins_preds']]
    masks = [torch.from_numpy(m).to(dev) for m in d['masks']]
    tgt = [torch.from_numpy(t).to(dev) for t in d['tgt_of']]
    with pytest.raises(RuntimeError, match='float32'):
        box_solov2_mask_losses(ctx, [p.half() for p in preds], masks, tgt, None, d['counts'])
    with pytest.raises(RuntimeError, match='ins_pred_rows'):
        box_solov2_mask_losses(ctx, preds, masks, tgt, None, [[1, 1], [1, 2]])
    with pytest.raises(RuntimeError, match='uint8'):
        box_solov2_mask_losses(ctx, preds, [m.float() for m in masks], tgt, None, d['counts'])
