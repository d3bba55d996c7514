"""GPU: Box2MaskHead.loss for all decoder layers (boxinstseg_amd/box2mask_loss.py on csrc/box2mask_loss.hip) against the per-instance
restatement of tests/b2m_loss_ref.py, on the cases of tests/b2m_cases.py (tests/test_host_b2m_loss.py takes their census).

TOLERANCE, the project's rule: every loss and every gradient element lies within max(4 |ref32 - ref64|, floor) of the fp64 restatement,
ref32 being the same restatement in float32.  The floor is 1e-4 of the tensor's largest magnitude (tests/test_gpu_levelset.py) for the
losses and the gradient of every layer's logits; for ``lst_feat.grad`` it is tests/test_gpu_tree_filter.py's bound on the embedding
gradient, EMB_GRAD_TOL * max(|gw|max, 1) per element of the 96x96 embedding, carried through the adjoint of the two resizes (each
element's bound times the column sum of the resize that reaches it; gw: the restatement's weight gradient, summed as the shared tree
sums it).  No element is skipped.  The largest share of the bound reached on an MI355X is in profiles/NOTES.md (R29-1).

In every case: two runs are bit-identical, and ``box2mask_mask_losses`` runs under torch.cuda.set_sync_debug_mode('error')."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import b2m_cases as K
from tests.test_gpu_tree_filter import EMB_GRAD_TOL

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev_inputs(name, dev):
    d = K.inputs(name)
    preds = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in d['mask_preds']]
    lst = torch.from_numpy(d['lst_feat']).to(dev).requires_grad_(True)
    img = torch.from_numpy(d['norm_img']).to(dev)
    gts = [torch.from_numpy(g).to(dev) for g in d['gt_masks']]
    pos = [torch.from_numpy(p).to(dev) for p in d['pos']]
    pos_gt = [torch.from_numpy(p).to(dev) for p in d['pos_gt']]
    trees = None if d['trees'] is None else tuple(torch.from_numpy(t).to(dev) for t in d['trees'])
    return d, preds, lst, img, gts, pos, pos_gt, trees


def _run(name, dev):
    from boxinstseg_amd import Box2MaskLossContext, box2mask_mask_losses
    c = K.CASES[name]
    d, preds, lst, img, gts, pos, pos_gt, trees = _dev_inputs(name, dev)
    ctx = Box2MaskLossContext(img, lst, c['pred'], gts, c['small'], trees)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp, ll = box2mask_mask_losses(ctx, preds, pos, pos_gt, d['counts'], K.LOSS_BOX_WEIGHT, K.LOSS_MASK_WEIGHT)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    (lp.sum() + ll.sum()).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss_project=lp.detach(), loss_levelset=ll.detach(), grads=[zero(p) for p in preds], lst_grad=zero(lst), ctx=ctx)


def _flat(run):
    return [run['loss_project'], run['loss_levelset'], *run['grads'], run['lst_grad']]


def _lst_floor(name, r64):
    """EMB_GRAD_TOL * max(gw, 1) per embedding element, through the adjoint of lst_feat -> pred_shape -> scaled_size: the column sums."""
    c = K.CASES[name]
    d = K.inputs(name)
    x = torch.ones((d['B'], 1) + tuple(d['lst_feat'].shape[-2:]), dtype=torch.float64, requires_grad=True)
    r = lambda t, s: F.interpolate(t, size=tuple(s), mode='bilinear', align_corners=False)
    r(r(x, c['pred']), c['small']).sum().backward()
    scale = EMB_GRAD_TOL * np.maximum(r64['gw_sum'], 1.0)
    return x.grad.numpy() * scale[:, None, None, None]


def _bounds(name, r32, r64):
    """(what, ref32, ref64, bound) per tensor: the project's rule, elementwise."""
    L = len(r64['grads'])
    items = [('loss_project', r32['loss_project'], r64['loss_project'], None), ('loss_levelset', r32['loss_levelset'], r64['loss_levelset'], None)]
    items += [(f'grad[{l}]', r32['grads'][l], r64['grads'][l], None) for l in range(L)]
    items.append(('lst_grad', r32['lst_grad'], r64['lst_grad'], _lst_floor(name, r64)))
    return [(what, a64, np.maximum(4.0 * np.abs(a32 - a64), TOL * max(np.abs(a64).max(), 1e-12) if floor is None else floor))
            for what, a32, a64, floor in items]


def _hold(name, run, shares=None, refs=None):
    r32, r64 = refs or (K.reference(name, 'float32'), K.reference(name, 'float64'))
    worst = 0.0
    items = [('loss_project', run['loss_project'], r32['loss_project'], r64['loss_project'], None),
             ('loss_levelset', run['loss_levelset'], r32['loss_levelset'], r64['loss_levelset'], None)]
    items += [(f'grad[{l}]', g, r32['grads'][l], r64['grads'][l], None) for l, g in enumerate(run['grads'])]
    items.append(('lst_grad', run['lst_grad'], r32['lst_grad'], r64['lst_grad'], _lst_floor(name, r64)))
    for what, got, a32, a64, floor in items:
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == a64.shape, (what, got.shape, a64.shape)
        assert np.isfinite(got).all(), what
        if floor is None:
            floor = TOL * max(np.abs(a64).max(), 1e-12)
        tol = np.maximum(4.0 * np.abs(a32 - a64), floor)
        err = np.abs(got - a64)
        # (an element of lst_feat that no resized pixel reads has a bound of exactly 0: its gradient is exactly 0 on both sides)
        assert (err[tol == 0] == 0).all(), f'{name}: {what}: an element with a zero bound is off'
        share = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
        print(f'{name}: {what}: max |want| {np.abs(a64).max() if a64.size else 0:.4g}, largest share of the bound {share:.3g}')
        worst = max(worst, share)
        assert share <= 1.0, f'{name}: {what}: {share:.3g} of the bound'
    if shares is not None:
        shares[name] = worst
    return worst


@pytest.mark.parametrize('name', [n for n in K.CASES if n not in ('hand', 'all_g0', 'inert')])
def test_case_against_the_restatement(dev, name):
    from tests import guarded as G
    a = _run(name, dev)
    b = _run(name, dev)
    for x, y in zip(_flat(a), _flat(b)):
        assert G.same(x, y), 'two runs differ'
    _hold(name, a)
    if K.CASES[name].get('own_trees'):
        from tests import b2m_loss_ref as R
        c, d = K.CASES[name], K.inputs(name)
        r = lambda t, s: F.interpolate(t, size=tuple(s), mode='bilinear', align_corners=False)
        want = (R.mst_trees(r(r(torch.from_numpy(d['norm_img']), c['pred']), c['small'])),
                R.mst_trees(r(r(torch.from_numpy(d['lst_feat']), c['pred']), c['small'])))
        for got, w in zip((a['ctx'].img_tree, a['ctx'].lst_tree), want):
            edges = lambda t: [set((int(min(u, v)), int(max(u, v))) for u, v in e.tolist()) for e in np.asarray(t)]
            assert edges(got.cpu().numpy()) == edges(w), 'the context built another tree than the restatement'


def test_every_image_without_ground_truth_is_the_zero_match_branch(dev):
    a = _run('all_g0', dev)
    assert a['loss_project'].tolist() == [0.0, 0.0] and a['loss_levelset'].tolist() == [0.0, 0.0]
    assert all(not bool(g.any()) for g in a['grads']) and not bool(a['lst_grad'].any())
    _hold('all_g0', a)


def test_inert_image_leaves_the_other_image_unchanged_bit_for_bit(dev, monkeypatch):
    """Image 0's slots hold -1 in both layers.  Nothing is read through an inert row: with image 0's logits replaced by NaN and its ground
    truths by other boxes, every loss and every gradient is bit-identical and image 0 gets exact zeros.  And the same call with image 0
    carrying no ground truth at all has the same live rows: the losses are per layer, not per image, and their sums run over another
    number of slots (the inert ones add exact zeros), so they and the gradients agree to a reordering of S fp32 additions."""
    from tests import guarded as G
    a = _run('inert', dev)
    b = _run('inert', dev)
    for x, y in zip(_flat(a), _flat(b)):
        assert G.same(x, y)
    _hold('inert', a)
    d = K.inputs('inert')
    n0 = d['n'][0]
    poisoned = [p.copy() for p in d['mask_preds']]
    for p in poisoned:
        p[0] = np.nan
    other = dict(d, mask_preds=poisoned, gt_masks=[np.ones_like(d['gt_masks'][0]), d['gt_masks'][1]])
    monkeypatch.setattr(K, 'inputs', lambda name: other)
    c = _run('inert', dev)
    for x, y in zip(_flat(a), _flat(c)):
        assert G.same(x, y), 'an inert row read something'
    assert all(not bool(g[0].any()) for g in a['grads']) and not bool(a['lst_grad'][0].any())
    alone = dict(d, gt_masks=[d['gt_masks'][0][:0], d['gt_masks'][1]], pos=[p[n0:] for p in d['pos']], pos_gt=[p[n0:] for p in d['pos_gt']],
                 counts=[0, d['counts'][1]], n=[0, d['n'][1]])
    monkeypatch.setattr(K, 'inputs', lambda name: alone)
    e = _run('inert', dev)
    S = sum(d['n'])
    for x, y in zip(_flat(a), _flat(e)):
        assert float((x - y).abs().max()) <= S * 2.0 ** -23 * float(y.abs().max())


def test_hand_case_is_exact(dev):
    """All logits 0 on a constant image, every resize the identity: p == 0.5 exactly, both level-set energies and the LCM term vanish."""
    from boxinstseg_amd.box2mask_loss import _Scores, build_row_table
    a = _run('hand', dev)
    assert a['loss_levelset'].tolist() == [0.0, 0.0]
    _hold('hand', a)
    d, preds, lst, img, gts, pos, pos_gt, trees = _dev_inputs('hand', dev)
    table = build_row_table(pos, pos_gt, d['counts'], d['B'], K.CASES['hand']['Q'], [0, 1, 3])
    row_plane = table[0]
    plane_row = torch.full((2, d['B'] * 3), -1, dtype=torch.int32, device=dev)
    p, ps = _Scores.apply(row_plane, plane_row, (16, 16), *preds)
    assert bool((p == 0.5).all()) and bool((ps == 0.5).all())


def test_index_order_at_the_c_abi(dev):
    """img_of and tgt_of permuted, not monotone: every row's loss and gradient equal, bit for bit, the row's values in the sorted call."""
    from boxinstseg_amd import _lib
    from tests import guarded as G
    lib = _lib.load()
    rng = np.random.default_rng(5)
    M, Gn, B, C, h, w = 7, 4, 3, 3, 19, 23
    p = torch.from_numpy(rng.random((M, h, w)).astype(np.float32)).to(dev)
    T = torch.from_numpy((rng.random((Gn, h, w)) > 0.4).astype(np.float32) * rng.random((Gn, h, w)).astype(np.float32)).to(dev)
    img = torch.from_numpy(rng.standard_normal((B, C, h, w)).astype(np.float32)).to(dev)
    aff = torch.softmax(torch.from_numpy(rng.standard_normal((B, 8, h, w)).astype(np.float32)), 1).contiguous().to(dev)
    pn = T.sum((1, 2)).clamp(min=1)
    gl = torch.from_numpy(rng.random(M).astype(np.float32)).to(dev)
    tgt = np.array([3, 0, 2, 2, 1, 0, 3], np.int32)
    im = np.array([2, 0, 1, 0, 2, 1, 0], np.int32)

    def call(order):
        o = torch.from_numpy(order).to(dev)
        pp = p[o.long()].contiguous()
        t_of, i_of = torch.from_numpy(tgt[order]).to(dev), torch.from_numpy(im[order]).to(dev)
        loss = torch.empty(M, device=dev)
        state = torch.empty(lib.bxi_b2m_levelset_state_bytes(M, C) // 8, dtype=torch.float64, device=dev)
        G.ok(lib.bxi_b2m_levelset_forward_f32(pp.data_ptr(), T.data_ptr(), img.data_ptr(), 1, t_of.data_ptr(), i_of.data_ptr(), pn.data_ptr(), M,
                                              Gn, B, C, h, w, 1.0, loss.data_ptr(), state.data_ptr(), G.stream(dev)))
        gp = torch.empty_like(pp)
        G.ok(lib.bxi_b2m_levelset_backward_f32(pp.data_ptr(), T.data_ptr(), img.data_ptr(), 1, t_of.data_ptr(), i_of.data_ptr(), pn.data_ptr(), M,
                                               Gn, B, C, h, w, 1.0, state.data_ptr(), gl[o.long()].contiguous().data_ptr(), gp.data_ptr(), None,
                                               G.stream(dev)))
        out = torch.empty_like(pp)
        ws = torch.empty(max(lib.bxi_lcm_workspace_bytes(M, h, w), 16), dtype=torch.uint8, device=dev)
        G.ok(lib.bxi_b2m_lcm_refine_f32(aff.data_ptr(), pp.data_ptr(), i_of.data_ptr(), B, M, h, w, 2, 10, 0, out.data_ptr(), ws.data_ptr(),
                                        ws.numel(), G.stream(dev)))
        return loss, gp, out

    ident = np.arange(M, dtype=np.int64)
    perm = np.array([4, 2, 6, 0, 5, 1, 3], np.int64)
    l0, g0, r0 = call(ident)
    l1, g1, r1 = call(perm)
    pt = torch.from_numpy(perm).to(dev)
    assert G.same(l1, l0[pt]) and G.same(g1, g0[pt]) and G.same(r1, r0[pt])
    # and the refinement through img_of equals bxi_lcm_refine_f32 on the gathered affinities
    from boxinstseg_amd.levelset import _refine
    want = _refine(aff[torch.from_numpy(im).to(dev).long()].contiguous(), p, 2, 10, 0)
    assert G.same(r0, want)


@pytest.mark.parametrize('name', list(K.CASES))
def test_box2mask_loss_against_the_per_layer_composition(dev, name):
    """``box2mask_loss`` with its own assignment, against (1) the fp64 restatement under that assignment, by the project's rule, and (2)
    loss_single composed per layer from the package's existing modules (tests/b2m_compose.py).  The composition is one more fp32
    evaluation of the same statements -- torch's own resizes and the per-instance kernels --, so it gets the same allowance against the
    fp64 restatement as the new path: the two lie within twice the rule's bound of each other, elementwise.  ``loss_cls`` is the same
    torch expression on both sides up to the order of one sum: 2 TOL."""
    from boxinstseg_amd import MaskHungarianAssigner, box2mask_loss, parse_box2mask_head_cfg
    from tests import b2m_compose as P
    from tests import b2m_loss_ref as R
    from tests import guarded as G
    c = K.CASES[name]
    d, preds, lst, img, gts, _, _, trees = _dev_inputs(name, dev)
    L, classes = len(preds), 4
    rng = np.random.default_rng(11)
    cls = [torch.from_numpy(rng.standard_normal((d['B'], c['Q'], classes + 1)).astype(np.float32)).to(dev).requires_grad_(True) for _ in preds]
    labels = [torch.from_numpy(rng.integers(0, classes, g)).to(dev) for g in c['G']]
    kw = parse_box2mask_head_cfg(dict(type='Box2MaskHead', num_things_classes=classes, num_stuff_classes=0, num_queries=c['Q'],
                                      loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=2.0, reduction='mean',
                                                    class_weight=[1.0] * classes + [0.1]),
                                      loss_mask=dict(type='LevelsetLoss', loss_weight=1.0), loss_box=dict(type='BoxProjectionLoss', loss_weight=5.0)))
    assigner = MaskHungarianAssigner(cls_cost=dict(type='ClassificationCost', weight=2.0),
                                     dice_cost=dict(type='BoxMatchingCost', weight=5.0, pred_act=True, eps=1.0))
    leaves = preds + cls + [lst]
    keys = ['loss_cls', 'loss_project', 'loss_levelset']
    order = [f'd{l}.{k}' for l in range(L - 1) for k in keys] + keys

    def evaluate(fn):
        for t in leaves:
            t.grad = None
        out = fn()
        assert sorted(out) == sorted(order)
        sum(out.values()).backward()
        return ({k: out[k].detach().clone() for k in order}, [torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in leaves])

    new = lambda: box2mask_loss(cls, preds, [lst] * L, labels, gts, None, img, assigner=assigner, scaled_size=c['small'], trees=trees, **kw)
    a, b = evaluate(new), evaluate(new)
    assert all(G.same(a[0][k], b[0][k]) for k in order) and all(G.same(x, y) for x, y in zip(a[1], b[1])), 'two runs differ'
    comp = evaluate(lambda: P.loss(cls, preds, lst, labels, gts, img, assigner=assigner, scaled_size=c['small'], **kw))
    # the assignment both used, and the restatement under it
    n, pos, pos_gt = d['n'], [], []
    off = np.concatenate([[0], np.cumsum(n)])
    for l in range(L):
        _, _, p_l, g_l, _ = assigner.assign_batch(cls[l].detach(), preds[l].detach(), labels, gts)
        p_l, g_l = p_l.cpu().numpy(), g_l.cpu().numpy()
        pos.append([p_l[off[i]:off[i + 1]].tolist() for i in range(d['B'])])
        pos_gt.append([g_l[off[i]:off[i + 1]].tolist() for i in range(d['B'])])
    refs = [R.all_layers(d['mask_preds'], d['lst_feat'], d['norm_img'], d['gt_masks'], pos, pos_gt, dt, c['small'], d['trees'], 5.0, 1.0)
            for dt in (torch.float32, torch.float64)]
    layer = lambda k: L - 1 if '.' not in k else int(k.split('.')[0][1:])
    def as_run(ev):
        per = lambda key: torch.stack([ev[0][k] for k in sorted((k for k in order if k.endswith(key)), key=layer)])
        return dict(loss_project=per('loss_project'), loss_levelset=per('loss_levelset'), grads=ev[1][:L], lst_grad=ev[1][-1])
    mine, theirs = as_run(a), as_run(comp)
    _hold(name, mine, refs=refs)
    for (what, _, bound), x, y in zip(_bounds(name, *refs), _flat(mine), _flat(theirs)):
        err = (x - y).abs().cpu().numpy().astype(np.float64)
        assert (err <= 2.0 * bound).all(), f'{name}: {what}: new path and composition differ by {float((err / np.maximum(2.0 * bound, 1e-300)).max()):.3g} of the bound'
    for k in order:
        if k.endswith('loss_cls'):
            assert abs(float(a[0][k]) - float(comp[0][k])) <= 2 * TOL * abs(float(comp[0][k])), k
    for x, y in zip(a[1][L:2 * L], comp[1][L:2 * L]):                          # d loss_cls / d cls_scores
        assert float((x - y).abs().max()) <= 2 * TOL * max(float(y.abs().max()), 1e-12)


def test_refusals(dev):
    from boxinstseg_amd import Box2MaskLossContext, box2mask_mask_losses
    d, preds, lst, img, gts, pos, pos_gt, trees = _dev_inputs('q_lt_g', dev)
    c = K.CASES['q_lt_g']
    with pytest.raises(RuntimeError, match='CUDA'):
        Box2MaskLossContext(img.cpu(), lst.detach().cpu(), c['pred'], [g.cpu() for g in gts], c['small'])
    with pytest.raises(RuntimeError, match='float32'):
        Box2MaskLossContext(img.half(), lst.detach().half(), c['pred'], gts, c['small'])
    ctx = Box2MaskLossContext(img, lst, c['pred'], gts, c['small'], trees)
    with pytest.raises(RuntimeError, match='float32'):
        box2mask_mask_losses(ctx, [p.detach().half() for p in preds], pos, pos_gt, d['counts'])
    with pytest.raises(NotImplementedError, match='at most 16'):
        box2mask_mask_losses(ctx, [preds[0]] * 17, [pos[0]] * 17, [pos_gt[0]] * 17, d['counts'])
