"""GPU: the kernels of csrc/corr.hip at the queue lengths, object counts, channel counts, solver settings and canvases of
tests/corr_edges.py, which tests/test_host_corr_edges.py shows to be what they claim.  The referee is tests/corr_ref.py in fp64 on the same
inputs; a case's conditions (no near tie among the arg-maxes of C, no score near its threshold) are asserted again before its GPU call.

Exact: count, ret_slot, ret_src, assign, num_ins, the bank and ptr afterwards, which elements of iiu are zero; the scores of the
block-mask case, bit for bit against the fp32 restatement, and the slots that pass with a threshold on a score and one ulp beside it;
superres_T of one-hot planes.  Toleranced as in tests/test_gpu_corr.py (its ``close``): Cu, C, loss_sum, the gradient, iiu.  Toleranced
by 4 x the fp32 restatement's own difference from the fp64 one, taken from the restatement alone: the scores of the generic cases
(pooled over the cases, as the fixture's tol_* are: a handful of slots can be exact in fp32 by chance), superres_T and the gradient of Cu
(per run).  What each test is the first to reach:

    many                 the second trip of the plan loop (j >= 256), compaction blocks 1..4, rank >= total - L, the wrap of ptr,
                         in_call_source with several objects of a call on one slot, > against >= of min_size, one dead retrieval wave
    queue100             slot groups 1..24 of the retrieval (blockIdx.y > 0), K = 8, min_objs = 1 with one retrieved object
    queue1..3[_one_class] three, two and one dead waves of the retrieval workgroup at its barriers; a queue made of in-call entries
    c15 / c16 / c17      one partial 16-channel stage / exactly one / a second stage of one channel (four channel groups idle)
    iter0, smooth0, dist1, dist13, it1sm3d3, dist1_it1, dist13_it1
                         no round (C = Cu on the window), the C = Cu + C branch, radius 0, radius 6 (everything near), three smoothing steps
    zero_cells           n > 0.0 ? ... : 0.0 of the gradient, an all-zero row and an all-zero column of Cu
    paste                blockIdx.y > 0 of the paste, the src < 0 clamp of its taps (h, w > 28), (int) of fractional corners, w = 1
    clip                 y >= y1 and x >= x1 with negative corners, boxes past the last row and column, a box wholly outside
    labels               the label checks of plan, retrieval, solve, ci, paste and append
    exact scores         > against >= of fg, bg and appearance, >= and <= of the ratio, 0 / 0 and x / 0 of a slot never written
    superres, solve      bxi_corr_superres_f32 and bxi_corr_cu_backward_f32 against the restatement (K = 1 and 8, C = 1 .. 17, a zero cell)
"""
import numpy as np
import pytest
import torch

from tests import corr_edges as E
from tests import corr_ref as R
from tests.test_gpu_corr import close

pytestmark = pytest.mark.gpu

NAMES = tuple(n for n in E.FUSED if n != 'clip_padded') + ('clip',)
_RUNS = {}


def launch(dev, c, thresholds=None):
    """One fused call on the case ``c`` (thresholds: overrides of the bank's), with the backward pass."""
    from boxinstseg_amd import ObjectBank, SemanticCorrSolver, corr_objects
    inp, cfg = c['inp'], dict(c['cfg'], **(thresholds or {}))
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    num_class, L, C = inp['bank_feature'].shape[:3]
    bank = ObjectBank(num_class, L, cfg['fg_iou_thresh'], cfg['bg_iou_thresh'], cfg['ratio_range'], cfg['appear_thresh'], cfg['max_retrieval_objs'])
    bank.ensure(C, dev)
    bank.feature.copy_(t['bank_feature']); bank.mask.copy_(t['bank_mask']); bank.box.copy_(t['bank_box']); bank.ptr.copy_(t['bank_ptr'])
    solver = SemanticCorrSolver(cfg['corr_exp'], cfg['corr_eps'], cfg['gaussian_filter_size'], cfg['low_score'], cfg['corr_num_iter'],
                                cfg['corr_num_smooth_iter'], cfg['dist_kernel'])
    s_feat = t['s_feat'].clone().requires_grad_(True)
    d = {}
    loss, num_ins, iiu = corr_objects(s_feat, t['s_mask'], t['t_feat'], t['t_mask'], t['boxes'], t['labels'], bank, solver, c['hw'], cfg['min_size'],
                                      cfg['min_objs'], details=d)
    loss.backward()
    d.pop('grad')
    return dict(bank=bank, loss=loss.detach(), num_ins=int(num_ins), iiu=iiu, grad=s_feat.grad, **d)


def run(dev, name):
    if name not in _RUNS:
        E.assert_conditions('clip_padded' if name == 'clip' else name)           # before the GPU call
        _RUNS[name] = launch(dev, E.case(name))
    return _RUNS[name]


def within(got, want64, tol, what):
    """``close`` of tests/test_gpu_corr.py with a relative tolerance that the restatement gave: the finite elements within
    MARGIN x tol x the largest fp64 magnitude, NaN and the infinities where the restatement has them."""
    got, want = got.detach().double().cpu(), want64.double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]), what
    top = float(want[fin].abs().max()) if bool(fin.any()) else 0.0
    err = float((got[fin] - want[fin]).abs().max()) if bool(fin.any()) else 0.0
    bound = E.MARGIN * tol * top
    print(f'{what}: max error {err:.3e}, bound {bound:.3e} (largest magnitude {top:.3e}, fp32 against fp64 restatement {tol:.3e})')
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e}'


@pytest.mark.parametrize('name', NAMES)
def test_exact_parts(dev, name):
    r, w = run(dev, name), E.want(name)
    assert torch.equal(r['count'].cpu().long(), w['count'])
    assert torch.equal(r['ret_slot'].cpu().long(), w['ret_slot'])
    assert torch.equal(r['ret_src'].cpu().long(), w['ret_src'])
    assert torch.equal(r['assign'].cpu().long(), w['assign'])
    assert r['num_ins'] == w['num_ins']
    bank = r['bank']
    for mine, key in ((bank.feature, 'after_feature'), (bank.mask, 'after_mask'), (bank.box, 'after_box')):
        assert torch.equal(mine.cpu(), w[key].float()), key
    assert torch.equal(bank.ptr.cpu(), w['after_ptr'])
    assert torch.equal(r['iiu'].cpu() == 0, w['iiu'] == 0)


@pytest.mark.parametrize('name', NAMES)
def test_toleranced_parts(dev, name):
    r, w = run(dev, name), E.want(name)
    close(r['Cu'], w['Cu'], 'Cu', 'Cu')
    close(r['C'], w['C'], 'C', 'C')
    close(r['loss'], w['loss_sum'], 'loss_sum', 'loss_sum')
    close(r['grad'], w['grad'], 'grad', 'gradient')
    close(r['iiu'], w['iiu'], 'iiu', 'iiu')


@pytest.mark.parametrize('name', NAMES)
def test_generic_scores(dev, name):
    r, w, tols = run(dev, name), E.want(name), E.score_tols()
    for k, what in enumerate(('fg IoU', 'bg IoU', 'appearance', 'box ratio')):
        within(r['scores'][..., k], w['scores'][..., k], tols[k], what)


def test_labels_outside_the_range(dev):
    """Two objects of the fixture's 'plain' case with labels -1 and num_class: they retrieve nothing, get no iiu and no gradient and
    are not appended, and everything else is bit-identical to the call without them."""
    E.assert_conditions('labels')
    a, b, w = launch(dev, E.case('labels')), launch(dev, E.case('labels_removed')), E.want('labels')
    keep = [i for i in range(len(w['count'])) if i not in E.BAD_LABELS]
    for i in E.BAD_LABELS:
        assert int(a['count'][i]) == 0 and bool((a['ret_slot'][i] == -1).all()) and bool((a['ret_src'][i] == -1).all()) and int(a['obj_slot'][i]) == -1
        assert bool((a['iiu'][i] == 0).all()) and bool((a['grad'][i] == 0).all()) and bool((a['assign'][i] == -1).all())
    assert torch.equal(a['count'].cpu().long(), w['count']) and torch.equal(a['ret_slot'].cpu().long(), w['ret_slot']) and a['num_ins'] == w['num_ins'] == b['num_ins']
    for k in ('count', 'ret_slot', 'assign', 'Cu', 'C', 'iiu', 'grad', 'scores'):
        x, y = a[k][keep], b[k]
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), k
    remap = torch.tensor([keep.index(i) if i in keep else -1 for i in range(len(w['count']))] + [-1], device=dev, dtype=torch.int32)
    assert torch.equal(remap[a['ret_src'][keep].long()], b['ret_src'])           # the same objects under their indices in the shorter call
    assert torch.equal(a['loss'], b['loss'])
    for x, y in ((a['bank'].feature, b['bank'].feature), (a['bank'].mask, b['bank'].mask), (a['bank'].box, b['bank'].box), (a['bank'].ptr, b['bank'].ptr)):
        assert torch.equal(x, y)
    assert torch.equal(a['bank'].ptr.cpu(), w['after_ptr']) and torch.equal(a['bank'].feature.cpu(), w['after_feature'].float())


@pytest.mark.parametrize('setting', list(E.threshold_settings()) + ['zero_query'])
def test_exact_scores_and_thresholds(dev, setting):
    """Scores bit-identical to ``R.slot_scores`` in fp32 on the CPU; the passing slots are the restatement's under every threshold."""
    zero_query = setting == 'zero_query'
    th = E.WIDE if zero_query else E.threshold_settings()[setting][0]
    c = E.exact_case(zero_query)
    r = launch(dev, c, th)
    want = E.exact_scores(zero_query=zero_query)
    got = r['scores'][0].cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got).view(torch.int32), torch.nan_to_num(want).view(torch.int32)), (got.tolist(), want.tolist())
    passing = E.exact_passing(th, zero_query)
    assert r['ret_slot'][0, :int(r['count'][0])].cpu().tolist() == passing and int(r['count'][0]) == len(passing)
    assert r['num_ins'] == 0 and torch.equal(r['bank'].feature.cpu(), torch.from_numpy(c['inp']['bank_feature'])) and r['bank'].ptr.cpu().tolist() == [0]


@pytest.mark.parametrize('K', E.SUPERRES_KS)
def test_superres_against_the_restatement(dev, K):
    from boxinstseg_amd import superres_T
    got = superres_T(torch.from_numpy(E.superres_T(K)).to(dev))
    within(got, E.superres_want(K), E.superres_tol(K), f'superres_T K = {K}')


def test_superres_of_one_hot_planes_is_exact(dev):
    from boxinstseg_amd import superres_T
    T = torch.from_numpy(E.onehot_T())
    got = superres_T(T.to(dev)).cpu()
    want = R.superres(T.double())
    assert torch.equal(got.double(), want) and int((want != 0).sum()) > 0


class _Query:
    def __init__(self, mask):
        self.mask = mask


@pytest.mark.parametrize('run_', E.SOLVE_RUNS, ids=lambda r: f'K{r[0]}-C{r[1]}' + ('-zero' if r[2] else ''))
def test_solve_and_backward_against_autograd(dev, run_):
    """``SemanticCorrSolver.solve`` and the backward of its Cu for a random upstream gradient, against autograd through ``R.solve``."""
    from boxinstseg_amd import SemanticCorrSolver
    K, C, _ = run_
    want_Cu, want_grad = E.solve_want(*run_)
    tol = E.solve_tol(run_)                                                      # from the restatement, before the GPU call
    f0, f1, g = (torch.from_numpy(a).to(dev) for a in E.solve_inputs(*run_))
    f0.requires_grad_(True)
    cfg = E.CFG
    solver = SemanticCorrSolver(cfg['corr_exp'], cfg['corr_eps'], cfg['gaussian_filter_size'], cfg['low_score'], cfg['corr_num_iter'],
                                cfg['corr_num_smooth_iter'], cfg['dist_kernel'])
    Cu, Cm, _, _ = solver.solve(_Query(torch.zeros(1, 28, 28, device=dev)), dict(feature=f1, mask=torch.zeros(K, 28, 28, device=dev)), f0)
    (Cu * g).sum().backward()
    close(Cu, want_Cu, 'Cu', 'Cu')
    assert tuple(Cm.shape) == (K, 49, 49) and bool(torch.isfinite(Cm).all())
    within(f0.grad, want_grad, tol, f'gradient of Cu, K = {K}, C = {C}')
