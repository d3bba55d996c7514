"""Host: the premise of tests/test_gpu_dynamic_head_exact.py, checked without a device for every case that file runs.

On the dyadic cases of tests/dyn_exact.py the dynamic mask head is exact in fp32, so a kernel owes the fp64 result bit for bit.
That is a claim about the cases, and it is established here: (1) the derived bound -- sum|terms| / (quantum * 2^24) < 1 for every
reduction of the forward and the backward --, (2) the reference evaluated in fp32 and in fp64 agrees exactly, (3) the ReLU
pre-activations hit zero exactly, and fall on both sides of it, often enough that the gate rule at zero is exercised, (4) one tiny
case counted by hand."""
import numpy as np
import pytest
import torch

from tests import dyn_exact as X


SPECS = [pytest.param(('plain', a, k), id=X.spec_name(a, k).replace(' ', '-')) for a, k in X.all_cases()] + \
        [pytest.param(('fused', f), id='fused-C%d-rel%d-N%d' % (f[0], f[1], f[5])) for f in X.FUSED]
_BUILT = {}


@pytest.fixture
def c(request):
    """The case of a spec, drawn once per session."""
    spec = request.param
    key = repr(spec)
    if key not in _BUILT:
        _BUILT[key] = X.dyadic_case(*spec[1], **spec[2]) if spec[0] == 'plain' else X.fused_batch(*spec[1])[2]
    return _BUILT[key]


@pytest.mark.parametrize('c', SPECS, indirect=True)
def test_premise_every_partial_sum_is_exact(c):
    """order_free_ratio < 1 for every quantity: a condition on the case (its densities were lowered until it held), not a measurement."""
    r = X.order_free_ratio(c)
    worst = max(r, key=r.get)
    print(f'{X.name_of(c)}: largest premise ratio {r[worst]:.4f} ({worst}); ' + ' '.join(f'{k}={v:.4f}' for k, v in r.items()))
    for k, v in r.items():
        assert v < 1, (X.name_of(c), k, v)


@pytest.mark.parametrize('c', SPECS, indirect=True)
def test_fp32_and_fp64_evaluations_agree_exactly(c):
    want = [a.astype(np.float32) for a in X.expected(c, torch.float64)]
    got = X.expected(c, torch.float32)
    for what, g, w in zip(('logits', 'd_feat', 'd_params'), got, want):
        assert not X.first_difference(c, what, g, w), X.first_difference(c, what, g, w)
    # the layer-by-layer restatement (the source of the premise, of the gate statistics and of the NaN-feature expectation) is the
    # same function, in both precisions
    for dtype in (torch.float64, torch.float32):
        r = X.restate(c, dtype)
        for what, g, w in zip(('logits', 'd_feat', 'd_params'), (r['logits'], r['d_feat'], r['d_params']), want):
            d = X.first_difference(c, what, g.numpy().astype(np.float32), w)
            assert not d, d
    if X.is_tuned(c):                                      # the two references (grouped convolutions / batched products) agree
        for what, g, w in zip(('logits', 'd_feat', 'd_params'), X.expected(c, torch.float64, general=True), want):
            d = X.first_difference(c, what, g.astype(np.float32), w)
            assert not d, d


@pytest.mark.parametrize('c', [p for p in SPECS if p.values[0][0] == 'fused' or p.values[0][2].get('layers', 3) > 1], indirect=True)
def test_relu_gates_are_exercised_at_zero(c):
    """ReLU's derivative at exactly 0 is 0 in the reference and in the kernels (`> 0.f`): the cases must visit that point, and both
    sides of it, in numbers -- at least one pre-activation in 64 exactly zero, at least one in 8 on each side."""
    pre = torch.cat([p.flatten() for p in X.restate(c)['pre']])
    zero, pos, neg = (float((pre == 0).double().mean()), float((pre > 0).double().mean()), float((pre < 0).double().mean()))
    print(f'{X.name_of(c)}: pre-activations zero {zero:.3f} positive {pos:.3f} negative {neg:.3f}')
    assert zero * 64 >= 1 and pos * 8 >= 1 and neg * 8 >= 1, (zero, pos, neg)


@pytest.mark.parametrize('c', SPECS, indirect=True)
def test_cases_are_dealt_as_described(c, request):
    assert np.all(np.mod(c['coors'], 64) == 4)
    assert set(np.unique(c['lvl'])) == set(range(min(5, c['N'])))
    for k in ('feat', 'params'):
        assert np.all(np.mod(c[k] * 2, 1) == 0) and np.abs(c[k]).max() <= 1 and not np.signbit(c[k][c[k] == 0]).any()
    assert set(np.unique(c['g'])) <= {-1.0, 0.0, 1.0}
    if not request.node.callspec.id.startswith('fused') and c['B'] > 1:
        per_image = np.bincount(c['img'], minlength=c['B'])
        assert (per_image == 0).sum() >= 1                              # an image without instances
        assert c['B'] < 3 or len(set(per_image[per_image > 0])) > 1      # unevenly


def test_one_case_counted_by_hand():
    """2 x 3 map, factor 2, one instance, no relative coordinates; only feature channel 0 and seven parameters are non-zero.

        x            = [[1, -1, 1/2], [0, 1, -1/2]]
        h1[0]        = relu(x)  = [[1, 0, 1/2], [0, 1, 0]]          h1[1] = relu(-x) = [[0, 1, 0], [0, 0, 1/2]]
        pre2[0]      = h1[0] + h1[1] / 2 - 1/2 = [[1/2, 0, 0], [-1/2, 1/2, -1/4]]         (two exact zeros)
        y            = 2 relu(pre2[0]) - 1/2   = [[1/2, -1/2, -1/2], [-1/2, 1/2, -1/2]]
    aligned_bilinear by 2: output row R samples source row max(R - 1, 0) / 2 of y padded by a replicated row -- rows (r0, r0,
    (r0 + r1) / 2, r1); columns (c0, c0, (c0 + c1) / 2, c1, (c1 + c2) / 2, c2).  d y is its transpose applied to g."""
    C, H, W = 8, 2, 3
    feat = np.zeros((1, C, H, W), np.float32)
    feat[0, 0] = [[1, -1, 0.5], [0, 1, -0.5]]
    wsz, bsz = X.param_sizes(C, 3, 8)
    params = np.zeros((1, sum(wsz) + sum(bsz)), np.float32)
    params[0, 0 * C + 0] = 1                    # W0[0, 0]
    params[0, 1 * C + 0] = -1                   # W0[1, 0]
    params[0, wsz[0] + 0] = 1                   # W1[0, 0]
    params[0, wsz[0] + 1] = 0.5                 # W1[0, 1]
    params[0, wsz[0] + wsz[1] + 0] = 2          # W2[0]
    params[0, sum(wsz) + bsz[0] + 0] = -0.5     # b1[0]
    params[0, sum(wsz) + bsz[0] + bsz[1]] = -0.5  # b2
    g = np.array([[1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, -1], [0, 1, 0, 0, -1, 0], [0, 0, 0, 1, 0, 0]], np.float32).reshape(1, 1, 4, 6)
    c = dict(seed=0, B=1, C=C, H=H, W=W, N=1, factor=2, rel=False, layers=3, channels=8, feat=feat, params=params,
             coors=np.array([[4.0, 4.0]], np.float32), lvl=np.zeros(1, np.int64), img=np.zeros(1, np.int64), g=g)
    logits = np.array([[0.5, 0.5, 0, -0.5, -0.5, -0.5],
                       [0.5, 0.5, 0, -0.5, -0.5, -0.5],
                       [0, 0, 0, 0, -0.25, -0.5],
                       [-0.5, -0.5, 0, 0.5, 0, -0.5]], np.float32)
    d_y = np.array([[2, 0.25, -1.25], [0.5, 0.75, -0.25]], np.float32)
    for dtype in (torch.float64, torch.float32):
        r = X.restate(c, dtype)
        assert np.array_equal(r['logits'].numpy()[0, 0], logits)
        assert np.array_equal(r['d_y'].numpy()[0, 0], d_y)
        assert np.array_equal(r['pre'][1].numpy()[0, 0], np.array([[0.5, 0, 0], [-0.5, 0.5, -0.25]]))
        assert np.array_equal(X.expected(c, dtype)[0][0, 0], logits)
    # d b2 = sum d y = 2; the gate at pre2 = 0 is closed: d W2[0] = sum d y * h2[0] = 2 * 1/2 + 3/4 * 1/2
    gp = X.expected(c, torch.float64)[2][0]
    assert gp[sum(wsz) + bsz[0] + bsz[1]] == 2.0 and gp[wsz[0] + wsz[1]] == 1.375
    # d b1[0] = 2 * (d y where pre2[0] > 0) = 2 * (2 + 3/4): the two pixels at exactly 0 contribute nothing
    assert gp[sum(wsz) + bsz[0]] == 5.5


def test_slot_formula():
    """slots_for restates the host code of csrc/dynamic_head.hip; on 256 compute units the shapes of SLOTS give 8, 6, 3, 1, 8 at
    factor 2 and 4 / 8 at the other factors."""
    got = [X.slots_for(256, a[1], a[3], a[4], a[5], a[6]) for a, _ in X.SLOTS]
    assert got == [8, 6, 3, 1, 8, 4, 8, 4, 8], got
    assert X.slot_of(dict(img=np.array([1, 0, 1, 1, 0])), 3, 2) == 0 and X.slot_of(dict(img=np.array([1, 0, 1, 1, 0])), 4, 2) == 1
