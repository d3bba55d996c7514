"""Host: the references of tests/tree_filter_ref.py, checked without a device -- embed_grad against torch autograd through the closed
form of the filter, the group layout of module_reference, the oracle itself on weights of exactly 0, exactly 1 and fp32 subnormals, and
the preconditions of the weight regimes at the sizes tests/test_gpu_tree_filter.py runs them."""
import numpy as np
import pytest
import torch

from oracle import tree_filter_oracle as tfo
from tests import tree_filter_ref as R


def _grid_mst(H, W, rng):
    V = H * W
    idx = tfo.grid_edges(H, W)
    fm = rng.standard_normal((3, H, W)).astype(np.float32)
    return idx[tfo.mst_edges(idx, tfo.grid_weights(fm), V)]


@pytest.mark.parametrize('low_tree', [False, True], ids=['high', 'low'])
@pytest.mark.parametrize('H,W', [(6, 9), (1, 40)], ids=['mst6x9', 'strip40'])
def test_embed_grad_matches_autograd(H, W, low_tree):
    """d loss / d embedding = embed_grad(refine_backward_weight) against float64 autograd through out_i = sum_j S(i,j) x_j / sum_j S(i,j),
    S the path products of w = exp(-|e_i - e_parent|^2 / s) built from the torch embedding"""
    rng = np.random.default_rng(H * 100 + W + low_tree)
    V, Ce, C, sigma = H * W, 3, 2, 0.02
    si, sp, sc = tfo.bfs_order(_grid_mst(H, W, rng), V)
    if H == 1:
        assert np.array_equal(si, np.arange(V)) and np.array_equal(sp[1:], np.arange(V - 1))
    embed = rng.standard_normal((Ce, V)) * (0.05 if low_tree else 0.4)
    x = rng.standard_normal((C, V)); g = rng.standard_normal((C, V))
    w = tfo.edge_weights(embed, si, sp, low_tree, sigma)
    out, saved = tfo.refine_forward(x, w, si, sp, sc)
    gw = tfo.refine_backward_weight(x, g, w, si, sp, sc, saved)
    got = R.embed_grad(embed, gw, si, sp, low_tree, sigma)

    et = torch.tensor(embed, requires_grad=True)
    sit, spt = torch.from_numpy(si).long(), torch.from_numpy(sp).long()
    es = et[:, sit]
    d = ((es - es[:, spt]) ** 2).sum(0)
    wt = torch.exp(-d / sigma) if low_tree else torch.exp(-d)
    assert np.abs(wt.detach().numpy()[1:] - w[1:]).max() < 1e-15
    S = [[None] * V for _ in range(V)]
    one = torch.ones((), dtype=torch.float64)
    for i in range(V):
        S[i][i] = one
        for j in range(i):
            S[i][j] = S[int(sp[i])][j] * wt[i]           # S[p][j] read symmetrically: filled for j < p and for j > p
            S[j][i] = S[i][j]
    Sf = torch.stack([torch.stack(r) for r in S])
    o = (Sf[None] * torch.tensor(x[:, si])[:, None, :]).sum(2) / Sf.sum(1)[None]
    assert np.abs(o.detach().numpy() - out[:, si]).max() < 1e-12
    (o * torch.tensor(g[:, si])).sum().backward()
    want = et.grad.numpy()
    err = np.abs(got - want).max()
    print(f'embed_grad vs autograd {H}x{W} low_tree={low_tree}: max error {err:.3g}, max |want| {np.abs(want).max():.3g}')
    assert np.abs(want).max() > 1e-3
    assert err <= 1e-12 * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize('low_tree', [False, True], ids=['high', 'low'])
def test_module_reference_group_layout(low_tree):
    """groups=2 is two groups=1 calls on the channel halves (feature half g with embedding half g)"""
    rng = np.random.default_rng(5)
    B, C, Ce, H, W = 2, 4, 6, 5, 7
    trees = np.stack([_grid_mst(H, W, rng) for _ in range(B)])
    feat = rng.standard_normal((B, C, H, W)); gout = rng.standard_normal((B, C, H, W))
    emb = rng.standard_normal((B, Ce, H, W)) * (0.05 if low_tree else 0.4)
    info = {}
    both = R.module_reference(feat, emb, trees, 2, low_tree, 0.02, gout, info)
    assert info['gw_absmax'].shape == (B, 2) and ((info['gw_absmax'] > 0).all() or low_tree)
    for g in range(2):
        fs, es = slice(2 * g, 2 * g + 2), slice(3 * g, 3 * g + 3)
        one = R.module_reference(feat[:, fs], emb[:, es], trees, 1, low_tree, 0.02, gout[:, fs])
        assert np.array_equal(both[0][:, fs], one[0]) and np.array_equal(both[1][:, fs], one[1])
        if low_tree:
            assert both[2] is None and one[2] is None
        else:
            assert np.array_equal(both[2][:, es], one[2])
    if not low_tree:            # the halves are different problems: the layout check above cannot pass by symmetry
        assert not np.allclose(both[2][:, :3], both[2][:, 3:]) and not np.allclose(both[0][:, :2], both[0][:, 2:])


@pytest.mark.parametrize('regime', R.REGIMES)
def test_oracle_on_weight_regimes(regime):
    """the fp64 oracle itself at w in {0, 1, subnormal}: finite, weight sums >= 1 (a node always counts itself), and on weights of exactly
    0 and 1 the filter is the mean over the connected component -- exactly"""
    rng = np.random.default_rng(17)
    H, W, C = 12, 17, 2
    V = H * W
    si, sp, sc = tfo.bfs_order(_grid_mst(H, W, rng), V)
    x = rng.integers(-8, 9, (C, V)).astype(np.float64); g = rng.integers(-8, 9, (C, V)).astype(np.float64)
    w = R.regime_weights(regime, V, rng).astype(np.float64)
    out, saved = tfo.refine_forward(x, w, si, sp, sc)
    gf = tfo.refine_backward_feature(g, w, si, sp, sc, saved)
    gw = tfo.refine_backward_weight(x, g, w, si, sp, sc, saved)
    assert np.isfinite(out).all() and np.isfinite(gf).all() and np.isfinite(gw).all()
    assert saved['WD'].min() >= 1
    if regime == 'mixed':
        return
    comp = R.components(w, sp)
    n = int(comp.max()) + 1
    assert n == {'ones': 1, 'zeros': V}.get(regime, n) and (regime != 'cut' or 2 <= n < V)
    s = np.zeros((C, n)); cnt = np.bincount(comp, minlength=n)
    for c in range(C):
        np.add.at(s[c], comp, x[c, si])
    assert np.array_equal(out[:, si], (s / cnt)[:, comp])
    assert np.array_equal((s / cnt).astype(np.float32), R.component_mean_f32(x[:, si], comp))     # integers / small counts: fp32(fp64 q) = fp32 q
    if regime == 'zeros':
        assert np.array_equal(out, x) and np.array_equal(gf, g)


@pytest.mark.parametrize('V', [256, 16384])
def test_regime_preconditions(V):
    """what test_refine_weight_regimes relies on, for the very draws it runs (regime_inputs) on the strip (sp[i] = i - 1): sums stay
    integers below 2^24, 'cut' has several components and a non-trivial one (on any tree: the components number 1 + the zeros among
    w[1:], and a single w[i] == 1 joins two nodes), 'mixed' holds every listed value, two of them subnormal"""
    sp = np.maximum(np.arange(V) - 1, 0)
    for regime in R.REGIMES:
        x, g, w = R.regime_inputs(regime, V)
        assert x.dtype == g.dtype == w.dtype == np.float32 and x.shape == g.shape == (2, 2, V) and w.shape == (2, V)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8 and np.abs(x).sum(-1).max() < 2 ** 24
        assert np.array_equal(g, np.round(g)) and np.abs(g).max() <= 8 and np.abs(g).sum(-1).max() < 2 ** 24
        assert not np.array_equal(x[0], x[1])
        if regime in ('cut', 'mixed'):
            assert not np.array_equal(w[0], w[1])
        for b in range(2):
            if regime == 'cut':
                assert set(np.unique(w[b]).tolist()) == {0.0, 1.0}
                sizes = np.bincount(R.components(w[b], sp))
                assert len(sizes) >= 2 and sizes.max() > 1
            if regime == 'mixed':
                want = np.asarray(R.MIXED_VALUES, np.float64).astype(np.float32)
                assert set(np.unique(w[b]).tolist()) == set(want.tolist()) and len(set(want.tolist())) == len(R.MIXED_VALUES)
    tiny = np.finfo(np.float32).tiny
    for v in (1e-45, 1e-40):
        f = np.float32(v)
        assert f != 0 and f < tiny and (f.view(np.uint32) >> 23) & 0xff == 0        # non-zero, exponent field 0: subnormal
    assert np.float32(1e-45).view(np.uint32) == 1                                  # the smallest one
    assert np.float32(1e-30) >= tiny
