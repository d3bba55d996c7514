"""GPU: BoxLevelSet's mask predictions (csrc/solo_dconv_level.hip, include/boxinst/boxinst_hip_dconvl.h) against the reference's own
statements as tests/golden/box_solo_masks.npz records them (box_solov2_head.py:205-216 and :317-320, fp64).

* every seeded case within ``tol_*`` (4 x the reference's own fp32 error) for the rows, grad_feat and every grad_kernel map, every element;
* the exact cases (integers, ratios 1, 2 and 4: weights 1 and 1/2) equal to fp64 with no tolerance;
* grad_kernel exactly zero outside the named cells; two runs the same bits; a row's bits unchanged when the other rows are removed;
* a NaN kernel value stays in its row, a NaN feature value in the output pixels whose taps name it; the feature of an image without
  rows is not read;
* a cell outside its map: the status word and an all-zero row; N == 0; a size outside the support set;
* ``box_solov2_set_cells`` against ``nonzero``; ``box_solov2_get_seg_single_kernels`` against ``box_solov2_get_seg_single`` on the masks
  of all cells, bit for bit; capture and replay of forward and backward in a hipGraph."""
import os

import numpy as np
import pytest
import torch

from tests import box_solo_masks_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'box_solo_masks.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def exact_refs():
    """The exact cases' fp64 results, computed once."""
    out = {}
    for name, spec in R.EXACT_CASES.items():
        case = R.make_case(**spec)
        out[name] = (case, R.run_ref(case, torch.float64))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gpu(case, dev, cells=None, need=(True, True), feat=None, maps=None, status=None, backward=True):
    """One forward (and backward with the case's upstream gradient): (rows per level, grad_feat, grad maps) on the device."""
    import boxinstseg_amd as B
    f, m, _, g = R.to_torch(case, torch.float32, dev)
    f = (f if feat is None else feat).requires_grad_(need[0])
    m = [x.requires_grad_(need[1]) for x in (m if maps is None else maps)]
    cells = R.cells_of(case, dev) if cells is None else cells
    rows = B.box_solov2_ins_preds(m, f, cells, case['sizes'], status=status)
    if not backward or not any(need):
        return [r.detach() for r in rows], None, None
    loss = sum((r * x).sum() for r, x in zip(rows, g))
    grads = torch.autograd.grad(loss, ([f] if need[0] else []) + (m if need[1] else []))
    return [r.detach() for r in rows], grads[0] if need[0] else None, list(grads[1:] if need[0] else grads) if need[1] else None


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('name', list(R.CASES))
def test_seeded_cases_within_the_references_own_error(dev, golden, name):
    case = R.make_case(**R.CASES[name])
    rows, gfeat, gmaps = _gpu(case, dev)
    for l in range(5):
        assert rows[l].dtype == torch.float32 and tuple(rows[l].shape) == golden[f'{name}/rows{l}'].shape, l
    want_rows = R.flat([golden[f'{name}/rows{l}'] for l in range(5)])
    want_gmap = R.flat([golden[f'{name}/gmap{l}'] for l in range(5)])
    R.assert_within(R.flat([_np(r) for r in rows]), want_rows, float(golden[f'{name}/tol_rows']), f'{name} rows')
    R.assert_within(_np(gfeat), golden[f'{name}/gfeat'], float(golden[f'{name}/tol_gfeat']), f'{name} grad_feat')
    R.assert_within(R.flat([_np(m) for m in gmaps]), want_gmap, float(golden[f'{name}/tol_gmap']), f'{name} grad_kernel')
    for l in range(5):                                                        # exactly zero for every cell no row names
        assert tuple(gmaps[l].shape) == case['maps'][l].shape
        unset = torch.from_numpy(~case['labels'][l]).to(dev)                   # [B, S^2]
        assert not bool(gmaps[l].flatten(2).permute(0, 2, 1)[unset].any()), l


@pytest.mark.parametrize('name', list(R.EXACT_CASES))
def test_exact_cases_equal_fp64(dev, exact_refs, name):
    case, (want_rows, want_gfeat, want_gmaps) = exact_refs[name]
    rows, gfeat, gmaps = _gpu(case, dev)
    for l in range(5):
        assert np.array_equal(_np(rows[l]), want_rows[l]), f'rows of level {l}'
        assert np.array_equal(_np(gmaps[l]), want_gmaps[l]), f'grad_kernel of level {l}'
    assert np.array_equal(_np(gfeat), want_gfeat)
    assert sum(r.shape[0] for r in rows) == sum(sum(c) for c in case['counts']) and float(np.abs(want_gfeat).max()) > 0
    # either gradient alone: the same bits
    only_f = _gpu(case, dev, need=(True, False))
    only_m = _gpu(case, dev, need=(False, True))
    assert only_f[2] is None and torch.equal(_bits(only_f[1]), _bits(gfeat))
    assert only_m[1] is None and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(only_m[2], gmaps))


def test_two_runs_give_the_same_bits(dev):
    case = R.make_case(**R.CASES['wide'])
    a, b = _gpu(case, dev), _gpu(case, dev)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize('name', ['ratios124', 'wide'])
def test_a_rows_bits_do_not_depend_on_the_other_rows(dev, name):
    """The last row of every (level, image) alone, and the rows of a segment in another order: the same bits."""
    case = R.make_case(**R.CASES[name])
    full, _, _ = _gpu(case, dev, backward=False)
    cells = R.cells_of(case, dev)
    B = case['feat'].shape[0]
    for l in range(5):
        at = 0
        for b in range(B):
            n = case['counts'][l][b]
            if n:
                alone = [[cells[l][b][-1:] if (k, i) == (l, b) else cells[k][i][:0] for i in range(B)] for k in range(5)]
                got, _, _ = _gpu(case, dev, cells=alone, backward=False)
                assert sum(r.shape[0] for r in got) == 1 and torch.equal(_bits(got[l][0]), _bits(full[l][at + n - 1])), (l, b)
            at += n
    flipped = [[c.flip(0) for c in row] for row in cells]
    got, _, _ = _gpu(case, dev, cells=flipped, backward=False)
    for l in range(5):
        at = 0
        for b in range(B):
            n = case['counts'][l][b]
            assert torch.equal(_bits(got[l][at:at + n]), _bits(full[l][at:at + n].flip(0))), (l, b)
            at += n


def test_launches_per_size_group(dev):
    """ratios124 has three size groups with rows: the first of the feature's own size (no resize), then ratio 2 and ratio 4.  Forward: per
    group the gather and ONE product, which reads the (resized) feature once; backward: per group the product's four launches, the resize
    before them where the group is resampled, and one adjoint pass at the end.  With rows in one group only, only that group launches."""
    import ctypes as C

    from boxinstseg_amd import _lib
    case = R.make_case(**R.CASES['ratios124'])
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()) if phase == 0 else None)
    lib = _lib.load()

    def launches(fn):
        del names[:]
        lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
        try:
            fn()
        finally:
            lib.bxi_dev_set_launch_hook(None, None)
        torch.cuda.synchronize()
        return list(names)

    product = ['solo_dconv_gather', 'solo_dconv_fwd']
    back = ['solo_dconv_gather', 'solo_dconv_bwd', 'solo_dconv_reduce', 'solo_dconv_scatter']
    assert launches(lambda: _gpu(case, dev, backward=False)) == product + ['solo_dconvl_resize'] + product + ['solo_dconvl_resize'] + product
    both = launches(lambda: _gpu(case, dev))
    assert both[8:] == back + ['solo_dconvl_resize'] + back + ['solo_dconvl_resize'] + back + ['solo_dconvl_adjoint']
    only = dict(R.CASES['ratios124'], counts=[[0, 0], [0, 0], [0, 2], [0, 0], [0, 0]])
    assert launches(lambda: _gpu(R.make_case(**only), dev, backward=False)) == ['solo_dconvl_resize'] + product


def test_nan_containment(dev):
    case = R.make_case(**R.CASES['ratios124'])
    clean, _, _ = _gpu(case, dev, backward=False)
    feat, maps, _, _ = R.to_torch(case, torch.float32, dev)
    # a kernel value: level 2, image 0, its second set cell -> row 1 of level 2 and nothing else
    cell = int(np.flatnonzero(case['labels'][2][0])[1])
    maps[2].view(2, 12, 9)[0, 5, cell] = float('nan')
    got, _, _ = _gpu(case, dev, maps=maps, backward=False)
    for l in range(5):
        nan = torch.isnan(got[l])
        if l == 2:
            assert bool(nan[1].all()) and not bool(nan[0].any())
        else:
            assert not bool(nan.any())
        assert torch.equal(_bits(got[l][~nan]), _bits(clean[l][~nan]))
    # a feature value of image 1: in every row of image 1 the output pixels whose taps name it, in no row of image 0
    y, x = 9, 14
    feat[1, 7, y, x] = float('nan')
    got, _, _ = _gpu(case, dev, feat=feat, backward=False)
    for l, (oh, ow) in enumerate(case['sizes']):
        y0, y1, _, _ = R.taps(16, oh, torch.float32)
        x0, x1, _, _ = R.taps(24, ow, torch.float32)
        hit = (((y0 == y) | (y1 == y))[:, None] & ((x0 == x) | (x1 == x))[None, :]).to(dev)
        if (oh, ow) == (16, 24):
            hit = torch.zeros(16, 24, dtype=torch.bool, device=dev)
            hit[y, x] = True                                                  # a level of the feature's own size is not resampled
        assert bool(hit.any())
        n0 = case['counts'][l][0]
        nan = torch.isnan(got[l])
        assert not bool(nan[:n0].any()) and bool((nan[n0:] == hit).all()), l
        assert torch.equal(_bits(got[l][~nan]), _bits(clean[l][~nan]))


def test_an_image_without_rows_is_not_read(dev):
    """Image 1 has no set cell: its feature and its kernels may hold anything."""
    case = R.make_case(**dict(R.CASES['ratios124'], counts=[[3, 0], [0, 0], [2, 0], [0, 0], [1, 0]]))
    clean = _gpu(case, dev)
    feat, maps, _, _ = R.to_torch(case, torch.float32, dev)
    feat[1] = float('nan')
    for m in maps:
        m[1] = float('nan')
    got = _gpu(case, dev, feat=feat, maps=maps)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[0], clean[0]))
    assert torch.equal(_bits(got[1]), _bits(clean[1])) and not bool(got[1][1].any()) and bool(got[1][0].any())
    assert all(torch.equal(_bits(a), _bits(b)) and not bool(a[1].any()) for a, b in zip(got[2], clean[2]))


def test_a_cell_outside_its_map(dev):
    case = R.make_case(**R.CASES['ratios124'])
    clean = _gpu(case, dev)
    for bad in (9, -1, 1 << 40):                                              # level 2 has 3 x 3 cells
        cells = R.cells_of(case, dev)
        cells[2][0] = torch.tensor([int(cells[2][0][0]), bad], device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        got = _gpu(case, dev, cells=cells, status=status)
        assert int(status) == 1 == __import__('boxinstseg_amd')._lib.DCONV_STATUS_BAD_CELL
        assert not bool(got[0][2][1].any()) and torch.equal(_bits(got[0][2][0]), _bits(clean[0][2][0]))
        assert all(torch.equal(_bits(got[0][l]), _bits(clean[0][l])) for l in (0, 1, 3, 4))
        assert bool(torch.isfinite(got[1]).all()) and all(bool(torch.isfinite(m).all()) for m in got[2])
        # the row contributes no gradient: what is left is the clean call without that row
        cells[2][0] = cells[2][0][:1]
        g2 = torch.from_numpy(case['g'][2][:1]).to(dev)
        less = dict(case, g=case['g'][:2] + [g2.cpu().numpy()] + case['g'][3:])
        want = _gpu(less, dev, cells=cells)
        assert torch.equal(_bits(got[1]), _bits(want[1])) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[2], want[2]))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _gpu(case, dev, status=status)
    assert int(status) == 0


def test_no_rows_at_all(dev):
    """N == 0: [0, oh, ow] per level, all-zero gradients for whoever asks, the status word untouched."""
    import boxinstseg_amd as B
    from tests import guarded as G
    case = R.make_case(**dict(R.CASES['ratios124'], counts=[[0, 0]] * 5))
    feat, maps, _, _ = R.to_torch(case, torch.float32, dev, requires_grad=True)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    with G.poisoned_empty():
        rows = B.box_solov2_ins_preds(maps, feat, R.cells_of(case, dev), case['sizes'], status=status)
        assert [tuple(r.shape) for r in rows] == [(0,) + s for s in case['sizes']] and all(r.dtype == torch.float32 for r in rows)
        grads = torch.autograd.grad(sum(r.sum() for r in rows), [feat, *maps])
    assert all(g.shape == t.shape and not bool(g.any()) and bool(torch.isfinite(g).all()) for g, t in zip(grads, [feat, *maps]))
    assert int(status) == 77


def test_a_size_outside_the_support_set_raises(dev):
    import boxinstseg_amd as B
    case = R.make_case(**R.CASES['ratios124'])
    feat, maps, _, _ = R.to_torch(case, torch.float32, dev)
    for bad in ((1, 6), (4, 2), (33, 24), (16, 49)):
        with pytest.raises(NotImplementedError, match='boxinst_hip_dconvl.h'):
            B.box_solov2_ins_preds(maps, feat, R.cells_of(case, dev), case['sizes'][:4] + [bad])
    with pytest.raises(RuntimeError, match='fp32 only'):
        B.box_solov2_ins_preds(maps, feat.half(), R.cells_of(case, dev), case['sizes'])
    # the limits themselves run: 16 / 2 = 24 / 3 = 8 down, 2 x up
    for edge in ((2, 3), (32, 48)):
        sizes = case['sizes'][:4] + [edge]
        rows = B.box_solov2_ins_preds(maps, feat, R.cells_of(case, dev), sizes)
        _, mp, labels, _ = R.to_torch(case, torch.float64)
        want = R.rows_ref(mp, torch.from_numpy(case['feat']).double(), labels, sizes)[4]
        assert tuple(rows[4].shape) == (3,) + edge and float((rows[4].cpu().double() - want).abs().max()) < 1e-5


def test_set_cells_is_nonzero_of_the_targets(dev):
    import boxinstseg_amd as B
    from tests import solo_ref as SR
    per_image = [SR.random_case(70 + i, 12, 128, 160, 7) for i in range(2)]
    boxes = [p[0][0].to(dev) for p in per_image]
    labels = [p[1][0].to(dev) for p in per_image]
    masks = [torch.from_numpy(p[2][0]).to(dev) for p in per_image]
    grids = [12, 10, 8, 6, 4]
    tg = B.box_solov2_targets(boxes, labels, masks, [(32, 40), (32, 40), (16, 20), (8, 10), (8, 10)], strides=[8, 8, 16, 32, 32], num_grids=grids,
                              scale_ranges=[(1, 14), (7, 24), (12, 32), (20, 48), (32, 256)], sigma=0.2, num_classes=7)
    cells = B.box_solov2_set_cells(tg)
    total = 0
    for l, S in enumerate(grids):
        lab = tg.ins_ind_labels[l].view(2, S * S)
        for b in range(2):
            want = lab[b].nonzero()[:, 0]
            assert cells[l][b].dtype == torch.int64 and cells[l][b].is_contiguous() and torch.equal(cells[l][b], want), (l, b)
            total += int(want.numel())
    assert total > 10
    # and they drive the masks: one row per set cell, in the order of ins_labels()
    feat = torch.randn(2, 8, 32, 40, device=dev)
    maps = [torch.randn(2, 8, S, S, device=dev) for S in grids]
    rows = B.box_solov2_ins_preds(maps, feat, cells, [(32, 40), (32, 40), (16, 20), (8, 10), (8, 10)])
    assert [r.shape[0] for r in rows] == [t.shape[0] for t in tg.ins_labels()]


def test_get_seg_single_from_the_kernels_is_the_same_bits(dev):
    """5 levels of at most 4 x 4 cells: the candidates' masks from the kernels against the existing function fed with every cell's mask."""
    import boxinstseg_amd as B
    rng = torch.Generator().manual_seed(41)
    grids, strides, E, hw = [4, 3, 3, 2, 2], [8, 8, 16, 32, 32], 8, (11, 17)
    cells = sum(g * g for g in grids)
    cate = (torch.rand(cells, 3, generator=rng) * 0.6).to(dev)
    feat = torch.randn(1, E, *hw, generator=rng).to(dev)
    kern = (1.5 * torch.randn(cells, E, generator=rng)).to(dev)
    cfg = dict(score_thr=0.3, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=20, kernel='gaussian', sigma=2.0)
    meta = dict(img_shape=(41, 66, 3), ori_shape=(60, 101, 3))
    every = B.solo_candidate_masks(feat, kern, None)
    want = B.box_solov2_get_seg_single(cate, every, hw, meta, cfg, grids, strides)
    got = B.box_solov2_get_seg_single_kernels(cate, feat, kern, hw, meta, cfg, grids, strides)
    assert want.masks.shape[0] > 3 and want.masks.dtype == torch.bool
    assert torch.equal(_bits(got.scores), _bits(want.scores)) and torch.equal(got.labels, want.labels) and torch.equal(got.masks, want.masks)
    assert torch.equal(got.mask_stats, want.mask_stats) and got.img_shape == want.img_shape and got.ori_shape == want.ori_shape
    none = B.box_solov2_get_seg_single_kernels(cate * 0, feat, kern, hw, meta, cfg, grids, strides)
    assert none.scores.numel() == 0 and tuple(none.masks.shape) == (0, 60, 101)


def test_captured_graph_follows_its_inputs(dev):
    """Forward and backward captured in a hipGraph on one stream; replayed after the inputs changed in place it gives the eager call's bits."""
    import boxinstseg_amd as B
    case = R.make_case(**R.CASES['ratios124'])
    feat, maps, _, g = R.to_torch(case, torch.float32, dev, requires_grad=True)
    cells = R.cells_of(case, dev)

    def step():
        rows = B.box_solov2_ins_preds(maps, feat, cells, case['sizes'])
        return torch.cat([r.detach().flatten() for r in rows]), torch.autograd.grad(sum((r * x).sum() for r, x in zip(rows, g)), [feat, *maps])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    with torch.no_grad():
        feat.mul_(0.75).add_(0.125)
        for m in maps:
            m.mul_(-1.5)
    graph.replay()
    torch.cuda.synchronize()
    want_out, want_grads = step()
    assert torch.equal(_bits(out), _bits(want_out)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, want_grads))
    assert not torch.equal(_bits(out), _bits(first[0]))
