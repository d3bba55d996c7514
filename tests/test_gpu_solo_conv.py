"""GPU: the dynamic mask convolution of the SOLOv2-style heads (boxinstseg_amd/solo_conv.py, csrc/solo_dconv.hip) against the reference's
statements as tests/solo_conv_ref.py restates them (tests/golden/make_golden_solo_conv.py ties the restatement to the reference).

Tolerances are the project's rule: for masks, grad_feat and grad_kernel 4 x the restatement's own fp32-against-fp64 difference on the CPU,
relative to the largest fp64 value -- recorded as ``tol_*`` in the fixture, computed live for the seeded cases.  Shapes are chosen where
the kernels can go wrong, not the workload's: E in {1, 5, 16, 258} (the odd tail of E, one and nine blocks of 32 channels), maps of 7 x 9,
13 x 21 and 64 x 65 pixels (one tile, several, a last tile of one pixel), 0 / 1 / 31 / 32 / 33 / 65 rows per image (the chunks of 32
forward and of 64 backward), an image without rows, a level with S = 1, levels nobody uses."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import solo_conv_ref as R

pytestmark = pytest.mark.gpu

# name -> make_case arguments.  Rows per image: s1 1 / 0 / 31, s2 32 / 1, s3 65 / 33, s4 31 / 0 / 4
SEEDED = {
    's1': dict(seed=21, B=3, E=1, H=7, W=9, grids=[1, 6, 3], counts=[[1, 0, 1], [0, 0, 30], [0, 0, 0]]),
    's2': dict(seed=22, B=2, E=5, H=13, W=21, grids=[6, 9], counts=[[20, 1], [12, 0]]),
    's3': dict(seed=23, B=2, E=16, H=64, W=65, grids=[9, 3], counts=[[60, 30], [5, 3]], dups=[(1, 0, 2)]),
    's4': dict(seed=24, B=3, E=258, H=13, W=21, grids=[6, 1, 2], counts=[[30, 0, 3], [1, 0, 1], [0, 0, 0]]),
}
_REF = {}


def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'solo_conv.npz'))


def _reference(name, sigmoid):
    """fp64 and fp32 restatement of a seeded case on the CPU, computed once."""
    key = (name, sigmoid)
    if key not in _REF:
        case = R.make_case(**SEEDED[name])
        _REF[key] = (case, R.run_ref(case, torch.float64, sigmoid), R.run_ref(case, torch.float32, sigmoid))
    return _REF[key]


def _gpu(case, dev, sigmoid=True, grad=True, dtype=torch.float32, need=(True, True)):
    """solo_dynamic_masks on the case: (masks [N,H,W], grad_feat, [grad_map], img_inds lists, feat, maps) as device tensors."""
    import boxinstseg_amd as B
    feat, maps, order, g = R.to_torch(case, dtype, dev)
    feat.requires_grad_(grad and need[0])
    for m in maps:
        m.requires_grad_(grad and need[1])
    masks, inds = B.solo_dynamic_masks(maps, order, feat, sigmoid=sigmoid)
    out = R.cat_levels(masks)
    if grad and out is not None and (need[0] or need[1]):
        (out * g.float()).sum().backward()
    return out, feat.grad, [m.grad for m in maps], masks, inds


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_lists(case, masks, inds, dev):
    """The reference's two lists: None for a level without rows, the image index of every row, views of one buffer."""
    B = case['feat'].shape[0]
    base = None
    for l, (m, i) in enumerate(zip(masks, inds)):
        counts = [len(case['order'][l][b]) for b in range(B)]
        if sum(counts) == 0:
            assert m is None and i is None
            continue
        assert m.shape == (sum(counts), *case['feat'].shape[-2:]) and m.dtype == torch.float32 and m.device == dev
        assert i.dtype == torch.int64 and i.device == dev and i.tolist() == [b for b in range(B) for _ in range(counts[b])]
        base = m.untyped_storage().data_ptr() if base is None else base
        assert m.untyped_storage().data_ptr() == base


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('name', ['a', 'b'])
def test_fixture_cases(dev, name, sigmoid):
    z = _golden()
    tag = 'sig' if sigmoid else 'lin'
    case = R.make_case(**R.CASES[name])
    out, gfeat, gmaps, masks, inds = _gpu(case, dev, sigmoid)
    _check_lists(case, masks, inds, dev)
    R.assert_within(_np(out), z[f'{name}/{tag}/out'], float(z[f'{name}/{tag}/tol_out']), f'{name} {tag} masks')
    R.assert_within(_np(gfeat), z[f'{name}/{tag}/gfeat'], float(z[f'{name}/{tag}/tol_gfeat']), f'{name} {tag} grad_feat')
    got = np.concatenate([_np(m).ravel() for m in gmaps])
    want = np.concatenate([z[f'{name}/{tag}/gmap{l}'].ravel() for l in range(len(gmaps))])
    R.assert_within(got, want, float(z[f'{name}/{tag}/tol_gmap']), f'{name} {tag} grad_kernel')


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('name', sorted(SEEDED))
def test_seeded_cases(dev, name, sigmoid):
    case, q64, q32 = _reference(name, sigmoid)
    out, gfeat, gmaps, masks, inds = _gpu(case, dev, sigmoid)
    _check_lists(case, masks, inds, dev)
    R.assert_within(_np(out), q64[0], R.bound(q32[0], q64[0]), f'{name} masks')
    R.assert_within(_np(gfeat), q64[1], R.bound(q32[1], q64[1]), f'{name} grad_feat')
    flat = lambda maps: np.concatenate([np.asarray(m).ravel() for m in maps])                              # noqa: E731
    R.assert_within(flat([_np(m) for m in gmaps]), flat(q64[2]), R.bound(flat(q32[2]), flat(q64[2])), f'{name} grad_kernel')


EXACT = {
    'x1': dict(seed=31, B=2, E=33, H=64, W=65, grids=[9, 2], counts=[[62, 30], [3, 3]], dups=[(1, 0, 2)], integers=True),
    'x2': dict(seed=32, B=3, E=258, H=13, W=21, grids=[6, 1], counts=[[30, 0, 32], [1, 0, 1]], integers=True),
    'x3': dict(seed=33, B=1, E=1, H=7, W=9, grids=[2], counts=[[4]], dups=[(0, 0, 3)], integers=True),
}


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_cases(dev, name):
    """Integer-valued feature and kernels in [-15, 15], upstream gradient in [-7, 7], no sigmoid: every partial sum is an integer below
    2^24 in any order, so logits, grad_feat and grad_kernel equal the fp64 result with no tolerance."""
    case = R.make_case(**EXACT[name])
    want = R.run_ref(case, torch.float64, sigmoid=False)
    out, gfeat, gmaps, _, _ = _gpu(case, dev, sigmoid=False)
    assert max(float(np.abs(w).max()) for w in (want[0], want[1], *want[2])) < 1 << 24
    assert np.array_equal(_np(out), want[0]) and np.array_equal(_np(gfeat), want[1])
    for got, w in zip(gmaps, want[2]):
        assert np.array_equal(_np(got), w)


@pytest.mark.parametrize('times', [2, 3])
def test_duplicates(dev, times):
    """One cell ``times`` times in one grid_order: equal rows bit for bit; the cell's gradient is the sum of its rows' (an exact case);
    every cell nobody selected gets exactly 0, with the gradient maps handed out pre-filled with a bit pattern."""
    case = R.make_case(41, 2, 16, 13, 21, [4, 2], [[3 + times, 2], [1, 0]], dups=[(0, 0, times)], integers=True)
    cell = int(case['order'][0][0][0])
    assert case['order'][0][0][:times].tolist() == [cell] * times and cell not in case['order'][0][0][times:].tolist()
    with G.poisoned_empty():
        out, gfeat, gmaps, _, _ = _gpu(case, dev, sigmoid=False)
    for k in range(1, times):
        assert torch.equal(out[0].view(torch.int32), out[k].view(torch.int32))
    want = R.run_ref(case, torch.float64, sigmoid=False)
    assert all(np.array_equal(_np(got), w) for got, w in zip(gmaps, want[2])) and np.array_equal(_np(gfeat), want[1])
    # the sum by hand: each of the rows alone gives g_k . feat; the cell holds their sum
    feat, g = case['feat'].astype(np.float64), case['g'].astype(np.float64)
    by_hand = sum(np.einsum('p,ep->e', g[k].ravel(), feat[0].reshape(16, -1)) for k in range(times))
    assert np.array_equal(_np(gmaps[0])[0, :, cell // 4, cell % 4], by_hand)
    for l, S in enumerate(case['grids']):
        for b in range(2):
            used = set(case['order'][l][b].tolist())
            free = [c for c in range(S * S) if c not in used]
            got = gmaps[l][b].reshape(16, -1)[:, free]
            assert free and torch.equal(got.view(torch.int32), torch.zeros_like(got).view(torch.int32)), (l, b)   # +0.0, every bit


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_a_row_does_not_depend_on_the_other_rows(dev):
    """The row of (image 0, level 0, cell c): alone, among others in another order, with its image in another slot of the batch, and as a
    row of the test-time layout -- the same bits."""
    import boxinstseg_amd as B
    case = R.make_case(51, 2, 16, 13, 21, [6, 3], [[5, 34], [3, 2]])
    feat, maps, order, _ = R.to_torch(case, torch.float32, dev)
    full = R.cat_levels(B.solo_dynamic_masks(maps, order, feat)[0])
    cell = order[0][0][2:3]
    want = full[2]
    empty = order[0][0][:0]
    alone = R.cat_levels(B.solo_dynamic_masks(maps, [[cell, empty], [empty, empty]], feat)[0])
    assert alone.shape[0] == 1 and torch.equal(_bits(alone[0]), _bits(want))
    # permuted: image 0's rows of level 0 reversed, image 1's rotated
    perm = [[order[0][0].flip(0), order[0][1].roll(7)], [order[1][0].flip(0), order[1][1]]]
    moved = R.cat_levels(B.solo_dynamic_masks(maps, perm, feat)[0])
    assert torch.equal(_bits(moved[5 - 1 - 2]), _bits(want))
    assert torch.equal(_bits(moved[5:5 + 34]), _bits(full[5:5 + 34].roll(7, 0)))
    # the two images swap their slots in the batch
    swap = R.cat_levels(B.solo_dynamic_masks([m.flip(0).contiguous() for m in maps], [[order[0][1], order[0][0]], [order[1][1], order[1][0]]],
                                             feat.flip(0).contiguous())[0])
    assert torch.equal(_bits(swap[34 + 2]), _bits(want)) and torch.equal(_bits(swap[:34]), _bits(full[5:39]))
    # the test-time layout on the same kernel rows and feature
    for b in range(2):
        rows = torch.cat([maps[l][b].reshape(16, -1).t() for l in range(2)]).contiguous()                 # [36 + 9, E]
        pick = torch.cat([order[0][b], order[1][b] + 36])
        got = B.solo_candidate_masks(feat[b:b + 1], rows, pick)
        mine = torch.cat([full[:5] if b == 0 else full[5:39], full[39:42] if b == 0 else full[42:44]])
        assert torch.equal(_bits(got), _bits(mine))
        gathered = B.solo_candidate_masks(feat[b:b + 1], rows[pick].contiguous())
        assert torch.equal(_bits(gathered), _bits(mine))


def test_two_runs_are_bit_identical(dev):
    case = R.make_case(**SEEDED['s3'])
    a = _gpu(case, dev)
    with G.poisoned_empty():
        b = _gpu(case, dev)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[2], b[2]))


def test_nan_containment(dev):
    """A NaN in a kernel row makes that row NaN and no other; a NaN in the feature makes that pixel NaN for the rows of its image only."""
    import boxinstseg_amd as B
    case = R.make_case(61, 2, 5, 13, 21, [6, 3], [[3, 34], [2, 1]])
    feat, maps, order, _ = R.to_torch(case, torch.float32, dev)
    clean = R.cat_levels(B.solo_dynamic_masks(maps, order, feat)[0])
    cell = int(order[0][1][33])                                               # row 3 + 33 = 36: the second chunk of image 1
    bad = [m.clone() for m in maps]
    bad[0][1, 2, cell // 6, cell % 6] = float('nan')
    for sigmoid in (True, False):
        out = R.cat_levels(B.solo_dynamic_masks(bad, order, feat, sigmoid=sigmoid)[0])
        nan = torch.isnan(out)
        assert bool(nan[36].all()) and int(nan.sum()) == 13 * 21
        if sigmoid:
            keep = torch.ones(out.shape[0], dtype=torch.bool, device=dev)
            keep[36] = False
            assert torch.equal(_bits(out[keep]), _bits(clean[keep]))
    f2 = feat.clone()
    f2[1, 4, 12, 20] = float('nan')                                           # the last pixel: the short last tile
    f2[1, 0, 0, 0] = float('nan')
    out = R.cat_levels(B.solo_dynamic_masks(maps, order, f2)[0])
    nan = torch.isnan(out)
    of_image_1 = torch.tensor([False] * 3 + [True] * 34 + [False] * 2 + [True], device=dev)
    assert bool(nan[of_image_1][:, 12, 20].all()) and bool(nan[of_image_1][:, 0, 0].all()) and int(nan.sum()) == 2 * 35
    assert torch.equal(_bits(out[~of_image_1]), _bits(clean[~of_image_1]))


def test_frozen_inputs_and_the_teacher(dev):
    import boxinstseg_amd as B
    case = R.make_case(**SEEDED['s2'])
    teacher = dict(R.make_case(**dict(SEEDED['s2'], seed=122)), order=case['order'], g=case['g'])      # its own maps, the student's grid_order
    both = _gpu(case, dev)
    only_feat = _gpu(case, dev, need=(True, False))
    only_maps = _gpu(case, dev, need=(False, True))
    assert all(g is None for g in only_feat[2]) and torch.equal(_bits(only_feat[1]), _bits(both[1]))
    assert only_maps[1] is None and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(only_maps[2], both[2]))
    none = _gpu(case, dev, need=(False, False))
    assert not none[0].requires_grad and torch.equal(_bits(none[0]), _bits(both[0]))
    # the pair: the student's call and the teacher's, bit for bit; the teacher carries no graph
    feat, maps, order, g = R.to_torch(case, torch.float32, dev, requires_grad=True)
    t_feat, t_maps, _, _ = R.to_torch(teacher, torch.float32, dev, requires_grad=True)
    s_masks, t_masks, inds = B.solo_dynamic_masks_pair(maps, t_maps, order, feat, t_feat)
    t_alone = _gpu(teacher, dev, grad=False)
    assert torch.equal(_bits(R.cat_levels(s_masks)), _bits(both[0])) and torch.equal(_bits(R.cat_levels(t_masks)), _bits(t_alone[0]))
    assert all(not t.requires_grad for t in t_masks if t is not None) and R.cat_levels(s_masks).requires_grad
    assert [i.tolist() for i in inds] == [i.tolist() for i in both[4]]
    (R.cat_levels(s_masks) * g).sum().backward()
    assert torch.equal(_bits(feat.grad), _bits(both[1])) and all(torch.equal(_bits(m.grad), _bits(w)) for m, w in zip(maps, both[2]))
    assert t_feat.grad is None and all(m.grad is None for m in t_maps)


def test_no_rows_at_all(dev):
    """N = 0: no mask, and all-zero gradients for whoever asks through another path of the graph."""
    import boxinstseg_amd as B
    case = R.make_case(71, 2, 5, 7, 9, [3, 2], [[0, 0], [0, 0]])
    feat, maps, order, _ = R.to_torch(case, torch.float32, dev, requires_grad=True)
    masks, inds = B.solo_dynamic_masks(maps, order, feat)
    assert masks == [None, None] and inds == [None, None]
    from boxinstseg_amd import solo_conv as SC
    plan = SC._plan(maps, order, feat, True, None)
    with G.poisoned_empty():
        out, _ = SC._DynamicMasks.apply(plan, feat, *maps)
        assert out.shape == (0, 7, 9)
        out.sum().backward()
    assert not bool(feat.grad.any()) and not any(bool(m.grad.any()) for m in maps)
    assert not bool(torch.isnan(feat.grad).any()) and not any(bool(torch.isnan(m.grad).any()) for m in maps)


def test_a_cell_outside_its_map_is_not_read(dev):
    import boxinstseg_amd as B
    case = R.make_case(72, 1, 5, 7, 9, [2], [[3]])
    feat, maps, order, g = R.to_torch(case, torch.float32, dev, requires_grad=True)
    clean = R.cat_levels(B.solo_dynamic_masks(maps, order, feat, sigmoid=False)[0]).detach()
    for bad in (4, -1, 1 << 40):
        o = [[order[0][0].clone()]]
        o[0][0][1] = bad
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        feat.grad = None
        maps[0].grad = None
        out = R.cat_levels(B.solo_dynamic_masks(maps, o, feat, sigmoid=False, status=status)[0])
        (out * g).sum().backward()
        assert int(status) == 1 and not bool(out[1].any())
        assert torch.equal(_bits(out[0]), _bits(clean[0])) and torch.equal(_bits(out[2]), _bits(clean[2]))
        assert bool(torch.isfinite(feat.grad).all()) and bool(torch.isfinite(maps[0].grad).all())
        used = [int(o[0][0][0]), int(o[0][0][2])]
        free = [c for c in range(4) if c not in used]
        assert not bool(maps[0].grad.reshape(5, 4)[:, free].any()) and bool(maps[0].grad.reshape(5, 4)[:, used].any())


@pytest.mark.parametrize('I', [0, 1, 33, 500])
def test_candidate_masks(dev, I):
    """The test-time product at E = 16, 24 x 40: rows out of order and repeated, against the fp64 statement of get_seg_single."""
    import boxinstseg_amd as B
    rng = np.random.default_rng(81)
    seg = (0.5 * rng.standard_normal((1, 16, 24, 40))).astype(np.float32)
    kern = (rng.standard_normal((61, 16)) / 4).astype(np.float32)
    rows = rng.integers(0, 61, size=I)
    if I > 1:
        rows[1] = rows[0]
    got = B.solo_candidate_masks(torch.from_numpy(seg).to(dev), torch.from_numpy(kern).to(dev), torch.from_numpy(rows).to(dev))
    assert got.shape == (I, 24, 40) and got.dtype == torch.float32
    if I == 0:
        return
    q = {dt: R.candidate_masks(torch.from_numpy(seg).to(dt), torch.from_numpy(kern).to(dt)[torch.from_numpy(rows)]).double().numpy()
         for dt in (torch.float64, torch.float32)}
    R.assert_within(_np(got), q[torch.float64], R.bound(q[torch.float32], q[torch.float64]), f'{I} candidates')
    if I > 1:
        assert torch.equal(_bits(got[0]), _bits(got[1]))
    every = B.solo_candidate_masks(torch.from_numpy(seg).to(dev), torch.from_numpy(kern).to(dev))
    assert every.shape == (61, 24, 40) and torch.equal(_bits(every[rows[0]]), _bits(got[0]))


def test_candidate_masks_fixture(dev):
    import boxinstseg_amd as B
    z = _golden()
    got = B.solo_candidate_masks(torch.from_numpy(z['test/seg']).to(dev), torch.from_numpy(z['test/kernels']).to(dev),
                                 torch.from_numpy(z['test/rows']).to(dev))
    R.assert_within(_np(got), z['test/out'], float(z['test/tol_out']), 'fixture candidates')


def test_get_seg_single_with_the_hip_product(dev):
    """discobox_get_seg_single(conv='hip') against conv='torch' on inputs whose probabilities keep a margin from mask_thr: feature values
    in {-1, 1}, kernel values odd in [-3, 3] and channel 15 switched off, so every logit is an odd integer (exact in fp32 and fp64) and
    every probability is at least sigmoid(1) - 0.5 = 0.23 away from mask_thr = 0.5.  Checked on the CPU first: the torch statement in
    fp32 and in fp64 agrees on every mask byte."""
    import boxinstseg_amd as B
    rng = np.random.default_rng(91)
    grids, strides, ncls, E, hw = [4, 3], [8, 16], 3, 16, (24, 40)
    feat = rng.choice([-1.0, 1.0], size=(1, E, *hw)).astype(np.float32)
    kern = rng.choice([-3.0, -1.0, 1.0, 3.0], size=(25, E)).astype(np.float32)
    kern[:, 15] = 0
    cate = (rng.uniform(0, 1, (25, ncls)) * (rng.random((25, ncls)) < 0.5)).astype(np.float32)
    cfg = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    meta = dict(img_shape=(90, 150, 3), ori_shape=(61, 93, 3))
    p = {dt: R.candidate_masks(torch.from_numpy(feat).to(dt), torch.from_numpy(kern).to(dt)) for dt in (torch.float32, torch.float64)}
    assert float((p[torch.float64] - 0.5).abs().min()) > 0.23
    assert torch.equal(p[torch.float32] > cfg['mask_thr'], p[torch.float64] > cfg['mask_thr'])
    args = (torch.from_numpy(cate).to(dev), torch.from_numpy(feat).to(dev), torch.from_numpy(kern).to(dev), hw, meta, cfg, grids, strides)
    want = B.discobox_get_seg_single(*args)
    assert want is not None and want.masks.shape[0] > 3 and B.discobox_get_seg_single(*args, conv='torch').masks.shape == want.masks.shape
    got = B.discobox_get_seg_single(*args, conv='hip')
    assert torch.equal(got.labels, want.labels) and torch.equal(got.masks, want.masks) and torch.equal(got.mask_stats, want.mask_stats)
    assert got.scores.dtype == want.scores.dtype and torch.allclose(got.scores, want.scores, rtol=1e-5, atol=0)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_half_precision_at_the_surface(dev, dtype):
    """Half-precision tensors are upcast: fp32 masks, equal to the fp32 call on the upcast values bit for bit, gradients in the inputs'
    dtype."""
    import boxinstseg_amd as B
    case = R.make_case(**SEEDED['s2'])
    feat, maps, order, g = R.to_torch(case, dtype, dev, requires_grad=True)
    masks, inds = B.solo_dynamic_masks(maps, order, feat)
    out = R.cat_levels(masks)
    assert out.dtype == torch.float32
    up = R.cat_levels(B.solo_dynamic_masks([m.detach().float() for m in maps], order, feat.detach().float())[0])
    assert torch.equal(_bits(out), _bits(up))
    (out * g.float()).sum().backward()
    assert feat.grad.dtype == dtype and all(m.grad.dtype == dtype for m in maps) and bool(torch.isfinite(feat.grad.float()).all())
    cand = B.solo_candidate_masks(feat[:1].detach(), maps[0][0].detach().reshape(5, -1).t().contiguous(), order[0][0])
    assert cand.dtype == torch.float32 and torch.equal(_bits(cand), _bits(out[:20]))
