"""GPU: the dynamic mask convolution on fp16 / bf16 tensors read in place (``compute='half'``, csrc/solo_dconv16.hip,
include/boxinst/boxinst_hip_dconv16.h) against the reference's statements as tests/solo_conv_ref.py restates them.

* exact cases: integer-valued operands that both half types hold exactly, every partial sum an integer below 2^24 (forward, fp32 output)
  or at most 256 (backward, half output): equal to fp64 with no tolerance, padding, tails, chunk crossings and repeated cells included;
* seeded cases: the arrays are rounded to the half type first; the yardstick is the project's rule, 4 x the REFERENCE's own error --
  here the restatement run in the half type on the CPU (``q16``) against fp64 on the same rounded values (``q64``); with
  ``out_dtype=torch.float32`` the masks are held against the restatement's fp32 run instead.  The measured fraction of every bound is
  printed.  The largest fractions measured on an MI355X are recorded in profiles/NOTES.md R26-1;
* independence, NaN containment, a cell outside its map, N == 0: bit for bit;
* fp16 subnormal kernel values are multiplied at their value (the header's statement);
* ``discobox_get_seg_single(conv='hip_half')`` against ``conv='torch'``; capture and replay in a hipGraph."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import solo_conv_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ['fp16', 'bf16']


def _rounded(case, dtype):
    """The case with feature, kernel maps and upstream gradient rounded to ``dtype`` (kept as float32 numpy arrays)."""
    r = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()                      # noqa: E731
    return dict(case, feat=r(case['feat']), maps=[r(m) for m in case['maps']], g=r(case['g']))


def _np(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _gpu(case, dev, dtype, sigmoid=True, out_dtype=None, grad=True):
    """solo_dynamic_masks(compute='half') on the case: (masks [N,H,W], grad_feat, [grad_map], mask list, img_inds list)."""
    import boxinstseg_amd as B
    feat, maps, order, g = R.to_torch(case, dtype, dev, requires_grad=grad)
    masks, inds = B.solo_dynamic_masks(maps, order, feat, sigmoid=sigmoid, compute='half', out_dtype=out_dtype)
    out = R.cat_levels(masks)
    if grad and out is not None:
        (out * g.to(out.dtype)).sum().backward()
    return out, feat.grad, [m.grad for m in maps], masks, inds


# rows per image 1 / 0 / 33 (a second chunk of 32); a level with S = 1; a cell named three times in a row
EXACT_LAYOUT = dict(B=3, grids=[3, 1, 6], counts=[[0, 0, 3], [1, 0, 0], [0, 0, 30]], dups=[(0, 2, 3)])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw', [(7, 9), (13, 21), (8, 24)], ids=['7x9', '13x21', '8x24'])
@pytest.mark.parametrize('E', [5, 16, 24, 40])
def test_exact_forward(dev, E, hw, dtype):
    """Feature and kernels integer-valued in [-15, 15] (exact in fp16 and bf16), no sigmoid, fp32 output: every partial sum is an integer
    below 2^24 in any order, so every logit equals the fp64 result.  E = 5 / 24 / 40 are padded to 16 / 32 / 48 (one, two, three k steps),
    7 x 9 is under one tile of 64 pixels, 13 x 21 is four tiles and a tail of 17 with an odd row length (the element loads), 8 x 24 is three
    tiles read in 16-byte pieces; the kernel has ONE tile width for every E."""
    case = R.make_case(seed=300 + E, E=E, H=hw[0], W=hw[1], integers=True, **EXACT_LAYOUT)
    assert case['order'][0][2][:3].tolist() == [int(case['order'][0][2][0])] * 3
    want = R.run_ref(case, torch.float64, sigmoid=False)[0]
    with G.poisoned_empty():
        out, _, _, masks, inds = _gpu(case, dev, dtype, sigmoid=False, out_dtype=torch.float32, grad=False)
    assert out.dtype == torch.float32 and float(np.abs(want).max()) < 1 << 24
    assert np.array_equal(_np(out), want)
    assert masks[1].shape[0] == 1 and inds[0].tolist() == [2, 2, 2] and inds[1].tolist() == [0] and inds[2].tolist() == [2] * 30
    assert torch.equal(_bits(out[0]), _bits(out[1])) and torch.equal(_bits(out[0]), _bits(out[2]))       # the cell named three times
    # the same logits in the half type: fp64 rounded once
    half, _, _, _, _ = _gpu(case, dev, dtype, sigmoid=False, grad=False)
    assert half.dtype == dtype and torch.equal(_bits(half), _bits(torch.from_numpy(want).to(dtype).to(dev)))


@pytest.mark.parametrize('hw', [(13, 17), (8, 24)], ids=['13x17', '8x24'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_exact_backward(dev, dtype, hw):
    """Feature, kernels and grad_out in {-1, 0, 1}, 13 x 17 pixels (and 8 x 24: the feature read in 16-byte pieces), at most 40 rows per
    image, E = 24, no sigmoid: every sum is an integer of magnitude <= 221 (<= 256 at the repeated cell, asserted), exact in both types, so
    grad_feat and EVERY element of every kernel map equal fp64 -- the zeros of unselected cells and of the image without rows and the sum
    at the repeated cell included."""
    case = R.make_case(seed=401, B=3, E=24, H=hw[0], W=hw[1], grids=[6, 2], counts=[[36, 0, 2], [4, 0, 1]], dups=[(0, 2, 2)], integers=True)
    case = dict(case, feat=np.sign(case['feat']), maps=[np.sign(m) for m in case['maps']], g=np.sign(case['g']))
    want = R.run_ref(case, torch.float64, sigmoid=False)
    assert max(float(np.abs(w).max()) for w in (want[0], want[1], *want[2])) <= 256
    with G.poisoned_empty():
        out, gfeat, gmaps, _, _ = _gpu(case, dev, dtype, sigmoid=False)
    assert out.dtype == dtype and gfeat.dtype == dtype and all(m.dtype == dtype for m in gmaps)
    assert np.array_equal(_np(out), want[0]) and np.array_equal(_np(gfeat), want[1])
    for got, w in zip(gmaps, want[2]):
        assert np.array_equal(_np(got), w)
    assert not bool(gfeat[1].any()) and not any(bool(m[1].any()) for m in gmaps) and bool(gfeat[0].any())
    cell = int(case['order'][0][2][0])
    assert case['order'][0][2].tolist() == [cell, cell]                       # rows 36 and 37: level 0 of image 2
    by_hand = sum(np.einsum('p,ep->e', case['g'][36 + k].ravel().astype(np.float64), case['feat'][2].reshape(24, -1).astype(np.float64))
                  for k in range(2))
    assert np.array_equal(_np(gmaps[0])[2, :, cell // 6, cell % 6], by_hand)


@pytest.mark.parametrize('hw', [(7, 9), (8, 24)], ids=['7x9', '8x24'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_exact_at_the_largest_E(dev, dtype, hw):
    """E = 1024, the limit: the forward tile of 64 pixels x (1024 + 8) halves is 129 KiB of LDS, above the 64 KiB a launch gets without
    asking.  Operands in {-1, 0, 1}: logits (fp32 output) and both gradients equal fp64."""
    case = R.make_case(seed=501, E=1024, H=hw[0], W=hw[1], integers=True, **EXACT_LAYOUT)
    case = dict(case, feat=np.sign(case['feat']), maps=[np.sign(m) for m in case['maps']], g=np.sign(case['g']))
    want = R.run_ref(case, torch.float64, sigmoid=False)
    assert max(float(np.abs(w).max()) for w in (want[1], *want[2])) <= 256
    out, gfeat, gmaps, _, _ = _gpu(case, dev, dtype, sigmoid=False, out_dtype=torch.float32)
    assert np.array_equal(_np(out), want[0]) and np.array_equal(_np(gfeat), want[1])
    assert all(np.array_equal(_np(got), w) for got, w in zip(gmaps, want[2]))


SEEDED = dict(R.CASES, c=dict(seed=14, B=3, E=40, H=13, W=21, grids=[7, 2], counts=[[33, 0, 2], [1, 0, 3]]))
_REF = {}
FRACTIONS = {}


def _reference(name, dtype, sigmoid):
    """The restatement on the CPU on the rounded arrays: fp64, the half type and fp32, computed once."""
    key = (name, dtype, sigmoid)
    if key not in _REF:
        case = _rounded(R.make_case(**SEEDED[name]), dtype)
        _REF[key] = (case, R.run_ref(case, torch.float64, sigmoid), R.run_ref(case, dtype, sigmoid), R.run_ref(case, torch.float32, sigmoid))
    return _REF[key]


def _flat(maps):
    return np.concatenate([np.asarray(m).ravel() for m in maps])


def _within(got, q64, qref, what):
    tol = R.bound(qref, q64)
    top = float(np.abs(np.asarray(q64)).max())
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(q64)).max())
    FRACTIONS[what] = err / (tol * top) if tol * top > 0 else 0.0
    print(f'{what}: {FRACTIONS[what]:.3f} of its bound')
    R.assert_within(got, q64, tol, what)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('sigmoid', [True, False], ids=['sig', 'lin'])
@pytest.mark.parametrize('name', sorted(SEEDED))
def test_seeded_cases(dev, name, sigmoid, dtype):
    case, q64, q16, q32 = _reference(name, dtype, sigmoid)
    tag = f'{name} {"sig" if sigmoid else "lin"} {str(dtype)[6:]}'
    out, gfeat, gmaps, _, _ = _gpu(case, dev, dtype, sigmoid)
    assert out.dtype == dtype and gfeat.dtype == dtype
    _within(_np(out), q64[0], q16[0], f'{tag} masks')
    _within(_np(gfeat), q64[1], q16[1], f'{tag} grad_feat')
    _within(_flat([_np(m) for m in gmaps]), _flat(q64[2]), _flat(q16[2]), f'{tag} grad_kernel')
    out32, gfeat32, gmaps32, _, _ = _gpu(case, dev, dtype, sigmoid, out_dtype=torch.float32)
    assert out32.dtype == torch.float32 and gfeat32.dtype == dtype
    _within(_np(out32), q64[0], q32[0], f'{tag} masks, fp32 out')
    _within(_np(gfeat32), q64[1], q16[1], f'{tag} grad_feat, fp32 out')
    _within(_flat([_np(m) for m in gmaps32]), _flat(q64[2]), _flat(q16[2]), f'{tag} grad_kernel, fp32 out')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_row_does_not_depend_on_the_other_rows(dev, dtype):
    """The row of (image 0, level 0, cell c): alone, among others in another order, with its image in another slot of the batch, and as a
    row of the test-time layout -- the same bits; the student's masks of the pair are the single call's."""
    import boxinstseg_amd as B
    case = R.make_case(51, 2, 24, 13, 21, [6, 3], [[5, 34], [3, 2]])
    feat, maps, order, _ = R.to_torch(case, dtype, dev)
    run = lambda m, o, f: R.cat_levels(B.solo_dynamic_masks(m, o, f, compute='half')[0])                   # noqa: E731
    full = run(maps, order, feat)
    assert full.dtype == dtype
    want = full[2]
    cell, empty = order[0][0][2:3], order[0][0][:0]
    alone = run(maps, [[cell, empty], [empty, empty]], feat)
    assert alone.shape[0] == 1 and torch.equal(_bits(alone[0]), _bits(want))
    perm = [[order[0][0].flip(0), order[0][1].roll(7)], [order[1][0].flip(0), order[1][1]]]
    moved = run(maps, perm, feat)
    assert torch.equal(_bits(moved[5 - 1 - 2]), _bits(want)) and torch.equal(_bits(moved[5:5 + 34]), _bits(full[5:5 + 34].roll(7, 0)))
    swap = run([m.flip(0).contiguous() for m in maps], [[order[0][1], order[0][0]], [order[1][1], order[1][0]]], feat.flip(0).contiguous())
    assert torch.equal(_bits(swap[34 + 2]), _bits(want)) and torch.equal(_bits(swap[:34]), _bits(full[5:39]))
    for b in range(2):
        rows = torch.cat([maps[l][b].reshape(24, -1).t() for l in range(2)]).contiguous()                 # [36 + 9, E]
        pick = torch.cat([order[0][b], order[1][b] + 36])
        got = B.solo_candidate_masks(feat[b:b + 1], rows, pick, compute='half')
        mine = torch.cat([full[:5] if b == 0 else full[5:39], full[39:42] if b == 0 else full[42:44]])
        assert got.dtype == dtype and torch.equal(_bits(got), _bits(mine))
        assert torch.equal(_bits(B.solo_candidate_masks(feat[b:b + 1], rows[pick].contiguous(), compute='half')), _bits(mine))
    # the pair: the student's masks and gradients are the single call's; the teacher carries no graph
    teacher = dict(R.make_case(151, 2, 24, 13, 21, [6, 3], [[5, 34], [3, 2]]), order=case['order'], g=case['g'])
    single = _gpu(case, dev, dtype)
    t_single = _gpu(teacher, dev, dtype, grad=False)
    feat, maps, order, g = R.to_torch(case, dtype, dev, requires_grad=True)
    t_feat, t_maps, _, _ = R.to_torch(teacher, dtype, dev, requires_grad=True)
    s_masks, t_masks, _ = B.solo_dynamic_masks_pair(maps, t_maps, order, feat, t_feat, compute='half')
    assert torch.equal(_bits(R.cat_levels(s_masks)), _bits(single[0])) and torch.equal(_bits(R.cat_levels(t_masks)), _bits(t_single[0]))
    assert all(not t.requires_grad for t in t_masks) and R.cat_levels(s_masks).requires_grad
    (R.cat_levels(s_masks) * g).sum().backward()
    assert torch.equal(_bits(feat.grad), _bits(single[1])) and all(torch.equal(_bits(m.grad), _bits(w)) for m, w in zip(maps, single[2]))
    assert t_feat.grad is None and all(m.grad is None for m in t_maps)
    again = _gpu(case, dev, dtype)                                            # and two runs are bit-identical
    assert torch.equal(_bits(again[1]), _bits(single[1])) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(again[2], single[2]))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_nan_containment(dev, dtype):
    """A NaN in a kernel row makes that row NaN and no other; a NaN in the feature makes that pixel NaN for the rows of its image only."""
    import boxinstseg_amd as B
    case = R.make_case(61, 2, 5, 13, 21, [6, 3], [[3, 34], [2, 1]])
    feat, maps, order, _ = R.to_torch(case, dtype, dev)
    run = lambda m, f, **k: R.cat_levels(B.solo_dynamic_masks(m, order, f, compute='half', **k)[0])        # noqa: E731
    clean = run(maps, feat)
    cell = int(order[0][1][33])                                               # row 3 + 33 = 36: the second chunk of image 1
    bad = [m.clone() for m in maps]
    bad[0][1, 2, cell // 6, cell % 6] = float('nan')
    for sigmoid in (True, False):
        nan = torch.isnan(run(bad, feat, sigmoid=sigmoid))
        assert bool(nan[36].all()) and int(nan.sum()) == 13 * 21
    keep = torch.ones(clean.shape[0], dtype=torch.bool, device=dev)
    keep[36] = False
    assert torch.equal(_bits(run(bad, feat)[keep]), _bits(clean[keep]))
    f2 = feat.clone()
    f2[1, 4, 12, 20] = float('nan')                                           # the last pixel: the short last tile
    f2[1, 0, 0, 0] = float('nan')
    out = run(maps, f2)
    nan = torch.isnan(out)
    of_image_1 = torch.tensor([False] * 3 + [True] * 34 + [False] * 2 + [True], device=dev)
    assert bool(nan[of_image_1][:, 12, 20].all()) and bool(nan[of_image_1][:, 0, 0].all()) and int(nan.sum()) == 2 * 35
    assert torch.equal(_bits(out[~of_image_1]), _bits(clean[~of_image_1]))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_cell_outside_its_map_and_no_rows_at_all(dev, dtype):
    import boxinstseg_amd as B
    from boxinstseg_amd import solo_conv as SC
    case = R.make_case(72, 1, 5, 7, 9, [2], [[3]])
    feat, maps, order, g = R.to_torch(case, dtype, dev, requires_grad=True)
    clean = R.cat_levels(B.solo_dynamic_masks(maps, order, feat, sigmoid=False, compute='half')[0]).detach()
    for bad in (4, -1, 1 << 40):
        o = [[order[0][0].clone()]]
        o[0][0][1] = bad
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        feat.grad = None
        maps[0].grad = None
        out = R.cat_levels(B.solo_dynamic_masks(maps, o, feat, sigmoid=False, status=status, compute='half')[0])
        (out * g).sum().backward()
        assert int(status) == 1 and not bool(out[1].any())                    # the zero-kernel row
        assert torch.equal(_bits(out[0]), _bits(clean[0])) and torch.equal(_bits(out[2]), _bits(clean[2]))
        assert bool(torch.isfinite(feat.grad.float()).all()) and bool(torch.isfinite(maps[0].grad.float()).all())
        used = [int(o[0][0][0]), int(o[0][0][2])]
        free = [c for c in range(4) if c not in used]
        assert not bool(maps[0].grad.reshape(5, 4)[:, free].any()) and bool(maps[0].grad.reshape(5, 4)[:, used].any())
    # N == 0: no mask, all-zero gradients
    case = R.make_case(71, 2, 5, 7, 9, [3, 2], [[0, 0], [0, 0]])
    feat, maps, order, _ = R.to_torch(case, dtype, dev, requires_grad=True)
    assert B.solo_dynamic_masks(maps, order, feat, compute='half') == ([None, None], [None, None])
    plan = SC._plan(maps, order, feat, True, None)
    plan.out_dtype = dtype
    with G.poisoned_empty():
        out, _ = SC._DynamicMasks.apply(plan, feat, *maps)
        assert out.shape == (0, 7, 9) and out.dtype == dtype
        out.sum().backward()
    assert feat.grad.dtype == dtype and not bool(feat.grad.any()) and not any(bool(m.grad.any()) for m in maps)
    assert not bool(torch.isnan(feat.grad).any()) and not any(bool(torch.isnan(m.grad).any()) for m in maps)


def test_fp16_subnormal_operands_keep_their_value(dev):
    """include/boxinst/boxinst_hip_dconv16.h: fp16 subnormal A / B operands are not flushed.  The smallest subnormal 2^-24 times 2^10 is
    2^-14 exactly, and 2^-24 * 1 + 2^-24 * 1 = 2^-23; a flushed operand would give 0."""
    import boxinstseg_amd as B
    tiny = 2.0 ** -24
    feat = torch.zeros(1, 2, 1, 8, dtype=torch.float16, device=dev)
    feat[0, 0, 0, :] = 1024.0
    feat[0, 0, 0, 1] = tiny                                                   # a subnormal on the B side, against a normal kernel value
    kern = torch.tensor([[tiny, 0.0], [1.0, 0.0]], dtype=torch.float16, device=dev)
    assert float(kern[0, 0]) == tiny and float(feat[0, 0, 0, 1]) == tiny
    out = B.solo_candidate_masks(feat, kern, sigmoid=False, compute='half', out_dtype=torch.float32)
    assert out[0, 0, 0].item() == 2.0 ** -14 and out[0, 0, 1].item() == 2.0 ** -48 and out[1, 0, 1].item() == tiny and out[1, 0, 0].item() == 1024.0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_get_seg_single_with_the_half_product(dev, dtype):
    """discobox_get_seg_single(conv='hip_half') on half tensors against conv='torch' on the fp32 upcast of the same values: the
    construction of tests/test_gpu_solo_conv.py (feature in {-1, 1}, kernel values odd in [-3, 3], channel 15 off: every logit an odd
    integer, every probability at least 0.23 from mask_thr), with the inputs rounded to the half type -- which changes none of them."""
    import boxinstseg_amd as B
    rng = np.random.default_rng(91)
    grids, strides, ncls, E, hw = [4, 3], [8, 16], 3, 16, (24, 40)
    feat = rng.choice([-1.0, 1.0], size=(1, E, *hw)).astype(np.float32)
    kern = rng.choice([-3.0, -1.0, 1.0, 3.0], size=(25, E)).astype(np.float32)
    kern[:, 15] = 0
    cate = (rng.uniform(0, 1, (25, ncls)) * (rng.random((25, ncls)) < 0.5)).astype(np.float32)
    cfg = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    meta = dict(img_shape=(90, 150, 3), ori_shape=(61, 93, 3))
    feat_h, kern_h = torch.from_numpy(feat).to(dtype), torch.from_numpy(kern).to(dtype)
    assert torch.equal(feat_h.float(), torch.from_numpy(feat)) and torch.equal(kern_h.float(), torch.from_numpy(kern))
    # the reference alone, on the CPU, after rounding: the margin, and the half run agrees with fp64 on every mask byte
    p = {dt: R.candidate_masks(feat_h.to(dt), kern_h.to(dt)) for dt in (dtype, torch.float64)}
    assert float((p[torch.float64] - 0.5).abs().min()) > 0.23 and float((p[dtype].double() - 0.5).abs().min()) > 0.23
    assert torch.equal(p[dtype] > cfg['mask_thr'], p[torch.float64] > cfg['mask_thr'])
    rest = (hw, meta, cfg, grids, strides)
    want = B.discobox_get_seg_single(torch.from_numpy(cate).to(dev), feat_h.float().to(dev), kern_h.float().to(dev), *rest, conv='torch')
    got = B.discobox_get_seg_single(torch.from_numpy(cate).to(dev), feat_h.to(dev), kern_h.to(dev), *rest, conv='hip_half')
    assert want is not None and want.masks.shape[0] > 3
    assert torch.equal(got.labels, want.labels) and torch.equal(got.masks, want.masks) and torch.equal(got.mask_stats, want.mask_stats)
    assert got.scores.dtype == want.scores.dtype and torch.allclose(got.scores, want.scores, rtol=1e-5, atol=0)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_captured_graph_follows_its_inputs(dev, dtype):
    """Forward and backward of the smallest seeded case captured in a hipGraph; replayed after the inputs changed in place it gives the
    eager call's bits."""
    import boxinstseg_amd as B
    case = _rounded(R.make_case(**SEEDED['a']), dtype)
    feat, maps, order, g = R.to_torch(case, dtype, dev, requires_grad=True)

    def step():
        out = R.cat_levels(B.solo_dynamic_masks(maps, order, feat, compute='half')[0])
        return out.detach(), torch.autograd.grad((out * g).sum(), [feat, *maps])

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
