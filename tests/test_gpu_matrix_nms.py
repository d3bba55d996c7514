"""GPU: Matrix NMS and mask scoring (csrc/matrix_nms.hip, boxinstseg_amd/matrix_nms.py) against the reference formulation.

* decay_iou is BIT-EQUAL to the reference's fp32 formulation on the CPU (``masks.float() @ masks.float().T``, the division, triu,
  the label matrix, matrix_nms.py:65-85), area exactly equal;
* decayed scores against the float64 restatement (tests/matrix_nms_ref.py) within 2e-6 relative.  Derived, not measured: the IoU
  is the reference's own fp32 value; then a square, a multiply by sigma <= 2, two expf of <= 1 ulp each, a divide and a multiply --
  about 1.1e-6 in all;
* maskness psum / area within 2e-6 relative of the float64 sum: all terms positive, a reduction tree of depth <= 24 at these
  shapes (<= 2 groups per lane, 2 + 6 + 3 levels above) loses at most 24 * 2^-24;
* order and cuts only where the float64 scores are more than 1e-4 relative apart (asserted, never skipped).
The bit layout is private to the library, so the tests decode it from outside: masks whose pixels carry the bits of their own
index tell where every pixel went (``layout``)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import matrix_nms_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'matrix_nms.npz')
RTOL = 2e-6
f32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_LAYOUT = {}


def layout(dev, h, w):
    """position (word * 64 + bit) -> pixel index, -1 where no pixel lives, found by packing masks of the pixels' index bits."""
    from boxinstseg_amd.matrix_nms import pack_masks
    if (h, w) not in _LAYOUT:
        hw = h * w
        nb = max(int(hw - 1).bit_length(), 1)
        idx = np.arange(hw)
        planes = np.stack([np.ones(hw, bool)] + [((idx >> k) & 1).astype(bool) for k in range(nb)]).reshape(nb + 1, h, w)
        bits, area = pack_masks(_t(planes, dev))
        b = unpack_words(bits)
        assert area.cpu().tolist() == planes.reshape(nb + 1, -1).sum(1).tolist()
        pos = sum(b[k + 1].astype(np.int64) << k for k in range(nb))
        pos = np.where(b[0], pos, -1)
        assert sorted(pos[pos >= 0].tolist()) == list(range(hw)), 'every pixel has exactly one bit'
        _LAYOUT[(h, w)] = pos
    return _LAYOUT[(h, w)]


def unpack_words(bits):
    wd = bits.cpu().numpy().view(np.uint64)
    return ((wd[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(len(wd), -1)


def decode(dev, bits, h, w):
    """bits [n, words] -> bool [n,h,w]; asserts that positions without a pixel are zero."""
    pos, b = layout(dev, h, w), unpack_words(bits)
    assert b.shape[1] == (h * w + 63) // 64 * 64
    assert not b[:, pos < 0].any(), 'a bit beyond h*w is set'
    out = np.zeros((len(b), h * w), bool)
    out[:, pos[pos >= 0]] = b[:, pos >= 0]
    return out.reshape(len(b), h, w)


def reference_decay_iou(masks, labels, order, area=None):
    """matrix_nms.py:60-85 as written, fp32 on the CPU."""
    m = torch.from_numpy(masks)[order]
    lab = torch.from_numpy(np.asarray(labels))[order]
    a = (m.sum((1, 2)).float() if area is None else torch.from_numpy(np.asarray(area)).float()[order])
    n = len(lab)
    flat = m.reshape(n, -1).float()
    inter = torch.mm(flat, flat.transpose(1, 0))
    ea = a.expand(n, n)
    iou = (inter / (ea + ea.transpose(1, 0) - inter)).triu(diagonal=1)
    el = lab.expand(n, n)
    label_matrix = (el == el.transpose(1, 0)).triu(diagonal=1)
    return (iou * label_matrix).numpy()


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{what}: NaN pattern differs'
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), \
        f'{what}: {int((got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan]).sum())} entries differ in their bits'


def assert_scores(got, want, what, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f'{what}: {got.shape} vs {want.shape}'
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-30)
    err = np.where(want[ok] == 0, np.abs(got[ok]), err)
    print(f'{what}: max relative error {err.max() if err.size else 0:.2e} (limit {rtol:.0e})')
    assert (err <= rtol).all(), f'{what}: {err.max():.3e} > {rtol}'


def make_labels(rng, n, mode):
    return {'one': np.zeros(n, np.int64), 'several': rng.integers(0, 4, n), 'distinct': rng.permutation(n).astype(np.int64)}[mode]


def run_stage(dev, masks, labels, scores, nms_pre=-1, kernel='gaussian', sigma=2.0, area=None):
    """pack -> sort -> the n x n stage; everything the kernels wrote, on the host."""
    from boxinstseg_amd.matrix_nms import matrix_nms_decay, pack_masks
    bits, a = pack_masks(_t(masks, dev))
    if area is not None:
        a = _t(np.asarray(area, np.int32), dev)
    s, order = torch.sort(_t(scores, dev), descending=True, stable=True)
    if nms_pre > 0:
        s, order = s[:nms_pre], order[:nms_pre]
    decayed, iou, comp = matrix_nms_decay(bits, a, _t(labels, dev), order, s, masks.shape[-2:], kernel, sigma)
    torch.cuda.synchronize()
    return dict(bits=bits, area=a.cpu().numpy(), order=order.cpu().numpy(), decayed=decayed.cpu().numpy(), decay_iou=iou.cpu().numpy(),
                compensate=comp.cpu().numpy())


# n x (h, w) x labels: every n with a shape and a label mode in rotation, every shape and every label mode at a tile edge
STAGE_CASES = [(1, (7, 9), 'one'), (2, (24, 40), 'one'), (2, (25, 38), 'distinct'), (31, (25, 38), 'several'), (32, (50, 76), 'one'),
               (33, (7, 9), 'several'), (33, (24, 40), 'distinct'), (33, (25, 38), 'one'), (33, (50, 76), 'several'),
               (65, (24, 40), 'several'), (65, (7, 9), 'one'), (130, (25, 38), 'one'), (130, (50, 76), 'distinct'),
               (130, (24, 40), 'several'), (300, (25, 38), 'several'), (300, (50, 76), 'one'),
               # past the 512 threads that fill the decay kernel's LDS tables: exactly one trip, one element of a second, a third, and
               # BXI_NMS_MAX_CANDIDATES = 2048 (four full trips, a 16 MB matrix)
               (512, (7, 9), 'several'), (513, (7, 9), 'one'), (1025, (24, 40), 'several'), (2048, (7, 9), 'several'),
               (2048, (25, 38), 'one')]


@pytest.mark.parametrize('n,hw,mode', STAGE_CASES)
def test_decay_iou_is_bit_equal_and_scores_within_limit(dev, n, hw, mode):
    h, w = hw
    rng = np.random.default_rng(1000 * n + h)
    masks, labels, scores = R.disc_masks(rng, n, h, w), make_labels(rng, n, mode), R.shuffled_scores(rng, n)
    for kernel, sigma in (('gaussian', 2.0), ('gaussian', 0.5), ('linear', 2.0)):
        s = run_stage(dev, masks, labels, scores, kernel=kernel, sigma=sigma)
        ref = R.matrix_nms_ref(masks, labels, scores, kernel=kernel, sigma=sigma)
        assert np.array_equal(s['area'], masks.reshape(n, -1).sum(1))
        assert np.array_equal(decode(dev, s['bits'], h, w), masks)
        assert np.array_equal(s['order'], ref['order'])
        want = reference_decay_iou(masks, labels, s['order'])
        assert_bit_equal(s['decay_iou'], want, f'decay_iou n={n} {hw} {mode}')
        assert_bit_equal(want, ref['decay_iou'], 'the restatement\'s IoU')
        assert_bit_equal(s['compensate'], want.max(0), 'compensate')
        assert_scores(s['decayed'], ref['decayed'], f'decayed n={n} {hw} {mode} {kernel} {sigma}')
        if mode == 'distinct':
            assert not s['decay_iou'].any() and np.array_equal(s['decayed'], np.sort(scores)[::-1])


def _golden(name):
    from tests.test_host_matrix_nms import golden_case
    return golden_case(np.load(GOLDEN), name)


@pytest.mark.parametrize('name', ['g20', 'g05', 'lin', 'cut'])
def test_mask_matrix_nms_order_and_cuts_against_the_fixture(dev, name):
    """n = 40: keep_inds in order, labels, masks, scores; cuts by nms_pre, filter_thr and max_num."""
    from boxinstseg_amd import mask_matrix_nms
    g, c = np.load(GOLDEN), _golden(name)
    ref = R.matrix_nms_ref(c['masks'], c['labels'], c['scores'], c['filter_thr'], c['nms_pre'], c['max_num'], c['kernel'], c['sigma'])
    assert R.min_rel_gap(ref['decayed'], (c['filter_thr'],)) > 1e-4          # precondition of an order check
    masks = _t(c['masks'], dev)
    for m in (masks, masks.to(torch.uint8) * 255):
        s, l, mk, k = mask_matrix_nms(m, _t(c['labels'], dev), _t(c['scores'], dev), filter_thr=c['filter_thr'], nms_pre=c['nms_pre'],
                                      max_num=c['max_num'], kernel=c['kernel'], sigma=c['sigma'])
        assert k.cpu().tolist() == g[f'{name}_keep_inds'].tolist() == ref['keep_inds'].tolist()
        assert l.cpu().tolist() == g[f'{name}_out_labels'].tolist()
        assert torch.equal(mk, m[k]) and s.dtype == torch.float32 and k.dtype == torch.int64
        assert_scores(s.cpu().numpy(), ref['scores'], f'{name} scores')
        assert_scores(s.cpu().numpy(), g[f'{name}_out_scores'], f'{name} scores vs the reference\'s fp32', rtol=RTOL + 1e-6)


def test_more_candidates_than_the_limit_is_an_error_that_names_it(dev):
    """2049 candidates and no nms_pre: an error that names the limit, never a truncated result; with nms_pre at the limit the same
    candidates pass."""
    from boxinstseg_amd import _lib, mask_matrix_nms
    from boxinstseg_amd.matrix_nms import matrix_nms_scores, pack_masks
    n_all = _lib.NMS_MAX_CANDIDATES + 1
    assert n_all == 2049
    rng = np.random.default_rng(n_all)
    masks, labels, scores = _t(R.disc_masks(rng, n_all, 7, 9), dev), _t(rng.integers(0, 3, n_all), dev), _t(R.shuffled_scores(rng, n_all), dev)
    for nms_pre in (-1, 0, n_all):
        with pytest.raises(NotImplementedError, match=r'2049 candidates.*BXI_NMS_MAX_CANDIDATES = 2048.*nms_pre'):
            mask_matrix_nms(masks, labels, scores, nms_pre=nms_pre)
    bits, area = pack_masks(masks)
    with pytest.raises(NotImplementedError, match='BXI_NMS_MAX_CANDIDATES = 2048'):
        matrix_nms_scores(bits, area, labels, scores, (7, 9))
    s, _, _, k = mask_matrix_nms(masks, labels, scores, nms_pre=n_all - 1)
    assert len(k) == len(s) == n_all - 1 and int(scores.argmin()) not in k.cpu().tolist()


@pytest.mark.parametrize('n_all,nms_pre,hw', [(130, -1, (25, 38)), (300, -1, (50, 76)), (700, 500, (50, 76)), (2048, -1, (7, 9)),
                                              (2100, 2048, (7, 9))])
def test_mask_matrix_nms_large_sets(dev, n_all, nms_pre, hw):
    """Near-ties are 1e-5 apart here: the set of keep_inds, the score of every index, and a non-increasing result."""
    from boxinstseg_amd import mask_matrix_nms
    rng = np.random.default_rng(n_all)
    masks, labels, scores = R.disc_masks(rng, n_all, *hw, centres=6), rng.integers(0, 3, n_all), R.shuffled_scores(rng, n_all)
    ref = R.matrix_nms_ref(masks, labels, scores, nms_pre=nms_pre)
    s, l, mk, k = mask_matrix_nms(_t(masks, dev), _t(labels, dev), _t(scores, dev), nms_pre=nms_pre)
    s, k = s.cpu().numpy(), k.cpu().numpy()
    assert len(k) == (nms_pre if nms_pre > 0 else n_all) and sorted(k.tolist()) == sorted(ref['keep_inds'].tolist())
    by_index = dict(zip(ref['keep_inds'].tolist(), ref['scores'].tolist()))
    assert_scores(s, np.array([by_index[i] for i in k.tolist()]), f'n_all={n_all} per-index scores')
    assert (np.diff(s) <= 0).all()
    assert l.cpu().tolist() == labels[k].tolist() and tuple(mk.shape) == (len(k), *hw)


def test_tied_scores_lower_index_first(dev):
    from boxinstseg_amd import mask_matrix_nms
    from boxinstseg_amd.matrix_nms import matrix_nms_scores, pack_masks
    rng = np.random.default_rng(5)
    n, h, w = 36, 24, 40
    masks, labels = R.disc_masks(rng, n, h, w), rng.integers(0, 2, n)
    scores = np.repeat(np.linspace(0.2, 0.9, n // 3), 3).astype(f32)[rng.permutation(n)]         # every score three times
    ref = R.matrix_nms_ref(masks, labels, scores)
    bits, area = pack_masks(_t(masks, dev))
    decayed, order = matrix_nms_scores(bits, area, _t(labels, dev), _t(scores, dev), (h, w))
    assert order.cpu().tolist() == ref['order'].tolist()
    for a, b in zip(ref['order'][:-1], ref['order'][1:]):
        assert scores[a] > scores[b] or (scores[a] == scores[b] and a < b)
    assert_scores(decayed.cpu().numpy(), ref['decayed'], 'tied inputs')
    s, _, _, k = mask_matrix_nms(_t(masks, dev), _t(labels, dev), _t(scores, dev))
    by_index = dict(zip(ref['keep_inds'].tolist(), ref['scores'].tolist()))
    assert sorted(k.cpu().tolist()) == list(range(n))
    assert_scores(s.cpu().numpy(), np.array([by_index[i] for i in k.cpu().tolist()]), 'tied inputs, result')


def test_three_identical_masks(dev):
    from boxinstseg_amd import mask_matrix_nms
    m = torch.ones(3, 9, 11, dtype=torch.bool, device=dev)
    lab, s = torch.zeros(3, dtype=torch.long, device=dev), torch.tensor([0.9, 0.8, 0.7], device=dev)
    out, _, _, k = mask_matrix_nms(m, lab, s)
    assert k.cpu().tolist() == [0, 1, 2]
    assert np.allclose(out.cpu().numpy(), [0.9, 0.1083, 0.0947], atol=5e-5)
    assert_scores(out.cpu().numpy(), R.matrix_nms_ref(np.ones((3, 9, 11), bool), np.zeros(3, np.int64), s.cpu().numpy())['scores'], 'identical, gaussian')
    out, _, _, k = mask_matrix_nms(m, lab, s, kernel='linear')                # the reference: [NaN, 0.9, 0]
    o = out.cpu().numpy()
    assert k.cpu().tolist() == [2, 0, 1] and np.isnan(o[0]) and o[1] == f32(0.9) and o[2] == 0
    out, l, mk, k = mask_matrix_nms(m, lab, s, kernel='linear', filter_thr=0.05)
    assert k.cpu().tolist() == [0] and out.cpu().numpy()[0] == f32(0.9) and tuple(mk.shape) == (1, 9, 11)
    out, l, mk, k = mask_matrix_nms(m, lab, s * 0.01, filter_thr=0.05)        # nothing survives: the reference's empty tensors
    assert out.numel() == 0 and l.numel() == 0 and tuple(mk.shape) == (0, 9, 11) and k.dtype == torch.int64 and mk.dtype == torch.bool
    out, l, mk, k = mask_matrix_nms(m[:0], lab[:0], s[:0])
    assert out.numel() == 0 and tuple(mk.shape) == (0, 9, 11) and k.numel() == 0
    with pytest.raises(NotImplementedError):
        mask_matrix_nms(m, lab, s, kernel='cosine')


def test_zero_area_gives_the_reference_nan(dev):
    """Caller-supplied areas of zero for two disjoint masks of one label: 0 / 0, a NaN IoU, and with it NaN scores everywhere, as the
    reference's minimum over all rows gives."""
    from boxinstseg_amd import mask_matrix_nms
    rng = np.random.default_rng(9)
    n, h, w = 35, 7, 9
    masks = R.disc_masks(rng, n, h, w)
    masks[0], masks[1] = False, False
    masks[0, 0, 0], masks[1, 6, 8] = True, True
    labels, scores = np.zeros(n, np.int64), R.shuffled_scores(rng, n)
    area = masks.reshape(n, -1).sum(1)
    area[:2] = 0
    s = run_stage(dev, masks, labels, scores, area=area)
    want = reference_decay_iou(masks, labels, s['order'], area)
    assert np.isnan(want).sum() == 1
    assert_bit_equal(s['decay_iou'], want, 'decay_iou with zero areas')
    ref = R.matrix_nms_ref(masks, labels, scores, mask_area=area)
    assert np.isnan(ref['decayed']).all() and np.isnan(s['decayed']).all() and np.isnan(s['compensate']).sum() == 1
    out, _, _, k = mask_matrix_nms(_t(masks, dev), _t(labels, dev), _t(scores, dev), mask_area=_t(area.astype(f32), dev))
    assert np.isnan(out.cpu().numpy()).all() and len(k) == n


@pytest.mark.parametrize('thr', [0.5, 0.55, 0.7])
def test_threshold_is_the_fp32_comparison(dev, thr):
    """Inputs that hold f32(mask_thr) and both its fp32 neighbours: bit for bit ``seg_preds > mask_thr`` of the CPU."""
    from boxinstseg_amd.matrix_nms import pack_probs
    rng = np.random.default_rng(int(thr * 100))
    n, h, w = 6, 25, 38
    t = f32(thr)
    near = np.array([t, np.nextafter(t, f32(1)), np.nextafter(t, f32(0))], f32)
    p = rng.uniform(0, 1, (n, h, w)).astype(f32)
    sel = rng.uniform(size=p.shape) < 0.5
    p[sel] = near[rng.integers(0, 3, int(sel.sum()))]
    want = (torch.from_numpy(p) > thr).numpy()
    assert want[p == near[1]].all() and not want[p == near[0]].any() and not want[p == near[2]].any()
    bits, area, psum = pack_probs(_t(p, dev), thr)
    assert np.array_equal(decode(dev, bits, h, w), want)
    assert np.array_equal(area.cpu().numpy(), want.reshape(n, -1).sum(1))
    assert_scores(psum.cpu().numpy(), (p.astype(np.float64) * want).reshape(n, -1).sum(1), f'psum at thr {thr}')


def _seg_case(rng, n, h, w):
    probs = R.disc_probs(rng, n, h, w, avoid=(0.5,))
    labels, cate = rng.integers(0, 3, n), R.shuffled_scores(rng, n)
    strides = rng.choice([8.0, 16.0, 0.12 * h * w], n).astype(f32)          # the last one drops the smaller discs
    return probs, labels, cate, strides


@pytest.mark.parametrize('n,hw,nms_pre', [(40, (25, 38), -1), (33, (7, 9), 20), (150, (50, 76), 100)])
def test_seg_nms_block(dev, n, hw, nms_pre):
    """area exact, maskness within 2e-6 of the float64 sum, the result of the fused block against the float64 restatement, and
    EQUAL to mask_matrix_nms fed the materialised masks, the same scores and areas."""
    from boxinstseg_amd import mask_matrix_nms, seg_nms
    from boxinstseg_amd.matrix_nms import pack_probs
    rng = np.random.default_rng(n)
    probs, labels, cate, strides = _seg_case(rng, n, *hw)
    cfg = dict(mask_thr=0.5, filter_thr=0.05, nms_pre=nms_pre, max_per_img=30, kernel='gaussian', sigma=2.0)
    ref = R.seg_nms_ref(probs, labels, cate, strides, 0.5, 0.05, nms_pre, 30, 'gaussian', 2.0)
    assert 0 < len(ref['kept']) < n, 'the area filter must drop some candidates'
    tp, tl, tc, ts = _t(probs, dev), _t(labels, dev), _t(cate, dev), _t(strides, dev)
    bits, area, psum = pack_probs(tp, 0.5)
    assert np.array_equal(area.cpu().numpy(), ref['area'])
    assert_scores((psum / area.float()).cpu().numpy()[ref['kept']], ref['maskness'], 'maskness')
    s, l, k = seg_nms(tp, tl, tc, ts, cfg)
    if n <= 40:
        assert R.min_rel_gap(ref['decayed'], (0.05,)) > 1e-4 and R.min_rel_gap(ref['scores_in']) > 1e-4
        assert k.cpu().tolist() == ref['keep_inds'].tolist()
        assert_scores(s.cpu().numpy(), ref['scores'], 'seg_nms scores')
    assert l.cpu().tolist() == labels[k.cpu().numpy()].tolist()
    # the same through the materialised masks
    masks = tp > 0.5
    kept = (area.float() > ts).nonzero(as_tuple=True)[0]
    scores = tc[kept] * (psum[kept] / area.float()[kept])
    s2, l2, _, k2 = mask_matrix_nms(masks[kept], tl[kept], scores, filter_thr=0.05, nms_pre=nms_pre, max_num=30, mask_area=area.float()[kept])
    assert torch.equal(s, s2) and torch.equal(l, l2) and torch.equal(k, kept[k2])
    none = seg_nms(tp, tl, tc, ts * 1e4, cfg)
    assert all(t.numel() == 0 for t in none) and none[2].dtype == torch.int64
    assert all(t.numel() == 0 for t in seg_nms(tp[:0], tl[:0], tc[:0], ts[:0], cfg))


def _p64_final(probs_kept, featmap, img_shape, ori_shape):
    x = torch.from_numpy(probs_kept).double().unsqueeze(0)
    x = F.interpolate(x, size=(featmap[0] * 4, featmap[1] * 4), mode='bilinear')[:, :, :img_shape[0], :img_shape[1]]
    return F.interpolate(x, size=tuple(ori_shape[:2]), mode='bilinear').squeeze(0).numpy()


@pytest.mark.parametrize('head', ['box_solov2', 'discobox'])
def test_get_seg_single_mirrors_against_the_fixture(dev, head):
    import boxinstseg_amd as B
    from tests.test_host_matrix_nms import golden_seg
    g = np.load(GOLDEN)
    cfg, idx, cate_scores, level = golden_seg(g)
    meta = dict(img_shape=tuple(int(v) for v in g['seg_img_shape']), ori_shape=tuple(int(v) for v in g['seg_ori_shape']))
    grids, strides = g['seg_grids'].tolist(), g['seg_strides'].tolist()
    if head == 'box_solov2':
        res = B.box_solov2_get_seg_single(_t(g['seg_cate'], dev), _t(g['seg_probs'], dev), (11, 17), meta, cfg, grids, strides)
    else:
        res = B.discobox_get_seg_single(_t(g['seg_cate'], dev), _t(g['seg_feat'], dev), _t(g['seg_kernels'], dev), (11, 17), meta, cfg, grids, strides)
    ref = R.seg_nms_ref(g['seg_probs'][idx[:, 0]], idx[:, 1], cate_scores, level, cfg['mask_thr'], cfg['filter_thr'], cfg['nms_pre'],
                        cfg['max_per_img'], cfg['kernel'], cfg['sigma'])
    assert R.min_rel_gap(ref['decayed'], (cfg['filter_thr'],)) > 1e-4 and R.min_rel_gap(ref['scores_in']) > 1e-4
    assert res.labels.cpu().tolist() == g['seg_out_labels'].tolist() == ref['labels'].tolist()
    assert_scores(res.scores.cpu().numpy(), ref['scores'], f'{head} scores')
    assert_scores(res.scores.cpu().numpy(), g['seg_out_scores'], f'{head} scores vs the reference\'s fp32', rtol=RTOL + 1e-6)
    oh, ow = meta['ori_shape'][:2]
    want = np.unpackbits(g['seg_out_masks'], axis=1)[:, :oh * ow].reshape(-1, oh, ow).astype(bool)
    got = res.masks.cpu().numpy()
    assert got.dtype == bool and got.shape == want.shape
    p64 = _p64_final(g['seg_probs'][idx[:, 0]][ref['keep_inds']], (11, 17), meta['img_shape'], meta['ori_shape'])
    outside = np.abs(p64 - cfg['mask_thr']) > 1e-6
    assert outside.mean() > 0.99
    assert np.array_equal(got[outside], want[outside]) and np.array_equal(got[outside], (p64 > cfg['mask_thr'])[outside])
    # nothing above the score threshold: the reference's empty results
    none = B.box_solov2_get_seg_single(_t(g['seg_cate'] * 0, dev), _t(g['seg_probs'], dev), (11, 17), meta, cfg, grids, strides)
    assert none.scores.numel() == 0 and tuple(none.masks.shape) == (0, oh, ow)


def test_two_calls_are_bit_identical(dev):
    from boxinstseg_amd import seg_nms
    from boxinstseg_amd.matrix_nms import pack_probs
    rng = np.random.default_rng(3)
    probs, labels, cate, strides = _seg_case(rng, 130, 50, 76)
    cfg = dict(mask_thr=0.5, filter_thr=-1, nms_pre=-1, max_per_img=-1, kernel='gaussian', sigma=2.0)
    tp, tl, tc, ts = _t(probs, dev), _t(labels, dev), _t(cate, dev), _t(strides, dev)
    a, b = pack_probs(tp, 0.5), pack_probs(tp.clone(), 0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    r1, r2 = seg_nms(tp, tl, tc, ts, cfg), seg_nms(tp.clone(), tl, tc, ts, cfg)
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(r1, r2))
    m, lab, sc = R.disc_masks(rng, 130, 25, 38), rng.integers(0, 2, 130), R.shuffled_scores(rng, 130)
    s1, s2 = run_stage(dev, m, lab, sc), run_stage(dev, m, lab, sc)
    for key in ('decayed', 'decay_iou', 'compensate'):
        assert np.array_equal(s1[key].view(np.uint32), s2[key].view(np.uint32)), key


def test_graph_capture_and_replay_with_changed_inputs(dev):
    """pack -> sort -> the n x n stage captured once; replays follow the contents of the input tensors."""
    from boxinstseg_amd.matrix_nms import matrix_nms_scores, pack_probs
    rng = np.random.default_rng(11)
    n, h, w = 70, 25, 38
    cases = [(R.disc_probs(rng, n, h, w), rng.integers(0, 3, n), R.shuffled_scores(rng, n)) for _ in range(3)]
    tp, tl, ts = (torch.empty_like(_t(a, dev)) for a in cases[0])

    def step():
        bits, area, psum = pack_probs(tp, 0.5)
        decayed, order = matrix_nms_scores(bits, area, tl, ts, (h, w), nms_pre=50)
        return decayed, order, psum

    def load(c):
        for dst, src in zip((tp, tl, ts), c):
            dst.copy_(_t(src, dev))

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for c in (cases[1], cases[2], cases[0]):
        load(c)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        want = step()
        torch.cuda.synchronize()
        assert torch.equal(got[1], want[1])
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
        ref = R.matrix_nms_ref(c[0] > f32(0.5), c[1], c[2], nms_pre=50)
        assert got[1].cpu().tolist() == ref['order'].tolist()
        assert_scores(got[0].cpu().numpy(), ref['decayed'], 'replayed')
