"""GPU: CondInst's test-time detections (boxinstseg_amd/box_nms.py, csrc/box_nms.hip) against the numpy restatement
(tests/box_nms_ref.py) and against what the reference's own code computed (tests/golden/det_nms.npz).

Keep lists are compared as lists.  That is only meaningful where no IoU sits within the fp32 arithmetic's reach of the threshold, so
every recipe input is taken at a seed whose comparable pairs all have |IoU - thr| > 1e-4 in float64 (about six fp32 roundings of
6e-8 decide the test), and the tests assert that margin before they compare.  Scores must be within 4 * tol of the float64 value,
tol being the fixture's own float32-against-float64 difference of the reference (the kernel has the same three roundings plus an
expf that may differ from ATen's by an ulp or two)."""
import os

import numpy as np
import pytest
import torch

from tests import box_nms_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'det_nms.npz')
MARGIN = 1e-4


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _segments(dev, segs, cap=None):
    """segs: list of (boxes [n,4], scores [n], labels [n] or None) -> padded device tensors (boxes, scores, labels, count)."""
    cap = cap or max(max(len(s[1]) for s in segs), 1)
    P = len(segs)
    boxes, scores, labels = np.zeros((P, cap, 4), np.float32), np.zeros((P, cap), np.float32), np.zeros((P, cap), np.int64)
    for p, (b, s, l) in enumerate(segs):
        n = min(len(s), cap)
        boxes[p, :n], scores[p, :n] = b[:n], s[:n]
        if l is not None:
            labels[p, :n] = l[:n]
    return _t(boxes, dev), _t(scores, dev), _t(labels, dev), torch.tensor([len(s[1]) for s in segs], dtype=torch.int32, device=dev)


def _run(dev, segs, thr=0.5, offset=0, max_num=-1, agnostic=False, order=None, cap=None):
    from boxinstseg_amd import box_nms
    b, s, l, c = _segments(dev, segs, cap)
    keep, n_keep, status = box_nms.box_nms(b, s, None if agnostic else l, c, thr, offset, max_num, order)
    keep, n_keep, status = keep.cpu().numpy(), n_keep.cpu().tolist(), status.cpu().tolist()
    out = []
    for p, n in enumerate(n_keep):
        if n >= 0:
            assert (keep[p, n:] == -1).all()
        out.append(None if n < 0 else keep[p, :n].tolist())
    return out, status


def _recipe(seed, n, nlab, thr=0.5, offset=0, agnostic=False):
    b, s, l = R.clustered_boxes_with_margin(seed, n, nlab, thr, offset, MARGIN, agnostic)
    assert R.iou_margin(b, None if agnostic else l, thr, offset) > MARGIN
    return b, s, l


def _counts():
    from boxinstseg_amd import box_nms
    r = box_nms.NMS_ROUND
    return [0, 1, 2, 63, 64, 65, 129, r, r + 1, 3 * r + 7]


def test_nms_counts_against_greedy(dev):
    """Every count at which the kernel takes another path, all in one call (one segment each): empty, one lane, chunk borders, one round,
    one round + 1, three rounds + 7."""
    segs = [tuple(a[:n] for a in _recipe(20 + i, max(n, 2), 3)) for i, n in enumerate(_counts())]
    got, status = _run(dev, segs)
    assert status == [0] * len(segs)
    for (b, s, l), g, n in zip(segs, got, _counts()):
        want = R.greedy_nms(b, s, l, 0.5)
        assert g == want, n
        assert n == 0 or 0 < len(g) <= n
    again, _ = _run(dev, segs)
    assert again == got                                               # run-to-run identical


def test_nms_mixed_segments_in_one_call(dev):
    segs = [tuple(a[:n] for a in _recipe(40, 200, 4)) for n in (0, 1, 200)]
    got, status = _run(dev, segs)
    assert status == [0, 0, 0] and got[0] == [] and got[1] == [0]
    assert got[2] == R.greedy_nms(*segs[2], 0.5) and len(got[2]) < 200


def test_nms_identical_disjoint_and_chain(dev):
    n = 150
    lab = (np.arange(n) % 3).astype(np.int64)
    sc = np.random.default_rng(0).permutation(np.linspace(0.1, 0.9, n)).astype(np.float32)
    same = np.tile(np.array([[10, 20, 50, 70]], np.float32), (n, 1))
    i = np.arange(n)
    disjoint = np.stack([(i % 16) * 20, (i // 16) * 20, (i % 16) * 20 + 10, (i // 16) * 20 + 10], 1).astype(np.float32)
    chain = (np.array([[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]], np.float32), np.array([0.9, 0.8, 0.7], np.float32), None)
    got, status = _run(dev, [(same, sc, lab), (disjoint, sc, lab), chain], thr=0.4)
    assert status == [0, 0, 0]
    order = R.sort_order(sc)
    assert got[0] == [int(next(j for j in order if lab[j] == c)) for c in sorted(range(3), key=lambda c: -sc[lab == c].max())]   # one per label
    assert got[1] == order.tolist()                                   # all kept, in score order
    assert got[2] == [0, 2]                                           # A suppresses B, B would suppress C, A does not: C is kept
    agn, _ = _run(dev, [(same, sc, lab)], thr=0.4, agnostic=True)
    assert agn[0] == [int(order[0])]


def test_nms_kept_list_past_a_chunk_and_past_the_lds_tile(dev):
    """2 * 64 + 9 kept of disjoint boxes with overlapping ones in between, and KEEP_TILE + 70 kept (the tail lives in the workspace) that
    later candidates are tested against."""
    from boxinstseg_amd import box_nms
    n = box_nms.KEEP_TILE + 70
    i = np.arange(n)
    grid = np.stack([(i % 64) * 10, (i // 64) * 10, (i % 64) * 10 + 8, (i // 64) * 10 + 8], 1).astype(np.float32)
    dup = grid[-200:] + np.float32(0.5)                              # IoU (7.5/8.5)^2-ish = 0.64 with its twin: suppressed by the LAST kept ones
    boxes = np.concatenate([grid, dup])
    scores = np.concatenate([np.linspace(0.95, 0.5, n), np.linspace(0.4, 0.1, 200)]).astype(np.float32)
    assert R.iou_margin(boxes[-400:], None, 0.5) > MARGIN
    got, status = _run(dev, [(boxes, scores, None), (grid[:137], scores[:137], None)], agnostic=True)
    assert status == [0, 0]
    assert got[0] == list(range(n)) and got[1] == list(range(137))
    lab = np.concatenate([np.zeros(n, np.int64), np.ones(200, np.int64)])   # another label: the twins survive
    got, _ = _run(dev, [(boxes, scores, lab)])
    assert got[0] == list(range(n + 200))


def test_nms_max_num_in_the_middle_of_a_chunk(dev):
    b, s, l = _recipe(50, 400, 2)
    full = R.greedy_nms(b, s, l, 0.5)
    assert len(full) > 70
    for max_num in (1, 5, 64, 70):
        got, status = _run(dev, [(b, s, l)], max_num=max_num)
        assert status == [0] and got[0] == full[:max_num] == R.greedy_nms(b, s, l, 0.5, max_num=max_num)


def test_nms_agnostic_offset_and_thresholds(dev):
    for seed, thr, offset, agnostic in ((60, 0.5, 0, True), (61, 0.6, 0, False), (62, 0.5, 1, False), (63, 0.3, 1, True)):
        b, s, l = _recipe(seed, 300, 3, thr, offset, agnostic)
        got, status = _run(dev, [(b, s, l)], thr=thr, offset=offset, agnostic=agnostic)
        assert status == [0] and got[0] == R.greedy_nms(b, s, None if agnostic else l, thr, offset), (thr, offset, agnostic)
    b, s, l = _recipe(64, 300, 3, agnostic=True)
    a, _ = _run(dev, [(b, s, l)], agnostic=True)
    z, _ = _run(dev, [(b, s, np.zeros_like(l))])                      # labels NULL == all labels equal
    assert a == z
    assert len(_run(dev, [(b, s, l)])[0][0]) > len(a[0])


def test_nms_ties_nan_and_zero_area(dev):
    from boxinstseg_amd import box_nms
    r = box_nms.NMS_ROUND
    b, s, l = _recipe(70, 2 * r + 40, 3)
    s = s.copy()
    first = R.sort_order(s)                                           # runs of equal scores at chosen positions of the sorted sequence:
    for lo, hi in ((63, 65), (r - 1, r + 2), (100, 170)):             # 2 across a chunk border, 3 across the round border, 70 across a chunk border
        s[first[lo:hi]] = s[first[lo]]
    order = R.sort_order(s)
    for lo, hi in ((63, 65), (r - 1, r + 2), (100, 170)):
        assert sorted(order[lo:hi].tolist()) == sorted(first[lo:hi].tolist()) == order[lo:hi].tolist() and len(set(s[order[lo:hi]])) == 1
        assert order[lo:hi].tolist() != first[lo:hi].tolist() or hi - lo == 2
    got, status = _run(dev, [(b, s, l)])
    assert status == [0] and got[0] == R.greedy_nms(b, s, l, 0.5)
    s2 = s.copy()
    s2[[5, 300]] = np.nan                                             # NaN scores come first, by index
    got, _ = _run(dev, [(b, s2, l)])
    want = R.greedy_nms(b, s2, l, 0.5)
    assert got[0] == want and want[0] == 5
    z = b.copy()
    z[::7, 2] = z[::7, 0]                                             # zero-area boxes: never suppress, never suppressed (inter 0 > thr * S is false)
    got, _ = _run(dev, [(z, s, l)])
    want = R.greedy_nms(z, s, l, 0.5)
    assert got[0] == want and set(range(0, len(s), 7)) <= set(want)


def test_nms_above_sort_max_and_over_cap(dev):
    from boxinstseg_amd import _lib, box_nms
    n = box_nms.SORT_MAX + 65
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 8 * 2000, (n, 2)) / 8
    wh = rng.integers(8 * 30, 8 * 120, (n, 2)) / 8
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    s = rng.permutation(np.linspace(0.05, 0.95, n)).astype(np.float32)
    l = rng.integers(0, 80, n)
    tb, ts, tl, tc = _segments(dev, [(b, s, l), (b[:50], s[:50], l[:50])])
    order = box_nms._stable_order(ts)
    assert order[0, :n].cpu().tolist() == R.sort_order(s).tolist()
    keep, n_keep, status = box_nms.box_nms(tb, ts, tl, tc, 0.5, 0, 100, order)
    assert status.cpu().tolist() == [0, 0]
    # max_num = 100 keeps the restatement affordable; the margin is asserted over the boxes the scan can compare
    want = R.greedy_nms(b, s, l, 0.5, max_num=100)
    assert keep[0, :int(n_keep[0])].cpu().tolist() == want and len(want) == 100
    full = R.sort_order(s)
    seen = full[:full.tolist().index(want[-1]) + 1]                  # everything the greedy scan looked at before it stopped
    assert R.iou_margin(b[seen], l[seen], 0.5) > MARGIN
    # the library's own sort refuses the long segment, loudly, and still does the short one
    keep, n_keep, status = box_nms.box_nms(tb, ts, tl, tc, 0.5, 0, 100, None)
    assert status.cpu().tolist() == [_lib.DET_STATUS_OVER_SORT, 0] and n_keep.cpu().tolist()[0] == -1
    assert bool((keep[0] == -1).all()) and keep[1, :int(n_keep[1])].cpu().tolist() == R.greedy_nms(b[:50], s[:50], l[:50], 0.5)
    # count > cap
    tc2 = torch.tensor([n + 1, 50], dtype=torch.int32, device=dev)
    keep, n_keep, status = box_nms.box_nms(tb, ts, tl, tc2, 0.5, 0, 100, order)
    assert status.cpu().tolist() == [_lib.DET_STATUS_OVER_CAP, 0] and n_keep.cpu().tolist()[0] == -1 and bool((keep[0] == -1).all())
    # a caller's order with an entry out of range: skipped and flagged
    bad = order.clone()
    bad[1, 3] = 50
    keep, n_keep, status = box_nms.box_nms(tb, ts, tl, tc, 0.5, 0, 100, bad)
    assert status.cpu().tolist() == [0, _lib.DET_STATUS_BAD_ORDER]


# ---- entries 1, 2 and 4 against the restatement ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    inp = {k: [g[f'in_{k}{lv}'] for lv in range(len(R.DET_SIZES))] for k in ('cls', 'bbox', 'ctr', 'params')}
    return g, inp


def _levels(dev, inp):
    from boxinstseg_amd import box_nms
    return box_nms._Levels(*[[_t(a, dev) for a in inp[k]] for k in ('cls', 'bbox', 'ctr', 'params')], R.DET_STRIDES)


def test_location_scores_candidates_and_gather(dev, golden):
    from boxinstseg_amd import box_nms
    g, inp = golden
    tol = float(g['lv3_tol'])
    lv = _levels(dev, inp)
    got = box_nms.location_scores(lv).cpu().numpy()
    want = R.location_scores(inp, np.float64)
    assert got.shape == want.shape and np.abs(got - want).max() <= 4 * tol
    for rescale in (False, True):
        for sel in (R.select(inp, 40, np.float64), None):
            want = R.candidates(inp, R.DET_STRIDES, R.det_img_dims(), rescale, 0.05, sel, np.float64)
            for cap in (48, 20):                                       # 20: fewer rows than candidates -- the count stays true
                cand = box_nms.det_candidates(lv, None if sel is None else _t(sel, dev), R.det_img_dims(), rescale, 0.05, cap)
                boxes, scores, labels, pos, count = (t.cpu().numpy() for t in cand)
                assert count.tolist() == [len(w['labels']) for w in want] and max(count) > 20
                for b, w in enumerate(want):
                    n = min(len(w['labels']), cap)
                    assert np.array_equal(boxes[b, :n].view(np.int32), w['boxes'][:n].view(np.int32))            # bit-equal
                    assert np.array_equal(labels[b, :n], w['labels'][:n]) and np.array_equal(pos[b, :n], w['pos'][:n])
                    assert np.abs(scores[b, :n] - w['scores'][:n]).max(initial=0) <= 4 * tol
            # gather: the first and the last candidates of every image, in a made-up keep list
            cand = box_nms.det_candidates(lv, None if sel is None else _t(sel, dev), R.det_img_dims(), rescale, 0.05, 48)
            keep = np.full((R.DET_B, 6), -1, np.int32)
            n_keep = []
            for b, w in enumerate(want):
                n = len(w['labels'])
                ks = [n - 1, 0, n // 2][:min(n, 3)]
                keep[b, :len(ks)] = ks
                n_keep.append(len(ks))
            out = box_nms.det_gather(lv, None if sel is None else _t(sel, dev), cand, _t(keep, dev), torch.tensor(n_keep, dtype=torch.int32, device=dev))
            dets, dl, dp, dc, dli = (t.cpu().numpy() for t in out)
            pts, lvl = R.points_of(R.DET_SIZES, R.DET_STRIDES)
            params = R.flatten_levels(inp['params'])
            for b, w in enumerate(want):
                k = keep[b, :n_keep[b]]
                loc = (np.arange(len(pts)) if sel is None else sel[b])[w['pos'][k]]
                assert np.array_equal(dets[b, :len(k), :4], w['boxes'][k]) and np.array_equal(dl[b, :len(k)], w['labels'][k])
                assert np.array_equal(dp[b, :len(k)], params[b, loc]) and np.array_equal(dc[b, :len(k)], pts[loc]) and np.array_equal(dli[b, :len(k)], lvl[loc])
                for a in (dets, dl, dp, dc, dli):
                    assert (a[b, len(k):] == 0).all()


def _metas():
    return [dict(img_shape=s, scale_factor=np.array(f, np.float32)) for s, f in zip(R.DET_IMG_SHAPES, R.DET_SCALES)]


def _cfg(name):
    rescale, c = R.DET_CASES[name]
    nms = dict(type='nms', iou_threshold=c['iou_threshold'])
    if c['class_agnostic']:
        nms['class_agnostic'] = True
    return rescale, dict(nms_pre=c['nms_pre'], min_bbox_size=0, score_thr=c['score_thr'], nms=nms, max_per_img=c['max_per_img'])


@pytest.mark.parametrize('max_candidates', [None, 64, 20])
@pytest.mark.parametrize('name', sorted(R.DET_CASES))
def test_condinst_get_bboxes_is_the_reference(dev, golden, name, max_candidates):
    """The four fixture cases: the same detections in the same order as the reference executed.  The images hold 32 and 33 candidates:
    max_candidates = 64 holds them all, 20 forces the overflow path (cap too small -> redo with the caller's order)."""
    import boxinstseg_amd as B
    g, inp = golden
    tol = float(g[f'{name}_tol'])
    rescale, cfg = _cfg(name)
    t = {k: [_t(a, dev) for a in inp[k]] for k in inp}
    kw = {} if max_candidates is None else dict(max_candidates=max_candidates)
    res = B.condinst_get_bboxes(t['cls'], t['bbox'], t['ctr'], t['params'], _metas(), cfg, R.DET_STRIDES, rescale=rescale, **kw)
    assert len(res) == R.DET_B
    for b, (dets, labels, params, coors, lvl) in enumerate(res):
        k = f'{name}{b}'
        n = len(g[f'{k}_labels'])
        assert tuple(dets.shape) == (n, 5) and tuple(labels.shape) == (n,) and tuple(params.shape) == (n, R.DET_P)
        assert tuple(coors.shape) == (n, 2) and tuple(lvl.shape) == (n,)
        assert dets.dtype == params.dtype == coors.dtype == torch.float32 and labels.dtype == lvl.dtype == torch.int64
        assert all(x.device == dev for x in (dets, labels, params, coors, lvl))
        d = dets.cpu().numpy()
        assert np.array_equal(d[:, :4].view(np.int32), g[f'{k}_dets32'][:, :4].view(np.int32))                  # bit-equal boxes
        assert np.abs(d[:, 4] - g[f'{k}_scores64']).max(initial=0) <= 4 * tol
        assert np.array_equal(labels.cpu().numpy(), g[f'{k}_labels']) and np.array_equal(params.cpu().numpy(), g[f'{k}_params'])
        assert np.array_equal(coors.cpu().numpy(), g[f'{k}_coors']) and np.array_equal(lvl.cpu().numpy(), g[f'{k}_level_inds'])
    assert res[R.DET_EMPTY_IMAGE][0].shape[0] == 0


def test_mmcv_names_against_the_restatement(dev):
    import boxinstseg_amd as B
    b, s, l = _recipe(80, 300, 4)
    tb, ts, tl = _t(b, dev), _t(s, dev), _t(l, dev)
    b2, s2, l2 = _recipe(81, 300, 4, agnostic=True)
    dets, inds = B.nms(_t(b2, dev), _t(s2, dev), 0.5)
    want = R.greedy_nms(b2, s2, None, 0.5)
    assert inds.dtype == torch.int64 and inds.cpu().tolist() == want
    assert torch.equal(dets.cpu(), torch.from_numpy(np.concatenate([b2[want], s2[want, None]], 1)))
    thr_keep = np.flatnonzero(s2 > 0.5)
    dets, inds = B.nms(_t(b2, dev), _t(s2, dev), 0.5, score_threshold=0.5, max_num=9)
    assert inds.cpu().tolist() == thr_keep[R.greedy_nms(b2[thr_keep], s2[thr_keep], None, 0.5, max_num=9)].tolist() and dets.shape == (len(inds), 5)
    b3, s3, _ = _recipe(82, 300, 4, offset=1, agnostic=True)
    dets, inds = B.nms(_t(b3, dev), _t(s3, dev), 0.5, offset=1)
    assert inds.cpu().tolist() == R.greedy_nms(b3, s3, None, 0.5, 1)
    cfg = dict(type='nms', iou_threshold=0.5, split_thr=10000)
    want_d, want_k = R.batched_nms_mmcv_style(b, s, l, cfg)           # mmcv's offset trick: exact on the 1/8-pixel grid
    dets, keep = B.batched_nms(tb, ts, tl, cfg)
    assert keep.cpu().tolist() == want_k.tolist() == R.greedy_nms(b, s, l, 0.5) and np.array_equal(dets.cpu().numpy(), want_d)
    dets, keep = B.batched_nms(_t(b2, dev), _t(s2, dev), _t(l2, dev), dict(cfg, class_agnostic=True, max_num=5))
    assert keep.cpu().tolist() == R.greedy_nms(b2, s2, None, 0.5, max_num=5)
    with pytest.raises(NotImplementedError):
        B.batched_nms(tb, ts, tl, dict(type='soft_nms', iou_threshold=0.5))
    with pytest.raises(TypeError):
        B.batched_nms(tb, ts, tl, dict(cfg, offset=1))
    empty = B.nms(tb[:0], ts[:0], 0.5)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0,)
    # nms_with_others: [n, C + 1] scores with the background column, score factors and two others
    rng = np.random.default_rng(5)
    n, C = 120, 4
    ms = np.where(rng.uniform(size=(n, C)) < 0.3, rng.permutation(np.linspace(0.2, 0.9, n * C)).reshape(n, C), 0.01).astype(np.float32)
    fac = rng.uniform(0.5, 0.95, n).astype(np.float32)
    mb = R.clustered_boxes_with_margin(90, n, 1, 0.5, agnostic=True)[0]
    others = [rng.normal(size=(n, 3)).astype(np.float32), np.arange(n)]
    m, c = np.nonzero(ms > 0.05)
    cs = (ms[m, c] * fac[m]).astype(np.float32)
    assert np.diff(np.sort(cs)).min() > 0
    want = np.array(R.greedy_nms(mb[m], cs, c, 0.5, max_num=15))
    dets, labels, oth = B.nms_with_others(_t(mb, dev), _t(np.concatenate([ms, np.zeros((n, 1), np.float32)], 1), dev), 0.05,
                                          dict(type='nms', iou_threshold=0.5), 15, _t(fac, dev), [_t(o, dev) for o in others])
    assert labels.device == dev and labels.cpu().tolist() == c[want].tolist() and np.array_equal(dets.cpu().numpy()[:, :4], mb[m][want])
    assert np.array_equal(dets.cpu().numpy()[:, 4], cs[want])
    assert np.array_equal(oth[0].cpu().numpy(), others[0][m[want]]) and oth[1].cpu().tolist() == m[want].tolist()
    dets, labels, oth = B.nms_with_others(_t(mb, dev), _t(np.full((n, C + 1), 0.01, np.float32), dev), 0.05, dict(type='nms', iou_threshold=0.5),
                                          15, _t(fac, dev), [_t(o, dev) for o in others])
    assert dets.shape == (0, 5) and labels.shape == (0,) and oth[0].shape == (0, 3) and oth[1].shape == (0,)


def test_outputs_feed_simple_test(dev, golden):
    """Shape / dtype / device: what condinst_get_bboxes returns is what CondInstMaskHead.simple_test takes (the masks themselves are
    test_gpu_mask_paste.py's business)."""
    import boxinstseg_amd as B
    g, inp = golden
    rescale, cfg = _cfg('lv3')
    t = {k: [_t(a, dev) for a in inp[k]] for k in inp}
    torch.manual_seed(0)
    num_classes = R.DET_C
    head = B.CondInstMaskHead(in_channels=8, in_stride=8, out_stride=4).to(dev)
    mask_feat = torch.randn(R.DET_B, 8, *R.DET_SIZES[0], device=dev)
    metas = [dict(m, ori_shape=m['img_shape']) for m in _metas()]
    pp = [torch.randn(R.DET_B, head.num_gen_params, h, w, device=dev) * 0.3 for h, w in R.DET_SIZES]
    res = B.condinst_get_bboxes(t['cls'], t['bbox'], t['ctr'], pp, metas, cfg, R.DET_STRIDES)
    det_bboxes, det_labels, det_params, det_coors, det_level_inds = zip(*res)
    assert all(p.shape[1] == head.num_gen_params for p in det_params)
    out = head.simple_test(mask_feat, det_labels, det_params, det_coors, det_level_inds, metas, num_classes)
    assert len(out) == R.DET_B
    for b in range(R.DET_B):
        assert len(out[b]) == num_classes
        assert sum(len(c) for c in out[b]) == len(g[f'lv3{b}_labels'])
        for c in range(num_classes):
            assert len(out[b][c]) == int((g[f'lv3{b}_labels'] == c).sum())
            assert all(tuple(m.shape[-2:]) == tuple(R.DET_IMG_SHAPES[b][:2]) for m in out[b][c])


def test_graph_capture_and_replay(dev, golden):
    """Entries 1-4 captured into one graph; replayed on changed inputs it gives the changed answer."""
    from boxinstseg_amd import box_nms
    g, inp = golden
    t = {k: [_t(a, dev).clone() for a in inp[k]] for k in inp}
    lv = box_nms._Levels(t['cls'], t['bbox'], t['ctr'], t['params'], R.DET_STRIDES)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(lv.cls, t['cls']))          # the graph reads the tensors we will change
    sel = _t(R.select(inp, 40, np.float64), dev)
    cfg = dict(score_thr=0.05, iou_threshold=0.5, class_agnostic=False)

    def run():
        loc = box_nms.location_scores(lv)
        cand, keep, n_keep, status, out = box_nms._det_pipeline(lv, sel, R.det_img_dims(), False, cfg, 48, 100, True)
        return loc, cand[4], keep, n_keep, status, out

    eager = [x.clone() if torch.is_tensor(x) else [y.clone() for y in x] for x in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[3], eager[3]) and torch.equal(captured[2], eager[2]) and torch.equal(captured[0], eager[0])
    for a, b in zip(captured[5], eager[5]):
        assert torch.equal(a, b)
    # image 0 loses its best candidate, image 1 (empty so far) gets one
    n0 = int(eager[3][0])
    best = eager[5][0][0, 0]
    for level in t['cls']:
        level[0].clamp_(max=-4.0)                                       # sigmoid(-4) = 0.018 < score_thr: image 0 has no candidate left
    t['cls'][2][1, 3, 1, 2] = 3.0
    t['ctr'][2][1, 0, 1, 2] = 2.0
    graph.replay()
    torch.cuda.synchronize()
    assert n0 > 0 and captured[3].cpu().tolist()[:2] == [0, 1] and captured[1].cpu().tolist()[:2] == [0, 1]
    d = captured[5][0][1, 0].cpu().numpy()
    want = 1 / (1 + np.exp(-3.0)) * 1 / (1 + np.exp(-2.0))
    assert abs(d[4] - want) < 1e-6 and int(captured[5][1][1, 0]) == 3 and int(captured[5][4][1, 0]) == 2
    assert captured[5][3][1, 0].cpu().tolist() == [2.5 * 32, 1.5 * 32] and not torch.equal(captured[5][0][0, 0], best)
    assert bool((captured[5][0][0] == 0).all())
