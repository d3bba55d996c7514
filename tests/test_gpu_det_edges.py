"""GPU: CondInst's test-time candidates (csrc/box_nms.hip) at the configs' level sizes: 20267 locations on five levels, 317 row tiles --
the sum over the earlier tiles' counts takes a second trip, candidates sit on both sides of the row tiles' edges, in tile 256, 257 and
in the last, 43-row tile.  The inputs are tests/box_nms_ref.py's edge recipe; tests/test_host_det.py shows what they reach and asserts
the margins (score threshold, distinct scores, IoU) that make exact comparisons meaningful.

Scores must be within 4 * lv3_tol of the float64 restatement: the fixture's own float32-against-float64 figure for the same two sigmoids
and product in the same score range."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import box_nms_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'det_nms.npz')
CFG = dict(nms_pre=1000, score_thr=0.05, iou_threshold=0.5, max_per_img=100, class_agnostic=False)
MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def _case():
    seed, inp = R.edge_inputs_with_margin(1, CFG, MARGIN)
    return inp, float(np.load(GOLDEN)['lv3_tol'])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _levels(dev, inp):
    from boxinstseg_amd import box_nms
    return box_nms._Levels(*[[_t(a, dev) for a in inp[k]] for k in ('cls', 'bbox', 'ctr', 'params')], R.EDGE_STRIDES)


def test_location_scores_on_five_levels(dev):
    from boxinstseg_amd import box_nms
    inp, tol = _case()
    got = box_nms.location_scores(_levels(dev, inp)).cpu().numpy()
    want = R.location_scores(inp, np.float64)
    err = np.abs(got - want).max()
    print(f'location scores {got.shape}: max error {err:.3e}, allowed {4 * tol:.3e}')
    assert got.shape == want.shape == (R.EDGE_B, 20267) and err <= 4 * tol


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('rows', ['every_location', 'top_1000_per_level'])
def test_candidates_and_gather_over_317_tiles(dev, rows, rescale):
    from boxinstseg_amd import box_nms
    inp, tol = _case()
    lv = _levels(dev, inp)
    sel = None if rows == 'every_location' else R.select(inp, CFG['nms_pre'], np.float64)
    assert sel is None or sel.shape == (R.EDGE_B, 3267)
    sel_dev = None if sel is None else _t(sel, dev)
    want = R.candidates(inp, R.EDGE_STRIDES, R.edge_img_dims(), rescale, CFG['score_thr'], sel, np.float64)
    counts = [len(w['labels']) for w in want]
    assert min(R.EDGE_CAPS) < counts[0] <= max(R.EDGE_CAPS) and counts[1] == 0
    for cap in R.EDGE_CAPS:
        cand = box_nms.det_candidates(lv, sel_dev, R.edge_img_dims(), rescale, CFG['score_thr'], cap)
        boxes, scores, labels, pos, count = (t.cpu().numpy() for t in cand)
        assert count.tolist() == counts
        for b, w in enumerate(want):
            n = min(len(w['labels']), cap)
            assert np.array_equal(boxes[b, :n].view(np.int32), w['boxes'][:n].view(np.int32))                    # bit-equal
            assert np.array_equal(labels[b, :n], w['labels'][:n]) and np.array_equal(pos[b, :n], w['pos'][:n])
            err = np.abs(scores[b, :n] - w['scores'][:n]).max(initial=0)
            print(f'{rows}, rescale {rescale}, cap {cap}, image {b}: {n} of {len(w["labels"])} candidates, score error {err:.3e} (allowed {4 * tol:.3e})')
            assert err <= 4 * tol
    # gather: the last, the first and a middle candidate of image 0 in a made-up keep list; image 1 keeps nothing
    cand = box_nms.det_candidates(lv, sel_dev, R.edge_img_dims(), rescale, CFG['score_thr'], max(R.EDGE_CAPS))
    keep = np.full((R.EDGE_B, 6), -1, np.int32)
    ks = [counts[0] - 1, 0, counts[0] // 2]
    keep[0, :3] = ks
    n_keep = [3, 0]
    out = box_nms.det_gather(lv, sel_dev, cand, _t(keep, dev), torch.tensor(n_keep, dtype=torch.int32, device=dev))
    dets, dl, dp, dc, dli = (t.cpu().numpy() for t in out)
    pts, lvl = R.points_of(R.EDGE_SIZES, R.EDGE_STRIDES)
    params = R.flatten_levels(inp['params'])
    w = want[0]
    loc = (np.arange(len(pts)) if sel is None else sel[0])[w['pos'][ks]]
    assert loc[0] == 20266 and (sel is not None or loc[1] == 0)         # the last row of the last tile (and the first of the first)
    assert np.array_equal(dets[0, :3, :4], w['boxes'][ks]) and np.array_equal(dl[0, :3], w['labels'][ks])
    assert np.array_equal(dets[0, :3, 4], cand[1][0].cpu().numpy()[ks])
    assert np.array_equal(dp[0, :3], params[0, loc]) and np.array_equal(dc[0, :3], pts[loc]) and np.array_equal(dli[0, :3], lvl[loc])
    for a in (dets, dl, dp, dc, dli):
        assert (a[0, 3:] == 0).all() and (a[1] == 0).all()


@pytest.mark.parametrize('nms_pre', [1000, -1])
def test_get_bboxes_end_to_end_at_the_configs_sizes(dev, nms_pre):
    """The same detections in the same order as the restatement, with the per-level top 1000 and with every location (nms_pre <= 0)."""
    import boxinstseg_amd as B
    inp, tol = _case()
    c = R.candidates(inp, R.EDGE_STRIDES, R.edge_img_dims(), False, CFG['score_thr'], None, np.float64)[0]
    assert R.iou_margin(c['boxes'], c['labels'], CFG['iou_threshold']) > MARGIN
    cfg = dict(nms_pre=nms_pre, min_bbox_size=0, score_thr=CFG['score_thr'], nms=dict(type='nms', iou_threshold=CFG['iou_threshold']),
               max_per_img=CFG['max_per_img'])
    metas = [dict(img_shape=s, scale_factor=np.array(f, np.float32)) for s, f in zip(R.EDGE_IMG_SHAPES, R.EDGE_SCALES)]
    t = {k: [_t(a, dev) for a in inp[k]] for k in inp}
    res = B.condinst_get_bboxes(t['cls'], t['bbox'], t['ctr'], t['params'], metas, cfg, R.EDGE_STRIDES, rescale=False)
    want = R.get_bboxes(inp, R.EDGE_STRIDES, R.edge_img_dims(), dict(CFG, nms_pre=nms_pre), False, np.float64)
    assert len(res) == R.EDGE_B and len(want[0]['labels']) > 0
    for b, (dets, labels, params, coors, lvl) in enumerate(res):
        w = want[b]
        d = dets.cpu().numpy()
        assert d.shape == (len(w['labels']), 5)
        assert np.array_equal(d[:, :4].view(np.int32), w['dets'][:, :4].astype(np.float32).view(np.int32))
        assert np.abs(d[:, 4] - w['dets'][:, 4]).max(initial=0) <= 4 * tol
        assert np.array_equal(labels.cpu().numpy(), w['labels']) and np.array_equal(params.cpu().numpy(), w['params'])
        assert np.array_equal(coors.cpu().numpy(), w['coors']) and np.array_equal(lvl.cpu().numpy(), w['level_inds'])
    assert res[1][0].shape[0] == 0
