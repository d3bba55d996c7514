"""Float64 restatement of Box2Mask's test-time path (a plain module: numpy and CPU torch only), shared by tests/test_host_inst_post.py,
tests/test_gpu_inst_post.py, tests/test_gpu_guarded_inst.py, the fixture generator and tools/inst_post_bench.py.

    softmax64(mask_cls)                  F.softmax(mask_cls, -1)[..., :-1] in float64 (maskformer_fusion_head.py:136)
    softmax_error_bound(mask_cls)        the derived bound of the kernel's fp32 scores against softmax64 (rows of any length)
    topk_ref(mask_cls, things, k)        :133-151 with the library's DEFINED order: descending score, equal scores by ascending flat index
                                         q * C + c, NaN last; then the is_thing filter -> (scores, labels, query, flat) of the kept rows
    p64(logits, query, up, crop, out)    box2mask_head.py:452-457 and maskformer_fusion_head.py:211-221 in float64: the two-stage composition
                                         of tests/seg_paste_ref.py ON THE FP32 SAMPLING GRID (grid64: the taps and weights are the ones ATen's
                                         fp32 kernel places, src = max(scale (dst + 0.5) - 0.5, 0) with scale = fp32(in) / fp32(out), as the
                                         header specifies them; only the products and sums are float64); a query outside [0, n_all) is an
                                         all-zero plane.  p64_torch is the same through F.interpolate on float64 tensors, whose taps are
                                         placed in float64: at a coordinate of a few hundred that is up to ~1e-5 pixel away, which is the
                                         grid and not the arithmetic -- against it the band is widened, pixel by pixel, by |p64 - p64_torch|
    instance_ref(p, cls_scores)          :153-160 on float64 p [n,H,W]: masks, stats (area, x_min, y_min, x_max, y_max / -1), mask scores,
                                         boxes [n,5] float64 (x_min, y_min, x_max + 1, y_max + 1, cls x mask score; zeros when empty)
    tie_band(logits, query) / check_masks  a mask byte may differ from ``p64 > 0`` only where |p64| <= 2^-20 * max|logit| of its source plane
                                         (p is a convex combination: every rounding of either grouping is at most half an ulp of that
                                         maximum, about ten roundings per pixel on each side, hence 16 ulp); at most 0.1 % of a case's
                                         pixels may lie inside the band
    format_ref(labels, bboxes, masks, things)   maskformer.py:160-169 restated: bbox2result and the per-mask numpy arrays
"""
import json
import os

import numpy as np

from tests import seg_paste_ref as S

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'box2mask_test.npz')
CFG_JSON = os.path.join(os.path.dirname(__file__), 'golden', 'box2mask_test_cfg.json')
BAND = 2.0 ** -20
BAND_SHARE = 1e-3

# the fixture's cases: Q queries, C = things + stuff classes, prediction hw, batch_input_shape up, img_shape crop, ori_shape, rescale
CASES = {
    'rescale': dict(Q=12, things=5, stuff=0, k=9, hw=(13, 21), up=(52, 84), crop=(50, 81), ori=(37, 61), rescale=True),
    'no_rescale': dict(Q=12, things=5, stuff=0, k=9, hw=(13, 21), up=(52, 84), crop=(50, 81), ori=(37, 61), rescale=False),
    'stuff': dict(Q=12, things=3, stuff=2, k=14, hw=(13, 21), up=(52, 84), crop=(52, 84), ori=(64, 100), rescale=True),
    'zero_plane': dict(Q=7, things=3, stuff=0, k=21, hw=(9, 11), up=(36, 44), crop=(33, 41), ori=(33, 41), rescale=True),
}


def case_inputs(name):
    """Seeded inputs of a fixture case: class logits [Q,C+1] with distinct scores, mask logits [Q,h,w] (smooth blobs, a few units high;
    plane 2 of 'zero_plane' is all zero and its query is made to win)."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    Q, C, (h, w) = c['Q'], c['things'] + c['stuff'], c['hw']
    cls = rng.normal(0, 2.0, (Q, C + 1)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.2 * h, 0.8 * h, Q), rng.uniform(0.2 * w, 0.8 * w, Q)
    r = rng.uniform(0.2, 0.45, Q) * min(h, w)
    d = np.sqrt((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2)
    pred = (3.0 * (r[:, None, None] - d) + rng.normal(0, 0.3, (Q, h, w))).astype(np.float32)
    if name == 'zero_plane':
        pred[2] = 0
        cls[2, 1] = 9.0
    return cls, pred


def softmax64(mask_cls):
    x = np.asarray(mask_cls, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(x - np.max(np.where(np.isnan(x), -np.inf, x), -1, keepdims=True))
        return (e / e.sum(-1, keepdims=True))[..., :-1]


def softmax_error_bound(mask_cls):
    """An upper bound of |inst_topk_kernel's fp32 score - softmax64|, element by element, from the kernel's stated arithmetic and
    nothing measured.  With e = 2^-24, d_c = max - x_c >= 0 and p the float64 softmax over all C + 1 columns:
      * the argument x_c - max is one fp32 subtraction, off by at most e d_c, which is a RELATIVE error e d_c of its exponential;
        expf is within one ulp, at most 2 e relative: a term is off by at most (d_c + 2) e;
      * the denominator inherits the terms' errors weighted by their shares, A = sum_c p_c (d_c + 2), and adds its own roundings:
        a lane adds its T = ceil((C + 1) / 64) terms one after the other (T - 1 roundings, the first addition is to zero), the wave total
        is six tree levels, every rounding at most e of a partial sum of positive terms, hence of the total: (T - 1 + 6) e;
      * one correctly rounded division: e.
    Relative error of score c at first order: e ((d_c + 2) + A + (T + 5) + 1); the second-order terms are below 2^-38 relative and are
    covered by counting expf at its worst-case ulp.  Returns the absolute bound without the background column, like softmax64."""
    x = np.asarray(mask_cls, np.float64)
    d = x.max(-1, keepdims=True) - x
    e = np.exp(-d)
    p = e / e.sum(-1, keepdims=True)
    terms = -(-x.shape[-1] // 64)
    rel = 2.0 ** -24 * ((d + 2) + (p * (d + 2)).sum(-1, keepdims=True) + (terms + 5) + 1)
    return (rel * p)[..., :-1]


def defined_order(scores_flat):
    """Indices of a flat score array in the library's order: descending score, ascending index among equals, NaN last."""
    s = np.asarray(scores_flat, np.float64)
    key = np.where(np.isnan(s), -np.inf, s)
    order = np.lexsort((np.arange(len(s)), -key))
    nan = np.isnan(s[order])
    return np.concatenate([order[~nan], order[nan]])


def topk_ref(mask_cls, things, k, scores=None):
    s = softmax64(mask_cls) if scores is None else np.asarray(scores)
    C = s.shape[-1]
    flat = defined_order(s.reshape(-1))[:k]
    labels, query = flat % C, flat // C
    keep = labels < things
    return s.reshape(-1)[flat][keep], labels[keep], query[keep], flat[keep]


def p64(logits, query, up, crop, out):
    return S.grid64(logits, query, up, crop, out)


def p64_torch(logits, query, up, crop, out):
    return S.p64(logits, query, up, crop, out)


def instance_ref(p, cls_scores):
    p = np.asarray(p, np.float64)
    with np.errstate(invalid='ignore'):
        m = p > 0
    n = len(p)
    stats = S.stats_of(m)
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-np.where(m, p, 0.0)))
    sums = (sig * m).reshape(n, -1).sum(1)
    mask_scores = sums / (stats[:, 0].astype(np.float64) + 1e-6)
    boxes = np.zeros((n, 5))
    full = stats[:, 0] > 0
    boxes[full, :4] = stats[full][:, [1, 2, 3, 4]] + np.array([0, 0, 1, 1])
    boxes[:, 4] = np.asarray(cls_scores, np.float64) * mask_scores
    return m.astype(np.uint8), stats, mask_scores, boxes


def tie_band(logits, query):
    """[n] float64: 2^-20 x the largest |logit| of every row's source plane (0 for a query outside the planes)."""
    logits, query = np.asarray(logits), np.asarray(query, np.int64)
    big = np.abs(logits.reshape(len(logits), -1).astype(np.float64)).max(1) if logits.size else np.zeros(len(logits))
    ok = (query >= 0) & (query < len(logits))
    out = np.zeros(len(query))
    out[ok] = BAND * big[query[ok]]
    return out


def band_share(p, logits, query):
    """The share of pixels with |p64| <= the band, over the rows whose plane is not constant zero (those are 'in the band' by design)."""
    tau = tie_band(logits, query)
    rows = tau > 0
    if not rows.any():
        return 0.0
    with np.errstate(invalid='ignore'):
        return float((np.abs(p[rows]) <= tau[rows, None, None]).mean())


def check_masks(got, p, logits, query, what='', widen=0.0):
    """The rule for mask bits (`widen`: added to the band, pixel by pixel); returns the mask of pixels outside the band."""
    got = np.asarray(got)
    assert got.shape == p.shape and got.dtype == np.uint8 and set(np.unique(got).tolist()) <= {0, 1}, (what, got.shape, p.shape, got.dtype)
    tau = tie_band(logits, query)[:, None, None] + widen
    with np.errstate(invalid='ignore'):
        outside = ~(np.abs(p) <= tau)
        bad = (got != (p > 0)) & outside
    assert not bad.any(), f'{what}: {int(bad.sum())} pixels off outside the band, e.g. p = {p[bad][:4]}'
    assert band_share(p, logits, query) <= BAND_SHARE, f'{what}: {band_share(p, logits, query):.5f} of the pixels lie inside the band'
    return outside


def format_ref(labels, bboxes, masks, things):
    """maskformer.py:160-169: bbox2result (float32 rows per class, np.zeros((0, 5), float32) lists when there is no detection at all) and
    the masks as numpy bool arrays per class, in result order."""
    labels, bboxes, masks = np.asarray(labels), np.asarray(bboxes, np.float32), np.asarray(masks).astype(bool)
    if len(bboxes) == 0:
        boxes = [np.zeros((0, 5), np.float32) for _ in range(things)]
    else:
        boxes = [bboxes[labels == c, :] for c in range(things)]
    per_class = [[] for _ in range(things)]
    for j, label in enumerate(labels):
        per_class[int(label)].append(masks[j])
    return boxes, per_class


def load_cfg():
    with open(CFG_JSON) as fh:
        return json.load(fh)
