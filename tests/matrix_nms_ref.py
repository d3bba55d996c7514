"""Float64 restatement of Matrix NMS and of the mask-scoring block in front of it (a plain module, numpy only), plus the
synthetic candidates the tests and the fixture generator share.

The IoU is the one quantity NOT taken to float64: it is computed from integer counts as the library specifies it --
``fp32(inter) / ((fp32(area_j) + fp32(area_i)) - fp32(inter))`` with fp32 operations -- which is what the reference's fp32 matrix
product and division give bit for bit (the counts are exact below 2^24).  Everything after it (squares, exp, ratios, the minimum
over ALL rows as the reference takes it, the score product) is float64.  Both sorts are stable and descending: among equal scores
the lower index goes first.
"""
import numpy as np

f32 = np.float32


def disc_masks(rng, n, h, w, centres=4):
    """n boolean masks [n,h,w]: discs of varying radius whose centres scatter closely around a few shared points."""
    yy, xx = np.mgrid[0:h, 0:w]
    cs = np.stack([rng.uniform(0.2 * h, 0.8 * h, centres), rng.uniform(0.2 * w, 0.8 * w, centres)], 1)
    which = rng.integers(0, centres, n)
    cy = cs[which, 0] + rng.normal(0, 0.06 * h, n)
    cx = cs[which, 1] + rng.normal(0, 0.06 * w, n)
    r = rng.uniform(0.15, 0.4, n) * min(h, w)
    m = (yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2 <= (r ** 2)[:, None, None]
    m[np.arange(n), np.clip(cy.round().astype(int), 0, h - 1), np.clip(cx.round().astype(int), 0, w - 1)] = True     # never empty
    return m


def disc_probs(rng, n, h, w, centres=4, avoid=(0.5,)):
    """fp32 probabilities [n,h,w] whose ``> thr`` masks are such discs; no value within 1e-3 of a threshold in `avoid`."""
    m = disc_masks(rng, n, h, w, centres)
    p = np.where(m, rng.uniform(0.75, 0.99, m.shape), rng.uniform(0.01, 0.4, m.shape)).astype(f32)
    for t in avoid:
        assert np.abs(p - t).min() > 1e-3
    return p


def shuffled_scores(rng, n, lo=0.1, hi=0.95):
    return rng.permutation(np.linspace(lo, hi, n)).astype(f32)


def decay_iou_f32(flat, area, labels):
    """[n,P] bool (sorted), [n] counts, [n] labels -> the reference's ``iou_matrix * label_matrix`` in fp32 from integer counts."""
    n = len(flat)
    x = flat.astype(np.float64)                  # 0 / 1: the products and their sums (below 2^24) are exact integers, and this is a BLAS call
    inter = (x @ x.T).astype(f32)
    a = np.asarray(area).astype(f32)
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = inter / ((a[None, :] + a[:, None]) - inter)
    assert iou.dtype == f32
    upper = np.triu(np.ones((n, n), bool), 1) & (np.asarray(labels)[None, :] == np.asarray(labels)[:, None])
    return np.where(upper, iou, f32(0))


def _sort_desc(x):
    """Stable descending order as torch.sort(descending=True, stable=True) gives it: NaN first."""
    key = np.where(np.isnan(x), np.inf, x)
    return np.argsort(-key, kind='stable')


def matrix_nms_ref(masks, labels, scores, filter_thr=-1, nms_pre=-1, max_num=-1, kernel='gaussian', sigma=2.0, mask_area=None):
    """-> dict: scores (float64), labels, keep_inds of the result; order, decay_iou (fp32), compensate, decayed (float64, in
    sorted order) of the n x n stage."""
    masks, labels = np.asarray(masks).astype(bool), np.asarray(labels)
    n_all = len(masks)
    flat = masks.reshape(n_all, -1)
    area = flat.sum(1) if mask_area is None else np.asarray(mask_area)
    s = np.asarray(scores).astype(np.float64)
    order = _sort_desc(s)
    if nms_pre > 0 and len(order) > nms_pre:
        order = order[:nms_pre]
    d32 = decay_iou_f32(flat[order], area[order], labels[order])
    d = d32.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = d.max(0) if len(order) else d.sum(0)
        c = np.where(np.isnan(d).any(0), np.nan, c)
        if kernel == 'gaussian':
            ratio = np.exp(-sigma * d ** 2) / np.exp(-sigma * c ** 2)[:, None]
        elif kernel == 'linear':
            ratio = (1 - d) / (1 - c)[:, None]
        else:
            raise NotImplementedError(kernel)
        coef = np.where(np.isnan(ratio).any(0), np.nan, np.nanmin(np.where(np.isnan(ratio), np.inf, ratio), 0))
    decayed = s[order] * coef
    out = dict(order=order, decay_iou=d32, compensate=c, decayed=decayed)
    keep_inds, sc = order, decayed
    if filter_thr > 0:
        keep = sc >= filter_thr
        keep_inds, sc = keep_inds[keep], sc[keep]
    o2 = _sort_desc(sc)
    keep_inds, sc = keep_inds[o2], sc[o2]
    if max_num > 0 and len(keep_inds) > max_num:
        keep_inds, sc = keep_inds[:max_num], sc[:max_num]
    out.update(scores=sc, keep_inds=keep_inds, labels=labels[keep_inds])
    return out


def seg_nms_ref(probs, cate_labels, cate_scores, strides, mask_thr, filter_thr, nms_pre, max_num, kernel, sigma):
    """box_solov2_head.py:546-574 in float64 on fp32 probabilities; the threshold test is the fp32 one.  keep_inds index the inputs."""
    probs = np.asarray(probs, f32)
    m = probs > f32(mask_thr)
    area = m.reshape(len(m), -1).sum(1)
    kept = np.nonzero(area.astype(np.float64) > np.asarray(strides, np.float64))[0]
    if len(kept) == 0:
        return dict(scores=np.zeros(0), keep_inds=np.zeros(0, np.int64), labels=np.zeros(0, np.int64), maskness=np.zeros(0), area=area, kept=kept)
    maskness = (probs.astype(np.float64) * m).reshape(len(m), -1).sum(1)[kept] / area[kept]
    s = np.asarray(cate_scores, np.float64)[kept] * maskness
    r = matrix_nms_ref(m[kept], np.asarray(cate_labels)[kept], s, filter_thr, nms_pre, max_num, kernel, sigma, mask_area=area[kept])
    r.update(keep_inds=kept[r['keep_inds']], maskness=maskness, area=area, kept=kept, scores_in=s)
    return r


def min_rel_gap(values, also=()):
    """Smallest relative distance between any two of `values`, and between any of them and any of `also`."""
    v = np.sort(np.asarray(values, np.float64))
    v = v[~np.isnan(v)]
    gaps = [np.inf]
    if len(v) > 1:
        gaps.append(float(np.min(np.diff(v) / np.maximum(np.abs(v[1:]), 1e-300))))
    for t in also:
        if t > 0 and len(v):
            gaps.append(float(np.min(np.abs(v - t) / t)))
    return min(gaps)
