"""A numpy restatement of CondInst's test-time detections (no torch): the order rule and the greedy NMS of bxi_box_nms_f32, mmcv's
batched_nms with its class-offset trick, the decode / filter of CondInstBoxHead._get_bboxes, and the input recipes of the tests.

Everything takes a ``dtype`` (float32 or float64) for the scores and the IoU arithmetic.  Boxes are always decoded in float32: each
coordinate is one addition or subtraction, a clamp and a correctly rounded division, so they are bit-exact whatever runs them."""
import numpy as np

F32 = np.float32


# ---- order and greedy NMS ---------------------------------------------------------------------------------------------------
def sort_order(scores):
    """Descending score, ties by ascending index, NaN first, -0 == +0."""
    s = np.asarray(scores, np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, 0.0, s), ~nan))


def suppresses(a, k, thr, offset, T, form='mul'):
    """Does the kept box k suppress a?  Every operation rounded to T."""
    off = T(offset)
    w = max(T(T(min(a[2], k[2]) - max(a[0], k[0])) + off), T(0))
    h = max(T(T(min(a[3], k[3]) - max(a[1], k[1])) + off), T(0))
    inter = T(w * h)
    sa = T(T(T(a[2] - a[0]) + off) * T(T(a[3] - a[1]) + off))
    sb = T(T(T(k[2] - k[0]) + off) * T(T(k[3] - k[1]) + off))
    union = T(T(sa + sb) - inter)
    if form == 'mul':
        return bool(inter > T(T(thr) * union))
    return bool(union > 0 and T(inter / union) > T(thr))


def greedy_nms(boxes, scores, labels, thr, offset=0, max_num=-1, dtype=np.float32, order=None, form='mul'):
    """Keep list (indices in score order) by the rule of include/boxinst/boxinst_hip_det.h.  ``labels`` None: class-agnostic."""
    T = dtype
    b = np.asarray(boxes).astype(T)
    order = sort_order(scores) if order is None else order
    keep = []
    for i in order:
        if max_num > 0 and len(keep) >= max_num:
            break
        ok = True
        for j in keep:
            if labels is not None and labels[i] != labels[j]:
                continue
            if suppresses(b[i], b[j], thr, offset, T, form):
                ok = False
                break
        if ok:
            keep.append(int(i))
    return keep


def iou_margin(boxes, labels, thr, offset=0):
    """Smallest |IoU - thr| in float64 over the pairs NMS can compare (same label; all pairs when ``labels`` is None)."""
    b = np.asarray(boxes, np.float64)
    n = len(b)
    if n < 2:
        return np.inf
    iw = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + offset, 0, None)
    ih = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + offset, 0, None)
    inter = iw * ih
    area = (b[:, 2] - b[:, 0] + offset) * (b[:, 3] - b[:, 1] + offset)
    union = area[:, None] + area[None, :] - inter
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)
    pair = ~np.eye(n, dtype=bool)
    if labels is not None:
        pair &= np.asarray(labels)[:, None] == np.asarray(labels)[None, :]
    return float(np.abs(iou[pair] - thr).min()) if pair.any() else np.inf


def batched_nms_mmcv_style(boxes, scores, idxs, nms_cfg, class_agnostic=False, dtype=np.float32, form='mul'):
    """mmcv.ops.nms.batched_nms restated: classes are kept apart by adding ``idx * (max coordinate + 1)`` to the boxes in their own
    precision, then one class-agnostic greedy NMS.  Returns (dets [k,5], keep [k]) in descending score order."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    assert cfg.pop('type', 'nms') == 'nms'
    cfg.pop('split_thr', None)
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    T = boxes.dtype.type
    if class_agnostic:
        shifted = boxes
    else:
        off = (np.asarray(idxs).astype(boxes.dtype) * T(boxes.max() + T(1))).astype(boxes.dtype)
        shifted = (boxes + off[:, None]).astype(boxes.dtype)
    keep = np.array(greedy_nms(shifted, scores, None, cfg['iou_threshold'], cfg.get('offset', 0), cfg.get('max_num', -1), dtype, form=form),
                    dtype=np.int64)
    return np.concatenate([boxes[keep], scores[keep, None]], 1), keep


# ---- the decode / filter of _get_bboxes -------------------------------------------------------------------------------------
def sigmoid(x, T):
    x = np.asarray(x).astype(T)
    return (T(1) / (T(1) + np.exp(-x))).astype(T)


def level_offsets(sizes):
    return np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)


def points_of(sizes, strides):
    """[M_all, 2] float32 (x, y) and [M_all] level index: ((x + 0.5) * stride, (y + 0.5) * stride), level-major, then y, then x."""
    pts, lvl = [], []
    for i, ((h, w), s) in enumerate(zip(sizes, strides)):
        yy, xx = np.mgrid[0:h, 0:w]
        pts.append(np.stack([(xx.reshape(-1) + 0.5) * s, (yy.reshape(-1) + 0.5) * s], 1).astype(F32))
        lvl.append(np.full(h * w, i, np.int64))
    return np.concatenate(pts), np.concatenate(lvl)


def flatten_levels(maps):
    """per level [B,K,H,W] -> [B, M_all, K]"""
    return np.concatenate([m.transpose(0, 2, 3, 1).reshape(m.shape[0], -1, m.shape[1]) for m in maps], 1)


def location_scores(inp, T=np.float32):
    """[B, M_all]: sigmoid(max_c cls) * sigmoid(ctr)"""
    cls, ctr = flatten_levels(inp['cls']), flatten_levels(inp['ctr'])[..., 0]
    return (sigmoid(cls.max(-1), T) * sigmoid(ctr, T)).astype(T)


def select(inp, nms_pre, T=np.float32):
    """[B, M] indices into M_all: the per-level top-k (descending location score, ties by ascending index), or every location."""
    sizes = [m.shape[-2:] for m in inp['cls']]
    off = level_offsets(sizes)
    score = location_scores(inp, T)
    B = score.shape[0]
    parts = []
    for i in range(len(sizes)):
        hw = int(off[i + 1] - off[i])
        if 0 < nms_pre < hw:
            parts.append(np.stack([sort_order(score[b, off[i]:off[i + 1]])[:nms_pre] + off[i] for b in range(B)]))
        else:
            parts.append(np.tile(np.arange(off[i], off[i + 1]), (B, 1)))
    return np.concatenate(parts, 1).astype(np.int64)


def decode_boxes(inp, strides, img_dims, rescale):
    """[B, M_all, 4] float32: distance2bbox, the clamp to img_shape and the division by the scale factors."""
    sizes = [m.shape[-2:] for m in inp['cls']]
    pts, _ = points_of(sizes, strides)
    d = flatten_levels(inp['bbox']).astype(F32)
    out = np.stack([pts[None, :, 0] - d[..., 0], pts[None, :, 1] - d[..., 1], pts[None, :, 0] + d[..., 2], pts[None, :, 1] + d[..., 3]], -1).astype(F32)
    for b, dim in enumerate(np.asarray(img_dims, F32)):
        mx = np.array([dim[1], dim[0], dim[1], dim[0]], F32)
        v = out[b]
        v = np.where(v < 0, F32(0), v)
        v = np.where(v > mx, mx, v)
        out[b] = (v / dim[2:6]).astype(F32) if rescale else v
    return out


def candidates(inp, strides, img_dims, rescale, score_thr, sel=None, T=np.float32):
    """Per image dict(boxes [n,4] f32, scores [n] T, labels [n], pos [n]) in the reference's ``nonzero`` order (row of sel, class)."""
    cls, ctr = flatten_levels(inp['cls']), flatten_levels(inp['ctr'])[..., 0]
    boxes = decode_boxes(inp, strides, img_dims, rescale)
    B, M_all, _ = cls.shape
    out = []
    for b in range(B):
        rows = np.arange(M_all) if sel is None else sel[b]
        s = sigmoid(cls[b, rows], T)
        m, c = np.nonzero(s > T(F32(score_thr)))
        out.append(dict(boxes=boxes[b, rows[m]], scores=(s[m, c] * sigmoid(ctr[b, rows[m]], T)).astype(T), labels=c.astype(np.int64),
                        pos=m.astype(np.int32)))
    return out


def get_bboxes(inp, strides, img_dims, cfg, rescale=False, T=np.float32):
    """CondInstBoxHead._get_bboxes + nms_with_others by the rules of the library.  ``cfg``: nms_pre, score_thr, iou_threshold,
    max_per_img, class_agnostic.  Per image dict(dets [n,5], labels, params [n,P], coors [n,2], level_inds, cand=..., sel=...)."""
    sizes = [m.shape[-2:] for m in inp['cls']]
    pts, lvl = points_of(sizes, strides)
    params = flatten_levels(inp['params'])
    sel = select(inp, cfg['nms_pre'], T)
    cand = candidates(inp, strides, img_dims, rescale, cfg['score_thr'], sel, T)
    out = []
    for b, c in enumerate(cand):
        labels = None if cfg.get('class_agnostic', False) else c['labels']
        keep = np.array(greedy_nms(c['boxes'], c['scores'], labels, cfg['iou_threshold'], 0, cfg['max_per_img'], T), dtype=np.int64)
        loc = sel[b][c['pos'][keep]]
        out.append(dict(dets=np.concatenate([c['boxes'][keep].astype(np.float64), c['scores'][keep, None].astype(np.float64)], 1),
                        labels=c['labels'][keep], params=params[b, loc], coors=pts[loc], level_inds=lvl[loc], keep=keep, cand=c, sel=sel[b]))
    return out


# ---- input recipes ----------------------------------------------------------------------------------------------------------
def clustered_boxes(seed, n, nlab, size=(160, 256)):
    """n boxes on a 1/8-pixel grid around n // 12 shared centres, labels, and scores that are a shuffled linspace."""
    rng = np.random.default_rng(seed)
    k = max(n // 12, 1)
    cy, cx = rng.uniform(20, size[0] - 20, k), rng.uniform(20, size[1] - 20, k)
    w, h = rng.uniform(16, 90, k), rng.uniform(16, 90, k)
    j = rng.integers(0, k, n)
    x1, y1 = cx[j] - w[j] / 2 + rng.normal(0, 6, n), cy[j] - h[j] / 2 + rng.normal(0, 6, n)
    x2, y2 = cx[j] + w[j] / 2 + rng.normal(0, 6, n), cy[j] + h[j] / 2 + rng.normal(0, 6, n)
    b = np.round(np.stack([x1, y1, x2, y2], 1) * 8) / 8
    b[:, 0::2] = b[:, 0::2].clip(0, size[1])
    b[:, 1::2] = b[:, 1::2].clip(0, size[0])
    b[:, 2] = np.maximum(b[:, 2], b[:, 0] + 0.125)          # well formed: x1 < x2, y1 < y2
    b[:, 3] = np.maximum(b[:, 3], b[:, 1] + 0.125)
    lab = rng.integers(0, nlab, n)
    sc = rng.permutation(np.linspace(0.06, 0.95, n)).astype(F32)
    return b.astype(F32), sc, lab.astype(np.int64)


def clustered_boxes_with_margin(seed, n, nlab, thr, offset=0, margin=1e-4, agnostic=False):
    """clustered_boxes at the first seed from ``seed`` on whose comparable pairs all have |IoU - thr| > margin in float64."""
    for s in range(seed, seed + 200):
        b, sc, lab = clustered_boxes(s, n, nlab)
        if iou_margin(b, None if agnostic else lab, thr, offset) > margin:
            return b, sc, lab
    raise AssertionError('no seed with the IoU margin')


DET_SIZES, DET_STRIDES, DET_C, DET_P, DET_B = ((12, 20), (6, 10), (3, 5)), (8, 16, 32), 5, 9, 3
DET_IMG_SHAPES = ((90, 155, 3), (96, 160, 3), (84, 141, 3))
DET_SCALES = ((1.25, 1.5, 1.25, 1.5), (1.0, 1.0, 1.0, 1.0), (0.8, 1.3125, 0.8, 1.3125))
DET_CASES = {   # name: (rescale, cfg)
    'lv3': (False, dict(nms_pre=40, score_thr=0.05, iou_threshold=0.5, max_per_img=100, class_agnostic=False)),
    'resc': (True, dict(nms_pre=40, score_thr=0.05, iou_threshold=0.5, max_per_img=100, class_agnostic=False)),
    'cut': (False, dict(nms_pre=40, score_thr=0.05, iou_threshold=0.5, max_per_img=7, class_agnostic=False)),
    'agn': (False, dict(nms_pre=40, score_thr=0.05, iou_threshold=0.5, max_per_img=100, class_agnostic=True)),
}
DET_EMPTY_IMAGE = 1


def det_img_dims(rescale=True):
    return [[float(s[0]), float(s[1])] + list(f) for s, f in zip(DET_IMG_SHAPES, DET_SCALES)]


def det_inputs(seed, sizes=None, strides=None, B=None, extra_picks=None):
    """dict(cls, bbox, ctr, params: per level [B,K,H,W] float32).  Distances on a 1/8-pixel grid; image DET_EMPTY_IMAGE has no candidate;
    the candidates' final scores are a shuffled linspace: pick the product, draw the centerness, solve for the class logit.
    ``sizes`` / ``strides`` / ``B``: other levels and another batch (default: DET_SIZES, DET_STRIDES, DET_B -- the stored fixture);
    ``extra_picks``: image -> [(level, y, x, class)] that become candidates as well, under the same shuffled linspace."""
    rng = np.random.default_rng(seed)
    sizes, strides = DET_SIZES if sizes is None else sizes, DET_STRIDES if strides is None else strides
    B, C, P = DET_B if B is None else B, DET_C, DET_P
    logit = lambda p: np.log(p / (1 - p))                   # noqa: E731
    inp = dict(cls=[], bbox=[], ctr=[], params=[])
    for (h, w), s in zip(sizes, strides):
        inp['cls'].append(logit(0.01 * rng.uniform(0.7, 1.3, (B, C, h, w))))
        inp['ctr'].append(logit(rng.uniform(0.05, 0.95, (B, 1, h, w))))
        inp['bbox'].append(np.round(rng.uniform(0.5, 3.0, (B, 4, h, w)) * s * 8) / 8)
        inp['params'].append(np.round(rng.normal(0, 1, (B, P, h, w)) * 64) / 64)
    for b in range(B):
        if b == DET_EMPTY_IMAGE:
            continue
        n_obj = 4
        picks = []
        for o in range(n_obj):
            cx, cy = rng.uniform(30, 130), rng.uniform(20, 75)
            bw, bh = rng.uniform(24, 70), rng.uniform(20, 50)
            lab = int(rng.integers(0, C))
            for lv, ((h, w), s) in enumerate(zip(sizes, strides)):
                ys, xs = np.mgrid[0:h, 0:w]
                px, py = (xs + 0.5) * s, (ys + 0.5) * s
                inside = np.flatnonzero((np.abs(px - cx) < bw / 4) & (np.abs(py - cy) < bh / 4))
                for yx in rng.permutation(inside)[:6 if lv == 0 else 3]:
                    y, x = divmod(int(yx), w)
                    box = np.array([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]) + rng.normal(0, 2.5, 4)
                    d = np.array([px[y, x] - box[0], py[y, x] - box[1], box[2] - px[y, x], box[3] - py[y, x]])
                    inp['bbox'][lv][b, :, y, x] = np.maximum(np.round(d * 8) / 8, 0.125)
                    picks.append((lv, y, x, lab))
                    if rng.uniform() < 0.25:
                        picks.append((lv, y, x, int((lab + 1 + rng.integers(0, C - 1)) % C)))
        picks = sorted(set(picks + list((extra_picks or {}).get(b, []))))
        prods = rng.permutation(np.linspace(0.06, 0.9, len(picks)))
        ctr_of = {}
        for (lv, y, x, lab), p in zip(picks, prods):
            key = (lv, y, x)
            if key not in ctr_of:                             # a location with two classes: one centerness, chosen for the larger product
                pmax = max(q for (k2, q) in zip(picks, prods) if k2[:3] == key)
                lo = max(0.5, pmax / 0.98)
                ctr_of[key] = rng.uniform(lo, max(lo + 0.005, 0.95))
                inp['ctr'][lv][b, 0, y, x] = logit(ctr_of[key])
            inp['cls'][lv][b, lab, y, x] = logit(p / ctr_of[key])
    return {k: [np.ascontiguousarray(m.astype(F32)) for m in v] for k, v in inp.items()}


# ---- the configs' level sizes: 20267 locations, 317 row tiles ---------------------------------------------------------------------
EDGE_SIZES, EDGE_STRIDES, EDGE_B = ((100, 152), (50, 76), (25, 38), (13, 19), (7, 10)), (8, 16, 32, 64, 128), 2
EDGE_IMG_SHAPES = ((800, 1216, 3), (768, 1184, 3))
EDGE_SCALES = ((1.25, 1.5, 1.25, 1.5), (1.0, 1.0, 1.0, 1.0))
EDGE_ROWS = (0, 63, 64, 16383, 16384, 16447, 16448, 20266)          # either side of a row tile's edge, of tile 256's, and the last row
EDGE_CAPS = (256, 20)                                                # rows for every candidate, and fewer rows than candidates


def edge_img_dims():
    return [[float(s[0]), float(s[1])] + list(f) for s, f in zip(EDGE_IMG_SHAPES, EDGE_SCALES)]


def edge_picks():
    """(level, y, x, class) of the planted candidates of image 0: EDGE_ROWS, one more location in the middle of every level, and a second
    class on the first and on the last row."""
    off = level_offsets(EDGE_SIZES)
    picks = []
    for i, m in enumerate(EDGE_ROWS):
        lv = int(np.searchsorted(off, m, side='right') - 1)
        y, x = divmod(int(m - off[lv]), EDGE_SIZES[lv][1])
        picks.append((lv, y, x, i % DET_C))
    for lv, (h, w) in enumerate(EDGE_SIZES):
        picks.append((lv, h // 2, w // 2, (lv + 2) % DET_C))
    picks.append(picks[0][:3] + ((picks[0][3] + 1) % DET_C,))
    picks.append(picks[len(EDGE_ROWS) - 1][:3] + ((picks[len(EDGE_ROWS) - 1][3] + 3) % DET_C,))
    return picks


def edge_inputs(seed):
    """The recipe of det_inputs on EDGE_SIZES with B = 2: image 1 has no candidate, image 0 the recipe's own and edge_picks()."""
    return det_inputs(seed, EDGE_SIZES, EDGE_STRIDES, EDGE_B, {0: edge_picks()})


def edge_inputs_with_margin(seed, cfg, margin=1e-4):
    """(seed, inputs) at the first seed from ``seed`` on whose candidates, of every location and of the per-level top ``cfg['nms_pre']``
    alike (the score filter leaves the same ones), keep ``margin`` between every comparable IoU and the threshold in float64."""
    for s in range(seed, seed + 50):
        inp = edge_inputs(s)
        c = candidates(inp, EDGE_STRIDES, edge_img_dims(), False, cfg['score_thr'], None, np.float64)[0]
        if iou_margin(c['boxes'], c['labels'], cfg['iou_threshold']) > margin:
            return s, inp
    raise AssertionError('no seed with the IoU margin')
