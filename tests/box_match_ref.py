"""Float64 numpy restatement of the Box2Mask target assignment (test infrastructure; nothing here is used by the package).

What the reference computes in torch (box2mask_head.py:152-189, match_cost.py:153-193, 365-425, mask_hungarian_assigner.py:46-132),
written out once more in numpy so that the tests have an independent statement of every step; tests/test_host_box_match.py checks it
against what the reference's own code produced (tests/golden/box_match.npz).  Also the case table and the loaders of that fixture.
"""
from __future__ import annotations

import numpy as np

CFG = dict(w_cls=2.0, w_dice=5.0, pred_act=True, eps=1.0)           # configs/box2mask/box2mask_r50_lsj_8x2_50e_coco.py:111-114
DEFAULTS = dict(w_cls=1.0, w_dice=1.0, pred_act=False, eps=1e-3)    # the classes' own defaults

# name: (seed, (h, w), (H, W), Q, G per image, parameter set, number of classes)
CASES = {
    'r4': (11, (13, 11), (52, 44), 67, (7,), 'cfg', 6),             # ratio exactly 4; query 0 all-negative, query 1 constant
    'frac': (12, (7, 9), (20, 30), 100, (1,), 'defaults', 4),       # non-integer ratio, both edge clamps
    'down': (13, (12, 10), (6, 5), 3, (5,), 'cfg', 3),              # down-sampling, more ground truths than queries
    'wide': (14, (5, 70), (20, 280), 5, (5,), 'defaults', 5),       # a row longer than a wave, H + W = 300
    'empty': (15, (7, 9), (20, 30), 5, (0,), 'cfg', 4),             # no ground truth
    'batch': (16, (13, 11), (52, 44), 12, (0, 4, 7), 'cfg', 5),     # three problems, one of them empty
    # class rows and label lists longer than a wave (the shipped COCO config has 81 columns), the solver past 64 rows in both orientations
    'coco': (17, (7, 9), (28, 36), 100, (70, 1), 'cfg', 80),        # 81 columns and 70 labels: two trips each; solver transposed, 70 x 100
    'crowd': (18, (7, 9), (28, 36), 70, (100,), 'cfg', 63),         # exactly 64 columns; solver NOT transposed, 70 rows x 100 columns
    'c65': (19, (7, 9), (14, 18), 5, (3,), 'defaults', 64),         # 65 columns: a one-element second trip
}
PARAMS = {'cfg': CFG, 'defaults': DEFAULTS}


LIMIT_SIDE = 1024                                                   # BXI_MATCH_MAX_SIDE: matrices of this size are built, not stored


def limit_uniform(Q, G):
    """The uniform fp32 cost of the solver's limit cases; the fixture pins the square one by a CRC32 of its bytes."""
    return np.random.default_rng(0).uniform(0, 10, (Q, G)).astype(np.float32)


def limit_ties(Q=LIMIT_SIDE, G=LIMIT_SIDE):
    """Exact small integers (0..1008) as fp32 with many optimal assignments."""
    i, j = np.arange(Q, dtype=np.int64)[:, None], np.arange(G, dtype=np.int64)[None, :]
    return ((i * 7919 + j * 104729 + i * j * 31 + i * i * 17 + j * j * 13) % 1009).astype(np.float32)


def make_inputs(name):
    """The inputs of a case, from its seed: per image ``logits`` [Q,h,w] fp32, ``cls`` [Q,C+1] fp32, ``labels`` [G] int64, ``masks``
    [G,H,W] uint8 box masks.  Predictions are noisy blobs, some of them near a ground-truth box, so that the optimum is well separated."""
    seed, (h, w), (H, W), Q, counts, _, C = CASES[name]
    rng = np.random.default_rng(seed)
    images = []
    for G in counts:
        masks = np.zeros((G, H, W), np.uint8)
        boxes = []
        for g in range(G):
            y0, x0 = int(rng.integers(0, max(H - 2, 1))), int(rng.integers(0, max(W - 2, 1)))
            y1, x1 = int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))
            masks[g, y0:y1, x0:x1] = 1
            boxes.append((y0 * h / H, y1 * h / H, x0 * w / W, x1 * w / W))
        yy, xx = np.mgrid[0:h, 0:w] + 0.5
        logits = rng.normal(-1.0, 1.5, (Q, h, w))
        for q in range(Q):
            if boxes and rng.uniform() < 0.7:
                y0, y1, x0, x1 = boxes[int(rng.integers(0, G))]
                y0, y1, x0, x1 = y0 + rng.normal(0, 0.5), y1 + rng.normal(0, 0.5), x0 + rng.normal(0, 0.5), x1 + rng.normal(0, 0.5)
                logits[q] += 4.0 * ((yy > y0) & (yy < y1) & (xx > x0) & (xx < x1))
        if name == 'r4':
            logits[0] = -np.abs(logits[0]) - 0.5                    # every logit negative: a maximum that started at 0 would show
            logits[1] = 0.75                                        # constant: every maximum is a tie
        images.append(dict(logits=logits.astype(np.float32), cls=rng.normal(0, 1.5, (Q, C + 1)).astype(np.float32),
                           labels=rng.integers(0, C, G).astype(np.int64), masks=masks))
    return images


def load_case(g, name):
    """The stored inputs of a case of the fixture, in the layout of make_inputs."""
    _, (h, w), (H, W), Q, counts, _, _ = CASES[name]
    images = []
    for i, G in enumerate(counts):
        k = f'{name}{i}'
        masks = np.unpackbits(g[f'{k}_masks'], axis=1)[:, :H * W].reshape(G, H, W) if G else np.zeros((0, H, W), np.uint8)
        images.append(dict(logits=g[f'{k}_logits'], cls=g[f'{k}_cls'], labels=g[f'{k}_labels'], masks=masks))
    return images


def source_index(out_size, in_size):
    """ATen's align_corners=False rule: src = (dst + 0.5) * in / out - 0.5 clamped at 0, the neighbour clamped at in - 1."""
    src = np.maximum((np.arange(out_size, dtype=np.float64) + 0.5) * (in_size / out_size) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def upsample(x, H, W):
    """``F.interpolate(x[:, None], (H, W), mode='bilinear', align_corners=False)[:, 0]`` in float64."""
    x = np.asarray(x, np.float64)
    y0, y1, ly0, ly1 = source_index(H, x.shape[1])
    x0, x1, lx0, lx1 = source_index(W, x.shape[2])
    top = lx0 * x[:, y0][:, :, x0] + lx1 * x[:, y0][:, :, x1]
    bot = lx0 * x[:, y1][:, :, x0] + lx1 * x[:, y1][:, :, x1]
    return ly0[None, :, None] * top + ly1[None, :, None] * bot


def pred_projections(logits, H, W, act):
    """(rows [n,H], cols [n,W]): max over every up-sampled row / column, after the sigmoid when ``act``.  NaN wins, as in torch.max."""
    up = upsample(logits, H, W)
    if act:
        up = 1.0 / (1.0 + np.exp(-up))
    return up.max(axis=2), up.max(axis=1)


def gt_projections(masks):
    m = np.asarray(masks, np.float64)
    return m.max(axis=2), m.max(axis=1)


def bin_dice(p, t, eps):
    num = 2.0 * p @ t.T
    den = (p ** 2).sum(1)[:, None] + (t ** 2).sum(1)[None, :]
    return 1.0 - (num + eps) / (den + eps)


def class_cost(cls, labels, weight, dtype=np.float64):
    """``dtype=np.float32``: the same statement in fp32 arithmetic, for a measured fp32-against-fp64 difference (bin_dice stays in the
    precision of its arguments)."""
    z = np.asarray(cls, dtype)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return -(e / e.sum(axis=1, keepdims=True))[:, labels] * weight


def match_cost(image, H, W, w_cls, w_dice, pred_act, eps):
    """The [Q, G] cost of one image: class_cost + w_dice (dice of the row projections + dice of the column projections)."""
    pr, pc = pred_projections(image['logits'], H, W, pred_act)
    tr, tc = gt_projections(image['masks'])
    return class_cost(image['cls'], image['labels'], w_cls) + w_dice * (bin_dice(pr, tr, eps) + bin_dice(pc, tc, eps))


def linear_sum_assignment(cost):
    """Exact rectangular assignment by shortest augmenting paths with duals (Jonker-Volgenant), plain Python for small matrices.
    Returns (rows, cols) sorted by row, as scipy.optimize.linear_sum_assignment does."""
    c = np.asarray(cost, np.float64)
    transposed = c.shape[1] < c.shape[0]
    if transposed:
        c = c.T
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = -np.ones(nr, np.int64), -np.ones(nc, np.int64)
    for cur in range(nr):
        shortest, path = np.full(nc, np.inf), -np.ones(nc, np.int64)
        in_rows, in_cols = np.zeros(nr, bool), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            in_rows[i] = True
            r = min_val + c[i] - u[i] - v
            better = (r < shortest) & ~in_cols
            path[better], shortest[better] = i, r[better]
            cand = np.where(in_cols, np.inf, shortest)
            min_val = cand.min()
            ties = np.flatnonzero(cand == min_val)
            free = ties[row4col[ties] < 0]
            j = int(free[0] if len(free) else ties[0])
            in_cols[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] += min_val
        others = in_rows.copy()
        others[cur] = False
        u[others] += min_val - shortest[col4row[others]]
        v[in_cols] -= min_val - shortest[in_cols]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows, cols = np.arange(nr), col4row
    if transposed:
        order = np.argsort(cols)
        rows, cols = cols[order], rows[order]
    return rows, cols


def assign(cost, labels):
    """Steps 1 and 4 of MaskHungarianAssigner.assign and the pseudo sampler: (gt_inds [Q], assigned_labels [Q], pos_inds,
    pos_assigned_gt_inds)."""
    Q, G = cost.shape
    gt_inds, out = np.zeros(Q, np.int64), -np.ones(Q, np.int64)
    if G:
        rows, cols = linear_sum_assignment(cost)
        gt_inds[rows], out[rows] = cols + 1, labels[cols]
    pos = np.flatnonzero(gt_inds > 0)
    return gt_inds, out, pos, gt_inds[pos] - 1


def is_matching(pos, pos_gt, Q, G):
    """``min(Q, G)`` pairs, every query and every ground truth at most once, all in range."""
    return (len(pos) == len(pos_gt) == min(Q, G) and len(set(pos.tolist())) == len(pos) and len(set(pos_gt.tolist())) == len(pos_gt)
            and (len(pos) == 0 or (0 <= pos.min() and pos.max() < Q and 0 <= pos_gt.min() and pos_gt.max() < G)))
