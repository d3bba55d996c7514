"""Case builders for the edge tests of the SOLOv2-style training targets (tests/test_host_solo_targets_edges.py checks on the CPU that
every planted case reaches the path it is built for; tests/test_gpu_solo_targets_edges.py runs the kernels on them).

The referee is tests/solo_ref.py.  Two things are added here, both checked against it by the host test:

  windows / targets_from_moments   ``R._window`` and ``R.targets`` over whole arrays of instances: torch's elementwise ``//`` on fp32
                                   tensors and NumPy's ``//`` on float64 -- the operators themselves, not a restatement of them;
  floor_div_branches               the fmod-based floor division written out in NumPy, ONLY to count which of its branches the planted
                                   inputs take (the host test first shows that it gives what the operators give).

Everything is built once per process (functools.lru_cache) and must not be modified by a test."""
import functools

import numpy as np
import torch

from tests import solo_ref as R

# ---- A: the configs' grids and the 256 edges ---------------------------------------------------------------------------------
GRIDS, STRIDES = [40, 36, 24, 16, 12], [8, 8, 16, 32, 32]
RANGES = [(1, 14), (7, 24), (12, 32), (20, 48), (32, 256)]
CANVAS, FEAT = (256, 320), (64, 80)
PLANES = [(64, 80), (64, 80), (32, 40), (16, 20), (16, 20)]          # BoxLevelSet: canvas / (stride / 2)
GRIDS64, STRIDES64, RANGES64, PLANES64 = [64, 1], [8, 32], [(1, 48), (1, 256)], [(64, 80), (16, 20)]
NUM_CLASSES, SIGMA = 7, 0.2
SEED, N_BIG = 3, 300
CUTS = (255, 256, 257, N_BIG)


@functools.lru_cache(maxsize=None)
def big_batch():
    """(boxes, labels, masks, moments) of two images on CANVAS: three hand-made instances, then R.random_case(SEED, 300, ...)."""
    H, W = CANVAS
    boxes0 = torch.tensor([[10., 20., 40., 50.], [100., 100., 180., 160.], [200., 8., 300., 200.]])
    labels0 = torch.tensor([1, 5, 0], dtype=torch.int64)
    m0 = np.zeros((3, H, W), np.uint8)
    m0[0, 22:48, 12:38] = 1
    m0[1, 100:160, 100:180] = 1
    m0[2, 8:200:2, 200:300] = 1
    b1, l1, m1 = R.random_case(SEED, N_BIG, H, W, NUM_CLASSES)
    return [boxes0, b1[0]], [labels0, l1[0]], [m0, m1[0]], [R.moments(m0), R.moments(m1[0])]


def assign_kw(grids64=False):
    if grids64:
        return dict(num_grids=GRIDS64, scale_ranges=RANGES64, sigma=SIGMA, num_classes=NUM_CLASSES)
    return dict(num_grids=GRIDS, scale_ranges=RANGES, sigma=SIGMA, num_classes=NUM_CLASSES)


def cut_batch(n):
    boxes, labels, masks, mom = big_batch()
    return [boxes[0], boxes[1][:n]], [labels[0], labels[1][:n]], [masks[0], masks[1][:n]], [mom[0], mom[1][:n]]


@functools.lru_cache(maxsize=None)
def big_want(mode, n, grids64=False):
    """What R.targets gives for the batch with image 1 cut to its first ``n`` instances."""
    boxes, labels, masks, mom = cut_batch(n)
    return R.targets(mode, boxes, labels, masks, canvas=CANVAS, mom=mom, **assign_kw(grids64))


# ---- the restatement over arrays ---------------------------------------------------------------------------------------------
def _cells32(v, size, S):
    return ((v / size) // (1. / S)).long().numpy()       # v: float32 tensor -> torch's fp32 floor division, elementwise


def windows(mode, boxes, mom, S, canvas, sigma):
    """``R._window`` of every instance at once.  ``boxes`` float32 [N,4] tensor, ``mom`` int64 [N,3] with m00 > 0.  Returns a dict of
    int64 arrays: top, down, left, right, and for the census coord_w / coord_h, the centre's numerators ``num_w`` / ``num_h`` in the
    mode's precision, the four edge numerators ``edge`` [4,N] (fp32: top, down, left, right) and their clipped cells ``box`` [4,N]."""
    boxes = boxes.float()
    mom = np.asarray(mom, np.int64)
    half_w, half_h = 0.5 * (boxes[:, 2] - boxes[:, 0]) * sigma, 0.5 * (boxes[:, 3] - boxes[:, 1]) * sigma
    m00, m10, m01 = (mom[:, k].astype(np.float64) for k in range(3))          # exact: every moment here is below 2^53
    if mode == 'discobox':
        d = torch.from_numpy(m00).float()
        cw, ch = torch.from_numpy(m10).float() / d, torch.from_numpy(m01).float() / d
        num_w, num_h = (cw / canvas[1]).numpy(), (ch / canvas[0]).numpy()
        coord_w, coord_h = _cells32(cw, canvas[1], S), _cells32(ch, canvas[0], S)
    else:
        cwd, chd = m10 / m00, m01 / m00
        num_w, num_h = cwd / canvas[1], chd / canvas[0]
        coord_w, coord_h = (num_w // (1. / S)).astype(np.int64), (num_h // (1. / S)).astype(np.int64)
        cw, ch = torch.from_numpy(cwd).float(), torch.from_numpy(chd).float()
    top_box = np.maximum(0, _cells32(ch - half_h, canvas[0], S))
    down_box = np.minimum(S - 1, _cells32(ch + half_h, canvas[0], S))
    left_box = np.maximum(0, _cells32(cw - half_w, canvas[1], S))
    right_box = np.minimum(S - 1, _cells32(cw + half_w, canvas[1], S))
    edge = np.stack([((ch - half_h) / canvas[0]).numpy(), ((ch + half_h) / canvas[0]).numpy(), ((cw - half_w) / canvas[1]).numpy(),
                     ((cw + half_w) / canvas[1]).numpy()])
    return dict(top=np.maximum(top_box, coord_h - 1), down=np.minimum(down_box, coord_h + 1), left=np.maximum(coord_w - 1, left_box),
                right=np.minimum(right_box, coord_w + 1), box=np.stack([top_box, down_box, left_box, right_box]), coord_w=coord_w, coord_h=coord_h, num_w=num_w, num_h=num_h, edge=edge)


def gt_areas(boxes):
    b = boxes.float()
    return torch.sqrt(((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).double()).float()       # correctly rounded fp32 sqrt, as R.targets


def targets_from_moments(mode, boxes, labels, mom, *, num_grids, scale_ranges, sigma, num_classes, canvas):
    """``R.targets`` of ONE image from planted moments, through :func:`windows`.  Returns per level: cate_labels (int64 [S*S]),
    cell_owner (int32), pair_cell / pair_inst (the reference's grid_order and its instances), sel_inst; and num_ins."""
    mom = np.asarray(mom, np.int64)
    areas = gt_areas(boxes).numpy()
    valid = mom[:, 0] > 0 if mode == 'discobox' else mom[:, 0] >= R.MIN_MASK_SUM
    lab = labels.numpy()
    out = dict(cate_labels=[], cell_owner=[], pair_cell=[], pair_inst=[], sel_inst=[], windows=[], hit=[])
    for S, (lo, hi) in zip(num_grids, scale_ranges):
        hit = np.nonzero((areas >= np.float32(lo)) & (areas <= np.float32(hi)) & valid)[0]
        w = windows(mode, boxes[hit], mom[hit], S, canvas, sigma)
        rows, cols = np.maximum(w['down'] - w['top'] + 1, 0), np.maximum(w['right'] - w['left'] + 1, 0)
        cnt = rows * cols
        rep = np.repeat(np.arange(len(hit)), cnt)
        k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        cell = (w['top'][rep] + k // np.maximum(cols[rep], 1)) * S + w['left'][rep] + k % np.maximum(cols[rep], 1)
        owner = np.full(S * S, -1, np.int64)
        np.maximum.at(owner, cell, hit[rep])                # instances ascend in loop order: the last writer is the largest
        cate = np.where(owner >= 0, lab[np.maximum(owner, 0)], num_classes).astype(np.int64)
        out['cate_labels'].append(cate), out['cell_owner'].append(owner.astype(np.int32))
        out['pair_cell'].append(cell.astype(np.int64)), out['pair_inst'].append(hit[rep].astype(np.int64))
        out['sel_inst'].append(owner[owner >= 0]), out['windows'].append(w), out['hit'].append(hit)
    out['num_ins'] = int(sum(len(s) for s in out['sel_inst']))
    return out


def floor_div_branches(a, b):
    """The fmod-based floor division of torch (float32 arrays) and Python / NumPy (float64), written out to COUNT its branches.
    Returns (quotient, dict of how many elements took the sign fix, the div == 0 branch and the ``div - floor > 0.5`` correction)."""
    a = np.asarray(a)
    b = a.dtype.type(b)
    mod = np.fmod(a, b)
    div = (a - mod) / b
    fix = (mod != 0) & ((b < 0) != (mod < 0))
    div = np.where(fix, div - a.dtype.type(1), div)
    fl = np.floor(div)
    corr = (div != 0) & (div - fl > a.dtype.type(0.5))
    q = np.where(div != 0, np.where(corr, fl + a.dtype.type(1), fl), a.dtype.type(0))
    return q, dict(sign_fix=int(fix.sum()), zero=int((div == 0).sum()), half_correction=int(corr.sum()))


# ---- B: planted moments ------------------------------------------------------------------------------------------------------
SWEEP_CANVASES = ((800, 1344), (2520, 2520))
SWEEP_GROUPS = tuple(tuple(range(g, g + 8)) for g in range(1, 65, 8))       # S = 1..64, eight levels per call
WIDE = (1.0, 65536.0)


def _labels(n, num_classes=NUM_CLASSES):
    return torch.from_numpy((np.arange(n) * 5 % num_classes).astype(np.int64))


@functools.lru_cache(maxsize=None)
def sweep_case(canvas, group):
    """Centres at and one sixteenth of a pixel beside every k/S of the eight grids of ``group``: m00 = 16, m10 = round(16 k W / S) + j.
    Every centre comes twice: under a small box (8 x 6, both edges inside the centre's cell or the next one: the window is what the edge
    cells say), and under a box ten canvases wide, whose edges are clipped away on every grid, so that the window is the centre's cell
    +-1 and a centre cell that is off by one shows -- under the small box alone it would not."""
    H, W = canvas
    mom = []
    for S in group:
        for k in range(S + 1):
            for j in (-1, 0, 1):
                mom.append([16, int(round(16 * k * W / S)) + j, int(round(16 * k * H / S)) + j])
    mom = np.asarray(mom + mom, np.int64)
    n = len(mom) // 2
    cx, cy = np.round(mom[:, 1] / 16.0), np.round(mom[:, 2] / 16.0)
    hx, hy = np.where(np.arange(2 * n) < n, 4, 5 * W), np.where(np.arange(2 * n) < n, 3, 5 * H)
    boxes = torch.from_numpy(np.stack([cx - hx, cy - hy, cx + hx, cy + hy], 1).astype(np.float32))
    return dict(boxes=boxes, labels=_labels(len(mom)), mom=mom, num_grids=list(group), scale_ranges=[WIDE] * 8, sigma=0.2, canvas=canvas,
                num_classes=NUM_CLASSES)


WINDOW_GRIDS = [40, 36, 24, 16, 12, 64, 63, 1]


@functools.lru_cache(maxsize=None)
def window_case():
    """sigma = 0.25, box sides that are multiples of 8 and integer centres on a 2520 x 2520 canvas: ``c - half`` and ``c + half`` are
    exact integers placed on k * 2520 / S and one pixel to either side of it, below 0 and above the canvas included; the larger boxes
    span more than three cells, so the window is the centre's cell +-1 and shows which precision the centre's cell was taken in."""
    size = 2520
    halves = (1, 4, 16, 64)
    cs, hs = [], []
    for S in WINDOW_GRIDS:
        for k in range(S + 1):
            if (k * size) % S:
                continue
            e = k * size // S
            for d in (-1, 0, 1):
                for half in halves:
                    for c in (e + d + half, e + d - half):              # the lower edge, then the upper edge, on e + d
                        if 0 <= c <= size:
                            cs.append(c), hs.append(half)
    cs, hs = np.asarray(cs, np.int64), np.asarray(hs, np.int64)
    n = len(cs)
    cy, hy = np.roll(cs, n // 3), np.roll(hs, n // 3)                    # another edge on the other axis
    mom = np.stack([np.full(n, 16), 16 * cs, 16 * cy], 1).astype(np.int64)
    boxes = torch.from_numpy(np.stack([cs - 4 * hs, cy - 4 * hy, cs + 4 * hs, cy + 4 * hy], 1).astype(np.float32))
    return dict(boxes=boxes, labels=_labels(n), mom=mom, num_grids=WINDOW_GRIDS, scale_ranges=[WIDE] * 8, sigma=0.25, canvas=(size, size),
                num_classes=NUM_CLASSES)


def _f32(v):
    return float(np.float32(v))


ROOT77, ROOT1001 = _f32(np.sqrt(77.0)), _f32(np.sqrt(1001.0))       # correctly rounded fp32 roots of products that have no exact root
RANGE_GRIDS = [8, 7, 6, 5, 4, 3, 9, 10]
RANGE_RANGES = [(1.0, 12.0), (12.0, 24.0), (24.0, 48.0), (1.0, ROOT77), (ROOT77, 100.0), (ROOT1001, ROOT1001), (6.0, 6.0), (48.0, 4096.0)]


@functools.lru_cache(maxsize=None)
def range_case():
    """Boxes whose area root sits on a range end, one fp32 step to either side of it, and on ends that are themselves inexact roots."""
    wh = [(9., 16.), (16., 9.), (12., 12.), (24., 24.), (18., 32.), (48., 48.), (36., 64.), (4., 9.), (6., 6.), (7., 11.), (11., 7.), (77., 1.),
          (7., 143.), (13., 77.), (91., 11.), (1001., 1.), (1., 1.), (0.5, 2.)]
    for base in (1.0, 6.0, 12.0, 24.0, 48.0, 100.0):
        b = np.float32(base)
        for steps in range(-4, 5):                                      # side x side', side' a few fp32 steps from side
            v = b
            for _ in range(abs(steps)):
                v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf))
            wh.append((float(b), float(v)))
    for p, q in ((7., 11.), (7., 143.)):                                # the same around the inexact roots
        for steps in range(-3, 4):
            v = np.float32(q)
            for _ in range(abs(steps)):
                v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf))
            wh.append((p, float(v)))
    wh = np.asarray(wh, np.float64)
    n = len(wh)
    H, W = 256, 320
    cx, cy = 20.0 + (np.arange(n) * 37 % 280), 20.0 + (np.arange(n) * 53 % 216)
    zero = np.zeros(n)                                                  # boxes at the origin: x2 - x1 is the planted side, bit for bit
    boxes = torch.from_numpy(np.stack([zero, zero, wh[:, 0], wh[:, 1]], 1)).float()
    mom = np.stack([np.full(n, 16), np.round(16 * cx).astype(np.int64), np.round(16 * cy).astype(np.int64)], 1).astype(np.int64)
    return dict(boxes=boxes, labels=_labels(n), mom=mom, num_grids=RANGE_GRIDS, scale_ranges=RANGE_RANGES, sigma=0.2, canvas=(H, W),
                num_classes=NUM_CLASSES)


@functools.lru_cache(maxsize=None)
def large_moment_case():
    """Moments no fp32 holds: m00 = 2^24 + 1 (a tie, rounds to even) and 2^24 + 2, m10 / m01 on fp32 ties above 2^25 and above 2^32."""
    H, W = 800, 1344
    m00s = (2 ** 24 + 1, 2 ** 24 + 2)
    firsts = (2 ** 25 + 2, 2 ** 25 + 6, 2 ** 25 + 4, 2 ** 32 + 2 ** 8, 2 ** 32 + 3 * 2 ** 8, 2 ** 33 + 2 ** 9 + 1, 2 ** 33 + 3 * 2 ** 9,
              700 * 2 ** 24 + 36, 1343 * (2 ** 24 + 1))
    mom = [[a, x, y] for a in m00s for x in firsts for y in firsts if y / a <= H]
    mom = np.asarray(mom, np.int64)
    n = len(mom)
    cx, cy = np.round(mom[:, 1] / mom[:, 0]), np.round(mom[:, 2] / mom[:, 0])
    side = 8.0 + 8.0 * (np.arange(n) % 3)
    boxes = torch.from_numpy(np.stack([cx - side, cy - side, cx + side, cy + side], 1)).float()
    return dict(boxes=boxes, labels=_labels(n), mom=mom, num_grids=[40, 36, 24, 16, 12, 64, 33, 7], scale_ranges=[WIDE] * 8, sigma=0.2,
                canvas=(H, W), num_classes=NUM_CLASSES)


def planted_cases():
    """name -> case of every direct call of part B."""
    out = {f'sweep_{c[0]}x{c[1]}_S{g[0]}-{g[-1]}': sweep_case(c, g) for c in SWEEP_CANVASES for g in SWEEP_GROUPS}
    out.update(windows=window_case(), ranges=range_case(), large_moments=large_moment_case())
    return out


@functools.lru_cache(maxsize=None)
def planted_want(name, mode):
    c = planted_cases()[name]
    return targets_from_moments(mode, c['boxes'], c['labels'], c['mom'], num_grids=c['num_grids'], scale_ranges=c['scale_ranges'],
                                sigma=c['sigma'], num_classes=c['num_classes'], canvas=c['canvas'])


# ---- C: mask pass ------------------------------------------------------------------------------------------------------------
def _rand_masks(rng, G, H, W, p=0.5):
    return (rng.random((G, H, W)) < p).astype(np.uint8)


def mask_pass_band(factors):
    f = max(factors)
    return f * ((16 + f - 1) // f)                       # source rows per workgroup, as the header's kMinBand rule


@functools.lru_cache(maxsize=None)
def mask_cases():
    """name -> dict(images=[uint8 [G,H,W] per image], factors, planes=[(h, w) per factor]) of every mask-pass case but the large one."""
    rng = np.random.default_rng(11)
    out = {}
    # 272 vectors per 16-row band: instance 0 has ones only from byte 4096 of each band on (what a second trip reads), instance 1 everywhere
    m = np.zeros((3, 32, 272), np.uint8)
    flat = m[0].reshape(2, 16 * 272)
    flat[:, 4096:] = 1
    m[1] = 1
    m[2] = _rand_masks(rng, 1, 32, 272)[0]
    out['second_trip'] = dict(images=[m], factors=[4, 8], planes=[(8, 68), (4, 34)])
    for H in (16, 32):
        for W in (4, 8, 12):
            mm = _rand_masks(rng, 5, H, W, 0.6)
            mm[3] = 1
            out[f'narrow_{H}x{W}'] = dict(images=[mm], factors=[4], planes=[(H // 4, W // 4)])
    # the last band half full; the shorter image has a wholly empty band
    out['half_band'] = dict(images=[_rand_masks(rng, 2, 24, 40), _rand_masks(rng, 3, 48, 24)], factors=[4, 8], planes=[(12, 10), (6, 5)])
    for factors in ([2], [2, 4, 8, 16], [32, 64]):
        imgs = [_rand_masks(rng, 2, 64, 64), _rand_masks(rng, 2, 128, 64, 0.4)]
        planes = [(128 // f + 1, 64 // f + 2) for f in factors]          # larger than H/f x W/f: the zero border
        out['factors_' + '_'.join(map(str, factors))] = dict(images=imgs, factors=factors, planes=planes)
    return out


def mask_want(case):
    """(moments int64 [G,3], [uint8 [G,h,w] per factor]) by R.moments and R.rescale, zeros outside the source."""
    mom = np.concatenate([R.moments(m) for m in case['images']])
    planes = []
    for f, (h, w) in zip(case['factors'], case['planes']):
        per = []
        for m in case['images']:
            p = np.zeros((m.shape[0], h, w), np.uint8)
            p[:, :m.shape[1] // f, :m.shape[2] // f] = R.rescale(m, f)
            per.append(p)
        planes.append(np.concatenate(per))
    return mom, planes


# (H, W, factor) of the full masks whose sums leave 32 bits: in the total (m10, m01 > 2^32 over 2048 x 2304), and over 64 x 196608
# under one band of 64 rows already in a workgroup's partial and in a single thread's
LARGE_MASKS = ((2048, 2304, 4), (64, 196608, 64))


def large_mask_moments(H, W):
    """Closed form for one full H x W mask followed by an empty one."""
    return [[H * W, H * (W * (W - 1) // 2), W * (H * (H - 1) // 2)], [0, 0, 0]]


# ---- E: category loss --------------------------------------------------------------------------------------------------------
CATE_SPEC = dict(B=2, num_classes=3, num_grids=[40, 36, 1, 2, 3])
CATE_SETTINGS = ((2.0, 0.25), (1.5, 0.3))
CATE_PLANTS = (30.0, -30.0, 90.0, -90.0, 200.0, -200.0)
CATE_LOSS_WEIGHT, CATE_UPSTREAM = 1.0, 0.375


@functools.lru_cache(maxsize=None)
def cate_case():
    """Labels of a ``R.targets`` call on two images (positives on the two large levels), seeded logits with +-30, +-90 and +-200 planted
    on positive elements (the logit of a set cell's own class) and on negative ones of levels 0 and 1."""
    B, C, grids = CATE_SPEC['B'], CATE_SPEC['num_classes'], CATE_SPEC['num_grids']
    boxes, labels, masks = [], [], []
    for b in range(B):
        bx, lb, mk = R.random_case(20 + b, 40, 256, 320, C)
        boxes.append(bx[0]), labels.append(lb[0]), masks.append(mk[0])
    tg = R.targets('discobox', boxes, labels, masks, num_grids=grids, scale_ranges=[(1, 24), (12, 64), (1, 256), (1, 256), (1, 256)],
                   sigma=0.2, num_classes=C, canvas=(256, 320))
    preds = [p.copy() for p in R.make_cate_inputs(CATE_SPEC, 9)]
    at = 0
    planted = []
    for l in (0, 1):
        hw = grids[l] ** 2
        lab = tg['cate_labels'][at:at + B * hw].reshape(B, hw)
        pos = np.argwhere(lab < C)
        neg = np.argwhere(lab == C)
        flat = preds[l].reshape(B, C, hw)
        for i, v in enumerate(CATE_PLANTS):
            b, yx = pos[(i * 7 + 3) % len(pos)]
            flat[b, lab[b, yx], yx] = v
            planted.append((l, int(b), int(lab[b, yx]), int(yx), v, True))
            b, yx = neg[(i * 131 + 17) % len(neg)]
            flat[b, i % C, yx] = v
            planted.append((l, int(b), i % C, int(yx), v, False))
        at += B * hw
    return dict(preds=preds, labels=tg['cate_labels'], num_ins=tg['num_ins'], planted=planted)
