"""Case builders for the edge tests of CondInst's box head in training (tests/test_host_box_head_edges.py shows on the CPU that every
case reaches the path it is named for; tests/test_gpu_box_head_edges.py runs the kernels of csrc/fcos_loss.hip on them).

The referee is tests/fcos_ref.py.  What is added here is only the arithmetic of the launch grids, restated from the header's constants
(``tiles``, ``workgroup_of``, ``focal_workgroups``), so that the host test can say which workgroup, tile and box chunk a location falls in.

Everything is built once per process (functools.lru_cache) and must not be modified by a test."""
import functools

import numpy as np
import torch

from tests import fcos_ref as R

LOC_TILE, ELEM_TILE, GT_CHUNK, MAX_IMAGES = 256, 1024, 64, 64          # BXI_FCOS_LOC_TILE, _ELEM_TILE, _GT_CHUNK, BXI_MAX_IMAGES
FINISH_THREADS = 256                                                    # fcos_finish_kernel: thread t takes partials t, t + 256, ...
SPEC = R.load_cases()
WIDE = (-1.0, 1e8)


# ---- the launch grids ----------------------------------------------------------------------------------------------------------
def tiles(sizes):
    return [(h * w + LOC_TILE - 1) // LOC_TILE for h, w in sizes]


def loc_workgroups(sizes, B):
    return B * sum(tiles(sizes))


def focal_workgroups(sizes, B, C):
    return sum((B * C * h * w + ELEM_TILE - 1) // ELEM_TILE for h, w in sizes)


def workgroup_of(sizes, B):
    """(workgroup, tile inside its level, offset inside the level's plane) of every location in training order (level, image, y, x)."""
    wg, tile, yx_all, first = [], [], [], 0
    for (h, w), t in zip(sizes, tiles(sizes)):
        yx = np.tile(np.arange(h * w), B)
        b = np.repeat(np.arange(B), h * w)
        wg.append(first + b * t + yx // LOC_TILE)
        tile.append(yx // LOC_TILE)
        yx_all.append(yx)
        first += B * t
    return np.concatenate(wg), np.concatenate(tile), np.concatenate(yx_all)


def settings(name, strides, ranges, **over):
    """The flat settings of case ``name`` of tests/golden/box_head_loss_cases.json on other levels."""
    from boxinstseg_amd import parse_box_head_cfg
    cfg = R.head_cfg(SPEC, name)
    cfg.update(strides=list(strides), regress_ranges=[tuple(r) for r in ranges])
    cfg.update(over)
    return parse_box_head_cfg(cfg)


def ref_targets(case, s, dtype=torch.float32):
    return R.targets(case['sizes'], s['strides'], [b.to(dtype) for b in case['boxes']], case['labels'], s['regress_ranges'], s['center_sampling'],
                     s['center_sample_radius'], s['norm_on_bbox'], s['num_classes'], dtype)


def _cycle(n, C=5):
    return torch.arange(n, dtype=torch.int64) % C


def _case(sizes, strides, ranges, boxes, C=5):
    boxes = [torch.from_numpy(np.asarray(b, np.float32).reshape(-1, 4)) for b in boxes]
    return dict(sizes=[tuple(s) for s in sizes], strides=list(strides), ranges=[tuple(r) for r in ranges], boxes=boxes,
                labels=[_cycle(len(b), C) for b in boxes], B=len(boxes), C=C)


# ---- A: the configs' level sizes -----------------------------------------------------------------------------------------------
SIZES_A = [(100, 152), (50, 76), (25, 38), (13, 19), (7, 10)]          # an 800 x 1216 input of configs/boxinst
STRIDES_A = [8, 16, 32, 64, 128]
RANGES_A = [(-1.0, 64.0), (64.0, 128.0), (128.0, 256.0), (256.0, 512.0), (512.0, 1e8)]
CANVAS_A = (800, 1216)
SEED_A = 7
COMBOS = sorted(SPEC['cases'])                                          # center_sampling on / off by norm_on_bbox on / off


def _draw(rng, n, lo, hi):
    """n boxes of side lo..hi inside the canvas: uniform draws cast to float32, on no pixel grid."""
    H, W = CANVAS_A
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def config_case():
    """B = 4 on SIZES_A: 70 shuffled boxes of three sizes, 3 boxes, none, and one box over the whole canvas."""
    rng = np.random.default_rng(SEED_A)
    img0 = np.concatenate([_draw(rng, 50, 12, 120), _draw(rng, 15, 100, 400), _draw(rng, 5, 400, 790)])
    img0 = img0[rng.permutation(len(img0))]
    img1 = _draw(rng, 3, 100, 400)
    img3 = np.array([[0.5, 0.25, 1215.5, 799.75]], np.float32)
    c = _case(SIZES_A, STRIDES_A, RANGES_A, [img0, img1, np.zeros((0, 4), np.float32), img3])
    assert not bool((c['boxes'][0] * 8 == (c['boxes'][0] * 8).round()).all(1).any())           # no box on the 1/8-pixel grid
    return c


def config_settings(name, **over):
    return settings(name, STRIDES_A, RANGES_A, **over)


@functools.lru_cache(maxsize=None)
def config_want(name, dtype=torch.float32):
    return ref_targets(config_case(), config_settings(name), dtype)


def stats_of(want32):
    """(positives, the float64 sum of the float32 centerness targets rounded once to float32)."""
    return float((want32['gt_inds'] >= 0).sum()), float(want32['ctr_targets'].double().sum().float())


# ---- B: tile, chunk and image-count edges --------------------------------------------------------------------------------------
SIZES_TILE = [(16, 16), (1, 257), (3, 85), (2, 256), (1, 511)]          # 256, 257, 255, 512, 511 locations


@functools.lru_cache(maxsize=None)
def tile_case():
    """Image 0: one box over every location of every level; image 1: none; image 2: the same box and a smaller one over x < 1030.7, which
    wins there (every level but the two narrow ones is split, the multi-tile ones inside a tile)."""
    everything = [-3.25, -1.5, 4090.75, 130.5]                          # the locations reach x = 510.5 * 8 and y = 15.5 * 8
    return _case(SIZES_TILE, [8] * 5, [WIDE] * 5, [[everything], [], [everything, [-2.75, -1.25, 1030.7, 129.3]]])


def tile_settings(norm_on_bbox):
    return settings('box_norm_ioulog' if norm_on_bbox else 'box_pix_ioulog', [8] * 5, [WIDE] * 5)


CHUNK_SIZE = (40, 40)                                                   # 1600 locations: 7 tiles, the last holds 64
CHUNK_ARRANGEMENTS = ('winner_in_last_chunk', 'tie_across_the_boundary', 'alternating')
ALTERNATING_CHUNKS = (1, 2, 0, 1, 0, 1, 0)                              # the chunk that wins tile t
_SLOTS = {0: [63, 1, 31, 62, 2, 32, 61, 3, 33], 1: [64, 127, 96, 65, 126, 97, 66, 125, 98], 2: [130, 128, 129]}


def _tile_rectangles(t, W, n):
    """The locations [256 t, min(256 t + 256, n)) of a W-wide plane as up to three (row0, row1, col0, col1) rectangles, ends inclusive."""
    a, b = t * LOC_TILE, min((t + 1) * LOC_TILE, n) - 1
    ra, ca, rb, cb = a // W, a % W, b // W, b % W
    if ra == rb:
        return [(ra, ra, ca, cb)]
    out = []
    if ca:
        out.append((ra, ra, ca, W - 1))
        ra += 1
    if cb != W - 1:
        out.append((rb, rb, 0, cb))
        rb -= 1
    if ra <= rb:
        out.append((ra, rb, 0, W - 1))
    return out


@functools.lru_cache(maxsize=None)
def chunk_case(arrangement):
    """One image on a 40 x 40 level of stride 8.  GT_CHUNK + 1 boxes with the winner last, or with two boxes of equal area on either side
    of the chunk boundary (the two arrangements of test_more_boxes_than_one_chunk, off the pixel grid); or 2 * GT_CHUNK + 3 boxes in
    which every tile's locations lie in small boxes of ONE chunk, ALTERNATING_CHUNKS[tile], under fillers that cover everything."""
    H, W = CHUNK_SIZE
    filler = [0.25, 0.5, 319.75, 319.5]
    if arrangement == 'alternating':
        n = 2 * GT_CHUNK + 3
        b = np.tile(np.array([filler], np.float64), (n, 1))
        slots = {k: list(v) for k, v in _SLOTS.items()}
        for t, k in enumerate(ALTERNATING_CHUNKS):
            for r0, r1, c0, c1 in _tile_rectangles(t, W, H * W):
                b[slots[k].pop(0)] = [8 * c0 + 0.3, 8 * r0 + 0.7, 8 * c1 + 7.6, 8 * r1 + 7.2]
    else:
        n = GT_CHUNK + 1
        b = np.tile(np.array([filler], np.float64), (n, 1))
        if arrangement == 'winner_in_last_chunk':
            b[n - 1] = [1.5, 1.25, 318.5, 318.75]
        else:
            b[n - 2], b[n - 1] = [2.5, 1.25, 318.5, 318.75], [3.5, 1.25, 319.5, 318.75]
    return _case([CHUNK_SIZE], [8], [WIDE], [b])


def chunk_settings():
    return settings('box_pix_ioulog', [8], [WIDE])


SIZES_MANY, STRIDES_MANY = [(3, 5), (17, 16)], [32, 8]                  # 15 and 272 locations: one tile and two
IMAGES_WITH_BOXES = (0, 31, MAX_IMAGES - 1)


@functools.lru_cache(maxsize=None)
def many_images_case():
    """B = BXI_MAX_IMAGES; boxes in images 0 (two), 31 (three) and 63 (two: global indices 5 and 6) only."""
    boxes = [np.zeros((0, 4), np.float32) for _ in range(MAX_IMAGES)]
    boxes[0] = [[3.3, 2.1, 120.7, 90.4], [40.6, 50.2, 127.9, 135.1]]
    boxes[31] = [[0.4, 0.6, 60.3, 70.9], [50.5, 10.1, 110.2, 100.8], [20.2, 80.7, 125.5, 133.3]]
    boxes[MAX_IMAGES - 1] = [[1.1, 1.3, 126.6, 64.4], [2.7, 60.9, 127.2, 134.8]]
    return _case(SIZES_MANY, STRIDES_MANY, [WIDE] * 2, boxes)


def many_images_settings():
    return settings('box_norm_ioulog', STRIDES_MANY, [WIDE] * 2)


# ---- C: losses and gradients over many tiles -----------------------------------------------------------------------------------
LOSS_CASES = ('cs_norm_giou', 'box_pix_ioulog')                         # gamma == 2 with GIoU; the general gamma (1.5) with IoU log
PLANTS = (30.0, -30.0, 90.0, -90.0, 200.0, -200.0)
SEED_MAPS = 11
UPSTREAM = (0.5, 3.0, 512.0)


def level_slices(sizes, B):
    at, out = 0, []
    for h, w in sizes:
        out.append(slice(at, at + B * h * w))
        at += B * h * w
    return out


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """The seeded maps of ``R.make_inputs`` on SIZES_A with +-30, +-90 and +-200 planted in the cls maps of levels 0 and 1: at flat
    elements 0, 1023, 1024, the last, and either side of the boundary between images 0 and 1 (negative elements unless a label falls
    there), on six positive elements (the first and the last, the ones nearest that image boundary, the ones nearest the start and the
    end of a 1024-element tile; others from the middle where these coincide) and on six other negative ones."""
    c = config_case()
    B, C = c['B'], c['C']
    maps = R.make_inputs(dict(levels=SIZES_A, num_classes=C, gt_bboxes=[None] * B), SEED_MAPS)
    labels = config_want(name)['labels'].numpy()
    planted = []
    for l, sl in zip((0, 1), level_slices(SIZES_A, B)):
        hw = SIZES_A[l][0] * SIZES_A[l][1]
        lab = labels[sl].reshape(B, hw)
        flat = maps['cls'][l].reshape(-1)
        onehot = np.zeros((B, C, hw), bool)
        bb, yx = np.nonzero(lab < C)
        onehot[bb, lab[bb, yx], yx] = True
        onehot = onehot.reshape(-1)
        pos = np.flatnonzero(onehot)
        edge = C * hw                                                   # first element of image 1
        below, above = pos[pos < edge], pos[pos >= edge]
        wanted = [pos[0], pos[-1], below[-1], above[0] if len(above) else pos[len(pos) // 2], pos[np.argmin(pos % ELEM_TILE)],
                  pos[np.argmax(pos % ELEM_TILE)], pos[len(pos) // 3], pos[2 * len(pos) // 3], pos[len(pos) // 5], pos[len(pos) // 7]]
        picks = list(dict.fromkeys(int(e) for e in wanted))[:6]
        fixed = [0, ELEM_TILE - 1, ELEM_TILE, flat.size - 1, edge - 1, edge]
        rng = np.random.default_rng(100 + l)
        neg = [int(e) for e in rng.permutation(np.flatnonzero(~onehot))[:6]]
        seen = set()
        for group in (picks, fixed, neg):
            for i, e in enumerate(group):
                if int(e) in seen:
                    continue
                seen.add(int(e))
                flat[int(e)] = PLANTS[i]
                planted.append((l, int(e), PLANTS[i], bool(onehot[int(e)])))
    return dict(maps=maps, planted=planted)


def maps_from_targets(bbox_targets, sizes, B):
    """bbox maps [B,4,H,W] per level that predict exactly the target on every location (``bbox_targets``: [N,4] numpy, training order)."""
    out = []
    for (h, w), sl in zip(sizes, level_slices(sizes, B)):
        out.append(np.ascontiguousarray(bbox_targets[sl].reshape(B, h * w, 4).transpose(0, 2, 1).reshape(B, 4, h, w)))
    return out
