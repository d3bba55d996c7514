"""The cases of tests/test_gpu_bls_loss.py, built without a device so that tests/test_host_bls_loss.py can take their census: seeded
inputs in the layout ``box_solov2_mask_losses`` takes (per level the logits of the set cells in (image, cell) order, the level's compact
uint8 target planes, ``tgt_of`` / ``img_of`` per row, the host counts per (level, image)), comb trees unless the case lets the context
build its own, and the fp32 / fp64 restatements of tests/bls_loss_ref.py (computed once per case and process, shared by the tests,
never modified).

The smallest shapes that reach each path of csrc/boxlevelset_loss.hip.  A workgroup serves a chunk of LPC = max(1, 1024 // w) lines of
one row (include/boxinst/boxinst_hip_bls.h), which is the only dispatch boundary the kernels have: there is no vector path."""
import functools

import numpy as np
import torch

from tests import bls_loss_ref as R

CHUNK_PIXELS = 1024                                     # BXI_BLS_CHUNK_PIXELS
THREE = dict(B=2, sizes=[(24, 40), (24, 40), (12, 20), (6, 10), (6, 10)], rows=[[3, 2], [1, 0], [2, 2], [0, 0], [1, 3]], Cf=5)
# name -> B, the levels' sizes, rows per (level, image), feature channels, and what the case is for
CASES = {
    'three_groups': dict(THREE, own_trees=True),       # a level without rows, an image without rows in a level, a group in two input segments
    'odd':          dict(B=2, sizes=[(25, 37), (13, 19)], rows=[[2, 1], [1, 2]], Cf=2),             # tail lanes in every line
    'empty_target': dict(B=1, sizes=[(12, 20), (6, 10)], rows=[[2], [2]], Cf=1, empty=True),       # pixel_num clamp, 1e-5 clamps
    'tree_edge':    dict(B=1, sizes=[(100, 102), (101, 102)], rows=[[2], [2]], Cf=1),              # V = kTfMaxV and kTfMaxV + 102
    'many_rows':    dict(B=2, sizes=[(8, 8), (8, 8), (16, 16)], rows=[[20, 15], [18, 17], [1, 2]], Cf=2),     # 70 rows of 8x8 + 3 of 16x16
    'inert':        dict(THREE, own_trees=True, inert=((0, 1, 'tgt'), (2, 3, 'img'), (4, 0, 'both'))),        # (level, row, which index is -1)
    'no_rows':      dict(B=2, sizes=[(12, 20), (6, 10)], rows=[[0, 0], [0, 0]], Cf=1),
    'chunk_edge':   dict(B=1, sizes=[(25, 40), (26, 40)], rows=[[2], [1]], Cf=1),                  # h = LPC and h = LPC + 1 (h = LPC - 1: three_groups)
    'wide':         dict(B=1, sizes=[(3, 1024), (3, 1025)], rows=[[1], [2]], Cf=1),                # 1024 // w = 1 and = 0 (clamped to one line)
}
LOSS_BOXPRO_WEIGHT, LOSS_LEVELSET_WEIGHT = 3.0, 1.0     # configs/boxlevelset/*: loss_boxpro, loss_levelset
GT_PER_IMAGE = 3


def lines_per_chunk(w):
    return max(1, CHUNK_PIXELS // w)


def groups_of(sizes):
    """The distinct sizes in order of first appearance and the group of every level."""
    distinct = list(dict.fromkeys(tuple(s) for s in sizes))
    return distinct, [distinct.index(tuple(s)) for s in sizes]


def comb_tree(h, w, spine):
    """A spanning tree of the h x w grid out of grid edges: a spine along column 0 ('col') or line 0 ('row') and one tooth per line /
    column.  int32 [h*w - 1, 2]; depth h + w - 2, at most two children per vertex."""
    ids = np.arange(h * w, dtype=np.int32).reshape(h, w)
    if spine == 'col':
        e = [np.stack([ids[:-1, 0], ids[1:, 0]], 1), np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1)]
    else:
        e = [np.stack([ids[0, :-1], ids[0, 1:]], 1), np.stack([ids[:-1, :].ravel(), ids[1:, :].ravel()], 1)]
    return np.concatenate(e).astype(np.int32)


def _planes(rng, g, h, w):
    m = np.zeros((g, h, w), np.uint8)
    for k in range(g):
        bh, bw = rng.integers(max(h // 4, 1), max(h // 2, 2) + 1), rng.integers(max(w // 4, 1), max(w // 2, 2) + 1)
        y, x = rng.integers(0, h - bh + 1), rng.integers(0, w - bw + 1)
        m[k, y:y + bh, x:x + bw] = 1
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of numpy inputs: norm_img [B,3,H,W], lst_feat [B,Cf,h0,w0], ins_preds (L x [N_l,h_l,w_l]), masks (L x uint8 [G,h_l,w_l], one
    array per size), tgt_of / img_of (L x int64 [N_l]), counts [l][b], level_sizes, trees (per distinct size (img, lst) [B,V-1,2]) or None."""
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, 'three_groups' if name == 'inert' else name)))
    B, sizes, rows, Cf = c['B'], c['sizes'], c['rows'], c['Cf']
    distinct, group = groups_of(sizes)
    h0, w0 = sizes[0]
    H, W = 2 * h0, 2 * w0
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([np.stack([np.sin(yy / (5.0 + ch + b)) + np.cos(xx / (7.0 + ch)) for ch in range(3)]) for b in range(B)])
    img = (img + 0.3 * rng.standard_normal(img.shape)).astype(np.float32)
    lst = rng.standard_normal((B, Cf, h0, w0)).astype(np.float32)
    G = GT_PER_IMAGE * B
    planes = [_planes(rng, G, h, w) for h, w in distinct]
    if c.get('empty'):
        for p in planes:
            p[0], p[1] = 0, 1                              # ground truth 0: no pixel at all; ground truth 1: every pixel
    preds, tgt_of, img_of = [], [], []
    for l, (h, w) in enumerate(sizes):
        n = sum(rows[l])
        x = (2.0 * rng.standard_normal((n, h, w))).astype(np.float32)
        i_of = np.concatenate([np.full(rows[l][b], b, np.int64) for b in range(B)]) if n else np.zeros(0, np.int64)
        t_of = (GT_PER_IMAGE * i_of + rng.integers(0, 2, n)).astype(np.int64)              # two of an image's three: rows share ground truths
        if c.get('empty'):
            # +-30 with a unique offset per pixel (multiples of 2^-17, the spacing of fp32 at 30 is 2^-19): the scores saturate, no logits tie
            sign = [rng.choice([-1.0, 1.0], (h, w)), -np.ones((h, w))] if l == 0 else [np.ones((h, w)), rng.choice([-1.0, 1.0], (h, w))]
            jitter = [rng.permutation(h * w).reshape(h, w) * 2.0 ** -17 for _ in range(n)]
            x = np.stack([30.0 * s + j for s, j in zip(sign, jitter)]).astype(np.float32)
            t_of = np.array([0, 1] if l == 0 else [1, 1], np.int64)
        preds.append(x)
        tgt_of.append(t_of)
        img_of.append(i_of)
    for l, r, which in c.get('inert', ()):
        if which in ('tgt', 'both'):
            tgt_of[l][r] = -1
        if which in ('img', 'both'):
            img_of[l][r] = -1
    trees = None
    if not c.get('own_trees'):
        trees = [(np.repeat(comb_tree(h, w, 'col')[None], B, 0), np.repeat(comb_tree(h, w, 'row')[None], B, 0)) for h, w in distinct]
    return dict(norm_img=img, lst_feat=lst, ins_preds=preds, masks=[planes[g] for g in group], tgt_of=tgt_of, img_of=img_of,
                counts=[list(r) for r in rows], level_sizes=[tuple(s) for s in sizes], trees=trees, B=B)


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name):
    """The per-row restatement (tests/bls_loss_ref.all_levels) in 'float32' or 'float64', upstream gradients of one for both losses."""
    d = inputs(name)
    return R.all_levels(d['ins_preds'], d['masks'], d['tgt_of'], d['img_of'], d['norm_img'], d['lst_feat'], d['level_sizes'],
                        getattr(torch, dtype_name), d['trees'], LOSS_BOXPRO_WEIGHT, LOSS_LEVELSET_WEIGHT)
