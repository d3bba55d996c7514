"""The cases of tests/test_gpu_b2m_loss.py, built without a device so that tests/test_host_b2m_loss.py can take their census: seeded
inputs, a synthetic one-to-one assignment per layer in the layout of ``MaskHungarianAssigner.assign_batch`` (per image min(Q, G_i)
slots, matched queries ascending, -1 for an inert image), and the fp32 / fp64 restatements of tests/b2m_loss_ref.py (computed once per
case and process, shared by the tests, never modified)."""
import functools

import numpy as np
import torch

from tests import b2m_loss_ref as R

# name -> L, B, Q, G per image, canvas, pred, scaled_size, own trees?, and what the case is for
CASES = {
    'small':       dict(L=3, Q=6, G=(2, 4), canvas=(64, 96), pred=(17, 23), small=(12, 12)),
    'up_to_small': dict(L=2, Q=6, G=(2, 4), canvas=(64, 96), pred=(40, 56), small=(96, 96)),
    'down':        dict(L=1, Q=4, G=(1, 2), canvas=(200, 304), pred=(200, 304), small=(96, 96)),
    'q_lt_g':      dict(L=2, Q=2, G=(3, 1), canvas=(32, 40), pred=(16, 20), small=(12, 12)),
    'one_g0':      dict(L=2, Q=5, G=(0, 3), canvas=(32, 40), pred=(16, 20), small=(12, 12)),
    'all_g0':      dict(L=2, Q=5, G=(0, 0), canvas=(32, 40), pred=(16, 20), small=(12, 12)),
    'inert':       dict(L=2, Q=5, G=(2, 3), canvas=(32, 40), pred=(16, 20), small=(12, 12), inert_image=0),
    'm1':          dict(L=1, Q=3, G=(1, 0), canvas=(32, 40), pred=(16, 20), small=(12, 12)),
    'c65':         dict(L=3, Q=24, G=(22, 1), canvas=(24, 32), pred=(10, 12), small=(8, 8)),
    'zero_target': dict(L=2, Q=4, G=(2, 2), canvas=(32, 40), pred=(16, 20), small=(12, 12), empty_gt=(0, 1), big_logits=True),
    'hand':        dict(L=2, Q=3, G=(1, 2), canvas=(16, 16), pred=(16, 16), small=(16, 16), hand=True),     # every resize is the identity
    'own_trees':   dict(L=2, Q=6, G=(2, 3), canvas=(48, 64), pred=(24, 32), small=(16, 16), own_trees=True),
    'real':        dict(L=2, Q=100, G=(7, 23), canvas=(256, 256), pred=(256, 256), small=(96, 96)),
}
LOSS_BOX_WEIGHT, LOSS_MASK_WEIGHT = 5.0, 1.0            # configs/box2mask/*: loss_box, loss_mask


def _boxes(rng, g, H, W):
    m = np.zeros((g, H, W), np.float32)
    for k in range(g):
        bh, bw = rng.integers(max(H // 6, 2), max(H // 2, 3)), rng.integers(max(W // 6, 2), max(W // 2, 3))
        y, x = rng.integers(0, H - bh + 1), rng.integers(0, W - bw + 1)
        m[k, y:y + bh, x:x + bw] = 1
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of numpy inputs: norm_img [B,3,H,W], lst_feat [B,1,h,w], mask_preds (L x [B,Q,h,w]), gt_masks (B x [G_i,H,W]),
    pos / pos_gt (L x int64 [S], -1 in the inert image's slots), counts, trees (img, lst) or None."""
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    L, Q, G, (H, W), (h, w), small = c['L'], c['Q'], c['G'], c['canvas'], c['pred'], c['small']
    B = len(G)
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([np.stack([np.sin(yy / (5.0 + ch + b)) + np.cos(xx / (7.0 + ch)) for ch in range(3)]) for b in range(B)])
    img = (img + 0.3 * rng.standard_normal(img.shape)).astype(np.float32)
    lst = rng.standard_normal((B, 1, h, w)).astype(np.float32)
    gts = [_boxes(rng, g, H, W) for g in G]
    for k in c.get('empty_gt', ()):
        gts[k][0] = 0                                                      # a ground truth whose resized target is all zero
    scale = 100.0 if c.get('big_logits') else 2.0
    preds = [(scale * rng.standard_normal((B, Q, h, w))).astype(np.float32) for _ in range(L)]
    if c.get('hand'):
        preds = [np.zeros((B, Q, h, w), np.float32) for _ in range(L)]
        img = np.full_like(img, 0.25)
    n = [min(Q, g) for g in G]
    pos, pos_gt = [], []
    for l in range(L):
        p, g = [], []
        for i in range(B):
            q = np.sort(rng.choice(Q, n[i], replace=False))
            t = rng.permutation(G[i])[:n[i]]
            if c.get('inert_image') == i:
                q, t = np.full(n[i], -1), np.full(n[i], -1)
            p.append(q)
            g.append(t)
        pos.append(np.concatenate(p).astype(np.int64))
        pos_gt.append(np.concatenate(g).astype(np.int64))
    trees = None
    if not c.get('own_trees'):
        im = torch.from_numpy(img)
        lf = torch.from_numpy(lst)
        r = lambda t, s: torch.nn.functional.interpolate(t, size=s, mode='bilinear', align_corners=False)
        trees = (R.mst_trees(r(r(im, (h, w)), small)), R.mst_trees(r(r(lf, (h, w)), small)))
    return dict(norm_img=img, lst_feat=lst, mask_preds=preds, gt_masks=gts, pos=pos, pos_gt=pos_gt, counts=list(G), trees=trees, B=B, n=n)


def live_lists(name):
    """pos / pos_gt of `inputs` as the restatement takes them: [l][i] -> the live slots of image i."""
    d = inputs(name)
    off = np.concatenate([[0], np.cumsum(d['n'])])
    cut = lambda a: [[int(v) for v in a[off[i]:off[i + 1]] if v >= 0] for i in range(d['B'])]
    return [cut(p) for p in d['pos']], [cut(g) for g in d['pos_gt']]


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name):
    """The per-instance restatement of all layers in 'float32' or 'float64' (tests/b2m_loss_ref.all_layers) with all-ones upstream gradients."""
    d = inputs(name)
    pos, pos_gt = live_lists(name)
    return R.all_layers(d['mask_preds'], d['lst_feat'], d['norm_img'], d['gt_masks'], pos, pos_gt, getattr(torch, dtype_name),
                        CASES[name]['small'], d['trees'], LOSS_BOX_WEIGHT, LOSS_MASK_WEIGHT)
