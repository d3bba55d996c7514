"""A torch / NumPy restatement of the SOLOv2-style heads' training targets and category loss for the tests:
``DiscoBoxSOLOv2Head.solov2_target_single`` (mode 'discobox'), ``BoxSOLOv2Head.solo_target_single`` (mode 'boxlevelset') and
``loss_cate``, with the library's rules where the reference leaves a choice or needs what is not here -- ``mmcv.imrescale`` is the
restated 2-of-4 rule (:func:`rescale`; unpinned: OpenCV itself never ran), the centre comes from the exact integer moments, an image
without boxes is all background.  It holds only what the tests need; tests/golden/make_golden_solo_targets.py checks it against the
reference's own functions, and tests/golden/solo_targets.npz holds what those gave.

Order of every flattened per-cell result: level-major, then image, then y, then x."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, 'golden', 'solo_targets_cases.json')
CFG_JSON = os.path.join(HERE, 'golden', 'solo_head_cfg.json')
GOLDEN = os.path.join(HERE, 'golden', 'solo_targets.npz')
F32_EPS = float(torch.finfo(torch.float32).eps)          # weight_reduce_loss: sum / (avg_factor + eps)
RESCALE_MIN_ONES = 2                                     # ones among the four sampled pixels for a 1 (0.5 rounds up)
MIN_MASK_SUM = 10                                        # box_solov2_head.py: `if seg_mask.sum() < 10: continue`
MODES = ('discobox', 'boxlevelset')
HEAD_TYPE = {'discobox': 'DiscoBoxSOLOv2Head', 'boxlevelset': 'BoxSOLOv2Head'}
CELL_KEYS = ('cate_labels', 'ins_ind_labels', 'cell_owner')


def load_cases():
    with open(CASES_JSON) as fh:
        return json.load(fh)


def head_cfg(spec, mode):
    """The ``bbox_head`` block of ``mode``: the shared part of the case file plus the mode's own loss_cate."""
    return dict(type=HEAD_TYPE[mode], num_classes=spec['num_classes'], strides=spec['strides'], scale_ranges=spec['scale_ranges'],
                sigma=spec['sigma'], num_grids=spec['num_grids'], loss_cate=spec['loss_cate'][mode])


def _axis(v):
    if isinstance(v, str):
        a, b = v.split(':')
        return np.arange(int(a), int(b))
    return np.asarray(v, dtype=np.int64)


def masks_of(case):
    """Per image uint8 [G,H,W]: every instance's mask is the union of its parts, each a product set rows x cols ('a:b' = range)."""
    out = []
    for img in case['images']:
        H, W = img['size']
        m = np.zeros((len(img['instances']), H, W), np.uint8)
        for g, inst in enumerate(img['instances']):
            for part in inst['mask']:
                m[g][np.ix_(_axis(part['rows']), _axis(part['cols']))] = 1
        out.append(m)
    return out


def gt_of(case, device='cpu'):
    boxes = [torch.tensor([i['box'] for i in img['instances']], dtype=torch.float32, device=device).reshape(-1, 4) for img in case['images']]
    labels = [torch.tensor([i['label'] for i in img['instances']], dtype=torch.int64, device=device) for img in case['images']]
    return boxes, labels


def level_planes(spec, mode):
    """(factor, (h, w)) of every level: DiscoBox rescales by 4 onto the mask feature map, BoxLevelSet by stride / 2."""
    h, w = spec['mask_feat_size']
    if mode == 'discobox':
        return [(4, (h, w))] * len(spec['strides'])
    return [(s // 2, (4 * h // (s // 2), 4 * w // (s // 2))) for s in spec['strides']]


def rescale(mask, f):
    """``mmcv.imrescale(mask, 1 / f)`` for an even f, restated: output (r, c) samples source rows f r + f/2 - 1, f r + f/2 and the same
    two columns with weight 1/2 each, and is 1 where at least RESCALE_MIN_ONES of the four are 1."""
    m = (np.asarray(mask) != 0).astype(np.int32)
    a = f // 2 - 1
    s = m[..., a::f, a::f] + m[..., a::f, a + 1::f] + m[..., a + 1::f, a::f] + m[..., a + 1::f, a + 1::f]
    return (s >= RESCALE_MIN_ONES).astype(np.uint8)


def sampled_sums(mask, f):
    m = (np.asarray(mask) != 0).astype(np.int32)
    a = f // 2 - 1
    return m[..., a::f, a::f] + m[..., a::f, a + 1::f] + m[..., a + 1::f, a::f] + m[..., a + 1::f, a + 1::f]


def moments(masks):
    """int64 [G,3]: m00, m10 (x), m01 (y), exact."""
    m = (np.asarray(masks) != 0).astype(np.int64)
    ys, xs = np.arange(m.shape[1], dtype=np.int64), np.arange(m.shape[2], dtype=np.int64)
    return np.stack([m.sum((1, 2)), (m * xs[None, None, :]).sum((1, 2)), (m * ys[None, :, None]).sum((1, 2))], 1)


def _cell32(v, size, S):
    return int((v / size) // (1. / S))                   # v: 0-dim float32 tensor -> torch's fp32 floor division


def _window(mode, box, mom, S, canvas, sigma):
    """The (top, down, left, right) window of one valid instance on a grid of S."""
    half_w, half_h = 0.5 * (box[2] - box[0]) * sigma, 0.5 * (box[3] - box[1]) * sigma          # 0-dim float32 tensors
    m00, m10, m01 = (int(v) for v in mom)
    if mode == 'discobox':
        cw, ch = torch.tensor(float(m10), dtype=torch.float32) / float(m00), torch.tensor(float(m01), dtype=torch.float32) / float(m00)
        coord_w, coord_h = _cell32(cw, canvas[1], S), _cell32(ch, canvas[0], S)
    else:
        cwd, chd = m10 / m00, m01 / m00                   # Python doubles, as scipy's center_of_mass
        coord_w, coord_h = int((cwd / canvas[1]) // (1. / S)), int((chd / canvas[0]) // (1. / S))
        cw, ch = torch.tensor(cwd, dtype=torch.float32), torch.tensor(chd, dtype=torch.float32)     # double - fp32 tensor: fp32
    top_box = max(0, _cell32(ch - half_h, canvas[0], S))
    down_box = min(S - 1, _cell32(ch + half_h, canvas[0], S))
    left_box = max(0, _cell32(cw - half_w, canvas[1], S))
    right_box = min(S - 1, _cell32(cw + half_w, canvas[1], S))
    return max(top_box, coord_h - 1), min(down_box, coord_h + 1), max(coord_w - 1, left_box), min(right_box, coord_w + 1)


def targets(mode, boxes, labels, masks, *, num_grids, scale_ranges, sigma, num_classes, canvas, mom=None):
    """Both target functions over a batch.  ``boxes`` / ``labels``: per image float32 [G,4] / int64 [G] (CPU); ``masks``: per image uint8
    [G,H,W] arrays.  Returns flat ``cate_labels`` (int64), ``ins_ind_labels`` (uint8), ``cell_owner`` (int32, global instance index or
    -1), and per (level, image) lists ``grid_order`` / ``pair_inst`` (the reference's grid_order and the instance of each entry) and
    ``sel_inst`` (the owner of every set cell in ascending cell order); ``moments`` int64 [G,3]; ``num_ins``."""
    B, L = len(boxes), len(num_grids)
    mom = [moments(m) for m in masks] if mom is None else mom
    offsets = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(int)
    out = {k: [] for k in CELL_KEYS}
    order, pinst, sel = [], [], []
    for l in range(L):
        S, (lo, hi) = num_grids[l], scale_ranges[l]
        order.append([]), pinst.append([]), sel.append([])
        for b in range(B):
            cate = np.full(S * S, num_classes, np.int64)
            owner = np.full(S * S, -1, np.int32)
            go, gi = [], []
            if boxes[b].shape[0]:
                bx = boxes[b].float()
                areas = torch.sqrt(((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])).double()).float()       # correctly rounded fp32 sqrt
                hit = ((areas >= lo) & (areas <= hi)).nonzero().flatten().tolist()
                for i in hit:
                    m00 = int(mom[b][i][0])
                    if (mode == 'discobox' and not m00 > 0) or (mode == 'boxlevelset' and m00 < MIN_MASK_SUM):
                        continue
                    top, down, left, right = _window(mode, bx[i], mom[b][i], S, canvas, sigma)
                    for y in range(top, down + 1):
                        for x in range(left, right + 1):
                            cate[y * S + x] = int(labels[b][i])
                            owner[y * S + x] = offsets[b] + i
                            go.append(y * S + x)
                            gi.append(offsets[b] + i)
            out['cate_labels'].append(cate)
            out['ins_ind_labels'].append((owner >= 0).astype(np.uint8))
            out['cell_owner'].append(owner)
            order[l].append(np.asarray(go, np.int64))
            pinst[l].append(np.asarray(gi, np.int64))
            sel[l].append(owner[owner >= 0].astype(np.int64))
    res = {k: np.concatenate(v) for k, v in out.items()}
    res.update(grid_order=order, pair_inst=pinst, sel_inst=sel, moments=np.concatenate(mom) if mom else np.zeros((0, 3), np.int64),
               num_ins=int(res['ins_ind_labels'].sum()))
    return res


def make_cate_inputs(spec, seed):
    """Seeded category logits, [B,C,S,S] per level."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((spec['B'], spec['num_classes'], s, s)) * 2.0 - 2.0).astype(np.float32) for s in spec['num_grids']]


def cate_loss(preds, flat_labels, num_ins, gamma, alpha, loss_weight, dtype=torch.float64):
    """(loss, [gradient per level]) of ``loss_cate(flatten_cate_preds, flatten_cate_labels, avg_factor=num_ins + 1)`` in ``dtype``."""
    maps = [torch.as_tensor(p).to(dtype).clone().requires_grad_(True) for p in preds]
    C = maps[0].shape[1]
    x = torch.cat([m.permute(0, 2, 3, 1).reshape(-1, C) for m in maps])
    t = F.one_hot(torch.as_tensor(flat_labels).long(), num_classes=C + 1)[:, :C].to(dtype)
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    w = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    # avg_factor is an int32 tensor: `avg_factor + eps` is a float32 sum whatever the dtype of the loss
    denom = float(np.float32(num_ins + 1) + np.float32(F32_EPS))
    loss = loss_weight * (F.binary_cross_entropy_with_logits(x, t, reduction='none') * w).sum() / denom
    grads = torch.autograd.grad(loss, maps)
    return loss.detach(), [g.detach() for g in grads]


def random_case(seed, n, H, W, num_classes):
    """One image of H x W with ``n`` small instances: boxes of 6..40 pixels a side, the mask a random sub-rectangle (some empty, some tiny)."""
    rng = np.random.default_rng(seed)
    boxes, labels, masks = [], [], np.zeros((n, H, W), np.uint8)
    for g in range(n):
        w, h = int(rng.integers(6, 41)), int(rng.integers(6, 41))
        x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        boxes.append([x1, y1, x1 + w, y1 + h])
        labels.append(int(rng.integers(0, num_classes)))
        kind = rng.integers(0, 10)
        if kind == 0:
            continue                                                    # an empty mask
        mh, mw = (2, 3) if kind == 1 else (int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1)))
        my, mx = y1 + int(rng.integers(0, h - mh + 1)), x1 + int(rng.integers(0, w - mw + 1))
        masks[g, my:my + mh, mx:mx + mw] = 1
    return [torch.tensor(boxes, dtype=torch.float32)], [torch.tensor(labels, dtype=torch.int64)], [masks]
