"""A torch restatement of the box head's training step for the tests (CPU or GPU tensors, float32 or float64; autograd supplies the
gradients): the FCOS target assignment of ``CondInstBoxHead.get_targets`` and the three losses of ``CondInstBoxHead.loss``, with the
library's two rules where the reference leaves a choice or fails -- the lowest box index wins among equal minimal areas, and an image
without boxes is all background.  It holds only what the GPU tests need; tests/golden/make_golden_box_head_loss.py checks it against
the reference's own functions, and tests/golden/box_head_loss.npz holds what those gave.

Order of every flattened result: level-major, then image, then y, then x."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, 'golden', 'box_head_loss_cases.json')
GOLDEN = os.path.join(HERE, 'golden', 'box_head_loss.npz')
INF = 1e8
F32_EPS = float(torch.finfo(torch.float32).eps)          # weight_reduce_loss: sum / (avg_factor + eps)
TARGET_KEYS = ('labels', 'bbox_targets', 'gt_inds', 'points', 'level_inds', 'img_inds', 'ctr_targets')


def load_cases():
    with open(CASES_JSON) as fh:
        return json.load(fh)


def head_cfg(spec, name):
    """The ``bbox_head`` block of case ``name``: the shared part of the file plus the case's own keys."""
    cfg = dict(type='CondInstBoxHead', num_classes=spec['num_classes'], strides=spec['strides'], regress_ranges=spec['regress_ranges'],
               center_sample_radius=spec['center_sample_radius'])
    cfg.update(spec['cases'][name])
    return cfg


def make_inputs(spec, seed):
    """Seeded predictions: cls and centerness logits are normal draws, the distances are relu of a shifted normal draw (exact zeros occur,
    as after the head's relu)."""
    rng = np.random.default_rng(seed)
    B, C = len(spec['gt_bboxes']), spec['num_classes']
    out = {'cls': [], 'bbox': [], 'ctr': []}
    for h, w in spec['levels']:
        out['cls'].append((rng.standard_normal((B, C, h, w)) * 2.0 - 2.0).astype(np.float32))
        out['bbox'].append(np.maximum(rng.standard_normal((B, 4, h, w)) * 2.0 + 3.0, 0.0).astype(np.float32))
        out['ctr'].append(rng.standard_normal((B, 1, h, w)).astype(np.float32))
    return out


def gt_of(spec, dtype=torch.float32, device='cpu'):
    boxes = [torch.tensor(b, dtype=dtype, device=device).reshape(-1, 4) for b in spec['gt_bboxes']]
    labels = [torch.tensor(v, dtype=torch.int64, device=device) for v in spec['gt_labels']]
    return boxes, labels


def level_points(sizes, strides, dtype, device='cpu'):
    pts = []
    for (h, w), s in zip(sizes, strides):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device), indexing='ij')
        pts.append(torch.stack([(xs.reshape(-1) + 0.5) * s, (ys.reshape(-1) + 0.5) * s], -1))
    return pts


def _first_min(values):
    """(min, lowest index that holds it) along dim 1."""
    m = values.min(dim=1)[0]
    idx = torch.arange(values.shape[1], device=values.device)[None].expand_as(values)
    first = torch.where(values == m[:, None], idx, torch.full_like(idx, values.shape[1])).min(dim=1)[0]
    return m, first


def _image_targets(points, ranges, radii, boxes, labels, center_sampling, num_classes):
    """One image, all levels concatenated: labels, distances (pixels), local gt index."""
    P, G = points.shape[0], boxes.shape[0]
    if G == 0:
        return labels.new_full((P,), num_classes), boxes.new_zeros((P, 4)), labels.new_full((P,), -1)
    xs, ys = points[:, 0:1], points[:, 1:2]
    x1, y1, x2, y2 = (boxes[None, :, k] for k in range(4))
    d = torch.stack((xs - x1, ys - y1, x2 - xs, y2 - ys), -1)                  # [P,G,4] l,t,r,b
    if center_sampling:
        cx, cy, r = (x1 + x2) / 2, (y1 + y2) / 2, radii[:, None]
        xmin, ymin, xmax, ymax = cx - r, cy - r, cx + r, cy + r
        c1 = torch.where(xmin > x1, xmin, x1.expand_as(xmin))
        c2 = torch.where(ymin > y1, ymin, y1.expand_as(ymin))
        c3 = torch.where(xmax > x2, x2.expand_as(xmax), xmax)
        c4 = torch.where(ymax > y2, y2.expand_as(ymax), ymax)
        inside = torch.stack((xs - c1, ys - c2, c3 - xs, c4 - ys), -1).min(-1)[0] > 0
    else:
        inside = d.min(-1)[0] > 0
    far = d.max(-1)[0]
    in_range = (far >= ranges[:, 0:1]) & (far <= ranges[:, 1:2])
    area = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[None].repeat(P, 1)
    area = torch.where(inside & in_range, area, torch.full_like(area, INF))
    best, idx = _first_min(area)
    bg = best == INF
    lab = torch.where(bg, torch.full_like(labels[idx], num_classes), labels[idx])
    return lab, d[torch.arange(P, device=d.device), idx], torch.where(bg, torch.full_like(idx, -1), idx)


def centerness(t):
    lr, tb = t[:, [0, 2]], t[:, [1, 3]]
    v = (lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0])
    # a correctly rounded float32 root (through float64, rounded once): torch's own float32 sqrt is an ulp off in some CPU builds
    return torch.sqrt(v.double()).float() if v.dtype == torch.float32 else torch.sqrt(v)


def targets(sizes, strides, gt_bboxes, gt_labels, regress_ranges, center_sampling, center_sample_radius, norm_on_bbox, num_classes,
            dtype=torch.float32):
    """dict of TARGET_KEYS + 'stats' (number of positives, centerness sum; float64) in training order."""
    dev = gt_bboxes[0].device
    B = len(gt_bboxes)
    pts = level_points(sizes, strides, dtype, dev)
    n_pts = [p.shape[0] for p in pts]
    allp = torch.cat(pts)
    ranges = torch.cat([torch.tensor(r, dtype=dtype, device=dev)[None].expand(n, 2) for r, n in zip(regress_ranges, n_pts)])
    radii = torch.cat([torch.full((n,), float(s * center_sample_radius), dtype=dtype, device=dev) for s, n in zip(strides, n_pts)])
    per_img, cum = [], 0
    for b in range(B):
        lab, d, gi = _image_targets(allp, ranges, radii, gt_bboxes[b].to(dtype), gt_labels[b], center_sampling, num_classes)
        gi = torch.where(gi >= 0, gi + cum, gi)
        cum += gt_bboxes[b].shape[0]
        per_img.append((lab.split(n_pts), d.split(n_pts), gi.split(n_pts)))
    out = {k: [] for k in TARGET_KEYS}
    for l, (n, s) in enumerate(zip(n_pts, strides)):
        for b in range(B):
            lab, d, gi = (per_img[b][k][l] for k in range(3))
            d = d / s if norm_on_bbox else d
            pos = gi >= 0
            ct = torch.zeros(n, dtype=dtype, device=dev)
            if bool(pos.any()):
                ct[pos] = centerness(d[pos])
            for k, v in zip(TARGET_KEYS, (lab, d, gi, pts[l], torch.full((n,), l, dtype=torch.int64, device=dev),
                                          torch.full((n,), b, dtype=torch.int64, device=dev), ct)):
                out[k].append(v)
    out = {k: torch.cat(v) for k, v in out.items()}
    out['stats'] = torch.stack([(out['gt_inds'] >= 0).sum().double(), out['ctr_targets'].double().sum()])
    return out


def flatten_maps(maps):
    return torch.cat([m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]) for m in maps])


def decode(points, dist):
    return torch.stack([points[:, 0] - dist[:, 0], points[:, 1] - dist[:, 1], points[:, 0] + dist[:, 2], points[:, 1] + dist[:, 3]], -1)


def aligned_overlaps(a, b, giou, eps):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    e = overlap.new_tensor([eps])
    union = torch.max(area_a + area_b - overlap, e)
    iou = overlap / union
    if not giou:
        return iou
    ewh = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    earea = torch.max(ewh[:, 0] * ewh[:, 1], e)
    return iou - (earea - union) / earea


def bbox_loss_elements(pred, target, kind, eps):
    if kind == 'giou':
        return 1 - aligned_overlaps(pred, target, True, eps)
    iou = aligned_overlaps(pred, target, False, 1e-6).clamp(min=eps)
    return {'iou_log': lambda: -iou.log(), 'iou_linear': lambda: 1 - iou, 'iou_square': lambda: 1 - iou ** 2}[kind]()


def focal_elements(pred, onehot, gamma, alpha):
    p = pred.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    w = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    return F.binary_cross_entropy_with_logits(pred, onehot, reduction='none') * w


def losses(cls, bbox, ctr, tg, s, norm=None):
    """(loss_cls, loss_bbox, loss_centerness) of the per-level maps (any float dtype; they may require grad) for targets ``tg`` (a dict
    of TARGET_KEYS or an object with those attributes) and flat settings ``s`` (what parse_box_head_cfg returns)."""
    get = (lambda k: tg[k]) if isinstance(tg, dict) else (lambda k: getattr(tg, k))
    dtype = cls[0].dtype
    C = cls[0].shape[1]
    fc, fb, fn = flatten_maps(cls), flatten_maps(bbox), flatten_maps(ctr).reshape(-1)
    labels = get('labels')
    pos = ((labels >= 0) & (labels < C)).nonzero().reshape(-1)
    ct = get('ctr_targets').to(dtype)[pos]
    if norm is None:
        norm = (float(len(pos)), float(ct.double().sum()))
    # the reference keeps num_pos as a float32 tensor, so "avg_factor + eps" is a float32 sum there in every run; the centerness sum
    # has the run's dtype
    num_pos = float(torch.tensor(max(float(norm[0]), 1.0), dtype=torch.float32) + F32_EPS)
    denorm = max(float(norm[1]), 1e-6) + F32_EPS
    onehot = F.one_hot(labels, C + 1)[:, :C].to(dtype)
    loss_cls = s['loss_weight_cls'] * focal_elements(fc, onehot, s['gamma'], s['alpha']).sum() / num_pos
    if len(pos) == 0:
        return loss_cls, fb[pos].sum(), fn[pos].sum()
    pts = get('points').to(dtype)[pos]
    el = bbox_loss_elements(decode(pts, fb[pos]), decode(pts, get('bbox_targets').to(dtype)[pos]), s['bbox_loss_kind'], s['eps'])
    loss_bbox = s['loss_weight_bbox'] * (el * ct).sum() / denorm
    loss_ctr = s['loss_weight_centerness'] * F.binary_cross_entropy_with_logits(fn[pos], ct, reduction='none').sum() / num_pos
    return loss_cls, loss_bbox, loss_ctr


def losses_and_grads(maps_np, tg, s, dtype=torch.float64, device='cpu', norm=None):
    """Three losses (python floats... as 0-d tensors) and the gradient of EACH loss w.r.t. its own maps: (losses [3], grad_cls, grad_bbox,
    grad_ctr), the gradients as lists per level."""
    t = lambda k: [torch.as_tensor(m).to(device=device, dtype=dtype).clone().requires_grad_(True) for m in maps_np[k]]   # noqa: E731
    cls, bbox, ctr = t('cls'), t('bbox'), t('ctr')
    out = losses(cls, bbox, ctr, tg, s, norm)
    grads = []
    for loss, maps in zip(out, (cls, bbox, ctr)):
        g = torch.autograd.grad(loss, maps, allow_unused=True, retain_graph=True) if loss.requires_grad else [None] * len(maps)
        grads.append([torch.zeros_like(m) if gi is None else gi for gi, m in zip(g, maps)])
    return torch.stack([o.detach() for o in out]), grads[0], grads[1], grads[2]
