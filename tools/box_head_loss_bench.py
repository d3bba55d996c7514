#!/usr/bin/env python3
"""Developer measurement of the box head's training step on the GPU box: boxinstseg_amd.condinst_box_loss (csrc/fcos_loss.hip), forward
and backward, against the reference's op sequence written out as torch ops (condinst_head.py:365-633, :855-874 with
py_sigmoid_focal_loss, giou_loss and binary_cross_entropy_with_logits; autograd for the backward) -- same box, same inputs, calls
alternated.  The composed path is a restatement kept in this file: the loop over the images, the [points, gts] expansions, the
permute + reshape + cat of all 15 maps, ``nonzero`` and ``len(pos_inds)``.  mmcv's device focal op is not available; the composed path
uses the reference's own py_sigmoid_focal_loss formula, which is MORE launches than mmcv's one kernel: read the launch count with that
in mind.

Shape: B = 2, 800 x 1024, five levels (100x128, 50x64, 25x32, 13x16, 7x8), C = 80, 20 seeded boxes per image, the config's head
settings (centre sampling 1.5, norm_on_bbox, focal 2 / 0.25, GIoU).
  ms, ms_p25, ms_p75, ms_min, ms_max   device events around one forward + backward, over the alternated repetitions after warm-up;
                                       inputs rotate over --sets independent copies.
  launches                             device kernels of one forward + backward (torch.profiler).
  host_syncs                           synchronising calls torch reports during one forward + backward (torch.cuda.set_sync_debug_mode).
  bytes_min                            what the step must move, from the shapes: every logit and distance read once, every gradient
                                       written once, the targets written and read once.
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r11_box_head_loss_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry

B, C, G = 2, 80, 20
SIZES, STRIDES = ((100, 128), (50, 64), (25, 32), (13, 16), (7, 8)), (8, 16, 32, 64, 128)
RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))
IMG = (800, 1024)
HEAD = dict(type='CondInstBoxHead', num_classes=C, center_sampling=True, center_sample_radius=1.5, norm_on_bbox=True, strides=list(STRIDES),
            loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox=dict(type='GIoULoss', loss_weight=1.0), loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
EPS32 = float(torch.finfo(torch.float32).eps)


def points(dev):
    out = []
    for (h, w), s in zip(SIZES, STRIDES):
        x = ((torch.arange(0, w, device=dev) + 0.5) * s).float()
        y = ((torch.arange(0, h, device=dev) + 0.5) * s).float()
        yy, xx = torch.meshgrid(y, x, indexing='ij')
        out.append(torch.stack([xx.reshape(-1), yy.reshape(-1)], -1))
    return out


def target_single(boxes, labels, pts, ranges, radii):
    P, n = pts.size(0), labels.size(0)
    areas = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[None].repeat(P, 1)
    ranges = ranges[:, None, :].expand(P, n, 2)
    bx = boxes[None].expand(P, n, 4)
    xs, ys = pts[:, 0][:, None].expand(P, n), pts[:, 1][:, None].expand(P, n)
    t = torch.stack((xs - bx[..., 0], ys - bx[..., 1], bx[..., 2] - xs, bx[..., 3] - ys), -1)
    cx, cy = (bx[..., 0] + bx[..., 2]) / 2, (bx[..., 1] + bx[..., 3]) / 2
    st = radii[:, None].expand(P, n)
    cg = torch.zeros_like(bx)
    cg[..., 0] = torch.where(cx - st > bx[..., 0], cx - st, bx[..., 0])
    cg[..., 1] = torch.where(cy - st > bx[..., 1], cy - st, bx[..., 1])
    cg[..., 2] = torch.where(cx + st > bx[..., 2], bx[..., 2], cx + st)
    cg[..., 3] = torch.where(cy + st > bx[..., 3], bx[..., 3], cy + st)
    inside = torch.stack((xs - cg[..., 0], ys - cg[..., 1], cg[..., 2] - xs, cg[..., 3] - ys), -1).min(-1)[0] > 0
    far = t.max(-1)[0]
    in_range = (far >= ranges[..., 0]) & (far <= ranges[..., 1])
    areas[inside == 0] = 1e8
    areas[in_range == 0] = 1e8
    min_area, idx = areas.min(dim=1)
    lab = labels[idx]
    lab[min_area == 1e8] = C
    t = t[range(P), idx]
    idx[min_area == 1e8] = -1
    return lab, t, idx


def composed_path(s, pts):
    """The reference's loss as torch ops, then backward; returns the three losses."""
    cls, bbox, ctr = s['cls'], s['bbox'], s['ctr']
    dev = cls[0].device
    n_pts = [p.size(0) for p in pts]
    ranges = torch.cat([pts[i].new_tensor(RANGES[i])[None].expand_as(pts[i]) for i in range(len(pts))])
    radii = torch.cat([pts[i].new_full((n_pts[i],), STRIDES[i] * 1.5) for i in range(len(pts))])
    allp = torch.cat(pts)
    per = [target_single(b, l, allp, ranges, radii) for b, l in zip(s['gt_bboxes'], s['gt_labels'])]
    cum = 0
    for (_, _, gi), b in zip(per, s['gt_bboxes']):
        gi[gi != -1] += cum
        cum += b.size(0)
    labels, targets, gt_inds = [], [], []
    for i in range(len(pts)):
        labels.append(torch.cat([p[0].split(n_pts, 0)[i] for p in per]))
        targets.append(torch.cat([p[1].split(n_pts, 0)[i] for p in per]) / STRIDES[i])
        gt_inds.append(torch.cat([p[2].split(n_pts, 0)[i] for p in per]))
    fc = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, C) for c in cls])
    fb = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, 4) for c in bbox])
    fn = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in ctr])
    fl, ft = torch.cat(labels), torch.cat(targets)
    fp = torch.cat([p.repeat(B, 1) for p in pts])
    img_inds = torch.cat([torch.arange(B, device=dev).repeat_interleave(n) for n in n_pts])
    lvl_inds = torch.cat([torch.full((B * n,), i, device=dev).long() for i, n in enumerate(n_pts)])
    pos = ((fl >= 0) & (fl < C)).nonzero().reshape(-1)
    num_pos = max(torch.tensor(len(pos), dtype=torch.float, device=dev), 1.0)
    onehot = F.one_hot(fl, C + 1)[:, :C].type_as(fc)
    p = fc.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    fw = (0.25 * onehot + 0.75 * (1 - onehot)) * pt.pow(2.0)
    loss_cls = (F.binary_cross_entropy_with_logits(fc, onehot, reduction='none') * fw).sum() / (num_pos + EPS32)
    pb, pc, ptg = fb[pos], fn[pos], ft[pos]
    lr, tb = ptg[:, [0, 2]], ptg[:, [1, 3]]
    ct = torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))
    denorm = max(ct.sum().detach(), 1e-6)
    pp = fp[pos]
    dec = lambda d: torch.stack([pp[:, 0] - d[:, 0], pp[:, 1] - d[:, 1], pp[:, 0] + d[:, 2], pp[:, 1] + d[:, 3]], -1)     # noqa: E731
    a, b = dec(pb), dec(ptg)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    e = overlap.new_tensor([1e-6])
    union = torch.max(area_a + area_b - overlap, e)
    ewh = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    earea = torch.max(ewh[:, 0] * ewh[:, 1], e)
    giou = overlap / union - (earea - union) / earea
    loss_bbox = ((1 - giou) * ct).sum() / (denorm + EPS32)
    loss_ctr = F.binary_cross_entropy_with_logits(pc, ct, reduction='none').sum() / (num_pos + EPS32)
    (loss_cls + loss_bbox + loss_ctr).backward()
    return torch.stack([loss_cls, loss_bbox, loss_ctr]).detach(), (fp, lvl_inds, img_inds, torch.cat(gt_inds))


def kernel_path(s):
    import boxinstseg_amd as bx
    out = bx.condinst_box_loss(s['cls'], s['bbox'], s['ctr'], s['gt_bboxes'], s['gt_labels'], None, s['cfg'])
    losses = out[0]
    (losses['loss_cls'] + losses['loss_bbox'] + losses['loss_centerness']).backward()
    return torch.stack([losses['loss_cls'], losses['loss_bbox'], losses['loss_centerness']]).detach(), out[1:]


def make_set(dev, seed, cfg):
    g = torch.Generator(device='cpu').manual_seed(seed)
    s = dict(cls=[], bbox=[], ctr=[], gt_bboxes=[], gt_labels=[], cfg=cfg)
    for (h, w) in SIZES:
        s['cls'].append((torch.randn(B, C, h, w, generator=g) * 2 - 3).to(dev).requires_grad_(True))
        s['bbox'].append(torch.relu(torch.randn(B, 4, h, w, generator=g) * 2 + 3).to(dev).requires_grad_(True))
        s['ctr'].append(torch.randn(B, 1, h, w, generator=g).to(dev).requires_grad_(True))
    for _ in range(B):
        wh = torch.rand(G, 2, generator=g) ** 2 * torch.tensor([600.0, 500.0]) + 16
        xy = torch.rand(G, 2, generator=g) * (torch.tensor([IMG[1], IMG[0]], dtype=torch.float32) - wh)
        s['gt_bboxes'].append(torch.cat([xy, xy + wh], 1).round().to(dev))
        s['gt_labels'].append(torch.randint(0, C, (G,), generator=g).to(dev))
    return s


def clear_grads(s):
    for k in ('cls', 'bbox', 'ctr'):
        for t in s[k]:
            t.grad = None


def count_syncs(fn):
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        n = sum('synchroniz' in str(x.message) for x in w)
    except Exception as e:                                               # noqa: BLE001
        n = f'not counted: {e!r}'
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return n


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                   and 'memset' not in e.name.lower())
    except Exception as e:                                               # noqa: BLE001
        return f'not counted: {e!r}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_box_head_loss_bench.json'))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--sets', type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_head_loss_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    cfg = bx.parse_box_head_cfg(HEAD)
    pts = points(dev)
    sets = [make_set(dev, 200 + i, cfg) for i in range(args.sets)]
    paths = {'kernel': lambda s: kernel_path(s), 'composed': lambda s: composed_path(s, pts)}
    a, b = paths['kernel'](sets[0]), None
    ga = [t.grad.clone() for k in ('cls', 'bbox', 'ctr') for t in sets[0][k]]
    clear_grads(sets[0])
    b = paths['composed'](sets[0])
    gb = [t.grad.clone() for k in ('cls', 'bbox', 'ctr') for t in sets[0][k]]
    clear_grads(sets[0])
    torch.cuda.synchronize()
    M_all = sum(h * w for h, w in SIZES)
    n_all = B * M_all
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, C=C, levels=SIZES, boxes_per_image=G, locations=n_all), 'reps': args.reps,
           'sets': args.sets, 'positives': int((a[1][3] >= 0).sum()), 'losses_kernel': [round(float(v), 6) for v in a[0]],
           'losses_composed': [round(float(v), 6) for v in b[0]], 'same_gt_inds': bool(torch.equal(a[1][3], b[1][3])),
           'max_grad_diff_rel': max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(ga, gb)),
           # maps read + gradients written (C + 4 + 1 floats per location each way), targets written then read (labels, gt_inds, level, img:
           # int64; bbox_targets 4, points 2, ctr_targets 1 floats; the loss reads labels, bbox_targets, ctr_targets again)
           'bytes_min': n_all * (2 * 4 * (C + 5) + (4 * 8 + 7 * 4) + (8 + 5 * 4)),
           'composed_focal': 'py_sigmoid_focal_loss as torch ops (mmcv\'s one-kernel device op is not available here)'}
    for f in paths.values():
        for i in range(3):
            f(sets[i % len(sets)])
            clear_grads(sets[i % len(sets)])
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for r in range(args.reps):                                           # alternated: both paths see the same neighbours on the box
        for k, f in paths.items():
            s = sets[r % len(sets)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(s)
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
            clear_grads(s)
    for k, f in paths.items():
        v = ts[k]

        def once(f=f):
            f(sets[0])
            clear_grads(sets[0])
        out[k] = dict(ms=round(float(np.median(v)), 4), ms_p25=round(float(np.percentile(v, 25)), 4), ms_p75=round(float(np.percentile(v, 75)), 4),
                      ms_min=round(min(v), 4), ms_max=round(max(v), 4), host_syncs=count_syncs(once), launches=count_launches(once))
    out['kernel']['GBps_of_bytes_min'] = round(out['bytes_min'] / (out['kernel']['ms'] * 1e-3) / 1e9, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
