#!/usr/bin/env python3
"""Developer measurement of the SOLOv2-style test-time block (threshold, area, mask scoring, Matrix NMS) on the GPU box:
boxinstseg_amd.seg_nms (csrc/matrix_nms.hip) against the torch composition -- the op sequence of box_solov2_head.py:546-574 and
matrix_nms.py:43-121, written out below -- from fp32 probabilities to keep_inds, same box, same inputs, calls alternated.

Shapes: 200x304 with 100, 500 and 2000 candidates, 100x152 with 500; nms_pre = 500, gaussian sigma 2, filter_thr 0.05, max 100.
Per shape and path:
  ms, ms_min, ms_max   host clock around one call that ends in a device synchronise (the block has data-dependent sizes, so both
                       paths synchronise inside as well), median / extremes of the alternated repetitions after warm-up;
  launches             device kernels and copies of one call as torch.profiler lists them;
  peak_MB              growth of max_memory_allocated during one call.
`same_keep` / `max_score_diff` compare the two results.  Writes one JSON object to --out (default
profiles/r08_matrix_nms_bench.json) and prints it.  GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

CFG = dict(mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
SHAPES = [(200, 304, 100), (200, 304, 500), (200, 304, 2000), (100, 152, 500)]


def composed_matrix_nms(masks, labels, scores, filter_thr, nms_pre, max_num, sigma, mask_area):
    """Matrix NMS as a torch op sequence: fp32 masks, their n x n matrix product, and elementwise passes over n x n."""
    scores, sort_inds = torch.sort(scores, descending=True)
    keep_inds = sort_inds
    if nms_pre > 0 and len(sort_inds) > nms_pre:
        sort_inds, keep_inds, scores = sort_inds[:nms_pre], keep_inds[:nms_pre], scores[:nms_pre]
    masks, mask_area, labels = masks[sort_inds], mask_area[sort_inds], labels[sort_inds]
    n = len(labels)
    flat = masks.reshape(n, -1).float()
    inter = torch.mm(flat, flat.transpose(1, 0))
    area = mask_area.expand(n, n)
    iou = (inter / (area + area.transpose(1, 0) - inter)).triu(diagonal=1)
    lab = labels.expand(n, n)
    same = (lab == lab.transpose(1, 0)).triu(diagonal=1)
    compensate, _ = (iou * same).max(0)
    compensate = compensate.expand(n, n).transpose(1, 0)
    decay = iou * same
    coef, _ = (torch.exp(-1 * sigma * (decay ** 2)) / torch.exp(-1 * sigma * (compensate ** 2))).min(0)
    scores = scores * coef
    if filter_thr > 0:
        keep = scores >= filter_thr
        keep_inds = keep_inds[keep]
        if not keep.any():
            return scores.new_zeros(0), labels.new_zeros(0), labels.new_zeros(0)
        scores, labels = scores[keep], labels[keep]
    scores, sort_inds = torch.sort(scores, descending=True)
    keep_inds = keep_inds[sort_inds]
    if max_num > 0 and len(sort_inds) > max_num:
        sort_inds, keep_inds, scores = sort_inds[:max_num], keep_inds[:max_num], scores[:max_num]
    return scores, labels[sort_inds], keep_inds


def composed_block(seg_preds, cate_labels, cate_scores, strides, cfg):
    """The block in torch: boolean masks, their sums, the filter, the mask scores, Matrix NMS.  keep_inds index the inputs."""
    seg_masks = seg_preds > cfg['mask_thr']
    sum_masks = seg_masks.sum((1, 2)).float()
    keep = sum_masks > strides
    if keep.sum() == 0:
        return cate_scores.new_zeros(0), cate_labels.new_zeros(0), cate_labels.new_zeros(0)
    kept = keep.nonzero(as_tuple=True)[0]
    seg_masks, seg_preds, sum_masks = seg_masks[keep, ...], seg_preds[keep, ...], sum_masks[keep]
    cate_scores, cate_labels = cate_scores[keep], cate_labels[keep]
    seg_scores = (seg_preds * seg_masks.float()).sum((1, 2)) / sum_masks
    scores, labels, keep_inds = composed_matrix_nms(seg_masks, cate_labels, cate_scores * seg_scores, cfg['filter_thr'], cfg['nms_pre'],
                                                    cfg['max_per_img'], cfg['sigma'], sum_masks)
    return scores, labels, kept[keep_inds]


def candidates(dev, n, h, w, seed):
    """Soft discs around eight shared centres: most candidates overlap others of their class."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)
    centres = torch.stack([0.15 * h + 0.7 * h * r(8), 0.15 * w + 0.7 * w * r(8)], 1)
    which = torch.randint(0, 8, (n,), device=dev, generator=g)
    cy = centres[which, 0] + 0.05 * h * torch.randn(n, device=dev, generator=g)
    cx = centres[which, 1] + 0.05 * w * torch.randn(n, device=dev, generator=g)
    rad = (0.06 + 0.2 * r(n)) * min(h, w)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    dist = ((yy - cy[:, None, None]) ** 2 + (xx - cx[:, None, None]) ** 2).sqrt()
    probs = torch.sigmoid(0.8 * (rad[:, None, None] - dist) + 0.3 * torch.randn(n, h, w, device=dev, generator=g))
    labels = torch.randint(0, 4, (n,), device=dev, generator=g)
    scores = 0.1 + 0.85 * r(n)
    strides = torch.tensor([8.0, 8.0, 16.0, 32.0, 32.0], device=dev)[torch.randint(0, 5, (n,), device=dev, generator=g)]
    return probs.contiguous(), labels, scores, strides


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def peak_mb(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_matrix_nms_bench.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('matrix_nms_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    out = {'gpu': torch.cuda.get_device_name(0), 'cfg': CFG, 'reps': args.reps, 'shapes': {}}
    for h, w, n in SHAPES:
        probs, labels, scores, strides = candidates(dev, n, h, w, seed=n + h)
        paths = {'kernel': lambda: bx.seg_nms(probs, labels, scores, strides, CFG),
                 'composed': lambda: composed_block(probs, labels, scores, strides, CFG)}
        res = {k: f() for k, f in paths.items()}
        torch.cuda.synchronize()
        ka, kb = res['kernel'][2].cpu().tolist(), res['composed'][2].cpu().tolist()
        r = {'kept': len(ka), 'same_keep': sorted(ka) == sorted(kb), 'same_order': ka == kb}
        if r['same_keep'] and ka:
            sa = dict(zip(ka, res['kernel'][0].cpu().tolist()))
            sb = dict(zip(kb, res['composed'][0].cpu().tolist()))
            r['max_score_rel_diff'] = max(abs(sa[i] - sb[i]) / abs(sb[i]) for i in ka)
        for f in paths.values():                          # warm-up of every shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ts = {k: [] for k in paths}
        for _ in range(args.reps):                        # alternated: both paths see the same neighbours on the box
            for k, f in paths.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k, f in paths.items():
            r[k] = dict(ms=round(float(np.median(ts[k])), 4), ms_min=round(min(ts[k]), 4), ms_max=round(max(ts[k]), 4),
                        ms_p25=round(float(np.percentile(ts[k], 25)), 4), ms_p75=round(float(np.percentile(ts[k], 75)), 4),
                        launches=count_launches(f), peak_MB=round(peak_mb(f, dev), 2))
        r['speedup_median'] = round(r['composed']['ms'] / r['kernel']['ms'], 2)
        r['faster_beyond_spread'] = r['kernel']['ms_p75'] < r['composed']['ms_p25']
        out['shapes'][f'{h}x{w}_n{n}'] = r
        print(f'{h}x{w} n={n}: {json.dumps(r)}', flush=True)
        del probs, res
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
