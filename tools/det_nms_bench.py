#!/usr/bin/env python3
"""Developer measurement of CondInst's test-time detections on the GPU box: boxinstseg_amd.condinst_get_bboxes (csrc/box_nms.hip)
against the reference's op sequence written out as torch ops (condinst_head.py:762-853 and :18-83) -- same box, same inputs, calls
alternated.  The NMS step of the composed path is a STAND-IN for mmcv's (whose source is not available here), in mmcv's shape: the
class offset copy, an IoU mask computed on the device, ``.cpu()``, a greedy scan on the host.

Shape: the config's own.  B = 2, 800 x 1024, five levels (100x128, 50x64, 25x32, 13x16, 7x8), C = 80, P = 169 dynamic parameters,
test_cfg nms_pre = 2000, score_thr = 0.05, IoU 0.5; max_per_img = 100 (--max-per-img).  The class logits are shifted per image until
about 3000 (image 0) and about 12000 (image 1) candidates pass the score threshold.
  ms, ms_p25, ms_p75, ms_min, ms_max   host clock around one call that ends in a device synchronise, over the alternated repetitions
                                       after warm-up; inputs rotate over --sets independent copies (cold data).
  peak_MB                              growth of max_memory_allocated during one call.
  host_syncs                           synchronising calls torch reports during one call (torch.cuda.set_sync_debug_mode).
  candidate_pass_ms                    event-timed bxi_det_candidates_f32 alone (median / min over the repetitions): on the top-k rows
                                       (M = 5064) and on every location (sel NULL: 17064 rows, 267 row tiles, each of which sums the
                                       counts of the tiles before it in the write pass).
  --shifts a,b                         the per-image logit shifts of an earlier run (skips the calibration and its launches).
  --loop N --path kernel|composed      only runs one path N times (for `rocprofv3 --kernel-trace --stats -- python tools/det_nms_bench.py
                                       --loop 20 --path kernel`); --kernel-stats-kernel / --kernel-stats-composed CSV fold that run's
                                       launch count per call into the JSON.
Writes one JSON object to --out (default profiles/r10_det_nms_bench.json) and prints it.  GPU only; reads nothing but this repository."""
import argparse
import csv
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as entry

B, C, P = 2, 80, 169
SIZES, STRIDES = ((100, 128), (50, 64), (25, 32), (13, 16), (7, 8)), (8, 16, 32, 64, 128)
IMG = (800, 1024, 3)
TARGETS = (3000, 12000)
CFG = dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)


def points(dev):
    out = []
    for (h, w), s in zip(SIZES, STRIDES):
        x = ((torch.arange(0, w, device=dev) + 0.5) * s).float()
        y = ((torch.arange(0, h, device=dev) + 0.5) * s).float()
        yy, xx = torch.meshgrid(y, x, indexing='ij')
        out.append(torch.stack([xx.reshape(-1), yy.reshape(-1)], -1))
    return out


def composed_path(s, pts, cfg):
    """The reference's _get_bboxes + nms_with_others as torch ops; the NMS is the stand-in described above."""
    mlvl = dict(coors=[], bboxes=[], scores=[], ctr=[], params=[])
    for cls, bbox, ctr, par, p in zip(s['cls'], s['bbox'], s['ctr'], s['params'], pts):
        scores = cls.permute(0, 2, 3, 1).reshape(B, -1, C).sigmoid()
        ctr = ctr.permute(0, 2, 3, 1).reshape(B, -1).sigmoid()
        bbox = bbox.permute(0, 2, 3, 1).reshape(B, -1, 4)
        par = par.permute(0, 2, 3, 1).reshape(B, -1, P)
        p = p.expand(B, -1, 2)
        if 0 < cfg['nms_pre'] < bbox.shape[1]:
            max_scores, _ = (scores * ctr[..., None]).max(-1)
            _, topk = max_scores.topk(cfg['nms_pre'])
            bi = torch.arange(B, device=cls.device).view(-1, 1).expand_as(topk)
            p, bbox, scores, ctr, par = p[bi, topk], bbox[bi, topk], scores[bi, topk], ctr[bi, topk], par[bi, topk]
        boxes = torch.stack([p[..., 0] - bbox[..., 0], p[..., 1] - bbox[..., 1], p[..., 0] + bbox[..., 2], p[..., 1] + bbox[..., 3]], -1)
        mx = boxes.new_tensor([IMG[1], IMG[0], IMG[1], IMG[0]])
        boxes = torch.where(boxes < 0, boxes.new_tensor(0), boxes)
        boxes = torch.where(boxes > mx, mx, boxes)
        for k, v in zip(('coors', 'bboxes', 'scores', 'ctr', 'params'), (p, boxes, scores, ctr, par)):
            mlvl[k].append(v)
    lvl = torch.cat([torch.full_like(c, i).long() for i, c in enumerate(mlvl['ctr'])], 1)
    cat = {k: torch.cat(v, 1) for k, v in mlvl.items()}
    out = []
    for b in range(B):
        scores = cat['scores'][b]
        n = scores.shape[0]
        boxes = cat['bboxes'][b][:, None].expand(n, C, 4).reshape(-1, 4)
        positions = torch.arange(n, device=scores.device).view(-1, 1).expand_as(scores).reshape(-1)
        labels = torch.arange(C, device=scores.device).view(1, -1).expand_as(scores).reshape(-1)
        flat = scores.reshape(-1)
        valid = flat > cfg['score_thr']
        flat = flat * cat['ctr'][b].view(-1, 1).expand(n, C).reshape(-1)
        inds = valid.nonzero(as_tuple=False).squeeze(1)
        boxes, flat, positions, labels = boxes[inds], flat[inds], positions[inds], labels[inds]
        if boxes.numel() == 0:
            out.append((torch.cat([boxes, flat[:, None]], -1), labels, cat['params'][b][positions], cat['coors'][b][positions], lvl[b][positions]))
            continue
        # stand-in for mmcv.ops.nms.batched_nms: offset copy, sort, IoU mask on the device, .cpu(), greedy scan on the host
        shifted = boxes + (labels.to(boxes) * (boxes.max() + 1))[:, None]
        order = flat.sort(descending=True, stable=True)[1]
        sb = shifted[order]
        area = (sb[:, 2] - sb[:, 0]) * (sb[:, 3] - sb[:, 1])
        keep, removed = [], np.zeros(len(order), bool)
        CH = 2048                                                        # the mask goes to the host in row blocks of 2048
        for lo in range(0, len(order), CH):
            blk = sb[lo:lo + CH]
            iw = (torch.min(blk[:, None, 2], sb[None, :, 2]) - torch.max(blk[:, None, 0], sb[None, :, 0])).clamp(min=0)
            ih = (torch.min(blk[:, None, 3], sb[None, :, 3]) - torch.max(blk[:, None, 1], sb[None, :, 1])).clamp(min=0)
            inter = iw * ih
            mask = (inter > 0.5 * (area[lo:lo + CH, None] + area[None, :] - inter)).cpu().numpy()
            for i in range(mask.shape[0]):
                if not removed[lo + i]:
                    keep.append(lo + i)
                    removed |= mask[i]
                    if len(keep) >= cfg['max_per_img']:
                        break
            if len(keep) >= cfg['max_per_img']:
                break
        keep = order[torch.tensor(keep, device=order.device)]
        dets = torch.cat([boxes[keep], flat[keep, None]], -1)
        out.append((dets, labels[keep], cat['params'][b][positions][keep], cat['coors'][b][positions][keep], lvl[b][positions][keep]))
    return out


def make_set(dev, seed, shifts):
    g = torch.Generator(device='cpu').manual_seed(seed)
    s = dict(cls=[], bbox=[], ctr=[], params=[])
    for (h, w), st in zip(SIZES, STRIDES):
        cls = torch.randn(B, C, h, w, generator=g)
        for b in range(B):
            cls[b] += shifts[b]
        s['cls'].append(cls.to(dev))
        s['bbox'].append((torch.rand(B, 4, h, w, generator=g) * 3.5 + 0.5).mul(st).mul(8).round().div(8).to(dev))
        s['ctr'].append(torch.randn(B, 1, h, w, generator=g).to(dev))
        s['params'].append(torch.randn(B, P, h, w, generator=g).to(dev))
    return s


def candidate_counts(s):
    from boxinstseg_amd import box_nms
    lv = box_nms._Levels(s['cls'], s['bbox'], s['ctr'], s['params'], STRIDES)
    sel = box_nms._select(lv, box_nms.location_scores(lv), CFG['nms_pre'])
    return box_nms.det_candidates(lv, sel, [[IMG[0], IMG[1], 1, 1, 1, 1]] * B, False, CFG['score_thr'], 1)[4].tolist()


def calibrate(dev):
    """Per image the shift of the class logits at which about TARGETS[b] candidates pass (bisection, 12 steps)."""
    lo, hi = [-8.0] * B, [0.0] * B
    for _ in range(12):
        mid = [(a + b) / 2 for a, b in zip(lo, hi)]
        n = candidate_counts(make_set(dev, 100, mid))
        for b in range(B):
            if n[b] > TARGETS[b]:
                hi[b] = mid[b]
            else:
                lo[b] = mid[b]
    return [(a + b) / 2 for a, b in zip(lo, hi)]


def candidate_pass_ms(s, reps):
    from boxinstseg_amd import box_nms
    lv = box_nms._Levels(s['cls'], s['bbox'], s['ctr'], s['params'], STRIDES)
    sel = box_nms._select(lv, box_nms.location_scores(lv), CFG['nms_pre'])
    dims, out = [[IMG[0], IMG[1], 1, 1, 1, 1]] * B, {}
    for name, rows in (('topk_rows', sel), ('all_locations', None)):
        ms = []
        for r in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cand = box_nms.det_candidates(lv, rows, dims, False, CFG['score_thr'], box_nms.SORT_MAX)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        out[name] = dict(rows=lv.M_all if rows is None else int(rows.shape[1]), candidates=cand[4].tolist(),
                         ms=round(float(np.median(ms)), 4), ms_min=round(min(ms), 4))
    return out


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


def launches_per_call(path, loop):
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    try:
        return round(sum(int(r['Calls']) for r in rows) / loop, 1)
    except (KeyError, ValueError) as e:
        return f'not read: {e!r}; columns {sorted(rows[0]) if rows else []}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r10_det_nms_bench.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--max-per-img', type=int, default=100)
    ap.add_argument('--loop', type=int, default=0)
    ap.add_argument('--path', default='kernel', choices=('kernel', 'composed'))
    ap.add_argument('--kernel-stats-kernel', default=None)
    ap.add_argument('--kernel-stats-composed', default=None)
    ap.add_argument('--stats-loop', type=int, default=20)
    ap.add_argument('--shifts', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('det_nms_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    cfg = dict(CFG, max_per_img=args.max_per_img)
    metas = [dict(img_shape=IMG, scale_factor=np.ones(4, np.float32))] * B
    pts = points(dev)
    shifts = [float(v) for v in args.shifts.split(',')] if args.shifts else calibrate(dev)
    sets = [make_set(dev, 100 + i, shifts) for i in range(args.sets)]
    paths = {'kernel': lambda s: bx.condinst_get_bboxes(s['cls'], s['bbox'], s['ctr'], s['params'], metas, cfg, STRIDES),
             'composed': lambda s: composed_path(s, pts, cfg)}
    if args.loop:
        for i in range(args.loop):
            paths[args.path](sets[i % len(sets)])
        torch.cuda.synchronize()
        return
    a, b = paths['kernel'](sets[0]), paths['composed'](sets[0])
    torch.cuda.synchronize()
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, C=C, P=P, levels=SIZES, cfg=cfg), 'reps': args.reps, 'sets': args.sets,
           'candidates': candidate_counts(sets[0]), 'logit_shifts': [round(v, 6) for v in shifts], 'kept': [int(x[0].shape[0]) for x in a],
           'same_boxes': all(torch.equal(x[0][:, :4], y[0][:, :4]) for x, y in zip(a, b)),
           'same_labels': all(torch.equal(x[1], y[1]) for x, y in zip(a, b)),
           'max_score_diff': max(float((x[0][:, 4] - y[0][:, 4]).abs().max()) if x[0].shape == y[0].shape and len(x[0]) else 0.0 for x, y in zip(a, b)),
           'composed_nms': 'stand-in for mmcv.ops.nms: class-offset copy, IoU mask on the device, .cpu(), greedy scan on the host'}
    for f in paths.values():
        for i in range(2):
            f(sets[i % len(sets)])
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for r in range(args.reps):                                           # alternated: both paths see the same neighbours on the box
        for k, f in paths.items():
            t0 = time.perf_counter()
            f(sets[r % len(sets)])
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    for k, f in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        f(sets[1 % len(sets)])
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        v = ts[k]
        out[k] = dict(ms=round(float(np.median(v)), 4), ms_p25=round(float(np.percentile(v, 25)), 4), ms_p75=round(float(np.percentile(v, 75)), 4),
                      ms_min=round(min(v), 4), ms_max=round(max(v), 4), peak_MB=round(peak, 2), host_syncs=count_syncs(lambda f=f: f(sets[0])))
    out['candidate_pass_ms'] = candidate_pass_ms(sets[0], args.reps)
    out['speedup_median'] = round(out['composed']['ms'] / out['kernel']['ms'], 2)
    out['faster_beyond_spread'] = out['kernel']['ms_p75'] < out['composed']['ms_p25']
    for k, path in (('kernel', args.kernel_stats_kernel), ('composed', args.kernel_stats_composed)):
        if path and os.path.exists(path):
            out[k]['launches_per_call'] = launches_per_call(path, args.stats_loop)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
