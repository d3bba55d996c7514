#!/usr/bin/env python3
"""Developer measurement of the Box2Mask target assignment of one decoder layer on the GPU box: boxinstseg_amd.box2mask_get_targets
(csrc/box_match.hip) against the same steps as plain torch ops plus ``.cpu()`` plus scipy -- the op sequence of box2mask_head.py:152-189,
match_cost.py:191-193, 386-425 and mask_hungarian_assigner.py:77-130, written out below -- same box, same inputs, calls alternated.

Shape: B = 2, Q = 100, 256x256 predictions, 1024x1024 ground-truth canvas, G = (7, 23), 80 classes; the configs' constants.
  ms, ms_p25, ms_p75, ms_min, ms_max   host clock around one call that ends in a device synchronise, over the alternated repetitions after
                                       warm-up.  Inputs rotate over --sets independent copies (5 x 84 MB > the 256 MB Infinity Cache),
                                       so every call reads cold data; `*_warm`: one set re-used, labelled as such.
  peak_MB                              growth of max_memory_allocated during one call.
  project_pred_us                      kernel (a) alone, HIP events around back-to-back calls on the rotating sets, and `copy_GBps`: the
                                       library's byte-only copy kernel (bxi_dev_sol_pairwise_f32 mode 1: 16-byte accesses, 10 bytes moved
                                       per input byte) timed the same way in the same run; `project_pred_fraction_of_copy` = the time that
                                       copy rate needs for kernel (a)'s bytes (logits read, projections and partial maxima written and
                                       re-read) over the kernel's time.
  --loop N                             only runs the path N times (for `rocprofv3 --kernel-trace --stats -- python tools/box_match_bench.py
                                       --loop 20`); --kernel-stats CSV folds that run's per-kernel averages into the JSON.
If scipy is missing on the box the composed path is not timed and the JSON says so.  Writes one JSON object to --out (default
profiles/r09_box_match_bench.json) and prints it.  GPU only; reads nothing but this repository."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry

B, Q, HP, HT, COUNTS, CLASSES = 2, 100, 256, 1024, (7, 23), 80
W_CLS, W_DICE, EPS = 2.0, 5.0, 1.0


def make_set(dev, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    masks, labels = [], []
    for n in COUNTS:
        m = torch.zeros(n, HT, HT, dtype=torch.uint8)
        for j in range(n):
            y0, x0 = (int(v) for v in torch.randint(0, HT - 200, (2,), generator=g))
            hh, ww = (int(v) for v in torch.randint(40, 200, (2,), generator=g))
            m[j, y0:y0 + hh, x0:x0 + ww] = 1
        masks.append(m.to(dev))
        labels.append(torch.randint(0, CLASSES, (n,), generator=g).to(dev))
    logits = (torch.randn(B, Q, HP, HP, generator=g) * 2 - 1).to(dev)
    cls = torch.randn(B, Q, CLASSES + 1, generator=g).to(dev)
    return dict(cls=cls, logits=logits, labels=labels, masks=masks)


def composed_single(cls_score, mask_pred, gt_labels, gt_masks, lsa):
    """One image as torch ops: up-sample, sigmoid, project, two einsums, the class cost, the host round trip, the gathers."""
    target_shape = gt_masks.shape[-2:]
    up = F.interpolate(mask_pred.unsqueeze(1), target_shape, mode='bilinear', align_corners=False)
    gt = gt_masks.unsqueeze(1)
    p = up.sigmoid()

    def dice(a, b):
        a, b = a.flatten(1), b.flatten(1).float()
        return 1 - (2 * torch.einsum('nc,mc->nm', a, b) + EPS) / (a.pow(2).sum(1)[:, None] + b.pow(2).sum(1)[None, :] + EPS)
    cost = -cls_score.softmax(-1)[:, gt_labels] * W_CLS + W_DICE * (dice(p.max(dim=3, keepdim=True)[0], gt.max(dim=3, keepdim=True)[0]) +
                                                                    dice(p.max(dim=2, keepdim=True)[0], gt.max(dim=2, keepdim=True)[0]))
    rows, cols = lsa(cost.detach().cpu())
    rows, cols = torch.from_numpy(rows).to(up.device), torch.from_numpy(cols).to(up.device)
    nq = mask_pred.shape[0]
    labels = gt_labels.new_full((nq,), CLASSES)
    labels[rows] = gt_labels[cols]
    weights = up.new_zeros((nq,))
    weights[rows] = 1.0
    return labels, gt_labels.new_ones((nq,)), gt[cols], weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_box_match_bench.json'))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--sets', type=int, default=5)
    ap.add_argument('--loop', type=int, default=0)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_match_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    from boxinstseg_amd import _lib
    from boxinstseg_amd import box_match as M
    dev = torch.device('cuda:0')
    assigner = bx.MaskHungarianAssigner(cls_cost=dict(type='ClassificationCost', weight=W_CLS),
                                        dice_cost=dict(type='BoxMatchingCost', weight=W_DICE, pred_act=True, eps=EPS))
    sets = [make_set(dev, 100 + i) for i in range(args.sets)]

    def kernel_path(s):
        return bx.box2mask_get_targets(s['cls'], s['logits'], s['labels'], s['masks'], assigner, CLASSES)
    if args.loop:
        for i in range(args.loop):
            kernel_path(sets[i % len(sets)])
        torch.cuda.synchronize()
        return
    try:
        from scipy.optimize import linear_sum_assignment as lsa
    except ImportError:
        lsa = None

    def composed_path(s):
        return [composed_single(s['cls'][i], s['logits'][i], s['labels'][i], s['masks'][i], lsa) for i in range(B)]
    paths = {'kernel': kernel_path}
    if lsa is not None:
        paths['composed'] = composed_path
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, Q=Q, pred=HP, canvas=HT, G=COUNTS, classes=CLASSES), 'reps': args.reps,
           'sets': args.sets, 'scipy': lsa is not None}
    if lsa is None:
        out['composed'] = 'not measured: scipy is not installed on this box'
    else:
        a, b = kernel_path(sets[0]), composed_path(sets[0])
        torch.cuda.synchronize()
        out['same_labels'] = all(torch.equal(a[0][i], b[i][0]) for i in range(B))
        out['same_mask_targets'] = all(torch.equal(a[2][i], b[i][2]) for i in range(B))
    for f in paths.values():
        for i in range(3):
            f(sets[i % len(sets)])
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    warm = {k: [] for k in paths}
    for r in range(args.reps):                            # alternated: both paths see the same neighbours on the box
        for k, f in paths.items():
            for store, s in ((ts, sets[r % len(sets)]), (warm, sets[0])):
                t0 = time.perf_counter()
                f(s)
                torch.cuda.synchronize()
                store[k].append((time.perf_counter() - t0) * 1e3)
    for k, f in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        f(sets[1])
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        v = ts[k]
        out[k] = dict(ms=round(float(np.median(v)), 4), ms_p25=round(float(np.percentile(v, 25)), 4), ms_p75=round(float(np.percentile(v, 75)), 4),
                      ms_min=round(min(v), 4), ms_max=round(max(v), 4), ms_warm=round(float(np.median(warm[k])), 4), peak_MB=round(peak, 2))
    if 'composed' in paths:
        out['speedup_median'] = round(out['composed']['ms'] / out['kernel']['ms'], 2)
        out['faster_beyond_spread'] = out['kernel']['ms_p75'] < out['composed']['ms_p25']

    def ev(fn, n=40, warm_n=5):
        for i in range(warm_n):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3
    lib = _lib.load()
    n = B * Q
    flat = [s['logits'].view(n, HP, HP) for s in sets]
    rows, cols, sumsq = (torch.empty((n, HT), device=dev), torch.empty((n, HT), device=dev), torch.empty((n, 2), device=dev))
    ws_bytes = lib.bxi_box_match_workspace_bytes(n, HT, HT)
    ws = torch.empty(ws_bytes // 4, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    a_us = ev(lambda i: lib.bxi_match_project_pred_f32(flat[i % len(flat)].data_ptr(), n, HP, HP, HT, HT, 1, rows.data_ptr(), cols.data_ptr(),
                                                       sumsq.data_ptr(), ws.data_ptr(), ws_bytes, st))
    a_bytes = n * HP * HP * 4 + 2 * ws_bytes + 2 * n * HT * 4
    planes = [torch.empty(n * 8 * HP * HP, device=dev) for _ in sets]
    outs = [torch.empty(n * HP * HP, device=dev) for _ in sets]
    copy_us = ev(lambda i: lib.bxi_dev_sol_pairwise_f32(flat[i % len(flat)].data_ptr(), planes[i % len(flat)].data_ptr(),
                                                        outs[i % len(flat)].data_ptr(), n, HP, HP, 1, st))
    copy_gbps = 10 * n * HP * HP * 4 / copy_us / 1e3
    out['project_pred'] = dict(us=round(a_us, 2), bytes=a_bytes, GBps=round(a_bytes / a_us / 1e3, 1), copy_us=round(copy_us, 2),
                               copy_GBps=round(copy_gbps, 1), project_pred_fraction_of_copy=round(a_bytes / copy_gbps / 1e3 / a_us, 3),
                               note='cold inputs (rotating sets); the copy moves 10 bytes per logit byte with 16-byte accesses, nothing computed')
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        with open(args.kernel_stats) as fh:
            rows = list(csv.DictReader(fh))
        try:
            out['kernel_stats_us'] = {r['Name'].split('(')[0][-48:]: dict(calls=int(r['Calls']), avg_us=round(float(r['AverageNs']) / 1e3, 2))
                                      for r in rows if 'match' in r['Name'] or 'project' in r['Name'] or 'lsa' in r['Name']}
        except (KeyError, ValueError) as e:
            out['kernel_stats_us'] = f'not read: {e!r}; columns {sorted(rows[0]) if rows else []}'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
