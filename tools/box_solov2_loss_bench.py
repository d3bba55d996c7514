#!/usr/bin/env python3
"""``box_solov2_loss`` against what the package offered before it, at the configs' shape (the one of tools/box_solo_masks_bench.py): B = 2,
E = 256, a mask feature of 200 x 336, num_grids 40 / 36 / 24 / 16 / 12, level sizes 200 x 336 (twice), 100 x 168, 50 x 84 (twice), 20
boxes per image assigned by ``box_solov2_targets``.  Forward + backward of the three losses, on COLD inputs (rotating input sets), the
three paths alternated in one run:

  new        box_solov2_loss
  composed   tests/bls_compose.compose_loss as written: the level loop with the reference's per-row repeats and one tree per row (a)
  shared     the same loop with trees, breadth-first orders and edge weights built once per (size, image) by hand and an image's rows
             filtered as channels (compose_loss(share=True)): the honest competitor (b)

Per path: ms (median, p25, p75, min, max; host clock around one forward + backward that ends in a device synchronise), device launches
(torch's profiler), host synchronisations (torch's sync debug mode) and peak memory above the inputs.  ``kernels``: the library's own
launches of one new call between device events placed by the launch hook, and for the front and the backward kernel the bytes they must
move and their share of the achievable HBM rate.  No ratio is fixed in advance.  Writes profiles/r31_box_solov2_loss_bench.json.
Nothing here is meaningful from a CPU run: it needs the GPU."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

import __graft_entry__ as entry
from box_solo_masks_bench import B, CANVAS, E, GRIDS, HW, SCALE_RANGES, SIZES, STRIDES, kernel_times
from corr_bench import count_launches, stats
from seg_paste_bench import peak_bytes
from solo_dconv_bench import HBM_ACHIEVABLE
from tests import bls_compose as C

HEAD = dict(type='BoxSOLOv2Head', num_classes=80, strides=STRIDES, scale_ranges=tuple(SCALE_RANGES), sigma=0.2, num_grids=GRIDS,
            loss_cate=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_boxpro=dict(type='BoxProjectionLoss', loss_weight=3.0), loss_levelset=dict(type='LevelsetLoss', loss_weight=1.0))
CF, PER_IMAGE = 8, 20


def make_set(dev, seed):
    rng = np.random.default_rng(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    boxes, labels, masks = [], [], []
    for _ in range(B):
        bx, m = [], np.zeros((PER_IMAGE, *CANVAS), np.uint8)
        for i in range(PER_IMAGE):
            side = float(np.exp(rng.uniform(np.log(24), np.log(700))))
            w, h = min(side * rng.uniform(0.6, 1.6), CANVAS[1] - 2), min(side * rng.uniform(0.6, 1.6), CANVAS[0] - 2)
            x1, y1 = rng.uniform(0, CANVAS[1] - w - 1), rng.uniform(0, CANVAS[0] - h - 1)
            bx.append([x1, y1, x1 + w, y1 + h])
            m[i, int(y1):int(y1 + h) + 1, int(x1):int(x1 + w) + 1] = 1
        boxes.append(torch.tensor(bx, dtype=torch.float32, device=dev))
        labels.append(torch.from_numpy(rng.integers(0, 80, PER_IMAGE)).to(dev))
        masks.append(torch.from_numpy(m).to(dev))
    r = lambda *s, scale=1.0: (scale * torch.randn(*s, device=dev, generator=g)).requires_grad_(True)
    return dict(kern=[r(B, E, S, S, scale=1 / 16) for S in GRIDS], cate=[r(B, 80, S, S) for S in GRIDS], feat=r(B, E, *HW, scale=0.5),
                lst=r(B, CF, *HW), img=torch.randn(B, 3, *CANVAS, device=dev, generator=g), boxes=boxes, labels=labels, masks=masks)


def run(which, s):
    import boxinstseg_amd as M
    if which == 'new':
        out = M.box_solov2_loss(s['kern'], s['cate'], s['feat'], s['lst'], s['boxes'], s['labels'], s['masks'], s['img'], None, HEAD)
    else:
        out, _ = C.compose_loss(s['kern'], s['cate'], s['feat'], s['lst'], s['boxes'], s['labels'], s['masks'], s['img'], HEAD, SIZES, share=which == 'shared')
    sum(out.values()).backward()
    return out


def clear(s):
    for t in s['kern'] + s['cate'] + [s['feat'], s['lst']]:
        t.grad = None


def census(which, s):
    clear(s)
    launches = count_launches(lambda: run(which, s))
    clear(s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        run(which, s)
    torch.cuda.set_sync_debug_mode('default')
    syncs = sum(1 for w in seen if 'synchroniz' in str(w.message).lower() and 'prototype' not in str(w.message).lower())
    clear(s)
    peak = peak_bytes(lambda: run(which, s))
    clear(s)
    return dict(launches=launches, host_syncs=syncs, peak_MB=round(peak / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--paths', default='new,composed,shared')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r31_box_solov2_loss_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_solov2_loss_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as M
    dev = torch.device('cuda:0')
    paths = a.paths.split(',')
    sets = [make_set(dev, 100 + i) for i in range(a.sets)]
    times, first = {k: [] for k in paths}, {}
    for r in range(a.warmup + a.reps):
        for k in paths:
            s = sets[r % a.sets]
            clear(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(k, s)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                first[k] = {n: float(v.detach()) for n, v in out.items()}
    head = M.parse_solo_head_cfg(HEAD)
    tg = M.box_solov2_targets(sets[0]['boxes'], sets[0]['labels'], sets[0]['masks'], SIZES,
                              **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')})
    counts = [[int(tg.counts[l][b][1]) for b in range(B)] for l in range(len(GRIDS))]
    res = dict(shape=dict(B=B, E=E, mask_feat=list(HW), level_sizes=[list(s) for s in SIZES], grids=GRIDS, per_image=PER_IMAGE, levelset_channels=CF,
                          rows_per_level_and_image=counts, rows=sum(map(sum, counts))), sets=a.sets, reps=a.reps, device=torch.cuda.get_device_name(0))
    for k in paths:
        res[k] = stats(times[k])
        res[k].update(census(k, sets[0]))
    res['first_call_losses'] = first
    if 'new' in paths:
        clear(sets[0])
        kt = kernel_times(lambda: (clear(sets[0]), run('new', sets[0])), reps=5)
        pix = sum(sum(c) * h * w for c, (h, w) in zip(counts, SIZES))
        need = {'bls_front_partial': pix * (4 + 1 + 12 + 4), 'bls_backward': pix * (4 + 4 + 1 + 12 + 4)}     # logit, byte, 3 image floats, p out | p, g_p, byte, image, grad out
        res['kernels'] = {n: dict(us=v) for n, v in kt.items() if n.startswith('bls_')}
        for n, nbytes in need.items():
            if n in res['kernels']:
                us = res['kernels'][n]['us'][0]
                res['kernels'][n].update(needed_bytes=nbytes, share_of_achievable_hbm=round(nbytes / HBM_ACHIEVABLE / (us * 1e-6), 4))
    for k in ('composed', 'shared'):
        if k in paths and 'new' in paths:
            spread = max(res[k]['ms_p75'] - res[k]['ms_p25'], res['new']['ms_p75'] - res['new']['ms_p25'])
            res[f'gain_over_{k}_exceeds_spread'] = bool(res[k]['ms'] - res['new']['ms'] > spread)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
