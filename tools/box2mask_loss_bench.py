#!/usr/bin/env python3
"""Developer measurement of Box2MaskHead.loss for all decoder layers on the GPU box: boxinstseg_amd.box2mask_loss (one call,
csrc/box2mask_loss.hip) against (a) loss_single composed per layer from the package's modules as they were before it
(tests/b2m_compose.py: the reference's statements around box2mask_get_targets, BoxProjectionLoss, LevelsetLoss, LCM, MinimumSpanningTree
and TreeFilter2D, with its per-instance repeats, boolean index and ``.cpu()``) -- same box, same inputs, calls alternated.
(b), the reference's statements as plain torch ops, is NOT measured: its tree filter and MST are a compiled extension with no torch form.

Shape: B = 2, Q = 100, L = 10 layers, 256x256 predictions and canvas, G = (7, 23), 80 classes; forward + backward.
  ms, ms_p25, ms_p75, ms_min, ms_max   host clock around one forward + backward that ends in a device synchronise, over the alternated
                                       repetitions after warm-up.  Inputs rotate over --sets independent copies (each 10 x 52 MB of
                                       logits, more than the 256 MB Infinity Cache between two uses), so every call reads cold data.
  launches                             device kernels of one forward + backward (torch.profiler, memcpy / memset nodes listed apart).
  host_syncs                           synchronising calls torch's sync debug mode reports during one forward + backward.
  peak_MB                              growth of max_memory_allocated during one forward + backward.
  kernels                              the two new streaming kernels alone (HIP events around back-to-back calls on rotating buffers): us, the
                                       bytes they must move, and that byte rate over the rate of a device-to-device copy of a 512 MB
                                       buffer timed the same way in the same run (`copy_GBps`).
  faster                               true only if the new call's p75 lies below (a)'s p25.
Writes one JSON object to --out (default profiles/r29_box2mask_loss_bench.json) and prints it.  GPU only; reads nothing but this repository."""
import argparse
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

B, Q, L, HP, COUNTS, CLASSES = 2, 100, 10, 256, (7, 23), 80


def make_set(dev, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    masks, labels = [], []
    for n in COUNTS:
        m = torch.zeros(n, HP, HP)
        for j in range(n):
            y0, x0 = (int(v) for v in torch.randint(0, HP - 60, (2,), generator=g))
            hh, ww = (int(v) for v in torch.randint(12, 60, (2,), generator=g))
            m[j, y0:y0 + hh, x0:x0 + ww] = 1
        masks.append(m.to(dev))
        labels.append(torch.randint(0, CLASSES, (n,), generator=g).to(dev))
    yy, xx = torch.meshgrid(torch.arange(HP), torch.arange(HP), indexing='ij')
    img = torch.stack([torch.stack([torch.sin(yy / (5.0 + c + b)) + torch.cos(xx / (7.0 + c)) for c in range(3)]) for b in range(B)])
    img = img + 0.3 * torch.randn(img.shape, generator=g)
    return dict(cls=[torch.randn(B, Q, CLASSES + 1, generator=g).to(dev).requires_grad_(True) for _ in range(L)],
                preds=[(torch.randn(B, Q, HP, HP, generator=g) * 2 - 1).to(dev).requires_grad_(True) for _ in range(L)],
                lst=torch.randn(B, 1, HP, HP, generator=g).to(dev).requires_grad_(True), img=img.to(dev), labels=labels, masks=masks)


def settings():
    from boxinstseg_amd import MaskHungarianAssigner
    return dict(assigner=MaskHungarianAssigner(cls_cost=dict(type='ClassificationCost', weight=2.0),
                                               dice_cost=dict(type='BoxMatchingCost', weight=5.0, pred_act=True, eps=1.0)),
                class_weight=[1.0] * CLASSES + [0.1], loss_cls_weight=2.0, loss_box=5.0, loss_mask=1.0, num_classes=CLASSES)


def run_new(s, kw):
    from boxinstseg_amd import box2mask_loss
    out = box2mask_loss(s['cls'], s['preds'], s['lst'], s['labels'], s['masks'], None, s['img'], **kw)
    sum(out.values()).backward()
    return out


def run_composed(s, kw):
    from tests import b2m_compose
    out = b2m_compose.loss(s['cls'], s['preds'], s['lst'], s['labels'], s['masks'], s['img'], **kw)
    sum(out.values()).backward()
    return out


def clear(s):
    for t in s['cls'] + s['preds'] + [s['lst']]:
        t.grad = None


def census(fn, s, kw):
    """launches, host syncs and peak memory of one forward + backward."""
    from torch.profiler import ProfilerActivity, profile
    clear(s)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(s, kw)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = sum(1 for n in names if 'memcpy' in n.lower() or 'memset' in n.lower() or n.startswith('Memcpy') or n.startswith('Memset'))
    clear(s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        fn(s, kw)
    torch.cuda.set_sync_debug_mode('default')
    syncs = sum(1 for w in seen if 'synchroniz' in str(w.message).lower() and 'prototype' not in str(w.message).lower())
    clear(s)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(s, kw)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    return dict(launches=len(names) - copies, copy_or_memset_nodes=copies, host_syncs=syncs, peak_MB=round(peak, 1))


def event_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for i in range(reps):
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(ts[2:]))


def kernels(dev, M=280, G=30, sh=96, sw=96, nbuf=6):
    """The scores kernel and the level-set forward + backward alone, on rotating buffers."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd._common import current_stream
    lib = _lib.load()
    st = current_stream(dev)
    layers = [[torch.randn(B * Q, HP, HP, device=dev) for _ in range(L)] for _ in range(2)]
    row_plane = torch.randperm(L * B * Q, device=dev)[:M].to(torch.int32)
    p = [torch.empty(M, HP, HP, device=dev) for _ in range(nbuf)]
    ps = torch.empty(M, sh, sw, device=dev)
    ptrs = [_lib.ptr_array([t.data_ptr() for t in ls]) for ls in layers]

    def scores(i):
        _lib.check('scores', lib.bxi_b2m_scores_f32(ptrs[i % 2], L, B * Q, HP, HP, row_plane.data_ptr(), M, sh, sw, p[i % nbuf].data_ptr(), ps.data_ptr(), st))

    T = (torch.rand(G, HP, HP, device=dev) > 0.8).float()
    img = torch.randn(B, 3, HP, HP, device=dev)
    tgt = torch.randint(0, G, (M,), device=dev, dtype=torch.int32)
    im = torch.randint(0, B, (M,), device=dev, dtype=torch.int32)
    pn = T.sum((1, 2)).clamp(min=1)
    loss, gl = torch.empty(M, device=dev), torch.ones(M, device=dev)
    state = torch.empty(lib.bxi_b2m_levelset_state_bytes(M, 3) // 8, dtype=torch.float64, device=dev)
    gp = [torch.empty(M, HP, HP, device=dev) for _ in range(nbuf)]
    for i in range(nbuf):
        scores(i)

    def ls_fwd(i):
        _lib.check('ls', lib.bxi_b2m_levelset_forward_f32(p[i % nbuf].data_ptr(), T.data_ptr(), img.data_ptr(), 1, tgt.data_ptr(), im.data_ptr(),
                                                           pn.data_ptr(), M, G, B, 3, HP, HP, 1.0, loss.data_ptr(), state.data_ptr(), st))

    def ls_bwd(i):
        _lib.check('ls', lib.bxi_b2m_levelset_backward_f32(p[i % nbuf].data_ptr(), T.data_ptr(), img.data_ptr(), 1, tgt.data_ptr(), im.data_ptr(),
                                                            pn.data_ptr(), M, G, B, 3, HP, HP, 1.0, state.data_ptr(), gl.data_ptr(),
                                                            gp[i % nbuf].data_ptr(), None, st))

    big = [torch.empty(128 * 2 ** 20, device=dev) for _ in range(3)]                        # 512 MB each

    def copy(i):
        big[(i + 1) % 3].copy_(big[i % 3])

    copy_us = event_us(copy, 12)
    copy_GBps = 2 * big[0].numel() * 4 / copy_us / 1e3
    plane = HP * HP * 4
    out = dict(copy_GBps=round(copy_GBps, 1))
    # bytes each kernel must move: the matched logit planes in, p and p_small out | p in, T and the image through L2 (G + 3 B planes from memory) | the same in, g_p out
    for name, fn, nbytes in (('b2m_scores', scores, M * (2 * plane + sh * sw * 4)), ('b2m_levelset_forward', ls_fwd, (M + G + 3 * B) * plane),
                             ('b2m_levelset_backward', ls_bwd, (2 * M + G + 3 * B) * plane)):
        us = event_us(fn, 14)
        out[name] = dict(us=round(us, 1), MB=round(nbytes / 1e6, 1), GBps=round(nbytes / us / 1e3, 1), fraction_of_copy=round(nbytes / us / 1e3 / copy_GBps, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_box2mask_loss_bench.json'))
    a = ap.parse_args()
    entry.build()
    dev = torch.device('cuda:0')
    kw = settings()
    sets = [make_set(dev, 100 + i) for i in range(a.sets)]
    paths = (('new', run_new), ('composed_per_layer', run_composed))
    times = {k: [] for k, _ in paths}
    first = {}
    for r in range(a.warmup + a.reps):
        for k, fn in paths:
            s = sets[r % a.sets]
            clear(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(s, kw)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                first[k] = {n: float(v.detach()) for n, v in out.items()}
    res = dict(shape=dict(B=B, Q=Q, L=L, pred=[HP, HP], canvas=[HP, HP], G=list(COUNTS), classes=CLASSES, rows=L * sum(COUNTS)), sets=a.sets, reps=a.reps,
               device=torch.cuda.get_device_name(0))
    for k, _ in paths:
        v = np.array(times[k])
        res[k] = dict(ms=round(float(np.median(v)), 3), ms_p25=round(float(np.percentile(v, 25)), 3), ms_p75=round(float(np.percentile(v, 75)), 3),
                      ms_min=round(float(v.min()), 3), ms_max=round(float(v.max()), 3))
    for k, fn in paths:
        res[k].update(census(fn, sets[0], kw))
    res['largest_relative_loss_difference'] = max(abs(first['new'][n] - first['composed_per_layer'][n]) / max(abs(first['composed_per_layer'][n]), 1e-12)
                                                  for n in first['new'])
    res['faster'] = bool(res['new']['ms_p75'] < res['composed_per_layer']['ms_p25'])
    res['reference_statements_as_torch_ops'] = 'not measured: the tree filter and the MST of the reference are a compiled extension without a torch form'
    res['kernels'] = kernels(dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
