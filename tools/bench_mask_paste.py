#!/usr/bin/env python3
"""Developer measurement of the test-time mask paste (csrc/mask_paste.hip) on the GPU box, at the COCO shape of a BoxInst
evaluation: canvas 800x1088 (logits 200x272 at stride 4), img_shape 800x1067, ori_shape 480x640, rescale=True.

Prints one JSON line: per N in {100, 500, 2000}
  kernel_us            mask_paste kernel alone, device events around >= 50 launches after warm-up;
  alg_bytes, hbm_frac  logits read + masks written, and that over kernel_us as a fraction of 8 TB/s;
  simple_test_ms       CondInstMaskHead.simple_test per image, host included (ends with the host arrays): the kernel path and
                       the torch composition it replaced (kept here as the A/B baseline), same box, same inputs;
  peak_MB              growth of max_memory_allocated during one simple_test call, both paths;
  d2h_ms               the mask buffer to the host: into pageable numpy memory (what paste_masks does) and into a pinned buffer
                       (allocated per call through torch's caching host allocator, and one buffer reused).
--quick: N = 2000 only, few repetitions (for a rocprofv3 run)."""
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
entry.build()
import boxinstseg_amd as bx
from boxinstseg_amd import dynamic as dyn

dev = torch.device('cuda:0')
QUICK = '--quick' in sys.argv
META = [dict(img_shape=(800, 1067, 3), ori_shape=(480, 640, 3))]
DIMS = (800, 1067, 480, 640)


def composed_simple_test(head, mask_feat, det_labels, det_params, det_coors, det_level_inds, img_metas, num_classes, rescale):
    """CondInstMaskHead.simple_test as it was before the kernel: torch ops over full-resolution float tensors."""
    counts = [int(p.size(0)) for p in det_params]
    img_inds = torch.cat([torch.full((c,), i, dtype=torch.long, device=mask_feat.device) for i, c in enumerate(counts)])
    logits = head.forward(mask_feat, torch.cat(det_params), torch.cat(det_coors), torch.cat(det_level_inds), img_inds)
    probs = dyn.aligned_bilinear(logits.sigmoid(), head.out_stride)
    results = []
    for cur, labels, meta in zip(probs.split(counts, dim=0), det_labels, img_metas):
        ih, iw = meta['img_shape'][:2]
        cur = cur[:, :, :ih, :iw]
        if rescale and cur.size(0):
            oh, ow = meta['ori_shape'][:2]
            cur = F.interpolate(cur, (oh, ow), mode='bilinear', align_corners=False)
        masks = (cur.squeeze(1) > 0.5).cpu().numpy().astype(np.uint8)
        lab = labels.detach().cpu().numpy()
        results.append([masks[lab == c] for c in range(num_classes)])
    return results


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def main():
    torch.manual_seed(0)
    head = bx.CondInstMaskHead(in_channels=8, in_stride=8, out_stride=4).to(dev)
    feat = torch.randn(1, 8, 100, 136, device=dev)
    out = {'shape': 'canvas 800x1088, img_shape 800x1067, ori 480x640, rescale', 'gpu': torch.cuda.get_device_name(0)}
    for N in ((2000,) if QUICK else (100, 500, 2000)):
        params = torch.randn(N, head.num_gen_params, device=dev) * 0.3
        coors = torch.rand(N, 2, device=dev) * torch.tensor([1088.0, 800.0], device=dev)
        lvl = torch.randint(0, 5, (N,), device=dev)
        labels = torch.randint(0, 80, (N,), device=dev)
        img = torch.zeros(N, dtype=torch.long, device=dev)
        with torch.no_grad():
            logits = head(feat, params, coors, lvl, img)
        offsets, _ = dyn.paste_order(img, labels, [N], [480 * 640], 80)
        total = N * 480 * 640
        launch = lambda: dyn._paste(logits, img, offsets, [DIMS], total, 4, 0.5)
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        reps = 10 if QUICK else 50
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        torch.cuda.synchronize()
        kernel_us = a.elapsed_time(b) / reps * 1e3
        alg = N * 200 * 272 * 4 + total
        r = dict(kernel_us=round(kernel_us, 1), alg_bytes=alg, hbm_frac=round(alg / (kernel_us * 1e-6) / 8e12, 3))
        if not QUICK:
            args = (feat, [labels], [params], [coors], [lvl], META, 80)
            new = lambda: head.simple_test(*args, rescale=True)
            old = lambda: composed_simple_test(head, *args, True)
            with torch.no_grad():
                r['simple_test_ms'] = dict(kernel=round(wall_ms(new, 5), 2), composed=round(wall_ms(old, 3), 2))
                r['simple_test_speedup'] = round(r['simple_test_ms']['composed'] / r['simple_test_ms']['kernel'], 2)
                r['peak_MB'] = dict(kernel=round(peak_mb(new), 1), composed=round(peak_mb(old), 1))
            masks = launch()
            torch.cuda.synchronize()
            pageable = lambda: torch.from_numpy(np.empty(total, np.uint8)).copy_(masks)
            pinned_alloc = lambda: torch.empty(total, dtype=torch.uint8, pin_memory=True).copy_(masks)
            keep = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            pinned_reused = lambda: keep.copy_(masks)
            r['d2h_ms'] = dict(pageable=round(wall_ms(pageable, 5), 2), pinned_cached_alloc=round(wall_ms(pinned_alloc, 5), 2),
                               pinned_reused=round(wall_ms(pinned_reused, 5), 2))
        out[f'N{N}'] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
