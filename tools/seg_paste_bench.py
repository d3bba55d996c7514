#!/usr/bin/env python3
"""Developer measurement of the final-mask kernel of the SOLOv2-style heads on the GPU box, at the configs' size: 300 candidates on a
200 x 304 feature map, canvas 800 x 1216, img_shape 800 x 1199, ori_shape 427 x 640; 100 kept masks and 20.

  kernel     boxinstseg_amd.seg_paste (csrc/seg_paste.hip): the paste step of _seg_tail, two launches
  composed   what _seg_tail ran before, restated here: seg_preds[keep_inds] -> F.interpolate to the canvas -> crop -> F.interpolate to
             ori_shape -> > mask_thr
  Both are warmed, then timed interleaved in one process between two device events over as many repetitions as make a window of at least
  0.5 s each (median, p25, p75, min, max in ms); before timing the two outputs are compared under the tie rule of tests/seg_paste_ref.py.
  peak_bytes      torch's peak allocation of one call above its inputs
  format_results  solo_format_results against the restated per-mask loop (sum / where / min / max / .cpu per mask) at 100 masks: wall
                  clock around the call, its kernel launches and the synchronising calls torch reports
  needed_bytes    what the kernel must move: the n source rows read once (n * h * w * 4) plus n * out_h * out_w bytes written; the
                  kernel's share of the achievable HBM rate is needed_bytes / HBM_ACHIEVABLE / kernel time, with the kernel time
                  from `rocprofv3 --kernel-trace --stats` in a run of its own (--trace-only runs just the kernel path a few times for it;
                  --kernel-us takes the traced time of seg_paste_kernel back in).
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r18_seg_paste_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from corr_bench import count_launches, count_syncs, stats
from tests import matrix_nms_ref as R
from tests import seg_paste_ref as S

N_ALL, HW, CROP, OUT, THR = 300, (200, 304), (800, 1199), (427, 640), 0.5
UP = (4 * HW[0], 4 * HW[1])
META = dict(img_shape=CROP + (3,), ori_shape=OUT + (3,))
HBM_ACHIEVABLE = 6.29e12            # bytes / s, a float4 copy on this part (8.0e12 is the data sheet's figure)


def composed(probs, keep):
    kept = F.interpolate(probs[keep].unsqueeze(0), size=UP, mode='bilinear')[:, :, :CROP[0], :CROP[1]]
    return F.interpolate(kept, size=OUT, mode='bilinear').squeeze(0) > THR


def kernel(probs, keep):
    from boxinstseg_amd import seg_paste
    return seg_paste(probs, keep, HW, META, THR)[0]


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(paths, window_s=0.5, samples=15):
    """Interleaved: every sample times each path once, `reps` calls between two events; reps sized so a path's samples add up to the window."""
    for f in paths.values():
        for _ in range(20):
            f()
    # sized from a warmed sample with half as much again, then checked: a path whose window came out short is timed again with more
    reps = {k: max(1, int(np.ceil(1.5 * window_s * 1e3 / samples / max(event_ms(f, 50), 1e-3)))) for k, f in paths.items()}
    while True:
        ts = {k: [] for k in paths}
        for _ in range(samples):
            for k, f in paths.items():
                ts[k].append(event_ms(f, reps[k]))
        short = [k for k, v in ts.items() if sum(v) * reps[k] < window_s * 1e3]
        if not short:
            break
        for k in short:
            reps[k] *= 2
    return {k: dict(stats(v), reps_per_sample=reps[k], samples=samples, window_ms=round(sum(v) * reps[k], 1)) for k, v in ts.items()}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def loop_format(res, num_classes):
    """The per-mask loop of single_stage_ts.py:88-103 restated where the reference runs it -- on the device tensors: the area test, where,
    the four extremes and the score each come to the host on their own."""
    rows = [[] for _ in range(num_classes)]
    kept_masks = [[] for _ in range(num_classes)]
    kept_scores = [[] for _ in range(num_classes)]
    for i in range(len(res.masks)):
        mask, c = res.masks[i], int(res.labels[i])
        if not bool(mask.sum() > 0):
            continue
        kept_masks[c].append(mask.cpu())
        kept_scores[c].append(res.scores[i].cpu())
        ys, xs = torch.where(mask)
        rows[c].append([xs.min().cpu().numpy(), ys.min().cpu().numpy(), xs.max().cpu().numpy() + 1, ys.max().cpu().numpy() + 1,
                        res.scores[i].cpu().numpy()])
    return [np.array(r) if r else np.zeros((0, 5)) for r in rows], (kept_masks, kept_scores)


def wall(fn, reps):
    fn()
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return stats(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_seg_paste_bench.json'))
    ap.add_argument('--trace-only', action='store_true', help='run the kernel path alone (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--kernel-us', type=float, nargs=2, metavar=('N100', 'N20'), help='traced seg_paste_kernel time at 100 and 20 kept masks')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seg_paste_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import types
    import boxinstseg_amd as bx
    from boxinstseg_amd.seg_paste import paste_results
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(1)
    small = torch.from_numpy(R.disc_probs(rng, N_ALL, 25, 38)).to(dev)
    probs = small.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()           # blocky discs at 200 x 304
    order = torch.from_numpy(rng.permutation(N_ALL)).to(dev)
    if args.trace_only:
        for n in (100, 20):
            for _ in range(10):
                kernel(probs, order[:n])
        torch.cuda.synchronize()
        return
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(n_all=N_ALL, featmap=HW, canvas=UP, img_shape=CROP, ori_shape=OUT, mask_thr=THR),
           'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE}
    for n, kernel_us in zip((100, 20), args.kernel_us or (None, None)):
        keep = order[:n]
        a, b = kernel(probs, keep).view(torch.uint8).cpu().numpy(), composed(probs, keep).view(torch.uint8).cpu().numpy()
        sub = np.arange(0, n, max(n // 4, 1))                                             # the float64 truth of a few masks
        pg = S.check_tie(a[sub], probs.cpu().numpy(), keep.cpu().numpy()[sub], UP, CROP, OUT, THR, f'kernel n={n}')
        S.check_tie(b[sub], probs.cpu().numpy(), keep.cpu().numpy()[sub], UP, CROP, OUT, THR, f'composed n={n}')
        needed = n * HW[0] * HW[1] * 4 + n * OUT[0] * OUT[1]
        row = dict(differing_bytes=int((a != b).sum()), differing_bytes_outside_band_of_sampled=int(((a[sub] != b[sub]) & (np.abs(pg - THR) > S.TIE)).sum()),
                   needed_bytes=needed, **timed({'kernel': lambda: kernel(probs, keep), 'composed': lambda: composed(probs, keep)}))
        row['kernel']['peak_bytes'] = peak_bytes(lambda: kernel(probs, keep))
        row['composed']['peak_bytes'] = peak_bytes(lambda: composed(probs, keep))
        row['kernel']['launches'] = count_launches(lambda: kernel(probs, keep))
        row['composed']['launches'] = count_launches(lambda: composed(probs, keep))
        row['seg_paste_kernel_us'] = kernel_us if kernel_us is not None else 'not measured'
        row['share_of_achievable_hbm'] = round(needed / HBM_ACHIEVABLE / (kernel_us * 1e-6), 4) if kernel_us else 'not measured'
        out[f'kept_{n}'] = row
    keep = order[:100]
    res = paste_results(types.SimpleNamespace(scores=torch.rand(100, device=dev), labels=torch.randint(0, 80, (100,), device=dev), masks=None),
                        probs, keep, HW, META, THR)
    out['format_results_100'] = {}
    for name, fn in (('solo_format_results', lambda: bx.solo_format_results(res, 80)), ('per_mask_loop', lambda: loop_format(res, 80))):
        out['format_results_100'][name] = dict(wall(fn, 7), launches=count_launches(fn), host_syncs=count_syncs(fn))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
