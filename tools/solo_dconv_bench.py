#!/usr/bin/env python3
"""Developer measurement of the dynamic mask convolution of the SOLOv2-style heads on the GPU box, at the configs' shape: B = 2, E = 256, a
mask feature of 200 x 336, num_grids 40 / 36 / 24 / 16 / 12.

  train      20 instances per image spread over the five levels, one cell named twice; student plus independent teacher, forward + backward
             of ``(masks * g).sum()`` with gradients to the student's kernel maps and feature:
               hip    boxinstseg_amd.solo_dynamic_masks_pair (csrc/solo_dconv.hip)
               torch  the reference's op sequence (tests/solo_conv_ref.py: the per-level gather, one F.conv2d per (level, image), the cats,
                      the sigmoid) as torch ops on the same GPU, student with autograd and teacher under no_grad
             Both warmed, then timed interleaved in one process between device events (median, p25, p75 over the samples); before timing
             masks and gradients of the two are compared.  launches: kernels in torch's profiler trace of one call; host_syncs: the
             synchronising calls torch's sync debug mode reports.
  rows_100 / rows_500   the test-time product, solo_candidate_masks against F.conv2d(seg, kernels[rows]).sigmoid(), the same feature.
  per kernel  the time of one C-ABI call between device events in a back-to-back window (``event_us``; forward = two launches, backward =
             four), or the kernel's own time where ``--kernel-stats`` hands in rocprofv3's kernel-stats CSV of a ``--trace-only SHAPE`` run;
             needed_bytes = what must move (forward: the feature of the images that have rows once + the masks written; backward: the
             feature once, grad_out and the saved masks read, the feature's size written); its share of the achievable HBM rate; for
             rows_500 the share of the 157 TFLOP/s fp32 matrix peak (2 * rows * E * H * W flop).
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r19_solo_dconv_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from corr_bench import count_launches, count_syncs
from seg_paste_bench import timed
from tests import solo_conv_ref as R

B, E, HW, GRIDS = 2, 256, (200, 336), [40, 36, 24, 16, 12]
COUNTS = [[6, 5], [5, 5], [4, 4], [3, 4], [2, 2]]                            # 20 instances per image
HBM_ACHIEVABLE = 6.29e12            # bytes / s, a float4 copy on this part (8.0e12 is the data sheet's figure)
FP32_MATRIX_PEAK = 157.3e12         # flop / s, v_mfma_f32_32x32x2_f32


def make(dev, seed):
    case = R.make_case(seed, B, E, *HW, GRIDS, COUNTS, dups=[(0, 0, 2)])
    feat, maps, order, g = R.to_torch(case, torch.float32, dev)
    return feat, maps, order, g


def hip_step(s, t, order, g):
    from boxinstseg_amd import solo_dynamic_masks_pair
    for x in (s[0], *s[1]):
        x.grad = None
    s_masks, t_masks, _ = solo_dynamic_masks_pair(s[1], t[1], order, s[0], t[0])
    (R.cat_levels(s_masks) * g).sum().backward()
    return s_masks, t_masks


def torch_step(s, t, order, g):
    for x in (s[0], *s[1]):
        x.grad = None
    s_masks, _ = R.dynamic_masks(s[1], order, s[0])
    with torch.no_grad():
        t_masks, _ = R.dynamic_masks(t[1], order, t[0])
    (R.cat_levels(s_masks) * g).sum().backward()
    return s_masks, t_masks


def event_us(fn, reps=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    v = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        v.append(e0.elapsed_time(e1) * 1e3 / reps)
    return round(float(np.median(v)), 2)


def abi_calls(feat, maps, order, g):
    """One forward call and one backward call of the C ABI on preallocated tensors: nothing but the library's launches is timed."""
    from boxinstseg_amd import _lib, solo_conv as SC
    from boxinstseg_amd._common import current_stream
    lib, dev = _lib.load(), feat.device
    plan = SC._plan(maps, order, feat, True, None)
    out, img = SC._call_forward(plan, feat, maps)
    head = (feat.data_ptr(), B, E, *HW, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), len(maps), plan.layout,
            plan.cells.data_ptr(), _lib.int_array(plan.counts), plan.N, plan.act)
    gf, gm = torch.empty_like(feat), [torch.empty_like(m) for m in maps]
    nbytes = lib.bxi_solo_dconv_backward_workspace_bytes(plan.N, B, E, *HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fbytes = lib.bxi_solo_dconv_forward_workspace_bytes(plan.N, B, E)
    gptr = _lib.ptr_array([m.data_ptr() for m in gm])
    st = current_stream(dev)
    fwd = lambda: _lib.check('fwd', lib.bxi_solo_dconv_forward_f32(*head, out.data_ptr(), img.data_ptr(), plan.status.data_ptr(), ws.data_ptr(), fbytes, st))       # noqa: E731
    bwd = lambda: _lib.check('bwd', lib.bxi_solo_dconv_backward_f32(*head, out.data_ptr(), g.data_ptr(), gf.data_ptr(), gptr,              # noqa: E731
                                                                    plan.status.data_ptr(), ws.data_ptr(), nbytes, st))
    return plan, fwd, bwd, nbytes


def rows_case(dev, n):
    rng = np.random.default_rng(7 + n)
    seg = torch.from_numpy((0.5 * rng.standard_normal((1, E, *HW))).astype(np.float32)).to(dev)
    kern = torch.from_numpy((rng.standard_normal((sum(s * s for s in GRIDS), E)) / 16).astype(np.float32)).to(dev)
    rows = torch.from_numpy(rng.permutation(kern.shape[0])[:n]).to(dev)
    return seg, kern, rows


def traced(path):
    """rocprofv3's kernel-stats CSV -> {kernel: average microseconds}."""
    out = {}
    if path and os.path.exists(path):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                for key in ('dconv_gather_kernel', 'dconv_fwd_kernel', 'dconv_bwd_kernel', 'dconv_reduce_kernel', 'dconv_scatter_kernel'):
                    if key in row['Name']:
                        out[key] = round(float(row['AverageNs']) / 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_solo_dconv_bench.json'))
    ap.add_argument('--trace-only', choices=['train', 'rows_100', 'rows_500'], help='run one shape a few times (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--kernel-stats', nargs=3, metavar=('TRAIN', 'ROWS100', 'ROWS500'), help="rocprofv3's *_kernel_stats.csv of the three --trace-only runs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('solo_dconv_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    from boxinstseg_amd import solo_candidate_masks
    dev = torch.device('cuda:0')
    if args.trace_only:
        if args.trace_only == 'train':
            feat, maps, order, g = make(dev, 1)
            _, fwd, bwd, _ = abi_calls(feat, maps, order, g)
            for _ in range(10):
                fwd()
                bwd()
        else:
            seg, kern, rows = rows_case(dev, int(args.trace_only.split('_')[1]))
            for _ in range(10):
                solo_candidate_masks(seg, kern, rows)
        torch.cuda.synchronize()
        return
    stats_csv = args.kernel_stats or (None, None, None)
    pix = HW[0] * HW[1]
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, E=E, feature=HW, num_grids=GRIDS, instances_per_image=20),
           'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'fp32_matrix_peak_flops': FP32_MATRIX_PEAK}
    # ---- training shape ------------------------------------------------------------------------------------------------------------
    feat, maps, order, g = make(dev, 1)
    t_feat, t_maps, _, _ = make(dev, 2)
    s = (feat.requires_grad_(True), [m.requires_grad_(True) for m in maps])
    t = (t_feat, t_maps)
    a = hip_step(s, t, order, g)
    ga = [s[0].grad.clone()] + [m.grad.clone() for m in s[1]]
    b = torch_step(s, t, order, g)
    gb = [s[0].grad.clone()] + [m.grad.clone() for m in s[1]]
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())                                         # noqa: E731
    agree = dict(student_masks=rel(R.cat_levels(a[0]), R.cat_levels(b[0])), teacher_masks=rel(R.cat_levels(a[1]), R.cat_levels(b[1])),
                 grad_feat=rel(ga[0], gb[0]), grad_kernel=max(rel(x, y) for x, y in zip(ga[1:], gb[1:])))
    paths = {'hip': lambda: hip_step(s, t, order, g), 'torch': lambda: torch_step(s, t, order, g)}
    row = dict(max_relative_difference_hip_vs_torch=agree, **timed(paths))
    for k, f in paths.items():
        row[k]['launches'] = count_launches(f)
        row[k]['host_syncs'] = count_syncs(f)
    spread = (row['hip']['ms_p75'] - row['hip']['ms_p25']) + (row['torch']['ms_p75'] - row['torch']['ms_p25'])
    row['torch_minus_hip_ms'] = round(row['torch']['ms'] - row['hip']['ms'], 4)
    row['sum_of_p25_p75_spreads_ms'] = round(spread, 4)
    row['faster_by_more_than_the_spread'] = bool(row['torch']['ms'] - row['hip']['ms'] > spread)
    plan, fwd, bwd, nbytes = abi_calls(feat.detach(), [m.detach() for m in maps], order, g)
    tr = traced(stats_csv[0])
    need_f = 4 * (B * E * pix + plan.N * pix)
    need_b = 4 * (2 * B * E * pix + 2 * plan.N * pix)
    k = dict(forward=dict(event_us=event_us(fwd), needed_bytes=need_f), backward=dict(event_us=event_us(bwd), needed_bytes=need_b, workspace_bytes=nbytes))
    for name, kern_name in (('forward', 'dconv_fwd_kernel'), ('backward', 'dconv_bwd_kernel')):
        k[name]['kernel_us'] = tr.get(kern_name, 'not measured')
        us = tr.get(kern_name) or k[name]['event_us']
        k[name]['time_used_for_the_share'] = 'kernel_us' if kern_name in tr else 'event_us (the whole call)'
        k[name]['share_of_achievable_hbm'] = round(k[name]['needed_bytes'] / HBM_ACHIEVABLE / (us * 1e-6), 4)
    k['forward']['gather_kernel_us'] = tr.get('dconv_gather_kernel', 'not measured')
    k['backward']['reduce_kernel_us'] = tr.get('dconv_reduce_kernel', 'not measured')
    k['backward']['scatter_kernel_us'] = tr.get('dconv_scatter_kernel', 'not measured')
    row['per_call'] = k
    out['train'] = row
    # ---- test time -----------------------------------------------------------------------------------------------------------------
    for n, path in ((100, stats_csv[1]), (500, stats_csv[2])):
        seg, kern, rows = rows_case(dev, n)
        hip = lambda: solo_candidate_masks(seg, kern, rows)                                               # noqa: E731
        ref = lambda: F.conv2d(seg, kern[rows].view(n, E, 1, 1), stride=1).squeeze(0).sigmoid()           # noqa: E731
        r = dict(max_relative_difference_hip_vs_torch=rel(hip(), ref()), **timed({'hip': hip, 'torch': ref}))
        r['hip']['launches'], r['torch']['launches'] = count_launches(hip), count_launches(ref)
        tr = traced(path)
        us = tr.get('dconv_fwd_kernel') or r['hip']['ms'] * 1e3
        r['kernel_us'] = tr.get('dconv_fwd_kernel', 'not measured')
        r['time_used_for_the_shares'] = 'kernel_us' if tr else 'the hip path\'s event time (the whole call, torch.zeros and the allocation included)'
        r['needed_bytes'] = 4 * (E * pix + n * pix)
        r['share_of_achievable_hbm'] = round(r['needed_bytes'] / HBM_ACHIEVABLE / (us * 1e-6), 4)
        r['flop'] = 2 * n * E * pix
        r['share_of_fp32_matrix_peak'] = round(r['flop'] / FP32_MATRIX_PEAK / (us * 1e-6), 4)
        out[f'rows_{n}'] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
