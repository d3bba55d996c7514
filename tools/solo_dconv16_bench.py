#!/usr/bin/env python3
"""Developer measurement of the half-precision dynamic mask convolution (csrc/solo_dconv16.hip) on the GPU box, at the shape of
tools/solo_dconv_bench.py (R19-1): B = 2, E = 256, a mask feature of 200 x 336, num_grids 40 / 36 / 24 / 16 / 12, fp16 tensors in.

  train      20 instances per image over the five levels, one cell named twice; student plus independent teacher, forward + backward of
             ``(masks * g).sum()`` with gradients to the student's kernel maps and feature.  Three legs on the SAME fp16 tensors:
               half     solo_dynamic_masks_pair(compute='half')                 (the tensors read in place, fp16 masks and gradients)
               upcast   solo_dynamic_masks_pair(...), the default               (what the parent commit does with them: fp32 copies of
                        both features and all maps, fp32 masks, the gradients cast back)
               torch    the reference's op sequence (tests/solo_conv_ref.py) as torch ops on the fp16 tensors
             and ``half`` again on bf16 tensors.  Inputs are COLD: every call takes the next of SETS input sets (4 x 2 features of 69 MB,
             beyond the 256 MB last-level cache), so no leg finds its feature in a cache.  All legs warmed, then timed interleaved in one
             process between device events (median, p25, p75).  ``accept``: p75 of half below p25 of upcast.
  rows_100 / rows_500   the test-time product on the same feature: solo_candidate_masks(compute='half') / the default / torch's
             F.conv2d(seg, kernels[rows]).sigmoid() in fp16.
  per call   one C-ABI call (forward: two launches, backward: four) between device events in a back-to-back window, the bytes it must
             move (forward: the feature once + the masks; backward: the feature once, grad_out and the saved masks, grad_feat written) and
             their share of the achievable HBM rate -- or the kernels' own times where ``--kernel-stats`` hands in rocprofv3's kernel-stats
             CSVs of the three ``--trace-only SHAPE`` runs; launches per leg from torch's profiler; peak memory above the inputs per leg.
There is no pass / fail ratio against torch.  Writes one JSON object to --out (default profiles/r26_solo_dconv16_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from corr_bench import count_launches
from seg_paste_bench import peak_bytes, timed
from solo_dconv_bench import B, COUNTS, E, GRIDS, HBM_ACHIEVABLE, HW, event_us
from tests import solo_conv_ref as R

SETS = 4
HALF_MATRIX_PEAK = 2.5e15           # flop / s, v_mfma_f32_32x32x16_{f16,bf16}, dense


def make_sets(dev, dtype, seed):
    """SETS x (student, teacher, grid_order, g) in ``dtype``; the feature and the maps differ from set to set, the grid_order does not."""
    case = R.make_case(seed, B, E, *HW, GRIDS, COUNTS, dups=[(0, 0, 2)])
    _, _, order, g = R.to_torch(case, dtype, dev)
    rng = torch.Generator(device=dev).manual_seed(seed)
    sets = []
    for _ in range(SETS):
        pair = []
        for leaf in (True, False):
            feat = (0.5 * torch.randn(B, E, *HW, device=dev, generator=rng)).to(dtype).requires_grad_(leaf)
            maps = [(torch.randn(B, E, S, S, device=dev, generator=rng) / 16).to(dtype).requires_grad_(leaf) for S in GRIDS]
            pair.append((feat, maps))
        sets.append(pair)
    return sets, order, g


class Rotor:
    """The next input set on every call."""

    def __init__(self, sets):
        self.sets, self.at = sets, 0

    def __call__(self):
        self.at = (self.at + 1) % len(self.sets)
        return self.sets[self.at]


def train_legs(sets, order, g):
    from boxinstseg_amd import solo_dynamic_masks_pair
    rot = Rotor(sets)
    g32 = g.float()

    def clear(s):
        for x in (s[0], *s[1]):
            x.grad = None

    def half():
        s, t = rot()
        clear(s)
        s_masks, t_masks, _ = solo_dynamic_masks_pair(s[1], t[1], order, s[0], t[0], compute='half')
        (R.cat_levels(s_masks) * g).sum().backward()
        return s_masks, t_masks

    def upcast():
        s, t = rot()
        clear(s)
        s_masks, t_masks, _ = solo_dynamic_masks_pair(s[1], t[1], order, s[0], t[0])
        (R.cat_levels(s_masks) * g32).sum().backward()
        return s_masks, t_masks

    def torch_ops():
        s, t = rot()
        clear(s)
        s_masks, _ = R.dynamic_masks(s[1], order, s[0])
        with torch.no_grad():
            t_masks, _ = R.dynamic_masks(t[1], order, t[0])
        (R.cat_levels(s_masks) * g).sum().backward()
        return s_masks, t_masks

    return {'half': half, 'upcast': upcast, 'torch': torch_ops}, rot


def abi_calls(feat, maps, order, g):
    """One forward call and one backward call of the half C ABI on preallocated tensors: nothing but the library's launches is timed."""
    from boxinstseg_amd import _lib, solo_conv as SC
    from boxinstseg_amd._common import current_stream
    lib, dev = _lib.load(), feat.device
    plan = SC._plan(maps, order, feat, True, None)
    plan.out_dtype = feat.dtype
    code = SC._HALF[feat.dtype]
    out, img = SC._call_forward(plan, feat, maps)
    head = (feat.data_ptr(), code, B, E, *HW, _lib.ptr_array([m.data_ptr() for m in maps]), _lib.int_array(plan.grids), len(maps), plan.layout,
            plan.cells.data_ptr(), _lib.int_array(plan.counts), plan.N, plan.act)
    gf, gm = torch.empty_like(feat), [torch.empty_like(m) for m in maps]
    nbytes = lib.bxi_solo_dconv16_backward_workspace_bytes(plan.N, B, E, *HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fbytes = lib.bxi_solo_dconv16_forward_workspace_bytes(plan.N, B, E)
    gptr = _lib.ptr_array([m.data_ptr() for m in gm])
    st = current_stream(dev)
    fwd = lambda: _lib.check('fwd', lib.bxi_solo_dconv16_forward(*head, out.data_ptr(), code, img.data_ptr(), plan.status.data_ptr(),    # noqa: E731
                                                                 ws.data_ptr(), fbytes, st))
    bwd = lambda: _lib.check('bwd', lib.bxi_solo_dconv16_backward(*head, out.data_ptr(), g.data_ptr(), code, gf.data_ptr(), gptr,        # noqa: E731
                                                                  plan.status.data_ptr(), ws.data_ptr(), nbytes, st))
    return plan, fwd, bwd, nbytes


def rows_case(dev, n, copies):
    rng = torch.Generator(device=dev).manual_seed(7 + n)
    segs = [(0.5 * torch.randn(1, E, *HW, device=dev, generator=rng)).half() for _ in range(copies)]
    kern = (torch.randn(sum(s * s for s in GRIDS), E, device=dev, generator=rng) / 16).half()
    rows = torch.randperm(kern.shape[0], device=dev, generator=rng)[:n]
    return segs, kern, rows


def traced(path):
    """rocprofv3's kernel-stats CSV -> {kernel: average microseconds} for the library's kernels (the gather as forward / backward form)."""
    out = {}
    if path and os.path.exists(path):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                for key in ('dconv_gather_kernel', 'dconv16_fwd_kernel', 'dconv16_bwd_kernel', 'dconv_reduce_kernel', 'dconv_scatter_kernel'):
                    if key in row['Name']:
                        form = '<Kr16>' if 'Kr16>' in row['Name'] else '<Kt16>' if 'Kt16>' in row['Name'] else ''      # the gather's layout tag
                        out[key + form] = round(float(row['AverageNs']) / 1e3, 2)
    return out


def rel(x, y):
    return float((x.float() - y.float()).abs().max() / y.float().abs().max())


def accept(row, a='half', b='upcast'):
    row[f'p75_of_{a}_ms'], row[f'p25_of_{b}_ms'] = row[a]['ms_p75'], row[b]['ms_p25']
    row[f'accept_p75_of_{a}_below_p25_of_{b}'] = bool(row[a]['ms_p75'] < row[b]['ms_p25'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_solo_dconv16_bench.json'))
    ap.add_argument('--trace-only', choices=['train', 'rows_100', 'rows_500'], help='run one shape a few times (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--kernel-stats', nargs=3, metavar=('TRAIN', 'ROWS100', 'ROWS500'), help="rocprofv3's *_kernel_stats.csv of the three --trace-only runs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('solo_dconv16_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    from boxinstseg_amd import solo_candidate_masks
    dev = torch.device('cuda:0')
    pix = HW[0] * HW[1]
    if args.trace_only:
        if args.trace_only == 'train':
            sets, order, g = make_sets(dev, torch.float16, 1)
            s0 = sets[0][0]
            _, fwd, bwd, _ = abi_calls(s0[0].detach(), [m.detach() for m in s0[1]], order, g)
            for _ in range(10):
                fwd()
                bwd()
        else:
            seg, kern, rows = rows_case(dev, int(args.trace_only.split('_')[1]), 1)
            for _ in range(10):
                solo_candidate_masks(seg[0], kern, rows, compute='half')
        torch.cuda.synchronize()
        return
    stats_csv = args.kernel_stats or (None, None, None)
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, E=E, feature=HW, num_grids=GRIDS, instances_per_image=20, dtype='float16'),
           'input_sets_rotated': SETS, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'half_matrix_peak_flops': HALF_MATRIX_PEAK}
    # ---- training shape ------------------------------------------------------------------------------------------------------------
    sets, order, g = make_sets(dev, torch.float16, 1)
    legs, rot = train_legs(sets, order, g)
    res = {}
    for k, f in legs.items():                                                 # every leg on the same input set, for the comparison
        rot.at = 0
        res[k] = f()
    agree = {k: dict(student_masks=rel(R.cat_levels(res[k][0]), R.cat_levels(res['torch'][0])),
                     teacher_masks=rel(R.cat_levels(res[k][1]), R.cat_levels(res['torch'][1]))) for k in ('half', 'upcast')}
    row = dict(max_relative_difference_vs_torch_fp16=agree, **timed(legs))
    for k, f in legs.items():
        row[k]['launches'] = count_launches(f)
        row[k]['peak_bytes_above_inputs'] = peak_bytes(f)
    accept(row)
    s0 = sets[0][0]
    plan, fwd, bwd, nbytes = abi_calls(s0[0].detach(), [m.detach() for m in s0[1]], order, g)
    need_f = 2 * (B * E * pix + plan.N * pix)
    need_b = 2 * (2 * B * E * pix + 2 * plan.N * pix)
    k = dict(forward=dict(event_us=event_us(fwd), needed_bytes=need_f), backward=dict(event_us=event_us(bwd), needed_bytes=need_b, workspace_bytes=nbytes))
    tr = traced(stats_csv[0])
    for name, kern_name in (('forward', 'dconv16_fwd_kernel'), ('backward', 'dconv16_bwd_kernel')):
        k[name]['kernel_us'] = tr.get(kern_name, 'not measured')
        us = tr.get(kern_name) or k[name]['event_us']
        k[name]['time_used_for_the_share'] = 'kernel_us' if kern_name in tr else 'event_us (the whole call on ONE warm input set)'
        k[name]['share_of_achievable_hbm'] = round(k[name]['needed_bytes'] / HBM_ACHIEVABLE / (us * 1e-6), 4)
    k['other_kernels_us'] = {n: v for n, v in tr.items() if n not in ('dconv16_fwd_kernel', 'dconv16_bwd_kernel')} or 'not measured'
    row['per_call'] = k
    out['train'] = row
    del sets, legs, res
    torch.cuda.empty_cache()
    sets, order, g = make_sets(dev, torch.bfloat16, 1)
    out['train_bf16'] = dict(timed({'half': train_legs(sets, order, g)[0]['half']}))
    del sets
    torch.cuda.empty_cache()
    # ---- test time -----------------------------------------------------------------------------------------------------------------
    for n, path in ((100, stats_csv[1]), (500, stats_csv[2])):
        segs, kern, rows = rows_case(dev, n, 2 * SETS)
        rot = Rotor(segs)
        legs = {'half': lambda: solo_candidate_masks(rot(), kern, rows, compute='half'),
                'upcast': lambda: solo_candidate_masks(rot(), kern, rows),
                'torch': lambda: F.conv2d(rot(), kern[rows].view(n, E, 1, 1), stride=1).squeeze(0).sigmoid()}
        ref = F.conv2d(segs[0], kern[rows].view(n, E, 1, 1), stride=1).squeeze(0).sigmoid()
        r = dict(max_relative_difference_vs_torch_fp16={k: rel(solo_candidate_masks(segs[0], kern, rows, **kw), ref)
                                                        for k, kw in (('half', dict(compute='half')), ('upcast', {}))}, **timed(legs))
        for k, f in legs.items():
            r[k]['launches'] = count_launches(f)
            r[k]['peak_bytes_above_inputs'] = peak_bytes(f)
        accept(r)
        accept(r, 'half', 'torch')
        tr = traced(path)
        us = tr.get('dconv16_fwd_kernel') or r['half']['ms'] * 1e3
        r['kernel_us'] = tr.get('dconv16_fwd_kernel', 'not measured')
        r['needed_bytes'] = 2 * (E * pix + n * pix)
        r['flop'] = 2 * n * E * pix
        r['time_used_for_the_shares'] = 'kernel_us' if tr else "the half leg's event time (the whole call, torch.zeros and the allocation included)"
        r['share_of_achievable_hbm'] = round(r['needed_bytes'] / HBM_ACHIEVABLE / (us * 1e-6), 4)
        r['share_of_half_matrix_peak'] = round(r['flop'] / HALF_MATRIX_PEAK / (us * 1e-6), 4)
        out[f'rows_{n}'] = r
        del segs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
