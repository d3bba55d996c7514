#!/usr/bin/env python3
"""Developer measurement of BoxLevelSet's mask predictions (csrc/solo_dconv_level.hip) on the GPU box, at the configs' shape: B = 2,
E = 256, a mask feature of 200 x 336, num_grids 40 / 36 / 24 / 16 / 12, level sizes 200 x 336 (twice), 100 x 168, 50 x 84 (twice), and
20 boxes per image assigned by ``box_solov2_targets`` with the configs' scale ranges.

  train      forward + backward of ``sum_l (rows_l * g_l).sum()`` with gradients to the kernel maps and the feature.  Three legs:
               reference   the reference's statements as torch ops (tests/box_solo_masks_ref.py): the grouped convolution over ALL
                           3 872 cells, F.interpolate of every level's whole result, the boolean selection
               composed    the composition available before this path: solo_dynamic_masks(sigmoid=False) at full resolution, then
                           F.interpolate per level
               kernel      box_solov2_ins_preds
             Inputs are COLD: every call takes the next of SETS input sets (features of 138 MB each, beyond the 256 MB last-level cache).
             All legs warmed, then timed interleaved in one process between device events, one call per sample (median, p25, p75).
             Per leg: device launches (torch's profiler), host synchronisations (torch's sync debug mode) and peak memory above the inputs.
  kernels    the library's own launches of one forward and one backward call, each between two device events placed by the launch hook
             (warm inputs), and for the two new kernels the bytes they must move and their share of the achievable HBM rate.
  test time  box_solov2_get_seg_single_kernels(cate, mask_feat, kernels) against box_solov2_get_seg_single fed with the [3872, h, w]
             tensor of all cells' probabilities (which is given to it ready-made: producing it is not in its time).
There is no pass / fail figure.  Writes one JSON object to --out (default profiles/r27_box_solo_masks_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import ctypes as C
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from corr_bench import count_launches, stats
from seg_paste_bench import peak_bytes
from solo_dconv_bench import HBM_ACHIEVABLE
from tests import box_solo_masks_ref as R

B, E, HW, GRIDS, STRIDES = 2, 256, (200, 336), [40, 36, 24, 16, 12], [8, 8, 16, 32, 32]
SIZES = [(200, 336), (200, 336), (100, 168), (50, 84), (50, 84)]
CANVAS = (800, 1344)
SCALE_RANGES = [(1, 96), (48, 192), (96, 384), (192, 768), (384, 2048)]
SETS = 3


def make_targets(dev, seed, boxes_per_image=20):
    from boxinstseg_amd import box_solov2_set_cells, box_solov2_targets
    rng = np.random.default_rng(seed)
    boxes, labels, masks = [], [], []
    for _ in range(B):
        bx, m = [], np.zeros((boxes_per_image, *CANVAS), np.uint8)
        for i in range(boxes_per_image):
            side = float(np.exp(rng.uniform(np.log(24), np.log(700))))
            w, h = min(side * rng.uniform(0.6, 1.6), CANVAS[1] - 2), min(side * rng.uniform(0.6, 1.6), CANVAS[0] - 2)
            x1, y1 = rng.uniform(0, CANVAS[1] - w - 1), rng.uniform(0, CANVAS[0] - h - 1)
            bx.append([x1, y1, x1 + w, y1 + h])
            m[i, int(y1):int(y1 + h) + 1, int(x1):int(x1 + w) + 1] = 1
        boxes.append(torch.tensor(bx, dtype=torch.float32, device=dev))
        labels.append(torch.from_numpy(rng.integers(0, 80, boxes_per_image)).to(dev))
        masks.append(torch.from_numpy(m).to(dev))
    tg = box_solov2_targets(boxes, labels, masks, SIZES, strides=STRIDES, num_grids=GRIDS, scale_ranges=SCALE_RANGES, sigma=0.2, num_classes=80)
    cells = box_solov2_set_cells(tg)
    labels_lb = [tg.ins_ind_labels[l].view(B, S * S) for l, S in enumerate(GRIDS)]
    return cells, labels_lb, [[int(tg.counts[l][b][1]) for b in range(B)] for l in range(len(GRIDS))]


def make_sets(dev, seed, counts):
    rng = torch.Generator(device=dev).manual_seed(seed)
    sets = []
    for _ in range(SETS):
        feat = (0.5 * torch.randn(B, E, *HW, device=dev, generator=rng)).requires_grad_(True)
        maps = [(torch.randn(B, E, S, S, device=dev, generator=rng) / 16).requires_grad_(True) for S in GRIDS]
        sets.append((feat, maps))
    g = [torch.randn(sum(c), oh, ow, device=dev, generator=rng) for c, (oh, ow) in zip(counts, SIZES)]
    return sets, g


class Rotor:
    """The next input set on every call."""

    def __init__(self, sets):
        self.sets, self.at = sets, 0

    def __call__(self):
        self.at = (self.at + 1) % len(self.sets)
        feat, maps = self.sets[self.at]
        for x in (feat, *maps):
            x.grad = None
        return feat, maps


def train_legs(sets, g, cells, labels_lb):
    from boxinstseg_amd import box_solov2_ins_preds, solo_dynamic_masks
    rot = Rotor(sets)

    def finish(rows):
        sum((r * x).sum() for r, x in zip(rows, g)).backward()
        return rows

    def reference():
        feat, maps = rot()
        return finish(R.rows_ref(maps, feat, labels_lb, SIZES))

    def composed():
        feat, maps = rot()
        masks, _ = solo_dynamic_masks(maps, cells, feat, sigmoid=False)
        return finish([feat.new_zeros((0, *hw)) if m is None else F.interpolate(m.unsqueeze(0), size=hw, mode='bilinear').squeeze(0)
                       for m, hw in zip(masks, SIZES)])

    def kernel():
        feat, maps = rot()
        return finish(box_solov2_ins_preds(maps, feat, cells, SIZES))

    return {'reference': reference, 'composed': composed, 'kernel': kernel}, rot


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(legs, warm=3, samples=15):
    """Interleaved: every sample times each leg once, one call between two events."""
    for f in legs.values():
        for _ in range(warm):
            f()
    ts = {k: [] for k in legs}
    for _ in range(samples):
        for k, f in legs.items():
            ts[k].append(event_ms(f))
    return {k: dict(stats(v), samples=samples, calls_per_sample=1) for k, v in ts.items()}


def count_syncs(fn):
    """Host synchronisations torch itself reports (sync debug mode 'warn'): a lower bound for code outside torch, exact for torch ops."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum(1 for w in seen if 'synchroniz' in str(w.message).lower())


def kernel_times(fn, reps=20):
    """{kernel label: [median microseconds of every launch of it, in call order]} of the library's launches inside ``fn``: the launch
    hook records a device event before and after each."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    runs = []
    for _ in range(reps + 3):
        marks = []

        def hook(name, phase, st, user):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name.decode(), phase, ev))
        cb = _lib.LAUNCH_HOOK(hook)
        lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
        try:
            fn()
        finally:
            lib.bxi_dev_set_launch_hook(None, None)
        torch.cuda.synchronize()
        runs.append([(a[0], a[2].elapsed_time(b[2]) * 1e3) for a, b in zip(marks[0::2], marks[1::2])])
    runs = runs[3:]
    out = {}
    for i, (name, _) in enumerate(runs[0]):
        out.setdefault(name, []).append(round(float(np.median([r[i][1] for r in runs])), 2))
    return out


def rel(x, y):
    return float((x.double() - y.double()).abs().max() / y.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r27_box_solo_masks_bench.json'))
    ap.add_argument('--samples', type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_solo_masks_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as M
    dev = torch.device('cuda:0')
    cells, labels_lb, counts = make_targets(dev, 1)
    n_rows = sum(sum(c) for c in counts)
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, E=E, feature=HW, num_grids=GRIDS, level_sizes=SIZES, boxes_per_image=20,
                                                              set_cells_per_level_image=counts, rows=n_rows, all_cells=sum(S * S for S in GRIDS)),
           'input_sets_rotated': SETS, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE}
    # ---- training ------------------------------------------------------------------------------------------------------------------
    sets, g = make_sets(dev, 2, counts)
    legs, rot = train_legs(sets, g, cells, labels_lb)
    res, grads = {}, {}
    for k, f in legs.items():                                                 # every leg on the same input set, for the comparison
        rot.at = 0
        res[k] = [r.detach() for r in f()]
        feat, maps = sets[1]
        grads[k] = [feat.grad.clone()] + [m.grad.clone() for m in maps]
    row = dict(max_relative_difference_vs_reference={
        k: dict(rows=max(rel(a, b) for a, b in zip(res[k], res['reference']) if b.numel()), grad_feat=rel(grads[k][0], grads['reference'][0]),
                grad_kernel=max(rel(a, b) for a, b in zip(grads[k][1:], grads['reference'][1:]))) for k in ('composed', 'kernel')})
    del res, grads
    row.update(timed(legs, samples=args.samples))
    for k, f in legs.items():
        row[k]['launches'] = count_launches(f)
        row[k]['host_synchronisations'] = count_syncs(f)
        row[k]['peak_bytes_above_inputs'] = peak_bytes(f)
    for a, b in (('kernel', 'composed'), ('kernel', 'reference')):
        row[f'p75_of_{a}_below_p25_of_{b}'] = bool(row[a]['ms_p75'] < row[b]['ms_p25'])
    # the library's own launches on one warm input set
    feat, maps = sets[0]
    fd, md = feat.detach(), [m.detach() for m in maps]
    fwd_k = kernel_times(lambda: M.box_solov2_ins_preds(md, fd, cells, SIZES))
    both_k = kernel_times(lambda: legs['kernel']())
    pix, planes = HW[0] * HW[1], B * E
    resized = [oh * ow for (oh, ow) in (SIZES[2], SIZES[3])]
    need = {'solo_dconvl_resize': [4 * planes * (min(pix, 4 * r) + r) for r in resized],   # the tapped pixels once, the resized feature written
            'solo_dconvl_adjoint': [4 * planes * (2 * pix + sum(resized))]}           # the three groups' gradients read, grad_feat written
    kern = dict(forward_launches_us=fwd_k, forward_and_backward_launches_us=both_k, needed_bytes=need, share_of_achievable_hbm={})
    for name, sizes in need.items():
        us = (both_k.get(name) or [])[-len(sizes):]
        kern['share_of_achievable_hbm'][name] = [round(nb / HBM_ACHIEVABLE / (t * 1e-6), 4) for nb, t in zip(sizes, us)] or 'not measured'
    row['kernels'] = kern
    out['train'] = row
    del sets, legs
    torch.cuda.empty_cache()
    # ---- test time -----------------------------------------------------------------------------------------------------------------
    rng = torch.Generator(device=dev).manual_seed(5)
    n_cells = sum(S * S for S in GRIDS)
    cate = torch.rand(n_cells, 80, device=dev, generator=rng) * 0.1
    hot = torch.randperm(n_cells, device=dev, generator=rng)[:100]
    cate[hot, torch.randint(0, 80, (100,), device=dev, generator=rng)] = 0.2 + 0.7 * torch.rand(100, device=dev, generator=rng)
    mask_feat = 0.5 * torch.randn(1, E, *HW, device=dev, generator=rng)
    kernels = torch.randn(n_cells, E, device=dev, generator=rng) / 8
    cfg = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    meta = dict(img_shape=(800, 1333, 3), ori_shape=(480, 800, 3))
    every = M.solo_candidate_masks(mask_feat, kernels, None)
    test = {'from_all_cells': lambda: M.box_solov2_get_seg_single(cate, every, HW, meta, cfg, GRIDS, STRIDES),
            'from_kernels': lambda: M.box_solov2_get_seg_single_kernels(cate, mask_feat, kernels, HW, meta, cfg, GRIDS, STRIDES)}
    a, b = test['from_all_cells'](), test['from_kernels']()
    trow = dict(candidates=int((cate > cfg['score_thr']).sum()), kept=int(a.masks.shape[0]), all_cells_tensor_bytes=int(every.numel() * 4),
                same_bits=bool(torch.equal(a.masks, b.masks) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)))
    trow.update(timed(test, samples=args.samples))
    for k, f in test.items():
        trow[k]['launches'] = count_launches(f)
        trow[k]['peak_bytes_above_inputs'] = peak_bytes(f)
    out['test_time'] = trow
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
