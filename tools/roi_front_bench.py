#!/usr/bin/env python3
"""Developer measurement of one level of DiscoBox's corr_loss on the GPU box: boxinstseg_amd.corr_level (csrc/roi_align.hip in front of
csrc/corr.hip) against the same lines written as torch ops -- the reference's statements of discobox_head.py:1018-1057 (one ``.sum()`` and
one ``torch.where`` per object, four ``torch.tensor([... .min() ...])``, four RoIAlign calls) with ``F.grid_sample`` + ``avg_pool2d`` standing
in for mmcv's op (tests/roi_ref.roi_align_grid_sample's form, on the device; mmcv is not a dependency of this project), feeding the same
``corr_objects``.  Same box, same inputs, calls alternated, forward and backward.

Shape: one level, N = 40 objects over B = 2 images, C = 256, features and mask predictions 200 x 336, boxes from 8 x 8 to the whole canvas,
two all-zero targets, 80 classes.  Every second kept object finds six entries like itself in the bank (it runs the solver); every call
starts from the same bank (restored outside the timed window).
  ms, ms_p25, ms_p75, ms_min, ms_max   wall clock of one forward + backward between two device synchronisations, over the alternated
                                       repetitions after warm-up;  event_ms: the same call of the kernel path between two device events.
  launches, host_syncs                 device kernels of one call (torch.profiler), synchronising calls torch reports.
  max_roi_*_diff, assign_rows_differing, relu_sign_flips, max_iiu_diff, *grad_diff_rel*   how far the two paths are apart (fp32 both);
                                       roi_align.against_grid_sample: the op alone, which has no discontinuity.
  roi_align                            RoIAlign alone at that shape (7 x 7, C = 256, the 40 boxes): forward and backward between device events
                                       (median of --reps calls), the bytes it must move -- the box areas of the feature read once, the
                                       gradient map written once -- and those bytes over the time as a share of the 8.0 TB/s HBM peak.
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r15_roi_front_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import json
import math
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

N, B, C, HW, NUM_CLASS, L, MIN_SIZE, FILLED = 40, 2, 256, (200, 336), 80, 100, 32, 6
EMPTY = (7, 23)
HBM_PEAK = 8.0e12
CFG = dict(fg_iou_thresh=0.7, bg_iou_thresh=0.7, appear_thresh=0.7, ratio_range=[0.9, 1.2], max_retrieval_objs=5, min_objs=5, dist_kernel=9,
           corr_num_iter=10, corr_num_smooth_iter=1)


def make_set(seed, dev):
    rng = np.random.RandomState(seed)
    H, W = HW
    yy, xx = np.mgrid[0:H, 0:W]
    target, logits, boxes = np.zeros((N, H, W), np.uint8), np.full((N, H, W), -6.0, np.float32), []
    sides = np.linspace(8, 150, N).astype(int)
    for i in range(N):
        if i in EMPTY:
            boxes.append(None)
            continue
        if i == N - 1:
            x1, y1, x2, y2 = 0, 0, W, H                                      # the whole canvas
        else:
            w, h = int(sides[i]), int(min(sides[i] * rng.uniform(0.8, 1.25), H))
            x1, y1 = int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1))
            x2, y2 = x1 + w, y1 + h
        boxes.append((x1, y1, x2, y2))
        target[i, y1:y2, x1:x2] = 1
        inside = ((yy - (y1 + y2 - 1) / 2) / ((y2 - y1) * 0.42)) ** 2 + ((xx - (x1 + x2 - 1) / 2) / ((x2 - x1) * 0.42)) ** 2 <= 1
        logits[i] = np.where(inside, 6.0, -6.0) + 0.3 * rng.standard_normal((H, W))
    s = dict(s_input=torch.from_numpy(logits).to(dev), target=torch.from_numpy(target).to(dev), img_inds=torch.arange(N, device=dev) % B,
             kernel_labels=torch.arange(N, device=dev) % NUM_CLASS, s_feat=torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev))
    s['t_feat'] = s['s_feat'] + 0.05 * torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    s['box_list'] = boxes
    return s


def make_bank(s, dev):
    """A bank in which every second kept object finds FILLED entries like itself (made from what the front gives it)."""
    import boxinstseg_amd as bx
    bank = bx.ObjectBank(NUM_CLASS, L, CFG['fg_iou_thresh'], CFG['bg_iou_thresh'], CFG['ratio_range'], CFG['appear_thresh'], CFG['max_retrieval_objs'])
    bank.ensure(C, dev)
    boxes, keep, labels = bx.target_boxes(s['target'], s['kernel_labels'])
    rois = torch.cat([s['img_inds'].float().view(N, 1), boxes], 1)
    feat, mask = bx.roi_feat_norm(s['t_feat'], rois), bx.sigmoid_roi_masks(s['s_input'], boxes)
    for i in range(0, N, 2):
        c = int(labels[i])
        if c >= 0:
            bank.feature[c, :FILLED], bank.mask[c, :FILLED], bank.box[c, :FILLED], bank.ptr[c] = feat[i], mask[i], boxes[i], FILLED
    return bank, {k: getattr(bank, k).clone() for k in ('feature', 'mask', 'box', 'ptr')}


def restore(bank, saved):
    for k, v in saved.items():
        getattr(bank, k).copy_(v)


def kernel_path(s, bank, solver):
    from boxinstseg_amd import corr_level
    f = s['s_feat'].clone().requires_grad_(True)
    d = {}
    loss, num_ins, iiu, keep = corr_level(s['s_input'], s['s_input'], s['target'], s['img_inds'], s['kernel_labels'], f, s['t_feat'], bank, solver,
                                          MIN_SIZE, CFG['min_objs'], details=d)
    (loss / (num_ins + 1e-4)).backward()
    return loss.detach(), num_ins, iiu, f.grad, keep, d


def grid_roi(feat, rois, P):
    """RoIAlign (aligned, adaptive grid, boxes inside the canvas) as F.grid_sample + avg_pool2d; the grid sizes come from the host copy of
    the boxes, which the reference's ``torch.tensor([...])`` statements leave on the host anyway."""
    Hf, Wf = feat.shape[-2:]
    out = []
    for r in rois.cpu().tolist():
        b, x1, y1, x2, y2 = int(r[0]), r[1] - 0.5, r[2] - 0.5, r[3] - 0.5, r[4] - 0.5
        rw, rh = x2 - x1, y2 - y1
        gh, gw = max(math.ceil(rh / P), 1), max(math.ceil(rw / P), 1)
        ys = y1 + (torch.arange(P * gh, device=feat.device, dtype=feat.dtype) + 0.5) * (rh / (P * gh))
        xs = x1 + (torch.arange(P * gw, device=feat.device, dtype=feat.dtype) + 0.5) * (rw / (P * gw))
        grid = torch.stack(torch.broadcast_tensors((xs / (Wf - 1) * 2 - 1)[None, :], (ys / (Hf - 1) * 2 - 1)[:, None]), -1)[None]
        out.append(F.avg_pool2d(F.grid_sample(feat[b:b + 1], grid, mode='bilinear', padding_mode='border', align_corners=True), (gh, gw))[0])
    return torch.stack(out)


def relu_l2(feat):
    feat = F.relu(feat)
    return feat / (((feat ** 2).sum(dim=1, keepdim=True) + 1e-6) ** 0.5 + 1e-6)


def composed_path(s, bank, solver):
    """The statements of :1018-1057 as the reference has them, then corr_objects."""
    from boxinstseg_amd import corr_objects
    s_feat = s['s_feat'].clone().requires_grad_(True)
    target, img_inds = s['target'], s['img_inds']
    s_input = torch.sigmoid(s['s_input'])
    t_input = s_input
    mask = torch.tensor([t.sum() for t in target]).to(s_input).bool()
    s_input, t_input, img_inds, target = s_input[mask], t_input[mask], img_inds[mask], target[mask]
    pos_inds = [torch.where(t) for t in target]
    min_y, max_y, min_x, max_x = torch.tensor([ids[0].min() for ids in pos_inds]), torch.tensor([ids[0].max() for ids in pos_inds]) + 1, \
        torch.tensor([ids[1].min() for ids in pos_inds]), torch.tensor([ids[1].max() for ids in pos_inds]) + 1
    boxes = torch.cat([min_x.unsqueeze(1), min_y.unsqueeze(1), max_x.unsqueeze(1), max_y.unsqueeze(1)], 1).to(s_input)
    rois = torch.cat([img_inds.to(s_feat).unsqueeze(1), boxes], 1)
    roi_s_feat = relu_l2(grid_roi(s_feat, rois, 7))
    with torch.no_grad():
        roi_t_feat = relu_l2(grid_roi(s['t_feat'].detach(), rois, 7))
        mrois = torch.cat([torch.arange(target.shape[0]).to(t_input).unsqueeze(1), boxes], 1)
        roi_s_mask = grid_roi(s_input.unsqueeze(1).detach(), mrois, 28).squeeze(1)
        roi_t_mask = roi_s_mask
    n = target.shape[0]
    d = dict(roi_s_feat=roi_s_feat, roi_s_mask=roi_s_mask)
    loss, num_ins, iiu = corr_objects(roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, s['kernel_labels'][:n], bank, solver, HW, MIN_SIZE,
                                      CFG['min_objs'], details=d)
    (loss / (num_ins + 1e-4)).backward()
    return loss.detach(), num_ins, iiu, s_feat.grad, None, d


def roi_align_alone(s, reps):
    """RoIAlign 7 x 7 on s_feat with the level's 40 rois: forward and backward between device events, and the bytes they must move."""
    from boxinstseg_amd import roi_align, target_boxes
    boxes, keep, _ = target_boxes(s['target'], s['kernel_labels'])
    rois = torch.cat([s['img_inds'].float().view(N, 1), boxes], 1)
    x = s['s_feat'].clone().requires_grad_(True)
    g = torch.randn(N, C, 7, 7, device=x.device)
    fwd, bwd = [], []
    for r in range(reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        y = roi_align(x, rois, 7)
        e[1].record()
        torch.cuda.synchronize()
        e[2].record()
        gx, = torch.autograd.grad(y, x, g)
        e[3].record()
        e[3].synchronize()
        if r >= 3:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[2].elapsed_time(e[3]))
    # the op alone is linear in its input: no relu, no threshold, so the two forms must agree to fp32 rounding, forward and gradient
    xr = s['s_feat'].clone().requires_grad_(True)
    kept = [i for i, b in enumerate(s['box_list']) if b is not None]
    yr = grid_roi(xr, rois[kept], 7)
    gr, = torch.autograd.grad(yr, xr, g[kept])
    gk, = torch.autograd.grad(roi_align(x, rois[kept], 7), x, g[kept])
    agree = dict(forward_max_diff_rel=float((y[kept] - yr).abs().max() / yr.abs().max()), backward_max_diff_rel=float((gk - gr).abs().max() / gr.abs().max()))
    area = sum((b[2] - b[0]) * (b[3] - b[1]) for b in s['box_list'] if b is not None)
    fwd_bytes, bwd_bytes = area * C * 4 + N * C * 49 * 4, B * C * HW[0] * HW[1] * 4 + N * C * 49 * 4
    out = dict(against_grid_sample=agree, forward_ms=stats(fwd), backward_ms=stats(bwd), forward_bytes=fwd_bytes, backward_bytes=bwd_bytes, box_area_pixels=int(area))
    out['forward_share_of_hbm_peak'] = round(fwd_bytes / (out['forward_ms']['ms'] * 1e-3) / HBM_PEAK, 5)
    out['backward_share_of_hbm_peak'] = round(bwd_bytes / (out['backward_ms']['ms'] * 1e-3) / HBM_PEAK, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_roi_front_bench.json'))
    ap.add_argument('--reps', type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('roi_front_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    s = make_set(1500, dev)
    solver = bx.SemanticCorrSolver(1.0, 0.05, 3, 0.3, CFG['corr_num_iter'], CFG['corr_num_smooth_iter'], CFG['dist_kernel'])
    bank, saved = make_bank(s, dev)
    paths = {'kernel': lambda: kernel_path(s, bank, solver), 'composed': lambda: composed_path(s, bank, solver)}
    a = paths['kernel']()
    restore(bank, saved)
    b = paths['composed']()
    restore(bank, saved)
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps,
           'shape': dict(N=N, B=B, C=C, hw=HW, num_class=NUM_CLASS, len_queue=L, min_size=MIN_SIZE, empty_targets=len(EMPTY)),
           'num_ins': int(a[1]), 'same_num_ins': int(a[1]) == int(b[1])}
    keep, da, db = a[4], a[5], b[5]
    # how far the two paths are apart (fp32 both; grid_sample normalises its coordinates to [-1, 1] and back): the RoI tensors, then what the
    # loop makes of them -- one arg-max of the solver that falls the other way moves a whole row of the gradient
    out.update(max_roi_feat_diff=float((da['roi_s_feat'][keep] - db['roi_s_feat']).abs().max()),
               max_roi_mask_diff=float((da['roi_s_mask'][keep] - db['roi_s_mask']).abs().max()),
               assign_rows_differing=int((da['assign'][keep] != db['assign']).sum()), assign_rows=int((db['assign'] >= 0).sum()),
               relu_sign_flips=int(((da['roi_s_feat'][keep] > 0) != (db['roi_s_feat'] > 0)).sum()), pooled_values=int(db['roi_s_feat'].numel()),
               max_iiu_diff=float((a[2][keep] - b[2]).abs().max()))
    if int(b[1]):                                                        # a pooled value that is +1e-6 on one path and -1e-6 on the other switches a whole term of the gradient
        rel = ((a[3] - b[3]).abs() / b[3].abs().max()).flatten()
        out.update(max_grad_diff_rel=float(rel.max()), grad_diff_rel_p999=float(torch.quantile(rel[::7].float(), 0.999)), grad_diff_rel_median=float(rel[::7].median()))
    for f in paths.values():                                             # warm-up of both paths
        for _ in range(2):
            f()
            restore(bank, saved)
    ts, ev = {k: [] for k in paths}, []
    for r in range(args.reps):                                           # alternated: the paths see the same neighbours on the box
        for name, f in paths.items():
            restore(bank, saved)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
        restore(bank, saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        paths['kernel']()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    for name, f in paths.items():
        out[name] = stats(ts[name])
        restore(bank, saved)
        out[name]['host_syncs'] = count_syncs(f)
        restore(bank, saved)
        out[name]['launches'] = count_launches(f)
    out['kernel']['event_ms'] = stats(ev)
    out['roi_align'] = roi_align_alone(s, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
