#!/usr/bin/env python3
"""Developer measurement of the SOLOv2-style heads' training targets on the GPU box: boxinstseg_amd.solov2_targets /
box_solov2_targets (csrc/solo_targets.hip) against the reference's op sequence written out as torch ops (discobox_head.py:1442-1529,
box_solov2_head.py:390-472 without its two F.interpolate) -- same box, same inputs, calls alternated.  The composed path is a
restatement kept in this file: the loops over images, levels, instances and cells, ``nonzero`` and ``int()`` on device tensors, the
upload of every level's masks (DiscoBox) or the host centre of mass (BoxLevelSet), and the rescale of every mask ON THE HOST followed
by an upload, where the reference runs ``mmcv.imrescale`` -- here the restated 2-of-4 rule in NumPy, which does less arithmetic than
OpenCV's resize: read the composed time with that in mind.

Shape: B = 2, 800 x 1344, 20 box masks per image, the COCO grids [40, 36, 24, 16, 12], strides [8, 8, 16, 32, 32] and scale ranges.
  ms, ms_p25, ms_p75, ms_min, ms_max   wall clock of one call between two device synchronisations (the call itself waits for the host
                                       once or many times, so device events alone would miss the point), over the alternated
                                       repetitions after warm-up; `kernel` has the masks on the device, `kernel_host_masks` uploads them.
  launches                             device kernels of one call (torch.profiler);  host_syncs: synchronising calls torch reports.
  mask_pass                            the one launch over the mask bytes alone (device events, inputs rotating over --sets copies so
                                       that the bytes come from HBM): ms, GB/s of the bytes read, and the fraction of the 8 TB/s peak.
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r13_solo_targets_bench.json) and prints it.
GPU only; reads nothing but this repository."""
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
from tests import solo_ref as R

B, G, C = 2, 20, 80
IMG = (800, 1344)
FEAT = (200, 336)
GRIDS, STRIDES = [40, 36, 24, 16, 12], [8, 8, 16, 32, 32]
RANGES = ((1, 96), (48, 192), (96, 384), (192, 768), (384, 2048))
SIGMA = 0.2
HBM_PEAK = 8.0e12
CFG = dict(num_grids=GRIDS, strides=STRIDES, scale_ranges=RANGES, sigma=SIGMA, num_classes=C)


def make_set(seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    boxes, labels, masks = [], [], []
    for _ in range(B):
        wh = (torch.rand(G, 2, generator=g) ** 2 * torch.tensor([700.0, 500.0]) + 12).round()
        xy = (torch.rand(G, 2, generator=g) * (torch.tensor([IMG[1], IMG[0]], dtype=torch.float32) - wh)).round()
        bx = torch.cat([xy, xy + wh], 1)
        m = np.zeros((G, *IMG), np.uint8)
        for i, (x1, y1, x2, y2) in enumerate(bx.int().tolist()):
            m[i, y1:y2, x1:x2] = 1                                      # box masks, as the box-supervised pipelines make them
        boxes.append(bx)
        labels.append(torch.randint(0, C, (G,), generator=g))
        masks.append(m)
    return boxes, labels, masks


def level_sizes(mode):
    return [FEAT] * 5 if mode == 'discobox' else [(IMG[0] // (s // 2), IMG[1] // (s // 2)) for s in STRIDES]


def composed_single(mode, boxes, labels, masks, dev):
    """One image, the reference's loop (labels, grid orders and planes are built and dropped; what is timed is the work)."""
    areas = torch.sqrt((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))
    sizes = level_sizes(mode)
    out = []
    for (lo, hi), stride, S, size in zip(RANGES, STRIDES, GRIDS, sizes):
        cate = torch.zeros([S, S], dtype=torch.int64, device=dev) + C
        ind = torch.zeros([S ** 2], dtype=torch.bool, device=dev)
        planes = torch.zeros([S ** 2, *size], dtype=torch.uint8, device=dev) if mode == 'boxlevelset' else []
        order = []
        hit = ((areas >= lo) & (areas <= hi)).nonzero().flatten()
        if len(hit) == 0:
            out.append((planes if mode == 'boxlevelset' else torch.zeros([0, *size], dtype=torch.uint8, device=dev), cate, ind, order))
            continue
        bx, lb, mk = boxes[hit], labels[hit], masks[hit.cpu().numpy(), ...]
        half_ws, half_hs = 0.5 * (bx[:, 2] - bx[:, 0]) * SIGMA, 0.5 * (bx[:, 3] - bx[:, 1]) * SIGMA
        if mode == 'discobox':
            pt = torch.from_numpy(mk).to(device=dev)
            ys, xs = torch.arange(0, IMG[0], dtype=torch.float32, device=dev), torch.arange(0, IMG[1], dtype=torch.float32, device=dev)
            m00 = pt.sum(dim=-1).sum(dim=-1).clamp(min=1e-6)
            cws, chs = (pt * xs).sum(dim=-1).sum(dim=-1) / m00, (pt * ys[:, None]).sum(dim=-1).sum(dim=-1) / m00
            valid = pt.sum(dim=-1).sum(dim=-1) > 0
            f = 4
        else:
            f = stride // 2
        for k, (seg, lab, hh, hw) in enumerate(zip(mk, lb, half_hs, half_ws)):
            if mode == 'discobox':
                if not valid[k]:
                    continue
                ch, cw = chs[k], cws[k]
            else:
                if seg.sum() < 10:
                    continue
                m00 = float(seg.sum())
                ch = float((seg.sum(1) * np.arange(IMG[0])).sum()) / m00          # scipy.ndimage.center_of_mass, float64
                cw = float((seg.sum(0) * np.arange(IMG[1])).sum()) / m00
            cell = lambda v, n: int((v / n) // (1. / S))                                    # noqa: E731
            coord_w, coord_h = cell(cw, IMG[1]), cell(ch, IMG[0])
            top = max(max(0, cell(ch - hh, IMG[0])), coord_h - 1)
            down = min(min(S - 1, cell(ch + hh, IMG[0])), coord_h + 1)
            left = max(coord_w - 1, max(0, cell(cw - hw, IMG[1])))
            right = min(min(S - 1, cell(cw + hw, IMG[1])), coord_w + 1)
            cate[top:(down + 1), left:(right + 1)] = lab
            small = torch.from_numpy(R.rescale(seg, f)).to(device=dev)                      # mmcv.imrescale on the host, then the upload
            for i in range(top, down + 1):
                for j in range(left, right + 1):
                    label = int(i * S + j)
                    if mode == 'discobox':
                        cur = torch.zeros(size, dtype=torch.uint8, device=dev)
                        cur[:small.shape[0], :small.shape[1]] = small
                        planes.append(cur)
                        order.append(label)
                    else:
                        planes[label, :small.shape[0], :small.shape[1]] = small
                    ind[label] = True
        if mode == 'discobox':
            planes = torch.stack(planes, 0) if planes else torch.zeros([0, *size], dtype=torch.uint8, device=dev)
        out.append((planes, cate, ind, order))
    return out


def composed_path(mode, s, dev):
    per = [composed_single(mode, b, l, m, dev) for b, l, m in zip(s['boxes'], s['labels'], s['host_masks'])]
    # what `loss` does next with the lists: concatenate the planes of every level over the images
    if mode == 'discobox':
        return [torch.cat([p[l][0] for p in per]) for l in range(5)]
    return [torch.cat([p[l][0][p[l][2]] for p in per]) for l in range(5)]


def kernel_path(mode, s, host_masks=False):
    import boxinstseg_amd as bx
    masks = [_Host(m) for m in s['host_masks']] if host_masks else s['masks']
    if mode == 'discobox':
        tg = bx.solov2_targets(s['boxes'], s['labels'], masks, FEAT, **CFG)
    else:
        tg = bx.box_solov2_targets(s['boxes'], s['labels'], masks, level_sizes(mode), **CFG)
    return tg.ins_labels(), tg


class _Host:
    def __init__(self, m):
        self.m = m

    def to_ndarray(self):
        return self.m


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


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                   and 'memset' not in e.name.lower())
    except Exception as e:                                               # noqa: BLE001
        return f'not counted: {e!r}'


def stats(v):
    return dict(ms=round(float(np.median(v)), 4), ms_p25=round(float(np.percentile(v, 25)), 4), ms_p75=round(float(np.percentile(v, 75)), 4),
                ms_min=round(min(v), 4), ms_max=round(max(v), 4))


def mask_pass_alone(mode, sets, reps, dev):
    """The mask pass by itself through the C ABI, device events, rotating over the sets."""
    from boxinstseg_amd import _lib
    lib, ia, pa = _lib.load(), _lib.int_array, _lib.ptr_array
    factors = [4] if mode == 'discobox' else [4, 8, 16]
    outs = [torch.empty(B * G, IMG[0] // f, IMG[1] // f, dtype=torch.uint8, device=dev) for f in factors]
    mom = torch.empty(B * G, 3, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(s):
        rc = lib.bxi_solo_mask_pass_u8(pa([m.data_ptr() for m in s['masks']]), ia([0, G, 2 * G]), ia([IMG[0]] * B), ia([IMG[1]] * B), B, ia(factors),
                                       ia([IMG[0] // f for f in factors]), ia([IMG[1] // f for f in factors]), len(factors),
                                       pa([o.data_ptr() for o in outs]), mom.data_ptr(), st)
        assert rc == 0, rc
    for s in sets:
        run(s)
    torch.cuda.synchronize()
    ts = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(sets[r % len(sets)])
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    nbytes = B * G * IMG[0] * IMG[1]
    out = stats(ts)
    out.update(bytes_read=nbytes, GBps=round(nbytes / (out['ms'] * 1e-3) / 1e9, 1), fraction_of_hbm_peak=round(nbytes / (out['ms'] * 1e-3) / HBM_PEAK, 3),
               sets=len(sets))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_solo_targets_bench.json'))
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--sets', type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('solo_targets_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    dev = torch.device('cuda:0')
    sets = []
    for i in range(args.sets):
        boxes, labels, masks = make_set(1300 + i)
        sets.append(dict(boxes=[b.to(dev) for b in boxes], labels=[t.to(dev) for t in labels], host_masks=masks,
                         masks=[torch.from_numpy(m).to(dev) for m in masks]))
    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, image=IMG, masks_per_image=G, num_grids=GRIDS, strides=STRIDES), 'reps': args.reps,
           'sets': args.sets, 'composed_imrescale': 'the restated 2-of-4 rule in NumPy on the host (OpenCV is not available here)'}
    for mode in R.MODES:
        paths = {'kernel': lambda s, m=mode: kernel_path(m, s), 'kernel_host_masks': lambda s, m=mode: kernel_path(m, s, True),
                 'composed': lambda s, m=mode: composed_path(m, s, dev)}
        a, tg = paths['kernel'](sets[0])
        b = paths['composed'](sets[0])
        res = {'same_planes': all(torch.equal(x, y) for x, y in zip(a, b)), 'pairs_or_cells_per_level': [int(x.shape[0]) for x in a],
               'num_ins': int(tg.num_ins.item())}
        for f in paths.values():
            f(sets[1 % len(sets)])
        torch.cuda.synchronize()
        ts = {k: [] for k in paths}
        for r in range(args.reps):                                       # alternated: the paths see the same neighbours on the box
            for k, f in paths.items():
                s = sets[r % len(sets)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(s)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k, f in paths.items():
            res[k] = stats(ts[k])
            res[k].update(host_syncs=count_syncs(lambda f=f: f(sets[0])), launches=count_launches(lambda f=f: f(sets[0])))
        res['mask_pass'] = mask_pass_alone(mode, sets, 4 * args.reps, dev)
        out[mode] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
