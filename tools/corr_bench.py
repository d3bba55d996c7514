#!/usr/bin/env python3
"""Developer measurement of DiscoBox's cross-image correspondence on the GPU box: boxinstseg_amd.corr_objects (csrc/corr.hip) against the
reference's op sequence written out as torch ops (tests/corr_ref.py:corr_objects, the restatement of discobox_head.py:1056-1127 that
tests/test_host_corr.py holds against the reference's own code) -- same box, same inputs, calls alternated, forward and backward.

Shape: N = 40 objects of one level, 80 classes, C = 256, len_queue = 100, mask predictions 200 x 336, the thresholds of configs/discobox.
Ten classes hold six matching entries each, the other classes two; twenty objects belong to the first kind (they retrieve five and run
the solver), twenty to the second (they retrieve two and stop there).  Every call starts from the same bank (it is restored outside the
timed window: the call appends to it).
  ms, ms_p25, ms_p75, ms_min, ms_max   wall clock of one forward + backward between two device synchronisations (the composed path waits for
                                       the host many times, so device events alone would miss the point), over the alternated repetitions
                                       after warm-up;  event_ms: the same call of the kernel path between two device events.
  launches                             device kernels of one call (torch.profiler);  host_syncs: synchronising calls torch reports.
  num_ins, same_num_ins, max_iiu_diff  what ran, and how far the two paths' iiu are apart (fp32 both).
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r14_corr_bench.json) and prints it.
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
from tests import corr_ref as R

N, NUM_CLASS, C, L, OUT_HW, MIN_SIZE = 40, 80, 256, 100, (200, 336), 32
CFG = dict(fg_iou_thresh=0.7, bg_iou_thresh=0.7, appear_thresh=0.7, ratio_range=[0.9, 1.2], max_retrieval_objs=5, min_objs=5, dist_kernel=9,
           corr_num_iter=10, corr_num_smooth_iter=1, min_size=MIN_SIZE)
RICH, FILLED_RICH, FILLED_POOR = 10, 6, 2


def make_set(seed, dev):
    rng = np.random.RandomState(seed)
    bases = [np.abs(rng.standard_normal((C, R.FEAT, R.FEAT))) for _ in range(NUM_CLASS)]

    def entry_of(c):
        m = R.blob(13.5 + rng.uniform(-0.4, 0.4), 13.5 + rng.uniform(-0.4, 0.4), 9.0 + rng.uniform(-0.3, 0.3))
        return R.feature(bases[c], rng).astype(np.float32), m.astype(np.float32)

    bank = dict(bank_feature=np.zeros((NUM_CLASS, L, C, 7, 7), np.float32), bank_mask=np.zeros((NUM_CLASS, L, 28, 28), np.float32),
                bank_box=np.zeros((NUM_CLASS, L, 4), np.float32), bank_ptr=np.zeros(NUM_CLASS, np.int32))
    for c in range(NUM_CLASS):
        n = FILLED_RICH if c < RICH else FILLED_POOR
        for s in range(n):
            bank['bank_feature'][c, s], bank['bank_mask'][c, s] = entry_of(c)
            bank['bank_box'][c, s] = [10, 10, 70, 70]
        bank['bank_ptr'][c] = n
    obj = dict(s_feat=np.zeros((N, C, 7, 7), np.float32), s_mask=np.zeros((N, 28, 28), np.float32), t_feat=np.zeros((N, C, 7, 7), np.float32),
               t_mask=np.zeros((N, 28, 28), np.float32), boxes=np.zeros((N, 4), np.float32), labels=np.zeros(N, np.int64))
    for i in range(N):
        c = int(rng.randint(0, RICH)) if i % 2 == 0 else int(rng.randint(RICH, NUM_CLASS))
        obj['s_feat'][i], obj['s_mask'][i] = entry_of(c)
        obj['t_feat'][i], obj['t_mask'][i] = entry_of(c)
        side = int(rng.randint(40, 90))
        x, y = int(rng.randint(0, OUT_HW[1] - side)), int(rng.randint(0, OUT_HW[0] - side))
        obj['boxes'][i], obj['labels'][i] = [x, y, x + side, y + side], c
    out = {k: torch.from_numpy(v).to(dev) for k, v in {**bank, **obj}.items()}
    out['bank0'] = {k: out[k].clone() for k in R.INPUT_KEYS[6:]}
    return out


def restore(s):
    for k, v in s['bank0'].items():
        s[k].copy_(v)


def kernel_path(s, bank, solver):
    from boxinstseg_amd import corr_objects
    f = s['s_feat'].clone().requires_grad_(True)
    loss, num_ins, iiu = corr_objects(f, s['s_mask'], s['t_feat'], s['t_mask'], s['boxes'], s['labels'], bank, solver, OUT_HW, MIN_SIZE, CFG['min_objs'])
    (loss / (num_ins + 1e-4)).backward()
    return loss.detach(), num_ins, iiu, f.grad


def composed_path(s):
    inp = {k: s[k] for k in R.INPUT_KEYS}
    inp['s_feat'] = s['s_feat'].clone().requires_grad_(True)
    out = R.corr_objects(inp, CFG, OUT_HW)
    if out['num_ins']:
        (out['loss_sum'] / (out['num_ins'] + 1e-4)).backward()
    return out['loss_sum'].detach(), out['num_ins'], out['iiu'], inp['s_feat'].grad


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_corr_bench.json'))
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--sets', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('corr_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    sets = [make_set(1400 + i, dev) for i in range(args.sets)]
    solver = bx.SemanticCorrSolver(1.0, 0.05, 3, 0.3, CFG['corr_num_iter'], CFG['corr_num_smooth_iter'], CFG['dist_kernel'])
    banks = []
    for s in sets:                                                       # the bank object works on the set's own tensors
        b = bx.ObjectBank(NUM_CLASS, L, CFG['fg_iou_thresh'], CFG['bg_iou_thresh'], CFG['ratio_range'], CFG['appear_thresh'], CFG['max_retrieval_objs'])
        b.feature, b.mask, b.box, b.ptr = s['bank_feature'], s['bank_mask'], s['bank_box'], s['bank_ptr']
        banks.append(b)
    paths = {'kernel': lambda k: kernel_path(sets[k], banks[k], solver), 'composed': lambda k: composed_path(sets[k])}
    a = paths['kernel'](0)
    restore(sets[0])
    b = paths['composed'](0)
    restore(sets[0])
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps, 'sets': args.sets,
           'shape': dict(N=N, num_class=NUM_CLASS, C=C, len_queue=L, out_hw=OUT_HW, min_size=MIN_SIZE, bank_bytes=sum(v.numel() * v.element_size() for v in sets[0]['bank0'].values())),
           'num_ins': int(a[1]), 'same_num_ins': int(a[1]) == int(b[1]), 'max_iiu_diff': float((a[2] - b[2]).abs().max()),
           'max_grad_diff_rel': float((a[3] - b[3]).abs().max() / b[3].abs().max()) if int(b[1]) else None}
    for k in range(len(sets)):                                           # warm-up of every set on both paths
        for f in paths.values():
            f(k)
            restore(sets[k])
    ts, ev = {k: [] for k in paths}, []
    for r in range(args.reps):                                           # alternated: the paths see the same neighbours on the box
        for name, f in paths.items():
            k = r % len(sets)
            restore(sets[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(k)
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
        k = r % len(sets)
        restore(sets[k])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        paths['kernel'](k)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    for name, f in paths.items():
        out[name] = stats(ts[name])
        restore(sets[0])
        out[name]['host_syncs'] = count_syncs(lambda f=f: f(0))
        restore(sets[0])
        out[name]['launches'] = count_launches(lambda f=f: f(0))
    out['kernel']['event_ms'] = stats(ev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
