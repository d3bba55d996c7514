#!/usr/bin/env python
"""``discobox_loss`` against the composition a user wrote before it (tests/dbx_compose.py: the reference's loops over the package's
existing modules), at B = 2, E = 256, mask feature 200 x 336, 20 instances per image over the five COCO grids, max_iter = 10, base = 0.1,
student + teacher, use_corr (``make_inputs(sharp=True)``: the banks retrieve, the solver runs, loss_corr > 0).  Forward + backward on cold inputs (rotating sets), the two paths alternated in one run.

  ms, ms_p25, ms_p75, ms_min, ms_max   host clock around one forward + backward that ends in a device synchronise.
  launches                             device kernels of one forward + backward (torch.profiler, memcpy / memset nodes listed apart).
  host_syncs                           synchronising calls torch's sync debug mode reports during one forward + backward.
  peak_MB                              peak memory above the inputs.
  legs                                 the same run alternates the two-leg step sequence against two one-leg sequences (prepare + steps
                                       + dice forward each), on the rows of the first set with a random competing iiu: the two-leg launch
                                       is kept only if its median is lower by more than the p25-p75 spread.
  step                                 one two-leg step launch alone: time, the bytes it must move (the affinities of the batch once per
                                       row that has a target word, the iiu planes, the state words) and its share of the copy rate.
Writes profiles/r30_discobox_loss_bench.json.  Nothing here is meaningful from a CPU run: it needs the GPU."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from tests import dbx_compose as C  # noqa: E402

GRIDS = dict(num_grids=[40, 36, 24, 16, 12], strides=[8, 8, 16, 32, 32], scale_ranges=((1, 96), (48, 192), (96, 384), (192, 768), (384, 2048)))
HW, E, NB, PER_IMAGE = (200, 336), 256, 2, 20


def make_set(dev, seed, block):
    import boxinstseg_amd as B
    d = C.make_inputs(GRIDS['num_grids'], hw=HW, E=E, B=NB, C=E, num_classes=2, seed=seed, boxes_per_image=PER_IMAGE, sharp=True)
    t = lambda a, g=False: torch.from_numpy(a).to(dev).requires_grad_(g)
    ccfg = B.parse_corr_cfg(block)
    return dict(cate=[t(a, True) for a in d['cate']], s_kern=[t(a, True) for a in d['s_kern']], t_kern=[t(a) for a in d['t_kern']], s_ins=t(d['s_ins'], True),
                t_ins=t(d['t_ins']), boxes=[t(b) for b in d['boxes']], labels=[t(l) for l in d['labels']], masks=[t(m) for m in d['masks']], img=t(d['img']),
                s_feat=t(d['s_feat'], True), t_feat=t(d['t_feat']), banks={k: (B.ObjectBank(**ccfg['bank']), B.SemanticCorrSolver(**ccfg['solver'])) for k in ('new', 'composed')})


def run(which, s, block):
    import boxinstseg_amd as B
    bank, solver = s['banks'][which]
    args = (s['cate'], s['s_kern'], s['t_kern'], s['s_ins'], s['t_ins'], s['boxes'], s['labels'], s['masks'])
    kw = dict(use_loss_ts=True, use_ind_teacher=True, use_corr=True, s_feat=[s['s_feat']], t_feat=[s['t_feat']], bank=bank, solver=solver, head_cfg=block)
    out = B.discobox_loss(*args, None, None, s['img'], **kw) if which == 'new' else C.compose_loss(*args, s['img'], **kw)
    sum(out.values()).backward()
    return out


def clear(s):
    for t in s['cate'] + s['s_kern'] + [s['s_ins'], s['s_feat']]:
        t.grad = None


def census(which, s, block):
    """launches, host syncs and peak memory of one forward + backward."""
    from torch.profiler import ProfilerActivity, profile
    clear(s)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run(which, s, block)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = sum(1 for n in names if 'memcpy' in n.lower() or 'memset' in n.lower())
    clear(s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        run(which, s, block)
    torch.cuda.set_sync_debug_mode('default')
    syncs = sum(1 for w in seen if 'synchroniz' in str(w.message).lower() and 'prototype' not in str(w.message).lower())
    clear(s)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run(which, s, block)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    return dict(launches=len(names) - copies, copy_or_memset_nodes=copies, dbx_launches=sum(1 for n in names if 'dbx_' in n),
                meanfield_launches=sum(1 for n in names if 'mf_' in n), host_syncs=syncs, peak_MB=round(peak, 1))


def stats(v):
    v = np.array(v)
    return dict(ms=round(float(np.median(v)), 4), ms_p25=round(float(np.percentile(v, 25)), 4), ms_p75=round(float(np.percentile(v, 75)), 4),
                ms_min=round(float(v.min()), 4), ms_max=round(float(v.max()), 4))


def legs(dev, reps, R=40, iters=10):
    """prepare + steps + dice forward: one two-leg sequence against two one-leg sequences, alternated; and one two-leg step launch alone."""
    import boxinstseg_amd as B
    from boxinstseg_amd import _lib
    from boxinstseg_amd._common import current_stream
    lib = _lib.load()
    H, W = HW
    g = torch.Generator(device='cpu').manual_seed(5)
    nset = 3
    sets = []
    for _ in range(nset):
        s, t = torch.rand(R, H, W, generator=g).to(dev), torch.rand(R, H, W, generator=g).to(dev)
        target = torch.zeros(R, H, W, dtype=torch.uint8)
        for i in range(R):
            bh, bw = int(torch.randint(20, H // 2, (1,), generator=g)), int(torch.randint(20, W // 2, (1,), generator=g))
            y0, x0 = int(torch.randint(0, H - bh, (1,), generator=g)), int(torch.randint(0, W - bw, (1,), generator=g))
            target[i, y0:y0 + bh, x0:x0 + bw] = 1
        inside = target.bool().to(dev)
        s, t = torch.where(inside, s.clamp(min=0.6), s), torch.where(inside, t.clamp(min=0.6), t)
        sets.append(dict(s=s, t=t, target=target.to(dev), img=torch.randint(0, NB, (R,), generator=g).to(dev),
                         kernel=B.meanfield_kernel(torch.randn(NB, 3, H, W, generator=g).to(dev), 3, 2.0, 0.5, 30.0),
                         iiu=(torch.rand(R, 2, H, W, generator=g) * 0.1).to(dev)))
    st = current_stream(dev)
    ws = {l: torch.empty(lib.bxi_dbx_workspace_bytes(R, H, W, l), dtype=torch.uint8, device=dev) for l in (1, 2)}
    ws1b = torch.empty_like(ws[1])
    live, n_live = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    loss, sums = torch.empty(2, R, device=dev), torch.empty(2, R, 2, dtype=torch.float64, device=dev)
    firsts = _lib.int_array([0])

    def seq(d, nlegs, w, with_iiu):
        ptrs = _lib.ptr_array([d['iiu'].data_ptr()])
        _lib.check('prepare', lib.bxi_dbx_prepare_f32(d['s'].data_ptr(), d['t'].data_ptr(), d['target'].data_ptr(), R, H, W, nlegs, live.data_ptr(),
                                                      n_live.data_ptr(), w.data_ptr(), w.numel(), st))
        if nlegs == 2 or not with_iiu:
            _lib.check('steps', lib.bxi_dbx_steps_f32(d['kernel'].data_ptr(), NB, H, W, 3, d['img'].data_ptr(), R, iters, 0.1, 0.01, nlegs, ptrs, firsts, 1,
                                                      w.data_ptr(), w.numel(), st))
        else:                                       # the leg with inter_img_mask alone: the existing one-leg entry point's step, same kernels
            B.meanfield_forward(d['kernel'], (d['t'] + d['s']) / 2, d['target'], iters, 0.1, d['img'], d['iiu'])
        _lib.check('dice', lib.bxi_dbx_dice_forward_f32(d['s'].data_ptr(), R, H, W, nlegs, iters, 0.01, w.data_ptr(), w.numel(), loss.data_ptr(),
                                                        sums.data_ptr(), st))

    def two(i):
        seq(sets[i % nset], 2, ws[2], True)

    def twice_one(i):
        seq(sets[i % nset], 1, ws[1], False)
        seq(sets[i % nset], 1, ws1b, True)

    times = {'two_leg': [], 'one_leg_twice': []}
    for r in range(2 + reps):
        for name, fn in (('two_leg', two), ('one_leg_twice', twice_one)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r)
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in times.items()}
    spread = max(out['two_leg']['ms_p75'] - out['two_leg']['ms_p25'], out['one_leg_twice']['ms_p75'] - out['one_leg_twice']['ms_p25'])
    out['keep_two_leg'] = bool(out['one_leg_twice']['ms'] - out['two_leg']['ms'] > spread)
    out['note'] = ('one_leg_twice is a HANDICAPPED competitor, an upper bound of what a one-leg pair costs: prepare + 10 one-leg steps + dice, then a second '
                   'prepare + the existing one-leg entry point with inter_img_mask through its Python wrapper (it materialises x with a torch op, allocates, '
                   'and runs mf_init, mf_ret and mf_valid, which a shipped pair of one-leg step sequences over one prepare would not) + dice')
    # one two-leg step launch alone, on rotating sets
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for i in range(14):
        d = sets[i % nset]
        ptrs = _lib.ptr_array([d['iiu'].data_ptr()])
        lib.bxi_dbx_prepare_f32(d['s'].data_ptr(), d['t'].data_ptr(), d['target'].data_ptr(), R, H, W, 2, live.data_ptr(), n_live.data_ptr(), ws[2].data_ptr(),
                                ws[2].numel(), st)
        a.record()
        lib.bxi_dbx_steps_f32(d['kernel'].data_ptr(), NB, H, W, 3, d['img'].data_ptr(), R, 1, 0.1, 0.01, 2, ptrs, firsts, 1, ws[2].data_ptr(), ws[2].numel(), st)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    us = float(np.median(ts[2:]))
    inside = sum(int(d['target'].sum()) for d in sets) / nset
    nbytes = inside * (9 + 2) * 4                                          # per in-target pixel: nine affinities and the two iiu planes (words are noise)
    big = [torch.empty(64 * 2 ** 20, device=dev) for _ in range(3)]
    cs = []
    for i in range(10):
        a.record()
        big[(i + 1) % 3].copy_(big[i % 3])
        b.record()
        b.synchronize()
        cs.append(a.elapsed_time(b) * 1000.0)
    copy_GBps = 2 * big[0].numel() * 4 / float(np.median(cs[2:])) / 1e3
    out['step'] = dict(us=round(us, 1), MB=round(nbytes / 1e6, 2), GBps=round(nbytes / us / 1e3, 1), copy_GBps=round(copy_GBps, 1),
                       fraction_of_copy=round(nbytes / us / 1e3 / copy_GBps, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r30_discobox_loss_bench.json'))
    a = ap.parse_args()
    entry.build()
    dev = torch.device('cuda:0')
    block = C.head_block(**GRIDS)
    sets = [make_set(dev, 100 + i, block) for i in range(a.sets)]
    times = {'new': [], 'composed': []}
    first = {}
    for r in range(a.warmup + a.reps):
        for k in ('new', 'composed'):
            s = sets[r % a.sets]
            clear(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(k, s, block)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                first[k] = {n: float(v.detach()) for n, v in out.items()}
    import boxinstseg_amd as B
    head = B.parse_solo_head_cfg(block)
    rows = [int(sum(p.numel() for p in B.solov2_targets(s['boxes'], s['labels'], s['masks'], HW, **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')}).pair_inst)) for s in sets]
    res = dict(shape=dict(B=NB, E=E, mask_feat=list(HW), per_image=PER_IMAGE, rows_per_set=rows, grids=GRIDS['num_grids'], max_iter=10, base=0.1), sets=a.sets, reps=a.reps,
               device=torch.cuda.get_device_name(0))
    for k in ('new', 'composed'):
        res[k] = stats(times[k])
        res[k].update(census(k, sets[0], block))
    res['first_call_losses'] = first
    res['not_slower'] = bool(res['new']['ms'] <= res['composed']['ms'])
    res['reference_statements_as_torch_ops'] = 'not measured here'
    res['legs'] = legs(dev, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
