#!/usr/bin/env python3
"""Developer measurement of the run-length encoding of the test-time masks on the GPU box, at the shapes of seg_paste_bench (R18) and
inst_post_bench (R25): 100 masks of 427 x 640 and of 480 x 640, the blobby masks those tools generate.

  (a) rle_encode       boxinstseg_amd.rle_encode (csrc/mask_rle.hip, four launches) on the mask block alone, without and with the masks'
                       statistics: device events, warmed, interleaved, as many repetitions as make a window of at least 0.5 s per leg
                       (median, p25, p75, min, max in ms).  needed_bytes is what the encoder must READ -- n * h * w without statistics, the
                       boxes' pixels with them; share_of_achievable_hbm = needed_bytes / HBM_ACHIEVABLE / the call's time.  That is the
                       whole call over the rate of a copy, not one kernel's share: the call is four dependent launches.
  (b) torch_composed   the same transitions from torch ops on the device: transpose -> flatten -> diff -> nonzero (the honest device
                       competitor; nonzero synchronises, and the counts still have to be cut per mask and turned into strings).  Checked
                       against our counts before timing.
  (c) results          solo_encode_results / box2mask_encode_results to host-ready results against solo_format_results /
                       box2mask_format_results, which stop BEFORE any encoding: wall clock around the call (each ends in a
                       synchronisation), bytes copied to the host, synchronising calls, kernel launches.
  kernel_us            the four kernels' times from `rocprofv3 --kernel-trace --stats` in a run of its own (`--trace-only plain|stats` runs just
                       rle_encode ten times per shape for it; --kernel-us takes the averages of the stats run back in)
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r28_mask_rle_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

import __graft_entry__ as entry
from corr_bench import count_launches, count_syncs
from inst_post_bench import blobs
from seg_paste_bench import HBM_ACHIEVABLE, timed, wall
from tests import rle_ref as R

N = 100
SHAPES = {'r18_427x640': (427, 640), 'r25_480x640': (480, 640)}


def torch_composed(masks):
    """-> (positions of the transitions [m, 2] = mask, linear index; transitions per mask [n])."""
    flat = masks.transpose(1, 2).flatten(1)
    d = torch.diff(flat, dim=1, prepend=flat.new_zeros((flat.shape[0], 1))) != 0
    return d.nonzero(), d.sum(1)


def counts_of(pos, h, w, n):
    """The counts the positions of torch_composed stand for (host; not timed)."""
    out = []
    pos = pos.cpu().numpy()
    for i in range(n):
        p = pos[pos[:, 0] == i, 1]
        out += np.diff(np.concatenate([[0], p, [h * w]])).tolist()
    return np.array(out, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r28_mask_rle_bench.json'))
    ap.add_argument('--trace-only', choices=('plain', 'stats'), help='run rle_encode alone ten times per shape, without or with the statistics '
                    '(for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--kernel-us', type=float, nargs=4, metavar=('BITS', 'SCAN', 'OFFSETS', 'EMIT'),
                    help='traced average times of the four kernels over both shapes of the `--trace-only stats` run')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mask_rle_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    from boxinstseg_amd.seg_paste import paste_results
    dev = torch.device('cuda:0')
    out = {'gpu': torch.cuda.get_device_name(0), 'masks': N, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE}
    for name, (h, w) in SHAPES.items():
        rng = np.random.default_rng(3)
        host = (blobs(rng, N, h, w) > 0).astype(np.uint8)
        stats_h = R.stats_of(host)
        masks, stats = torch.from_numpy(host).to(dev), torch.from_numpy(stats_h).to(dev)
        if args.trace_only:
            for _ in range(10):
                bx.rle_encode(masks, stats if args.trace_only == 'stats' else None)
            torch.cuda.synchronize()
            continue
        want = R.packed(host)
        enc = bx.rle_encode(masks, stats)
        rles = enc.to_coco()
        torch.cuda.synchronize()
        assert not enc.retried and rles == [R.encode(m, fast=True) for m in host]
        assert np.array_equal(enc.counts.cpu().numpy().view(np.uint32)[:len(want[1])], want[1])
        pos, per_mask = torch_composed(masks)
        assert np.array_equal(counts_of(pos, h, w, N), want[1]) and np.array_equal(per_mask.cpu().numpy() + 1, np.diff(want[0]))
        box_bytes = int(((stats_h[:, 3] - stats_h[:, 1] + 1) * (stats_h[:, 4] - stats_h[:, 2] + 1))[stats_h[:, 0] > 0].sum())
        row = dict(shape=(h, w), mask_bytes=N * h * w, box_bytes=box_bytes, runs=int(want[0][-1]), chars=int(want[2][-1]),
                   capacities=dict(runs=enc.cap_runs, chars=enc.cap_chars),
                   **timed({'rle_encode': lambda: bx.rle_encode(masks), 'rle_encode_stats': lambda: bx.rle_encode(masks, stats),
                            'torch_composed': lambda: torch_composed(masks)}))
        for key, needed in (('rle_encode', N * h * w), ('rle_encode_stats', box_bytes)):
            row[key].update(needed_bytes=needed, share_of_achievable_hbm=round(needed / HBM_ACHIEVABLE / (row[key]['ms'] * 1e-3), 4),
                            launches=count_launches(lambda: bx.rle_encode(masks, stats if key.endswith('stats') else None)),
                            host_syncs=count_syncs(lambda: bx.rle_encode(masks, stats if key.endswith('stats') else None)))
        row['torch_composed'].update(launches=count_launches(lambda: torch_composed(masks)), host_syncs=count_syncs(lambda: torch_composed(masks)))
        out[name] = row
    if args.trace_only:
        return
    out['kernel_us'] = dict(zip(('rle_bits_kernel', 'rle_scan_kernel', 'rle_offsets_kernel', 'rle_emit_kernel'), args.kernel_us)) if args.kernel_us \
        else 'not measured'
    # (c) the results objects of the two pipelines at their own shapes
    from seg_paste_bench import HW, META, N_ALL, THR
    from tests import matrix_nms_ref as M
    rng = np.random.default_rng(1)
    small = torch.from_numpy(M.disc_probs(rng, N_ALL, 25, 38)).to(dev)
    probs = small.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    keep = torch.from_numpy(rng.permutation(N_ALL)).to(dev)[:N]
    res = paste_results(types.SimpleNamespace(scores=torch.rand(N, device=dev), labels=torch.randint(0, 80, (N,), device=dev), masks=None),
                        probs, keep, HW, META, THR)
    from inst_post_bench import SHAPES as INST_SHAPES
    s = INST_SHAPES['landscape']
    rng = np.random.default_rng(3)
    pred = torch.from_numpy(blobs(rng, 100, *s['hw'])[None]).to(dev)
    cls = torch.from_numpy(rng.normal(0, 2.0, (1, 100, 81)).astype(np.float32)).to(dev)
    inst = bx.box2mask_instances(cls, pred, [dict(batch_input_shape=s['up'], img_shape=s['crop'] + (3,), ori_shape=s['ori'] + (3,))],
                                 dict(max_per_image=100), 80, 0, rescale=True)[0]
    legs = {'solo_427x640': (res, lambda: bx.solo_encode_results(res, 80), lambda: bx.solo_format_results(res, 80)),
            'box2mask_480x640': (inst, lambda: bx.box2mask_encode_results(inst, 80), lambda: bx.box2mask_format_results(inst, 80))}
    out['results'] = {}
    for name, (obj, encode, fmt) in legs.items():
        n, oh, ow = obj.masks.shape
        head = obj.host_block.numel() - n * oh * ow
        cap_chars = 2 * min(n * (2 * ow + 2), n * (oh * ow + 1))
        row = {'encode_results': dict(wall(encode, 15), launches=count_launches(encode), host_syncs=count_syncs(encode),
                                      bytes_to_host=(head + 7) // 8 * 8 + 4 + 8 * (n + 1) + cap_chars),
               'format_results_parent': dict(wall(fmt, 15), launches=count_launches(fmt), host_syncs=count_syncs(fmt),
                                             bytes_to_host=obj.host_block.numel())}
        out['results'][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
