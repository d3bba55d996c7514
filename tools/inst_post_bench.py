#!/usr/bin/env python3
"""Developer measurement of Box2Mask's test-time path on the GPU box, at the test pipeline's shape (configs/box2mask/*_coco.py:157-163):
B = 1, Q = 100 queries, C = 80 classes, prediction 200 x 336, batch_input_shape 800 x 1344, img_shape 800 x 1333, ori_shape 480 x 640 with
rescale=True; and one portrait image: prediction 336 x 200, canvas 1344 x 800, img_shape 1333 x 800, ori_shape 640 x 427.

  ours     boxinstseg_amd.box2mask_instances (csrc/inst_post.hip): the top-k launch, the two paste launches, two small device copies
  torch    the reference's statements restated as torch ops on the same GPU: Box2MaskHead.simple_test's F.interpolate
           (box2mask_head.py:452-457), the crop and the second F.interpolate (maskformer_fusion_head.py:211-221), instance_postprocess
           (:133-160) with mask2bbox's loop (mmdet/core/mask/utils.py:68-89)
  Both are warmed, then timed interleaved in one process between two device events over as many repetitions as make a window of at least
  0.5 s each (median, p25, p75, min, max in ms).  Before timing the two results are compared: the same selection, mask bytes that differ,
  the largest det-score difference.
  topk_leg        the selection alone on both sides: instance_topk against the softmax / arange / topk / index statements
  peak_bytes      torch's peak allocation of one call above its inputs
  launches        kernel launches of one call (torch's profiler trace); host_syncs: synchronising calls (torch's sync debug mode)
  format          box2mask_format_results against the detector's loop (maskformer.py:160-169 restated: bbox2result and one
                  ``.detach().cpu().numpy()`` per mask) on the same 100 detections: wall clock around the call, launches, synchronisations
  kernel_us_landscape   the three kernels' times from `rocprofv3 --kernel-trace --stats` in a run of its own (--trace-only runs just our
                  path ten times per shape for it; --kernel-us takes the traced times back in)
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r25_inst_post_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
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
from seg_paste_bench import peak_bytes, timed, wall

Q, C, K = 100, 80, 100
SHAPES = {
    'landscape': dict(hw=(200, 336), up=(800, 1344), crop=(800, 1333), ori=(480, 640)),
    'portrait': dict(hw=(336, 200), up=(1344, 800), crop=(1333, 800), ori=(640, 427)),
}


def blobs(rng, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.2 * h, 0.8 * h, n), rng.uniform(0.2 * w, 0.8 * w, n)
    r = rng.uniform(0.1, 0.35, n) * min(h, w)
    d = np.sqrt((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2)
    return (0.5 * (r[:, None, None] - d) + rng.normal(0, 0.2, (n, h, w))).astype(np.float32)


def mask2bbox(masks):
    n = masks.shape[0]
    bboxes = masks.new_zeros((n, 4), dtype=torch.float32)
    x_any, y_any = torch.any(masks, dim=1), torch.any(masks, dim=2)
    for i in range(n):
        x, y = torch.where(x_any[i, :])[0], torch.where(y_any[i, :])[0]
        if len(x) > 0 and len(y) > 0:
            bboxes[i, :] = bboxes.new_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1])
    return bboxes


def torch_path(mask_cls, mask_pred, s):
    """-> (labels, bboxes, masks, top_indices) of image 0."""
    x = F.interpolate(mask_pred, size=s['up'], mode='bilinear', align_corners=False)
    x = x[0][:, :s['crop'][0], :s['crop'][1]]
    x = F.interpolate(x[:, None], size=s['ori'], mode='bilinear', align_corners=False)[:, 0]
    cls = mask_cls[0]
    scores = F.softmax(cls, dim=-1)[:, :-1]
    labels = torch.arange(C, device=cls.device).unsqueeze(0).repeat(Q, 1).flatten(0, 1)
    scores_per_image, top_indices = scores.flatten(0, 1).topk(K, sorted=False)
    labels_per_image = labels[top_indices]
    x = x[top_indices // C]
    is_thing = labels_per_image < C
    scores_per_image, labels_per_image, x = scores_per_image[is_thing], labels_per_image[is_thing], x[is_thing]
    binary = (x > 0).float()
    mask_scores = (x.sigmoid() * binary).flatten(1).sum(1) / (binary.flatten(1).sum(1) + 1e-6)
    det = scores_per_image * mask_scores
    binary = binary.bool()
    return labels_per_image, torch.cat([mask2bbox(binary), det[:, None]], dim=-1), binary, top_indices


def torch_topk(mask_cls):
    """The selection alone (maskformer_fusion_head.py:136-151)."""
    cls = mask_cls[0]
    scores = F.softmax(cls, dim=-1)[:, :-1]
    labels = torch.arange(C, device=cls.device).unsqueeze(0).repeat(Q, 1).flatten(0, 1)
    scores_per_image, top_indices = scores.flatten(0, 1).topk(K, sorted=False)
    labels_per_image = labels[top_indices]
    is_thing = labels_per_image < C
    return scores_per_image[is_thing], labels_per_image[is_thing], (top_indices // C)[is_thing]


def loop_format(labels, bboxes, masks):
    b, lab = bboxes.detach().cpu().numpy(), labels.detach().cpu().numpy()
    bbox_results = [b[lab == i, :] for i in range(C)]
    mask_results = [[] for _ in range(C)]
    for j, label in enumerate(labels):
        mask_results[label].append(masks[j].detach().cpu().numpy())
    return bbox_results, mask_results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r25_inst_post_bench.json'))
    ap.add_argument('--trace-only', action='store_true', help='run our path alone a few times (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--kernel-us', type=float, nargs=3, metavar=('TOPK', 'PASTE', 'STATS'),
                    help='traced times of inst_topk_kernel, inst_paste_kernel and inst_stats_kernel at the landscape shape')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inst_post_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    out = {'gpu': torch.cuda.get_device_name(0), 'queries': Q, 'classes': C, 'max_per_image': K}
    cfg = dict(max_per_image=K)
    for name, s in SHAPES.items():
        rng = np.random.default_rng(3)
        pred = torch.from_numpy(blobs(rng, Q, *s['hw'])[None]).to(dev)
        cls = torch.from_numpy(rng.normal(0, 2.0, (1, Q, C + 1)).astype(np.float32)).to(dev)
        metas = [dict(batch_input_shape=s['up'], img_shape=s['crop'] + (3,), ori_shape=s['ori'] + (3,))]

        def ours():
            return bx.box2mask_instances(cls, pred, metas, cfg, C, 0, rescale=True)[0]

        def ref():
            return torch_path(cls, pred, s)
        if args.trace_only:
            for _ in range(10):
                ours()
            torch.cuda.synchronize()
            continue
        r, (t_labels, t_boxes, t_masks, t_top) = ours(), ref()
        mine = (r.query * C + r.labels).cpu().numpy()
        theirs = t_top.cpu().numpy()
        assert sorted(mine.tolist()) == sorted(theirs.tolist())
        order = torch.from_numpy(np.array([theirs.tolist().index(f) for f in mine])).to(dev)
        row = dict(shape=s, output_bytes=K * s['ori'][0] * s['ori'][1],
                   differing_mask_bytes=int((r.masks != t_masks[order]).sum()),
                   box_corners_equal=bool(torch.equal(r.bboxes[:, :4], t_boxes[order, :4])),
                   max_det_score_difference=float((r.bboxes[:, 4] - t_boxes[order, 4]).abs().max()),
                   **timed({'ours': ours, 'torch': ref}))
        for key, fn in (('ours', ours), ('torch', ref)):
            row[key].update(peak_bytes=peak_bytes(fn), launches=count_launches(fn), host_syncs=count_syncs(fn))
        if name == 'landscape':                                                   # the selection leg does not depend on the image's shape
            legs = {'ours': lambda: bx.instance_topk(cls, C, 0, K), 'torch': lambda: torch_topk(cls)}
            out['topk_leg'] = timed(legs)
            for key, fn in legs.items():
                out['topk_leg'][key].update(launches=count_launches(fn), host_syncs=count_syncs(fn))
        row['format'] = {}
        for key, fn in (('box2mask_format_results', lambda: bx.box2mask_format_results(r, C)),
                        ('per_mask_loop', lambda: loop_format(t_labels, t_boxes, t_masks))):
            row['format'][key] = dict(wall(fn, 7), launches=count_launches(fn), host_syncs=count_syncs(fn))
        out[name] = row
    if args.trace_only:
        return
    out['kernel_us_landscape'] = dict(zip(('inst_topk_kernel', 'inst_paste_kernel', 'inst_stats_kernel'), args.kernel_us)) if args.kernel_us \
        else 'not measured'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
