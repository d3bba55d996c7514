"""Regenerate tests/golden/matrix_nms.npz by EXECUTING the reference's own code on the CPU (developer tool; needs the upstream
checkout, BOXINST_REFERENCE_ROOT or /root/reference).  Nothing of the reference is copied: ``mask_matrix_nms`` is loaded from its
file where it lies (it imports only torch), ``BoxSOLOv2Head.get_seg_single`` is taken out of its class by AST and compiled in
memory with a stand-in ``InstanceData``.  The fixture holds arrays only (masks through np.packbits).

Cases
  g20 / g05 / lin / cut   mask_matrix_nms at n = 40: gaussian sigma 2.0 and 0.5, linear; without cuts, and with nms_pre,
                          filter_thr and max_num.  Overlapping discs around a few shared centres, shuffled linspace scores.
  seg                     get_seg_single at an 11 x 17 feature map with two FPN levels.  The candidates' probabilities are
                          sigmoid(conv1x1(feat, kernels)) with kernels that have two non-zero taps (exact in any summation order),
                          so the same case also feeds the DiscoBox mirror, whose block after the sigmoid is the same text
                          (discobox_head.py:1610-1660).
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import matrix_nms_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
NMS_FILE = os.path.join(REF, 'mmdet/core/post_processing/matrix_nms.py')
HEAD_FILE = os.path.join(REF, 'mmdet/models/dense_heads/box_solov2_head.py')

CASES = {   # name: (seed, h, w, labels, kernel, sigma, nms_pre, filter_thr, max_num)
    'g20': (1, 24, 40, 3, 'gaussian', 2.0, -1, -1, -1),
    'g05': (2, 25, 38, 2, 'gaussian', 0.5, 30, 0.4, -1),
    'lin': (3, 24, 40, 3, 'linear', 2.0, -1, 0.15, 12),
    'cut': (5, 25, 38, 1, 'gaussian', 2.0, 25, 0.3, 10),
}
SEG_CFG = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=20, kernel='gaussian', sigma=2.0)
SEG_GRIDS, SEG_STRIDES = (6, 4), (8, 32)


class InstanceData:
    def __init__(self, meta):
        for k, v in meta.items():
            setattr(self, k, v)


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_matrix_nms', NMS_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(HEAD_FILE) as fh:
        tree = ast.parse(fh.read(), filename=HEAD_FILE)
    fn = None
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == 'BoxSOLOv2Head':
            fn = next(s for s in node.body if isinstance(s, ast.FunctionDef) and s.name == 'get_seg_single')
    fn.decorator_list = []
    m = ast.Module(body=[fn], type_ignores=[])
    ast.fix_missing_locations(m)
    env = {'torch': torch, 'F': F, 'InstanceData': InstanceData, 'mask_matrix_nms': mod.mask_matrix_nms}
    exec(compile(m, HEAD_FILE, 'exec'), env)
    return mod.mask_matrix_nms, env['get_seg_single']


def seg_inputs():
    """feat [1,8,11,17], kernels [52,8] (two exact taps each), cate_preds [52,3]."""
    rng = np.random.default_rng(77)
    h, w, C, cells, ncls = 11, 17, 8, sum(g * g for g in SEG_GRIDS), 3
    yy, xx = np.mgrid[0:h, 0:w]
    feat = np.zeros((1, C, h, w), np.float32)
    for c in range(6):
        cy, cx = (3.5, 5.0) if c < 3 else (7.0, 11.5)
        cy, cx, r = cy + rng.normal(0, 0.7), cx + rng.normal(0, 0.7), rng.uniform(2.5, 4.0)
        feat[0, c] = 1.5 * (r - np.hypot(yy - cy, xx - cx)) + rng.normal(0, 0.2, (h, w))
    feat[0, 6] = 1.0
    feat[0, 7] = rng.normal(0, 1.0, (h, w))
    kernels = np.zeros((cells, C), np.float32)
    kernels[np.arange(cells), rng.integers(0, 6, cells)] = 1.0
    kernels[:, 6] = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0], cells)
    cate = np.where(rng.uniform(size=(cells, ncls)) < 0.3, rng.uniform(0.12, 0.95, (cells, ncls)), rng.uniform(0.0, 0.08, (cells, ncls))).astype(np.float32)
    return feat, kernels, cate


def main():
    ref_nms, ref_get_seg_single = load_reference()
    out = {}
    for name, (seed, h, w, nlab, kernel, sigma, nms_pre, thr, max_num) in CASES.items():
        rng = np.random.default_rng(seed)
        n = 40
        masks = R.disc_masks(rng, n, h, w)
        labels = rng.integers(0, nlab, n)
        scores = R.shuffled_scores(rng, n)
        s, l, m, k = ref_nms(torch.from_numpy(masks), torch.from_numpy(labels), torch.from_numpy(scores), filter_thr=thr, nms_pre=nms_pre,
                             max_num=max_num, kernel=kernel, sigma=sigma)
        full = ref_nms(torch.from_numpy(masks), torch.from_numpy(labels), torch.from_numpy(scores), kernel=kernel, sigma=sigma, nms_pre=nms_pre)
        decayed_frac = float((full[0].numpy() < scores[full[3].numpy()] * (1 - 1e-6)).mean())
        gap = R.min_rel_gap(R.matrix_nms_ref(masks, labels, scores, thr, nms_pre, max_num, kernel, sigma)['decayed'], (thr,))
        print(f'{name}: kept {len(k)} of {n}, decayed {decayed_frac:.0%}, smallest relative gap of the decayed scores {gap:.1e}')
        assert gap > 1e-4, 'the tests assert this gap before they compare orders: pick another seed'
        assert torch.equal(m, torch.from_numpy(masks)[k])
        out.update({f'{name}_masks': np.packbits(masks.reshape(n, -1), axis=1), f'{name}_hw': np.array([h, w]), f'{name}_labels': labels,
                    f'{name}_scores': scores, f'{name}_kernel': np.array(0 if kernel == 'gaussian' else 1), f'{name}_sigma': np.array(sigma),
                    f'{name}_nms_pre': np.array(nms_pre), f'{name}_filter_thr': np.array(thr), f'{name}_max_num': np.array(max_num),
                    f'{name}_out_scores': s.numpy(), f'{name}_out_labels': l.numpy(), f'{name}_keep_inds': k.numpy()})

    feat, kernels, cate = seg_inputs()
    probs = F.conv2d(torch.from_numpy(feat), torch.from_numpy(kernels)[:, :, None, None]).squeeze(0).sigmoid()
    exact = torch.sigmoid(torch.from_numpy((feat[0][None] * kernels[:, :, None, None]).astype(np.float64).sum(1).astype(np.float32)))
    assert torch.equal(probs, exact), 'the two-tap kernels are meant to make the convolution exact'
    meta = dict(img_shape=(41, 66, 3), ori_shape=(60, 101, 3))
    self = types.SimpleNamespace(seg_num_grids=list(SEG_GRIDS), strides=list(SEG_STRIDES))
    res = ref_get_seg_single(self, torch.from_numpy(cate).clone(), probs.clone(), (11, 17), meta, types.SimpleNamespace(**SEG_CFG))
    print(f'seg: {len(res.scores)} kept, labels {sorted(set(res.labels.tolist()))}')
    out.update({'seg_feat': feat, 'seg_kernels': kernels, 'seg_cate': cate, 'seg_probs': probs.numpy(),
                'seg_grids': np.array(SEG_GRIDS), 'seg_strides': np.array(SEG_STRIDES),
                'seg_img_shape': np.array(meta['img_shape']), 'seg_ori_shape': np.array(meta['ori_shape']),
                'seg_cfg': np.array([SEG_CFG[k] for k in ('score_thr', 'mask_thr', 'filter_thr', 'nms_pre', 'max_per_img', 'sigma')], np.float64),
                'seg_out_scores': res.scores.numpy(), 'seg_out_labels': res.labels.numpy(),
                'seg_out_masks': np.packbits(res.masks.numpy().reshape(len(res.masks), -1), axis=1)})
    path = os.path.join(HERE, 'matrix_nms.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
