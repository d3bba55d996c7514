"""Regenerate tests/golden/box2mask_test.npz and box2mask_test_cfg.json by EXECUTING the reference's own statements on the CPU (developer
tool; needs the upstream checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied: the functions and statements are taken out
of its files by AST and compiled in memory --

    mmdet/models/dense_heads/box2mask_head.py       Box2MaskHead.simple_test: the ``mask_pred_results = F.interpolate(...)`` statement
    mmdet/models/seg_heads/panoptic_fusion_heads/maskformer_fusion_head.py
                                                    MaskFormerFusionHead.instance_postprocess and .simple_test (whole methods), and the
                                                    statements of instance_postprocess once more at top level, for the intermediate values
                                                    (top_indices, scores_per_image, mask_scores_per_image)
    mmdet/core/mask/utils.py                        mask2bbox
    mmdet/core/bbox/transforms.py                   bbox2result
    mmdet/models/detectors/maskformer.py            MaskFormer.simple_test: the ``for i in range(len(results))`` formatting loop

-- and run on the seeded inputs of tests/inst_post_ref.py (CASES).  Recorded per case: the inputs, the reference's labels, boxes, masks
(packed to bits), the flat indices it selected, its class and mask scores, and what the detector's loop makes of them.  Checked before
anything is written: the input conditions of the tests (at most 0.1 % of a case's pixels inside the mask band, at most two indices inside
the top-k band) and that the float64 restatement agrees with the reference under those rules.  The panoptic_fusion_head and test_cfg blocks
of every configs/box2mask file go to box2mask_test_cfg.json."""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import inst_post_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/box2mask_head.py'
FUSION = 'mmdet/models/seg_heads/panoptic_fusion_heads/maskformer_fusion_head.py'
MASK_UTILS = 'mmdet/core/mask/utils.py'
TRANSFORMS = 'mmdet/core/bbox/transforms.py'
DETECTOR = 'mmdet/models/detectors/maskformer.py'


def _tree(rel):
    path = os.path.join(REF, rel)
    with open(path) as fh:
        return ast.parse(fh.read(), filename=path), path


def _function(tree, name, cls=None):
    body = tree.body if cls is None else next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)


def _compile(nodes, path):
    m = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(m)
    return compile(m, path, 'exec')


def load_reference():
    env = dict(torch=torch, F=F, np=np)
    tree, path = _tree(MASK_UTILS)
    exec(_compile([_function(tree, 'mask2bbox')], path), env)
    tree, path = _tree(TRANSFORMS)
    exec(_compile([_function(tree, 'bbox2result')], path), env)
    tree, path = _tree(FUSION)
    post, simple = _function(tree, 'instance_postprocess', 'MaskFormerFusionHead'), _function(tree, 'simple_test', 'MaskFormerFusionHead')
    exec(_compile([post, simple], path), env)
    assert isinstance(post.body[-1], ast.Return) and 'topk' in ast.unparse(post) and 'mask2bbox' in ast.unparse(post)
    statements = _compile([n for n in post.body[:-1] if not (isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant))], path)
    tree, path = _tree(HEAD)
    head = _function(tree, 'simple_test', 'Box2MaskHead')
    resize = [n for n in head.body if isinstance(n, ast.Assign) and 'F.interpolate' in ast.unparse(n)]
    assert len(resize) == 1 and [t.id for t in resize[0].targets] == ['mask_pred_results'], [ast.unparse(n) for n in resize]
    resize = _compile(resize, path)
    tree, path = _tree(DETECTOR)
    det = _function(tree, 'simple_test', 'MaskFormer')
    loop = [n for n in det.body if isinstance(n, ast.For) and 'bbox2result' in ast.unparse(n)]
    assert len(loop) == 1 and '.cpu().numpy()' in ast.unparse(loop[0])
    return env, statements, resize, _compile(loop, path)


def run_case(name, ref):
    env, statements, resize, loop = ref
    c = R.CASES[name]
    cls, pred = R.case_inputs(name)
    things, C = c['things'], c['things'] + c['stuff']
    test_cfg = dict(panoptic_on=False, semantic_on=False, instance_on=True, max_per_image=c['k'], iou_thr=0.8, filter_low_score=True)
    head = types.SimpleNamespace(test_cfg=test_cfg, num_classes=C, num_things_classes=things, num_stuff_classes=c['stuff'])
    head.instance_postprocess = lambda mask_cls, mask_pred: env['instance_postprocess'](head, mask_cls, mask_pred)
    meta = dict(batch_input_shape=c['up'], img_shape=(*c['crop'], 3), ori_shape=(*c['ori'], 3))
    # the head's resize, then the fusion head
    e1 = dict(env, mask_pred_results=torch.from_numpy(pred)[None], img_shape=c['up'])
    exec(resize, e1)
    up = e1['mask_pred_results']
    assert tuple(up.shape) == (1, c['Q'], *c['up'])
    results = env['simple_test'](head, torch.from_numpy(cls)[None], up, [meta], rescale=c['rescale'])
    labels, bboxes, masks = results[0]['ins_results']
    out = tuple(c['ori']) if c['rescale'] else tuple(c['crop'])
    assert tuple(masks.shape[1:]) == out and masks.dtype == torch.bool and bboxes.dtype == torch.float32
    # the same statements at top level, for the intermediates
    x = up[0][:, :c['crop'][0], :c['crop'][1]]
    if c['rescale']:
        x = F.interpolate(x[:, None], size=out, mode='bilinear', align_corners=False)[:, 0]
    e2 = dict(env, self=head, mask_cls=torch.from_numpy(cls), mask_pred=x)
    exec(statements, e2)
    assert torch.equal(e2['labels_per_image'], labels) and torch.equal(e2['bboxes'], bboxes) and torch.equal(e2['mask_pred_binary'], masks)
    flat = e2['top_indices'][e2['is_thing']]
    # the detector's loop
    det = types.SimpleNamespace(num_things_classes=things, num_stuff_classes=c['stuff'])
    e3 = dict(env, self=det, results=[dict(results[0])])
    exec(loop, e3)
    bbox_results, mask_results = e3['results'][0]['ins_results']
    rec = {
        'cls': cls, 'pred': pred, 'labels': labels.numpy(), 'bboxes': bboxes.numpy(), 'flat': flat.numpy(),
        'masks': np.packbits(masks.numpy().reshape(len(masks), -1), axis=1), 'cls_scores': e2['scores_per_image'].numpy(),
        'mask_scores': e2['mask_scores_per_image'].numpy(), 'fmt_boxes': np.concatenate(bbox_results).astype(np.float32),
        'fmt_box_counts': np.array([len(b) for b in bbox_results]), 'fmt_mask_counts': np.array([len(m) for m in mask_results]),
        'fmt_mask_areas': np.array([int(m.sum()) for per in mask_results for m in per], np.int64),
    }
    assert all(isinstance(m, np.ndarray) and m.dtype == np.bool_ for per in mask_results for m in per)
    assert all(b.dtype == np.float32 for b in bbox_results)
    check_case(name, rec)
    return rec


def check_case(name, rec):
    """The input conditions of the tests, and the restatement against what the reference gave."""
    c = R.CASES[name]
    C = c['things'] + c['stuff']
    out = tuple(c['ori']) if c['rescale'] else tuple(c['crop'])
    s64 = R.softmax64(rec['cls']).reshape(-1)
    cut = np.sort(s64)[::-1][c['k'] - 1]
    near = int(((s64 >= cut * (1 - 2.0 ** -20)) & (s64 <= cut * (1 + 2.0 ** -20))).sum()) - 1
    assert near <= 2, (name, near)
    scores, labels, query, flat = R.topk_ref(rec['cls'], c['things'], c['k'])
    assert sorted(flat.tolist()) == sorted(rec['flat'].tolist()), name
    order = np.array([flat.tolist().index(f) for f in rec['flat']], np.int64)          # the reference's rows in our order
    assert np.array_equal(labels[order], rec['labels']) and np.array_equal(rec['flat'] % C, rec['labels'])
    assert np.allclose(scores[order], rec['cls_scores'], rtol=1e-5, atol=0)
    p = R.p64(rec['pred'], query[order], c['up'], c['crop'], out)
    assert R.band_share(p, rec['pred'], query[order]) <= R.BAND_SHARE, (name, R.band_share(p, rec['pred'], query[order]))
    ref_masks = np.unpackbits(rec['masks'], axis=1)[:, :out[0] * out[1]].reshape(-1, *out)
    R.check_masks(ref_masks, p, rec['pred'], query[order], name)
    m, stats, mask_scores, boxes = R.instance_ref(p, scores[order])
    same = (m == ref_masks).reshape(len(m), -1).all(1)
    assert same.mean() >= 0.75, (name, same)
    assert np.array_equal(boxes[same, :4], rec['bboxes'][same, :4].astype(np.float64)), name
    assert np.allclose(mask_scores[same], rec['mask_scores'][same], rtol=1e-5, atol=1e-7), name
    assert np.allclose(boxes[same, 4], rec['bboxes'][same, 4], rtol=1e-5, atol=1e-7), name
    if name == 'zero_plane':
        z = np.nonzero(query[order] == 2)[0]
        assert len(z) >= 1 and not ref_masks[z].any() and not rec['bboxes'][z].any()


def main():
    import boxinstseg_amd as B
    ref = load_reference()
    arrays = {}
    for name in sorted(R.CASES):
        for key, value in run_case(name, ref).items():
            arrays[f'{name}/{key}'] = value
    np.savez_compressed(R.GOLDEN, **arrays)
    print(f'wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes, {len(arrays)} arrays')
    blocks = {}
    for f in sorted(os.listdir(os.path.join(REF, 'configs/box2mask'))):
        model = B.load_config(os.path.join(REF, 'configs/box2mask', f))['model']
        blocks[f] = dict(panoptic_fusion_head=model['panoptic_fusion_head'], test_cfg=model['test_cfg'])
    with open(R.CFG_JSON, 'w') as fh:
        json.dump(blocks, fh, indent=1)
        fh.write('\n')
    print(f'wrote {R.CFG_JSON}: {len(blocks)} configs')


if __name__ == '__main__':
    main()
