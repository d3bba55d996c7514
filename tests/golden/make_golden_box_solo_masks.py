"""Regenerate tests/golden/box_solo_masks.npz by EXECUTING the reference's own statements on the CPU (developer tool; needs the upstream
checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied: the statements are taken out of
mmdet/models/dense_heads/box_solov2_head.py by AST and compiled in memory --

    BoxSOLOv2Head.forward   ``N, c, h, w = feature_pred.shape`` through the loop over the five levels (:205-216), run with ``eval=False``;
    BoxSOLOv2Head.loss      ``ins_preds = [torch.cat([ins_preds_level_img[ins_ind_labels_level_img, ...] ...`` (:317-320).

Cases: CASES of tests/box_solo_masks_ref.py, inputs from its make_case.  Recorded per case: the inputs, the fp64 rows of every level and
the gradients of ``sum_l (rows_l * g_l).sum()`` with respect to the feature and every kernel map (through the restatement, which the
check below ties to the reference), and the tests' relative bounds ``tol_*``: 4 x the fp32-against-fp64 difference of the reference's own
statements, relative to the largest fp64 value.

Checked before anything is written: tests/box_solo_masks_ref.py equals the reference's statements EXACTLY, in fp64 and in fp32; and the
fp32 torch composition in the OTHER order (resize the feature, then multiply -- the order of the kernels) stays within ``tol_*`` on every
recorded case, rows and gradients, so that a correct kernel can pass."""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import box_solo_masks_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/box_solov2_head.py'
OUT = os.path.join(HERE, 'box_solo_masks.npz')


def _method(tree, cls, name):
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)


def _compile(nodes, path):
    m = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(m)
    return compile(m, path, 'exec')


def load_statements():
    """(forward block, loss statement) as code objects."""
    path = os.path.join(REF, HEAD)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    fwd = _method(tree, 'BoxSOLOv2Head', 'forward')
    first = next(i for i, n in enumerate(fwd.body) if isinstance(n, ast.Assign) and ast.unparse(n.value) == 'feature_pred.shape' and
                 isinstance(n.targets[0], ast.Tuple) and [e.id for e in n.targets[0].elts] == ['N', 'c', 'h', 'w'])
    last = next(i for i, n in enumerate(fwd.body) if isinstance(n, ast.For) and i > first and 'ins_pred.append' in ast.unparse(n))
    block = fwd.body[first:last + 1]
    text = ast.unparse(ast.Module(body=block, type_ignores=[]))
    assert len(block) == 4 and 'F.conv2d(feature_pred, kernel, groups=N)' in text and "mode='bilinear'" in text and 'range(5)' in text, text
    loss = _method(tree, 'BoxSOLOv2Head', 'loss')
    sel = next(n for n in loss.body if isinstance(n, ast.Assign) and [getattr(t, 'id', None) for t in n.targets] == ['ins_preds'])
    assert 'ins_preds_level_img[ins_ind_labels_level_img, ...]' in ast.unparse(sel)
    return _compile(block, path), _compile([sel], path)


class _HalfOf:
    """A featmap size h such that ``h * 2`` is the level's size, odd sizes included (the reference writes ``featmap_sizes[i][0] * 2``)."""

    def __init__(self, twice):
        self.twice = int(twice)

    def __mul__(self, k):
        assert k == 2
        return self.twice


def reference_rows(code, maps, feat, labels, sizes):
    """The reference's statements: per level [N_l, oh_l, ow_l]."""
    block, sel = code
    assert len(maps) == 5
    B = feat.shape[0]
    env = dict(torch=torch, F=F, eval=False, feature_pred=feat, kernel_pred=maps,
               self=types.SimpleNamespace(seg_num_grids=[int(m.shape[-1]) for m in maps]),
               featmap_sizes=[(_HalfOf(oh), _HalfOf(ow)) for oh, ow in sizes])
    exec(block, env)
    env2 = dict(torch=torch, ins_preds=env['ins_pred'], ins_ind_label_list=[[labels[l][b] for l in range(5)] for b in range(B)])
    exec(sel, env2)
    return env2['ins_preds']


def pipeline_settings():
    """Per configs/boxlevelset file what decides the level sizes: the Resize scales and Pad divisor of the training and the test pipeline
    and the head's strides (settings only)."""
    from boxinstseg_amd import load_config
    folder, out = os.path.join(REF, 'configs', 'boxlevelset'), {}

    def steps(pipeline):
        for step in pipeline:
            yield step
            yield from steps(step.get('transforms', []))
    for f in sorted(os.listdir(folder)):
        if not f.endswith('.py'):
            continue
        cfg = load_config(os.path.join(folder, f))
        scales, divisors = [], []
        for which in ('train', 'test'):
            data = cfg['data'][which]
            for step in steps(data['pipeline'] if 'pipeline' in data else data['dataset']['pipeline']):
                if 'img_scale' in step:
                    sc = step['img_scale']
                    scales += [list(x) for x in (sc if isinstance(sc, list) else [sc])]
                if step.get('type') == 'Pad':
                    divisors.append(int(step['size_divisor']))
        assert scales and divisors
        out[f] = dict(img_scales=sorted({tuple(x) for x in scales}), size_divisors=sorted(set(divisors)),
                      strides=list(cfg['model']['bbox_head']['strides']), seg_num_grids=list(cfg['model']['bbox_head']['num_grids']))
    return out


def main():
    import json
    with open(os.path.join(HERE, 'box_solo_masks_cfg.json'), 'w') as fh:
        json.dump(pipeline_settings(), fh, indent=1, sort_keys=True)
        fh.write('\n')
    code = load_statements()
    arrays = {}
    for name, spec in R.CASES.items():
        case = R.make_case(**spec)
        res, other = {}, {}
        for dtype in (torch.float64, torch.float32):
            feat, maps, labels, _ = R.to_torch(case, dtype)
            ref = reference_rows(code, maps, feat, labels, case['sizes'])
            mine = R.rows_ref(maps, feat, labels, case['sizes'])
            assert len(ref) == len(mine) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(ref, mine)), name
            res[dtype] = R.run_ref(case, dtype)
            other[dtype] = R.run_ref(case, dtype, R.resized_first)
            assert all(np.array_equal(a, b.double().numpy()) for a, b in zip(res[dtype][0], ref))
        q64, q32, o32 = res[torch.float64], res[torch.float32], other[torch.float32]
        arrays[f'{name}/feat'] = case['feat']
        for l in range(5):
            arrays[f'{name}/map{l}'], arrays[f'{name}/labels{l}'], arrays[f'{name}/g{l}'] = case['maps'][l], case['labels'][l], case['g'][l]
            arrays[f'{name}/rows{l}'], arrays[f'{name}/gmap{l}'] = q64[0][l], q64[2][l]
        arrays[f'{name}/gfeat'] = q64[1]
        tols = dict(rows=R.bound(R.flat(q32[0]), R.flat(q64[0])), gfeat=R.bound(q32[1], q64[1]), gmap=R.bound(R.flat(q32[2]), R.flat(q64[2])))
        for what, tol in tols.items():
            arrays[f'{name}/tol_{what}'] = np.float64(tol)
        # the order of the kernels, in fp32 torch: inside the bound, so a correct kernel can pass
        for what, got, want in (('rows', R.flat(o32[0]), R.flat(q64[0])), ('gfeat', o32[1], q64[1]), ('gmap', R.flat(o32[2]), R.flat(q64[2]))):
            err = float(np.abs(np.asarray(got, np.float64) - want).max()) / float(np.abs(want).max())
            print(f'  {name}/{what}: bound {tols[what]:.3e}, resize-then-multiply in fp32 {err:.3e}')
            assert err <= tols[what], (name, what, err, tols[what])
        # in fp64 the two orders agree to rounding
        o64 = other[torch.float64]
        assert np.abs(R.flat(o64[0]) - R.flat(q64[0])).max() <= 1e-12 and np.abs(o64[1] - q64[1]).max() <= 1e-12
    np.savez_compressed(OUT, **arrays)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays')


if __name__ == '__main__':
    main()
