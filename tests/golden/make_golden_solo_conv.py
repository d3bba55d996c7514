"""Regenerate tests/golden/solo_conv.npz by EXECUTING the reference's own statements on the CPU (developer tool; needs the upstream
checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied: the statements are taken out of
mmdet/models/dense_heads/discobox_head.py by AST and compiled in memory --

    DiscoBoxSOLOv2Head.loss            the statements from ``s_kernel_preds = ...`` (:1180) through the mask loop (:1246) except the two
                                       that belong to other steps (``kernel_label_list``, ``color_feats``), and ``s_input =
                                       torch.sigmoid(s_input)`` with its teacher twin out of the loss loop (:1275-1279);
    DiscoBoxSOLOv2Head.get_seg_single  ``I, N = kernel_preds.shape`` .. ``seg_preds = F.conv2d(...).squeeze(0).sigmoid()`` (:1606-1608)

-- and run with ``use_ind_teacher=True`` (what configs/discobox ship), the teacher on its own seeded maps.  Cases: CASES / TEST_CASE of
tests/solo_conv_ref.py, inputs from its make_case.  Recorded per case: the inputs, the fp64 masks, logits and the three gradients (of
``(masks * g).sum()`` through the restatement, which the check below ties to the reference), and the tests' relative bounds ``tol_*``: 4 x
the fp32-against-fp64 difference of the reference's own statements, relative to the largest fp64 value.

Checked before anything is written: tests/solo_conv_ref.py equals the reference's statements EXACTLY, in fp64 and in fp32, student and
teacher, masks and image indices, training and test time."""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import solo_conv_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/discobox_head.py'
OUT = os.path.join(HERE, 'solo_conv.npz')

CASES, TEST_CASE = R.CASES, R.TEST_CASE


def _method(tree, cls, name):
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)


def _targets(node):
    return [t.id for t in getattr(node, 'targets', []) if isinstance(t, ast.Name)]


def _compile(nodes, path):
    m = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(m)
    return compile(m, path, 'exec')


def load_statements():
    """(loss block, sigmoid block, get_seg_single block) as code objects."""
    path = os.path.join(REF, HEAD)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    loss = _method(tree, 'DiscoBoxSOLOv2Head', 'loss')
    first = next(i for i, n in enumerate(loss.body) if 's_kernel_preds' in _targets(n))
    last = next(i for i, n in enumerate(loss.body) if isinstance(n, ast.For) and i > first and 's_kernel_preds' in ast.dump(n.iter))
    block = [n for n in loss.body[first:last + 1] if not set(_targets(n)) & {'kernel_label_list', 'color_feats'}]
    names = [t for n in block for t in _targets(n)]
    assert names[:4] == ['s_kernel_preds', 's_ins_pred_list', 't_ins_pred_list', 'img_ind_list'], names
    loop = next(n for n in loss.body[last + 1:] if isinstance(n, ast.For) and 's_ins_pred_list' in ast.dump(n.iter))
    at = next(i for i, n in enumerate(loop.body) if _targets(n) == ['s_input'] and 'sigmoid' in ast.dump(n.value))
    sig = loop.body[at:at + 2]
    assert isinstance(sig[1], ast.If) and 'use_ind_teacher' in ast.dump(sig[1].test)
    seg = _method(tree, 'DiscoBoxSOLOv2Head', 'get_seg_single')
    at = next(i for i, n in enumerate(seg.body) if isinstance(n, ast.Assign) and 'kernel_preds.shape' in ast.unparse(n))
    test = seg.body[at:at + 3]
    assert _targets(test[2]) == ['seg_preds'] and 'conv2d' in ast.unparse(test[2]) and 'sigmoid' in ast.unparse(test[2])
    return _compile(block, path), _compile(sig, path), _compile(test, path)


def reference_masks(code, s_maps, t_maps, order, s_feat, t_feat, sigmoid):
    """The reference's statements on (student, teacher): (s list, t list, img_ind_list)."""
    block, sig, _ = code
    B, L = s_feat.shape[0], len(s_maps)
    env = dict(torch=torch, F=F, use_ind_teacher=True, s_kernel_preds_raw=s_maps, t_kernel_preds_raw=t_maps, s_ins_pred=s_feat, t_ins_pred=t_feat,
               grid_order_list=[[order[l][b] for l in range(L)] for b in range(B)], zip=zip, enumerate=enumerate, len=len)
    exec(block, env)
    s_list, t_list = list(env['s_ins_pred_list']), list(env['t_ins_pred_list'])
    if sigmoid:
        for l in range(L):
            if s_list[l] is None:
                continue
            e2 = dict(torch=torch, use_ind_teacher=True, s_input=s_list[l], t_input=t_list[l])
            exec(sig, e2)
            s_list[l], t_list[l] = e2['s_input'], e2['t_input']
    return s_list, t_list, env['img_ind_list']


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        assert x is None or (x.dtype == y.dtype and torch.equal(x, y))


def main():
    code = load_statements()
    arrays = {}
    for name, spec in CASES.items():
        case = R.make_case(**spec)
        teacher = R.make_case(**dict(spec, seed=spec['seed'] + 100))
        res = {}
        for dtype in (torch.float64, torch.float32):
            for sigmoid in (True, False):
                feat, maps, order, _ = R.to_torch(case, dtype)
                t_feat, t_maps, _, _ = R.to_torch(teacher, dtype)
                s_ref, t_ref, ind_ref = reference_masks(code, maps, t_maps, order, feat, t_feat, sigmoid)
                s_mine, ind_mine = R.dynamic_masks(maps, order, feat, sigmoid)
                t_mine, _ = R.dynamic_masks(t_maps, order, t_feat, sigmoid)
                _same(s_ref, s_mine), _same(t_ref, t_mine), _same(ind_ref, ind_mine)
                res[dtype, sigmoid] = R.run_ref(case, dtype, sigmoid)
                assert np.array_equal(res[dtype, sigmoid][0], R.cat_levels(s_ref).double().numpy())
        arrays[f'{name}/feat'], arrays[f'{name}/g'] = case['feat'], case['g']
        for l, m in enumerate(case['maps']):
            arrays[f'{name}/map{l}'] = m
            for b, o in enumerate(case['order'][l]):
                arrays[f'{name}/order{l}_{b}'] = o
        for sigmoid, tag in ((True, 'sig'), (False, 'lin')):
            q64, q32 = res[torch.float64, sigmoid], res[torch.float32, sigmoid]
            arrays[f'{name}/{tag}/out'], arrays[f'{name}/{tag}/gfeat'] = q64[0], q64[1]
            for l, gm in enumerate(q64[2]):
                arrays[f'{name}/{tag}/gmap{l}'] = gm
            arrays[f'{name}/{tag}/tol_out'] = np.float64(R.bound(q32[0], q64[0]))
            arrays[f'{name}/{tag}/tol_gfeat'] = np.float64(R.bound(q32[1], q64[1]))
            arrays[f'{name}/{tag}/tol_gmap'] = np.float64(R.bound(np.concatenate([x.ravel() for x in q32[2]]), np.concatenate([x.ravel() for x in q64[2]])))
    # test time: the statements of get_seg_single on gathered rows
    tc = TEST_CASE
    rng = np.random.default_rng(tc['seed'])
    seg = (0.5 * rng.standard_normal((1, tc['E'], tc['h'], tc['w']))).astype(np.float32)
    kern = (rng.standard_normal((tc['rows_all'], tc['E'])) / np.sqrt(tc['E'])).astype(np.float32)
    rows = np.asarray(tc['rows'], np.int64)
    got = {}
    for dtype in (torch.float64, torch.float32):
        env = dict(torch=torch, F=F, seg_preds=torch.from_numpy(seg).to(dtype), kernel_preds=torch.from_numpy(kern).to(dtype)[torch.from_numpy(rows)])
        exec(code[2], env)
        mine = R.candidate_masks(torch.from_numpy(seg).to(dtype), torch.from_numpy(kern).to(dtype)[torch.from_numpy(rows)])
        assert torch.equal(env['seg_preds'], mine)
        got[dtype] = env['seg_preds'].double().numpy()
    arrays['test/seg'], arrays['test/kernels'], arrays['test/rows'] = seg, kern, rows
    arrays['test/out'], arrays['test/tol_out'] = got[torch.float64], np.float64(R.bound(got[torch.float32], got[torch.float64]))
    np.savez_compressed(OUT, **arrays)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays')
    for k, v in arrays.items():
        if '/tol_' in k:
            print(f'  {k} = {float(v):.3e}')


if __name__ == '__main__':
    main()
