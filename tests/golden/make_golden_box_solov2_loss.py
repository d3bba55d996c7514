#!/usr/bin/env python3
"""Writes tests/golden/box_solov2_loss.npz (arrays only): the reference's own statements of the mask part of ``BoxSOLOv2Head.loss``
(mmdet/models/dense_heads/box_solov2_head.py:331-367: the two lists, the level loop and the two means) executed from the reference
checkout by AST, the way tests/golden/make_golden_box2mask_block.py runs ``loss_single``: the statements run unmodified, under autograd,
in float32 on the CPU, with ``self.loss_boxpro`` / ``self.loss_levelset`` the reference's own classes (oracle/reference_extract.py).

What the loop iterates over -- ``ins_preds``, ``ins_labels``, ``img_target``, ``lst_target`` per level -- is built here from case
``three_groups`` of tests/bls_cases.py the way :294-320 and :412-416 build it: the level's rows, their target planes, and the per-row
copies of ``F.interpolate(norm_img[i], size, mode='bilinear')`` and of the same resize of the level-set feature.

PROVENANCE of the tree filter, recorded in the file's ``provenance`` key: ``self.mst`` and ``self.tree_filter`` are NOT the reference's
modules/tree_filter.py bound to a stand-in ``_C`` but the fp64 oracle of oracle/tree_filter_oracle.py behind the module's call signature
(tests/b2m_loss_ref.py: mst_trees, _TreeFilter).  Everything else is the reference's text.

Needs the reference checkout (REFERENCE_ROOT of oracle/reference_extract.py); run from the repository root:
    python tests/golden/make_golden_box_solov2_loss.py
Stores both losses, the per-row values and the gradients per level, ``lst_feat.grad`` and a checksum of the case's inputs."""
import ast
import os
import sys
import types
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from oracle import reference_extract as rx
from tests import b2m_loss_ref as R2
from tests import bls_cases as K

HEAD_FILE = 'mmdet/models/dense_heads/box_solov2_head.py'
LINES = (331, 367)
CASE = 'three_groups'


def load_block():
    """-> block(self, ins_preds, ins_labels, img_target, lst_target) returning (loss_project, loss_levelset, per-level lists)."""
    path = os.path.join(rx.REFERENCE_ROOT, HEAD_FILE)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    head = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'BoxSOLOv2Head')
    fn = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'loss')
    keep = [s for s in fn.body if LINES[0] <= s.lineno <= LINES[1]]
    assert keep[0].lineno == 331 and keep[-1].lineno == 367 and any(isinstance(s, ast.For) and s.lineno == 334 for s in keep), [s.lineno for s in keep]
    # the per-row lists are kept beside the means: `rows = (list(loss_project), list(loss_levelset))` in front of :366
    rows = ast.parse('rows = (list(loss_project), list(loss_levelset))').body[0]
    ret = ast.parse('return loss_project, loss_levelset, rows').body[0]
    body = keep[:-2] + [rows] + keep[-2:] + [ret]
    args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ('self', 'ins_preds', 'ins_labels', 'img_target', 'lst_target')],
                         kwonlyargs=[], kw_defaults=[], defaults=[])
    mod = ast.Module(body=[ast.FunctionDef(name='block', args=args, body=body, decorator_list=[])], type_ignores=[])
    ast.fix_missing_locations(mod)
    ls = rx.load_levelset()
    env = {'torch': torch, 'F': F}
    exec(compile(mod, path, 'exec'), env)
    stub = types.SimpleNamespace(
        loss_boxpro=ls.BoxProjectionLoss(loss_weight=K.LOSS_BOXPRO_WEIGHT), loss_levelset=ls.LevelsetLoss(loss_weight=K.LOSS_LEVELSET_WEIGHT),
        mst=lambda fm: torch.from_numpy(R2.mst_trees(fm)),
        tree_filter=lambda feature_in, embed_in, tree, low_tree=True: R2._TreeFilter.apply(feature_in, embed_in, tree.numpy(), low_tree, None))
    return env['block'], stub


def checksum(d):
    crc = 0
    for a in [d['norm_img'], d['lst_feat'], *d['ins_preds'], *d['masks'], *d['tgt_of'], *d['img_of']]:
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return crc


def main():
    block, stub = load_block()
    d = K.inputs(CASE)
    preds = [torch.from_numpy(p).requires_grad_(True) for p in d['ins_preds']]
    lf = torch.from_numpy(d['lst_feat']).requires_grad_(True)
    img = torch.from_numpy(d['norm_img'])
    B = d['B']
    ins_labels, img_target, lst_target = [], [], []
    for l, size in enumerate(d['level_sizes']):
        # :412-416 per image, :300-314 the copies per set cell (rows of a level are in image order)
        scale_img = [F.interpolate(img[i].unsqueeze(dim=0), size=size, mode='bilinear') for i in range(B)]
        scale_lst = [F.interpolate(lf[i].unsqueeze(dim=0), size=size, mode='bilinear') for i in range(B)]
        n = d['counts'][l]
        ins_labels.append(torch.from_numpy(d['masks'][l])[torch.from_numpy(d['tgt_of'][l])])
        img_target.append(torch.cat([scale_img[i].repeat(n[i], 1, 1, 1) for i in range(B)], 0))
        lst_target.append(torch.cat([scale_lst[i].expand(n[i], -1, -1, -1) for i in range(B)], 0))
    loss_project, loss_levelset, (rows_p, rows_l) = block(stub, preds, ins_labels, img_target, lst_target)
    (loss_project + loss_levelset).backward()
    out = {'provenance': np.array('statements box_solov2_head.py:331-367, LevelsetLoss, BoxProjectionLoss: the reference, by AST; mst and '
                                  'tree_filter: oracle/tree_filter_oracle.py (fp64) behind the module signature, NOT the reference modules on a '
                                  'stand-in _C; the loop\'s inputs: case three_groups of tests/bls_cases.py, built as :294-320 and :412-416 build them'),
           'case': np.array(CASE), 'inputs_crc32': np.array(checksum(d), np.int64),
           'loss_boxpro': loss_project.detach().numpy(), 'loss_levelset': loss_levelset.detach().numpy(), 'lst_grad': lf.grad.numpy()}
    live = [l for l in range(len(preds)) if len(d['ins_preds'][l])]
    for l in range(len(preds)):
        k = live.index(l) if l in live else None
        out[f'proj_{l}'] = rows_p[k].detach().numpy() if k is not None else np.zeros(0, np.float32)
        out[f'levelset_{l}'] = rows_l[k].detach().numpy() if k is not None else np.zeros(0, np.float32)
        out[f'grad_{l}'] = preds[l].grad.numpy() if preds[l].grad is not None else np.zeros(d['ins_preds'][l].shape, np.float32)
    print(float(loss_project.detach()), float(loss_levelset.detach()))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'box_solov2_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
