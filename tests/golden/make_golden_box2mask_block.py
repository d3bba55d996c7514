#!/usr/bin/env python3
"""Writes tests/golden/box2mask_block.npz (arrays only): the reference's own statements of ``Box2MaskHead.loss_single`` after its
classification loss (mmdet/models/dense_heads/box2mask_head.py:230-233 and :260-335) executed from the reference checkout by AST, the way
tests/golden/make_golden.py loads the level-set classes (oracle/reference_extract.py): the statements run unmodified, under autograd,
in float32 on the CPU, with ``self.loss_box`` / ``self.loss_mask`` / ``LCM`` / ``_scale_target`` the reference's own classes and function.

PROVENANCE of the tree filter, recorded in the file's ``provenance`` key: ``self.mst`` and ``self.tree_filter`` are NOT the reference's
modules/tree_filter.py bound to a stand-in ``_C`` -- that binding was not built -- but the fp64 oracle of oracle/tree_filter_oracle.py
behind the module's call signature (tests/b2m_loss_ref.py: mst_trees, _TreeFilter).  Everything else is the reference's text.

Needs the reference checkout (REFERENCE_ROOT of oracle/reference_extract.py); run from the repository root:
    python tests/golden/make_golden_box2mask_block.py
Cases: 'a' 2 images x (3 + 5) boxes, 6 queries, predictions 64x64; 'tiny' 1 image, 1 box, 2 queries, 8x8.  Each stores its inputs, the
assignment, both losses, ``mask_preds.grad`` and ``lst_feat.grad``."""
import ast
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from oracle import reference_extract as rx
from tests import b2m_loss_ref as R

HEAD_FILE = 'mmdet/models/dense_heads/box2mask_head.py'
MISC_FILE = 'mmdet/models/utils/misc.py'
LINES = (230, 233, 260, 335)                      # [230, 233] and [260, 335] of loss_single


def load_block():
    """-> block(self, mask_preds, lst_feat, norm_img, mask_weights, mask_targets, num_imgs): the statements of loss_single in LINES."""
    path = os.path.join(rx.REFERENCE_ROOT, HEAD_FILE)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    head = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Box2MaskHead')
    fn = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'loss_single')
    keep = [s for s in fn.body if LINES[0] <= s.lineno <= LINES[1] or LINES[2] <= s.lineno <= LINES[3]]
    assert keep[0].lineno == 230 and keep[-1].lineno == 335 and isinstance(keep[-1], ast.Return), [s.lineno for s in keep]
    args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ('self', 'mask_preds', 'lst_feat', 'norm_img', 'mask_weights', 'mask_targets',
                                                                        'num_imgs', 'loss_cls')],
                         kwonlyargs=[], kw_defaults=[], defaults=[])
    block = ast.FunctionDef(name='block', args=args, body=keep, decorator_list=[])
    with open(os.path.join(rx.REFERENCE_ROOT, MISC_FILE)) as fh:
        misc = ast.parse(fh.read())
    scale = next(n for n in misc.body if isinstance(n, ast.FunctionDef) and n.name == '_scale_target')
    mod = ast.Module(body=[scale, block], type_ignores=[])
    ast.fix_missing_locations(mod)
    ls = rx.load_levelset()
    env = {'torch': torch, 'F': F, 'LCM': ls.LCM}
    exec(compile(mod, path, 'exec'), env)
    stub = types.SimpleNamespace(
        loss_box=ls.BoxProjectionLoss(loss_weight=5.0), loss_mask=ls.LevelsetLoss(loss_weight=1.0),
        mst=lambda fm: torch.from_numpy(R.mst_trees(fm)),
        tree_filter=lambda feature_in, embed_in, tree, low_tree=True: R._TreeFilter.apply(feature_in, embed_in, tree.numpy(), low_tree, None))
    return env['block'], stub


def make_case(seed, counts, Q, size):
    rng = np.random.default_rng(seed)
    B, (h, w) = len(counts), size
    yy, xx = np.mgrid[:h, :w]
    img = np.stack([np.stack([np.sin(yy / (3.0 + c + b)) + np.cos(xx / (4.0 + c)) for c in range(3)]) for b in range(B)])
    img = (img + 0.3 * rng.standard_normal(img.shape)).astype(np.float32)
    lst = rng.standard_normal((B, 1, h, w)).astype(np.float32)
    preds = (2.0 * rng.standard_normal((B, Q, h, w))).astype(np.float32)
    gts, pos, pos_gt = [], [], []
    for g in counts:
        m = np.zeros((g, h, w), np.float32)
        for k in range(g):
            bh, bw = rng.integers(max(h // 4, 2), h // 2 + 1), rng.integers(max(w // 4, 2), w // 2 + 1)
            y, x = rng.integers(0, h - bh + 1), rng.integers(0, w - bw + 1)
            m[k, y:y + bh, x:x + bw] = 1
        gts.append(m)
        pos.append(np.sort(rng.choice(Q, g, replace=False)).astype(np.int64))
        pos_gt.append(rng.permutation(g).astype(np.int64))
    return dict(norm_img=img, lst_feat=lst, mask_preds=preds, gt_masks=gts, pos=pos, pos_gt=pos_gt)


def run_case(block, stub, c):
    mp = torch.from_numpy(c['mask_preds']).requires_grad_(True)
    lf = torch.from_numpy(c['lst_feat']).requires_grad_(True)
    B, Q = mp.shape[:2]
    mask_weights = torch.zeros(B, Q)
    targets = []
    for i in range(B):                            # :184-186 for the given assignment
        mask_weights[i, torch.from_numpy(c['pos'][i])] = 1.0
        targets.append(torch.from_numpy(c['gt_masks'][i]).unsqueeze(1)[torch.from_numpy(c['pos_gt'][i])])
    _, loss_project, loss_levelset = block(stub, mp, lf, torch.from_numpy(c['norm_img']), mask_weights, torch.cat(targets, 0), B, torch.zeros(()))
    (loss_project + loss_levelset).backward()
    return loss_project.detach().numpy(), loss_levelset.detach().numpy(), mp.grad.numpy(), lf.grad.numpy()


def main():
    block, stub = load_block()
    out = {'provenance': np.array('statements box2mask_head.py:230-233,260-335, LCM, LevelsetLoss, BoxProjectionLoss, _scale_target: the reference, '
                                  'by AST; mst and tree_filter: oracle/tree_filter_oracle.py (fp64) behind the module signature, NOT the '
                                  'reference modules on a stand-in _C (that binding was not built)')}
    for name, (seed, counts, Q, size) in (('a', (1, (3, 5), 6, (64, 64))), ('tiny', (2, (1,), 2, (8, 8)))):
        c = make_case(seed, counts, Q, size)
        lp, ll, gm, gl = run_case(block, stub, c)
        out.update({f'{name}_norm_img': c['norm_img'], f'{name}_lst_feat': c['lst_feat'], f'{name}_mask_preds': c['mask_preds'],
                    f'{name}_gt_masks': np.concatenate(c['gt_masks']).astype(np.uint8), f'{name}_counts': np.array(counts),
                    f'{name}_pos': np.concatenate(c['pos']), f'{name}_pos_gt': np.concatenate(c['pos_gt']),
                    f'{name}_loss_project': lp, f'{name}_loss_levelset': ll, f'{name}_grad_mask_preds': gm, f'{name}_grad_lst_feat': gl})
        print(name, float(lp), float(ll))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'box2mask_block.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
