"""Regenerate tests/golden/box_match.npz by EXECUTING the reference's own code on the CPU (developer tool; needs scipy and the
upstream checkout, BOXINST_REFERENCE_ROOT or /root/reference).  Nothing of the reference is copied: ``ClassificationCost`` and
``BoxMatchingCost`` are taken out of match_cost.py by AST with the registry decorator dropped, ``MaskHungarianAssigner.assign`` out
of mask_hungarian_assigner.py with a stand-in ``AssignResult``, and ``Box2MaskHead._get_target_single`` out of box2mask_head.py with a
stub ``self``; all are compiled in memory.  The fixture holds arrays only (masks through np.packbits).

Per image of every case (tests/box_match_ref.py: CASES) the fixture stores the inputs, the reference's fp32 cost, the same code run in
fp64, the fp64 projections, scipy's row and column indices on the fp32 cost and its total, what ``assign`` returned and what
``_get_target_single`` returned.  Per case it stores ``tol`` = max |cost32 - cost64| over its images (``ref32_vs_ref64``): the kernel's
cost has to be within 4 x tol of the fp64 cost.  The generator asserts that every optimum is separated: with each matched pair forbidden
in turn, the best other assignment costs more than the optimum by over 100 x tol -- otherwise the seed is rejected.

``lsa_*``: cost matrices for the solver alone.  ``rand``: uniform fp32 (unique optimum, separated the same way); ``ties``: small
integers, where many assignments share the optimal total and only the total is stored as the expectation.  ``lsa_limit_*``: the
1024 x 1024 matrices of tests/box_match_ref.py (limit_uniform, limit_ties) are too large to store and are rebuilt by the test; stored
are a CRC32 of the uniform matrix's bytes, scipy's column indices on it (int16) and scipy's total on the tied one.
"""
import ast
import contextlib
import os
import sys
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import box_match_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
COST_FILE = os.path.join(REF, 'mmdet/core/bbox/match_costs/match_cost.py')
ASSIGNER_FILE = os.path.join(REF, 'mmdet/core/bbox/assigners/mask_hungarian_assigner.py')
HEAD_FILE = os.path.join(REF, 'mmdet/models/dense_heads/box2mask_head.py')
CONFIG_FILE = os.path.join(REF, 'configs/box2mask/box2mask_r50_lsj_8x2_50e_coco.py')

# the first LSA_STREAM[0] / LSA_STREAM[1] matrices come from one shared stream (rand, then ties); every later one has a stream of its
# own, so that an addition never moves an earlier matrix.  (100, 120): not transposed with both sides above a wave; (65, 65), (65, 64),
# (64, 65): one past a wave in each orientation
LSA_RAND = ((67, 7), (5, 5), (3, 5), (100, 23), (64, 64), (1, 1), (1, 4), (130, 70), (100, 120), (65, 65), (65, 64), (64, 65))
LSA_TIES = ((20, 9), (6, 6), (4, 9), (64, 40), (100, 120))
LSA_STREAM = (8, 4)
SEPARATION = 100.0


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class PseudoSampler:
    """What MaskPseudoSampler.sample hands to _get_target_single: the indices of the matched and of the background queries."""

    @staticmethod
    def sample(assign_result, masks, gt_masks):
        pos = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return types.SimpleNamespace(pos_inds=pos, neg_inds=neg, pos_assigned_gt_inds=assign_result.gt_inds[pos] - 1)


@contextlib.contextmanager
def floats_are(dt):
    """``Tensor.float()`` converts to ``dt`` inside the block: bin_dice_loss calls ``gt_box_masks.float()`` (match_cost.py:389), which
    would otherwise take the fp64 run of the same text back to fp32."""
    real = torch.Tensor.float
    if dt != torch.float32:
        torch.Tensor.float = lambda self, *a, **k: self.to(dt)
    try:
        yield
    finally:
        torch.Tensor.float = real


def _from_class(path, cls_name, names, env):
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    if names is None:                                                # the whole class, without its registry decorator and bases
        node.decorator_list, node.bases = [], []
        body = [node]
    else:
        body = [s for s in node.body if isinstance(s, ast.FunctionDef) and s.name in names]
        for s in body:
            s.decorator_list = []
    m = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, 'exec'), env)
    return env


def load_reference():
    env = {'torch': torch, 'F': F}
    _from_class(COST_FILE, 'ClassificationCost', None, env)
    _from_class(COST_FILE, 'BoxMatchingCost', None, env)
    a = _from_class(ASSIGNER_FILE, 'MaskHungarianAssigner', ('assign',), {'torch': torch, 'AssignResult': AssignResult,
                                                                         'linear_sum_assignment': linear_sum_assignment})
    h = _from_class(HEAD_FILE, 'Box2MaskHead', ('_get_target_single',), {'torch': torch, 'F': F})
    return env['ClassificationCost'], env['BoxMatchingCost'], a['assign'], h['_get_target_single']


def assigner_config():
    """The ``assigner=dict(...)`` block of the reference's Box2Mask config, evaluated as a literal."""
    with open(CONFIG_FILE) as fh:
        tree = ast.parse(fh.read())
    for node in ast.walk(tree):
        if isinstance(node, ast.keyword) and node.arg == 'assigner':
            return eval(compile(ast.Expression(node.value), CONFIG_FILE, 'eval'), {'dict': dict})
    raise RuntimeError('no assigner block')


def separation(cost, rows, cols):
    """Optimum of the best assignment that differs in at least one pair, minus the optimum."""
    c = np.asarray(cost, np.float64)
    best = c[rows, cols].sum()
    gap = np.inf
    if min(c.shape) == 1 and max(c.shape) == 1:
        return gap
    big = np.abs(c).sum() + 1.0
    for r, k in zip(rows, cols):
        d = c.copy()
        d[r, k] = big
        rr, cc = linear_sum_assignment(d)
        gap = min(gap, d[rr, cc].sum() - best)
    return gap


def reference_case(name, ref=None):
    """Everything the fixture stores for one case, computed by the reference's code from the case's inputs."""
    ClsCost, BoxCost, assign, get_target_single = ref or load_reference()
    _, (h, w), (H, W), Q, counts, pset, C = R.CASES[name]
    prm = R.PARAMS[pset]
    out, tol = {}, 0.0
    images = R.make_inputs(name)
    for i, im in enumerate(images):
        k = f'{name}{i}'
        G = counts[i]
        cls_cost, dice_cost = ClsCost(weight=prm['w_cls']), BoxCost(weight=prm['w_dice'], pred_act=prm['pred_act'], eps=prm['eps'])
        assigner = types.SimpleNamespace(cls_cost=cls_cost, mask_cost=types.SimpleNamespace(weight=0.0), dice_cost=dice_cost)
        assigner.assign = types.MethodType(assign, assigner)
        logits, cls = torch.from_numpy(im['logits']), torch.from_numpy(im['cls'])
        labels, masks = torch.from_numpy(im['labels']), torch.from_numpy(im['masks'])
        costs, projs = {}, {}
        for dt in (torch.float32, torch.float64):
            up = F.interpolate(logits.to(dt).unsqueeze(1), (H, W), mode='bilinear', align_corners=False)
            act = up.sigmoid() if prm['pred_act'] else up
            projs[dt] = (act.max(dim=3)[0][:, 0], act.max(dim=2)[0][:, 0])
            with floats_are(dt):
                costs[dt] = (cls_cost(cls.to(dt), labels) + dice_cost(up, masks.unsqueeze(1))) if G else torch.zeros((Q, 0), dtype=dt)
        cost32, cost64 = costs[torch.float32].numpy(), costs[torch.float64].numpy()
        assert cost32.dtype == np.float32 and cost64.dtype == np.float64
        rows, cols = linear_sum_assignment(cost32) if G else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        total = float(cost32.astype(np.float64)[rows, cols].sum())
        if G:
            tol = max(tol, float(np.abs(cost32 - cost64).max()))
        up32 = F.interpolate(logits.unsqueeze(1), (H, W), mode='bilinear', align_corners=False)
        res = assigner.assign(cls, up32, labels, masks.unsqueeze(1), None)
        head = types.SimpleNamespace(assigner=assigner, sampler=PseudoSampler(), num_queries=Q, num_classes=C)
        tgt = get_target_single(head, cls, logits, labels, masks, None)
        out.update({f'{k}_logits': im['logits'], f'{k}_cls': im['cls'], f'{k}_labels': im['labels'],
                    f'{k}_masks': np.packbits(im['masks'].reshape(G, H * W), axis=1), f'{k}_cost32': cost32, f'{k}_cost64': cost64,
                    f'{k}_proj_rows64': projs[torch.float64][0].numpy(), f'{k}_proj_cols64': projs[torch.float64][1].numpy(),
                    f'{k}_rows': rows.astype(np.int64), f'{k}_cols': cols.astype(np.int64), f'{k}_total': np.array(total),
                    f'{k}_gt_inds': res.gt_inds.numpy(), f'{k}_assigned_labels': res.labels.numpy(),
                    f'{k}_t_labels': tgt[0].numpy(), f'{k}_t_label_weights': tgt[1].numpy(),
                    f'{k}_t_mask_targets': np.packbits(tgt[2].numpy().reshape(len(tgt[2]), H * W).astype(np.uint8), axis=1),
                    f'{k}_t_mask_weights': tgt[3].numpy(), f'{k}_t_pos_inds': tgt[4].numpy(), f'{k}_t_neg_inds': tgt[5].numpy()})
    out[f'{name}_tol'] = np.array(tol)
    return out


def main():
    ref = load_reference()
    cfg = assigner_config()
    assert cfg == dict(type='MaskHungarianAssigner', cls_cost=dict(type='ClassificationCost', weight=R.CFG['w_cls']),
                       dice_cost=dict(type='BoxMatchingCost', weight=R.CFG['w_dice'], pred_act=R.CFG['pred_act'], eps=R.CFG['eps'])), cfg
    out = {}
    for name, (_, hw, HW, Q, counts, pset, _) in R.CASES.items():
        case = reference_case(name, ref)
        tol = float(case[f'{name}_tol'])
        for i, G in enumerate(counts):
            k = f'{name}{i}'
            gap = separation(case[f'{k}_cost32'], case[f'{k}_rows'], case[f'{k}_cols']) if G else np.inf
            print(f'{k}: {hw}->{HW} Q={Q} G={G} {pset}: ref32_vs_ref64 {tol:.3e}, optimum {float(case[f"{k}_total"]):.6f}, '
                  f'next best assignment +{gap:.3e} ({gap / tol if tol else np.inf:.0f} x tol)')
            assert gap > SEPARATION * tol, 'the optimum is not separated: pick another seed'
        out.update(case)
    shared = np.random.default_rng(2024)
    for n, (Q, G) in enumerate(LSA_RAND):
        rng = shared if n < LSA_STREAM[0] else np.random.default_rng([2024, 0, n])
        c = rng.uniform(0, 10, (Q, G)).astype(np.float32)
        rows, cols = linear_sum_assignment(c)
        gap = separation(c, rows, cols)
        print(f'lsa_rand{n}: {Q}x{G} next best assignment +{gap:.3e}')
        assert gap > 1e-4
        out.update({f'lsa_rand{n}_cost': c, f'lsa_rand{n}_rows': rows.astype(np.int64), f'lsa_rand{n}_cols': cols.astype(np.int64)})
    for n, (Q, G) in enumerate(LSA_TIES):
        rng = shared if n < LSA_STREAM[1] else np.random.default_rng([2024, 1, n])
        c = rng.integers(1, 6, (Q, G)).astype(np.int8)
        rows, cols = linear_sum_assignment(c)
        print(f'lsa_ties{n}: {Q}x{G} optimal total {int(c[rows, cols].sum())}')
        out.update({f'lsa_ties{n}_cost': c, f'lsa_ties{n}_total': np.array(int(c[rows, cols].sum()))})
    side = R.LIMIT_SIDE
    c = R.limit_uniform(side, side)
    rows, cols = linear_sum_assignment(c)
    assert np.array_equal(rows, np.arange(side)) and np.array_equal(R.linear_sum_assignment(c)[1], cols), 'the restatement is not scipy here'
    out.update({'lsa_limit_crc': np.array(zlib.crc32(c.tobytes()), np.uint32), 'lsa_limit_cols': cols.astype(np.int16)})
    t = R.limit_ties()
    rows, cols = linear_sum_assignment(t)
    total = int(t[rows, cols].astype(np.int64).sum())
    rr, rc = R.linear_sum_assignment(t)
    assert int(t[rr, rc].astype(np.int64).sum()) == total
    out['lsa_limit_ties_total'] = np.array(total)
    print(f'lsa_limit: uniform {side}x{side} crc {int(out["lsa_limit_crc"]):#010x}, ties optimal total {total}')
    path = os.path.join(HERE, 'box_match.npz')
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, 'box_match_assigner_cfg.json'), 'w') as fh:      # constants only: the config block as data
        import json
        json.dump(cfg, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
