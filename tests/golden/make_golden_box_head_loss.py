"""Regenerate tests/golden/box_head_loss.npz and tests/golden/box_head_cfg.json by EXECUTING the reference's own code on the CPU
(developer tool; needs the upstream checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied:
``CondInstBoxHead.loss`` / ``get_targets`` / ``_get_target_single`` / ``centerness_target``, ``py_sigmoid_focal_loss``,
``weight_reduce_loss``, ``bbox_overlaps``, ``fp16_clamp``, ``giou_loss``, ``iou_loss``, ``distance2bbox``, ``multi_apply`` and
``MlvlPointGenerator`` are taken out of their files by AST and compiled in memory.  What stands in for the rest: ``reduce_mean`` is the
identity (one process); the three loss modules are closures that call the functions above the way FocalLoss / GIoULoss / IoULoss /
CrossEntropyLoss(use_sigmoid=True) do on the CPU (one-hot labels into py_sigmoid_focal_loss; binary_cross_entropy_with_logits into
weight_reduce_loss).  The fixture holds arrays only; box_head_cfg.json holds the ``bbox_head`` block of every configs/boxinst file as
``load_config`` reads it (settings only).

Inputs and cases: tests/golden/box_head_loss_cases.json (levels 12x20, 6x10, 3x5 at strides 8 / 16 / 32 on a 96x160 image, C = 5;
image 0 with five boxes, image 1 with two overlapping boxes of equal area).  Predictions: tests/fcos_ref.py:make_inputs(seed).

Every case runs twice, in float32 and in float64.  Recorded per case: the targets of the float32 run (the GPU must match them bit for
bit), the losses of both runs and the float64 gradients.  Recorded once, as the tests' tolerances (they allow 4x):
  tol_grad_cls / _bbox / _ctr   largest |g32 - g64| over the cases, relative to max |g64| of that case's maps of the kind
  tol_losses                    largest relative |l32 - l64| over all cases and all three losses (pooled, so that one lucky exact scalar
                                cannot make a limit zero)
  tol_stats                     largest relative |sum32 - sum64| of the centerness sum
``torch.sqrt`` of a float32 tensor is not correctly rounded in every CPU build of torch (in the build this was written with it is one
ulp off in about 0.7 % of the arguments, in every dispatch path), while on a device -- where the reference trains -- it is.  So that the
float32 run is the IEEE one, ``centerness_target`` sees a ``torch`` whose ``sqrt`` goes through float64 (the square root of a float32
number, taken in float64 and rounded once, is the correctly rounded float32 root: 53 >= 2 * 24 + 2 bits); everything else of that
namespace is torch's own.  The tool prints how many centerness targets this changes.

A seed is rejected unless every elementwise min / max / clamp operand pair of the IoU computation is separated on every positive of
every case (relative 1e-4 in float64; against an eps: half of it): ties have their own test."""
import ast
import functools
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.modules.utils import _pair

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import fcos_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD_FILE = os.path.join(REF, 'mmdet/models/dense_heads/condinst_head.py')
FILES = dict(transforms='mmdet/core/bbox/transforms.py', points='mmdet/core/anchor/point_generator.py', misc='mmdet/core/utils/misc.py',
             focal='mmdet/models/losses/focal_loss.py', utils='mmdet/models/losses/utils.py', iou_loss='mmdet/models/losses/iou_loss.py',
             overlaps='mmdet/core/bbox/iou_calculators/iou2d_calculator.py')
SEED0 = 180
MAPS = ('cls', 'bbox', 'ctr')


def have_reference():
    return os.path.exists(HEAD_FILE)


def _take(path, name, env, cls=None):
    """Compile one function (of class ``cls``) or one class of the file into ``env``, decorators dropped."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = tree.body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name)
    node.decorator_list = []
    m = ast.Module(body=[node], type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, 'exec'), env)
    return env[name]


class _IeeeSqrtTorch:
    """torch, with a correctly rounded float32 ``sqrt`` (see the module docstring)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def sqrt(x):
        return torch.sqrt(x.double()).float() if x.dtype == torch.float32 else torch.sqrt(x)


def load_reference(s):
    """An object that carries the reference's methods and the settings ``s`` (flat, from parse_box_head_cfg)."""
    p = lambda k: os.path.join(REF, FILES[k])                                         # noqa: E731
    env = {'torch': torch, 'np': np, 'F': F, 'INF': 1e8, 'partial': functools.partial, 'warnings': __import__('warnings'),
           'reduce_mean': lambda t: t, '_pair': _pair}
    for key, name in (('misc', 'multi_apply'), ('transforms', 'distance2bbox'), ('utils', 'reduce_loss'), ('utils', 'weight_reduce_loss'),
                      ('focal', 'py_sigmoid_focal_loss'), ('overlaps', 'fp16_clamp'), ('overlaps', 'bbox_overlaps'), ('iou_loss', 'giou_loss'),
                      ('iou_loss', 'iou_loss'), ('points', 'MlvlPointGenerator')):
        _take(p(key), name, env)
    C = s['num_classes']

    def loss_cls(pred, labels, avg_factor=None):
        onehot = F.one_hot(labels, num_classes=C + 1)[:, :C]
        return s['loss_weight_cls'] * env['py_sigmoid_focal_loss'](pred, onehot, None, gamma=s['gamma'], alpha=s['alpha'], reduction='mean',
                                                                    avg_factor=avg_factor)

    def loss_bbox(pred, target, weight=None, avg_factor=None):
        if s['bbox_loss_kind'] == 'giou':
            el = env['giou_loss'](pred, target, eps=s['eps'])
        else:
            el = env['iou_loss'](pred, target, mode=s['bbox_loss_kind'][4:], eps=s['eps'])
        return s['loss_weight_bbox'] * env['weight_reduce_loss'](el, weight, 'mean', avg_factor)

    def loss_centerness(pred, target, avg_factor=None):
        el = F.binary_cross_entropy_with_logits(pred, target, reduction='none')
        return s['loss_weight_centerness'] * env['weight_reduce_loss'](el, None, 'mean', avg_factor)

    me = types.SimpleNamespace(num_classes=C, cls_out_channels=C, strides=list(s['strides']), regress_ranges=tuple(s['regress_ranges']),
                               center_sampling=s['center_sampling'], center_sample_radius=s['center_sample_radius'],
                               norm_on_bbox=s['norm_on_bbox'], loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness,
                               prior_generator=env['MlvlPointGenerator'](list(s['strides'])))
    for name in ('loss', 'get_targets', '_get_target_single', 'centerness_target'):
        setattr(me, name, types.MethodType(_take(HEAD_FILE, name, dict(env, torch=_IeeeSqrtTorch()), cls='CondInstBoxHead'), me))
    return me


def settings_of(spec, name):
    from boxinstseg_amd.box_head_loss import parse_box_head_cfg
    return parse_box_head_cfg(R.head_cfg(spec, name))


def run_reference(spec, inp, name, dtype):
    """The reference's loss (and get_targets) on case ``name`` in ``dtype``."""
    s = settings_of(spec, name)
    me = load_reference(s)
    maps = {k: [torch.from_numpy(m).to(dtype).requires_grad_(True) for m in inp[k]] for k in MAPS}
    boxes, labels = R.gt_of(spec, dtype)
    losses, points, level_inds, img_inds, gt_inds = me.loss(maps['cls'], maps['bbox'], maps['ctr'], boxes, labels, None)
    total = losses['loss_cls'] + losses['loss_bbox'] + losses['loss_centerness']           # each loss reaches its own maps only
    grads = torch.autograd.grad(total, maps['cls'] + maps['bbox'] + maps['ctr'])
    n = len(inp['cls'])
    pts = me.prior_generator.grid_priors([m.shape[-2:] for m in maps['cls']], dtype, 'cpu')
    lab, tgt, _ = me.get_targets(pts, boxes, labels)
    lab, tgt = torch.cat(lab), torch.cat(tgt)
    pos = (gt_inds >= 0).nonzero().reshape(-1)
    ct = torch.zeros(lab.shape[0], dtype=dtype)
    ct[pos] = me.centerness_target(tgt[pos])
    return dict(labels=lab, bbox_targets=tgt, gt_inds=gt_inds, points=points, level_inds=level_inds, img_inds=img_inds, ctr_targets=ct,
                losses=torch.stack([losses['loss_cls'], losses['loss_bbox'], losses['loss_centerness']]).detach(),
                grads={k: [g for g in grads[i * n:(i + 1) * n]] for i, k in enumerate(MAPS)})


def reference_case(spec, inp, name):
    """name -> ({fixture key: array}, {tolerance name: value of this case}) from two runs of the reference."""
    r32, r64 = run_reference(spec, inp, name, torch.float32), run_reference(spec, inp, name, torch.float64)
    for k in ('labels', 'gt_inds', 'level_inds', 'img_inds'):
        assert torch.equal(r32[k], r64[k]), (name, k)
    assert torch.equal(r32['points'].double(), r64['points']), name
    out = {f'{name}_{k}': r32[k].numpy() for k in ('labels', 'gt_inds', 'level_inds', 'img_inds', 'points', 'bbox_targets', 'ctr_targets')}
    s32, s64 = float(r32['ctr_targets'].sum()), float(r64['ctr_targets'].sum())
    out[f'{name}_stats64'] = np.array([float((r64['gt_inds'] >= 0).sum()), s64])
    out[f'{name}_losses32'], out[f'{name}_losses64'] = r32['losses'].numpy(), r64['losses'].numpy()
    tol = {'tol_stats': abs(s32 - s64) / s64,
           'tol_losses': float(((r32['losses'].double() - r64['losses']).abs() / r64['losses'].abs()).max())}
    for k in MAPS:
        g32, g64 = torch.cat([g.reshape(-1) for g in r32['grads'][k]]).double(), torch.cat([g.reshape(-1) for g in r64['grads'][k]])
        tol[f'tol_grad_{k}'] = float((g32 - g64).abs().max() / g64.abs().max())
        for lv, g in enumerate(r64['grads'][k]):
            out[f'{name}_grad_{k}{lv}'] = g.numpy()
    return out, tol


def tie_margin(spec, inp, name):
    """Smallest separation (1 = the required one) of the operand pairs of every min / max / clamp in the IoU computation, float64."""
    s = settings_of(spec, name)
    boxes, labels = R.gt_of(spec, torch.float64)
    tg = R.targets(spec['levels'], s['strides'], boxes, labels, s['regress_ranges'], s['center_sampling'], s['center_sample_radius'],
                   s['norm_on_bbox'], s['num_classes'], torch.float64)
    pos = tg['gt_inds'] >= 0
    pts = tg['points'][pos]
    a = R.decode(pts, R.flatten_maps([torch.from_numpy(m).double() for m in inp['bbox']])[pos])
    b = R.decode(pts, tg['bbox_targets'][pos])
    rel = lambda x, y: ((x - y).abs() / (1e-4 * torch.maximum(torch.maximum(x.abs(), y.abs()), torch.ones_like(x)))).min()   # noqa: E731
    vs_eps = lambda x, e: ((x - e).abs() / (0.5 * e)).min()                                                                   # noqa: E731
    zero = torch.zeros(a.shape[0], dtype=torch.float64)
    m = [rel(a[:, k], b[:, k]) for k in range(4)]
    wh = torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])
    ewh = torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])
    m += [rel(wh[:, 0], zero), rel(wh[:, 1], zero), rel(ewh[:, 0], zero), rel(ewh[:, 1], zero)]
    whc, ewhc = wh.clamp(min=0), ewh.clamp(min=0)
    overlap = whc[:, 0] * whc[:, 1]
    union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - overlap
    eps_u = s['eps'] if s['bbox_loss_kind'] == 'giou' else 1e-6
    m.append(vs_eps(union, eps_u))
    if s['bbox_loss_kind'] == 'giou':
        m.append(vs_eps(ewhc[:, 0] * ewhc[:, 1], s['eps']))
    else:
        m.append(vs_eps(overlap / union.clamp(min=eps_u), s['eps']))
    return float(torch.stack(m).min())


def restatement_agrees(spec, inp, name, case):
    """tests/fcos_ref.py gives the reference's targets bit for bit in float32 and its losses and gradients in float64."""
    s = settings_of(spec, name)
    boxes, labels = R.gt_of(spec, torch.float32)
    tg = R.targets(spec['levels'], s['strides'], boxes, labels, s['regress_ranges'], s['center_sampling'], s['center_sample_radius'],
                   s['norm_on_bbox'], s['num_classes'], torch.float32)
    for k in R.TARGET_KEYS:
        if not np.array_equal(tg[k].numpy(), case[f'{name}_{k}']):
            print(f'{name}: restated {k} differ')
            return False
    boxes64, _ = R.gt_of(spec, torch.float64)
    tg64 = R.targets(spec['levels'], s['strides'], boxes64, labels, s['regress_ranges'], s['center_sampling'], s['center_sample_radius'],
                     s['norm_on_bbox'], s['num_classes'], torch.float64)
    got = R.losses_and_grads(inp, tg64, s, torch.float64)
    if not np.allclose(got[0].numpy(), case[f'{name}_losses64'], rtol=1e-12, atol=0):
        print(f'{name}: restated losses differ', got[0].numpy(), case[f'{name}_losses64'])
        return False
    for k, grads in zip(MAPS, got[1:]):
        for lv, g in enumerate(grads):
            want = case[f'{name}_grad_{k}{lv}']
            if not np.allclose(g.numpy(), want, rtol=1e-10, atol=1e-13 * np.abs(want).max()):
                print(f'{name}: restated grad_{k}{lv} differ by', np.abs(g.numpy() - want).max())
                return False
    return True


def census_ok(spec, case):
    """The positives the case file promises: per level for image 0, and image 1's all on its first box."""
    sizes = [h * w for h, w in spec['levels']]
    B = len(spec['gt_bboxes'])
    for name, c in spec['cases'].items():
        gi = case[name][f'{name}_gt_inds']
        at, counts = 0, []
        for n in sizes:
            counts.append(int((gi[at:at + n] >= 0).sum()))
            img1 = gi[at + n:at + 2 * n]
            if not set(img1[img1 >= 0].tolist()) <= {len(spec['gt_bboxes'][0])}:
                return False
            at += B * n
        want = spec['positives_image0']['center_sampling' if c['center_sampling'] else 'inside_box']
        n1 = int((case[name][f'{name}_img_inds'][gi >= 0] == 1).sum())
        print(f'{name}: positives of image 0 per level {counts}, of image 1 {n1}')
        if counts != want or n1 != spec['positives_image1']:
            return False
    return True


def config_blocks():
    from boxinstseg_amd import load_config
    d = os.path.join(REF, 'configs', 'boxinst')
    return {f: load_config(os.path.join(d, f))['model']['bbox_head'] for f in sorted(os.listdir(d)) if f.endswith('.py')}


def main():
    spec = R.load_cases()
    for seed in range(SEED0, SEED0 + 200):
        inp = R.make_inputs(spec, seed)
        margin = min(tie_margin(spec, inp, name) for name in spec['cases'])
        if margin <= 1.0:
            print(f'seed {seed} rejected: tie margin {margin:.2e}')
            continue
        cases, tols = {}, {}
        for name in spec['cases']:
            cases[name], t = reference_case(spec, inp, name)
            for k, v in t.items():
                tols[k] = max(tols.get(k, 0.0), v)
        if all(v > 0 for v in tols.values()) and census_ok(spec, cases) and all(restatement_agrees(spec, inp, n, cases[n]) for n in cases):
            break
        print(f'seed {seed} rejected')
    else:
        raise SystemExit('no seed passed')
    out = {'seed': np.array(seed)}
    for k, maps in inp.items():
        for lv, m in enumerate(maps):
            out[f'in_{k}{lv}'] = m
    for case in cases.values():
        out.update(case)
    for k, v in tols.items():
        out[k] = np.array(v)
        print(f'{k} = {v:.3e}')
    for name, case in cases.items():
        ct, t = torch.from_numpy(case[f'{name}_ctr_targets']), torch.from_numpy(case[f'{name}_bbox_targets'])
        pos = ct > 0
        plain = torch.sqrt((t[pos][:, [0, 2]].min(-1)[0] / t[pos][:, [0, 2]].max(-1)[0]) * (t[pos][:, [1, 3]].min(-1)[0] / t[pos][:, [1, 3]].max(-1)[0]))
        print(f'{name}: {int((plain != ct[pos]).sum())} of {int(pos.sum())} centerness targets differ from this build\'s float32 torch.sqrt')
    zeros = sum(int((m == 0).sum()) for m in inp['bbox'])
    print(f'seed {seed}: tie margin {margin:.2e}, exact zeros among the distances: {zeros}')
    assert zeros > 0
    path = os.path.join(HERE, 'box_head_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    with open(os.path.join(HERE, 'box_head_cfg.json'), 'w') as fh:
        json.dump(config_blocks(), fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
