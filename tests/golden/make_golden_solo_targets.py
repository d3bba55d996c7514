"""Regenerate tests/golden/solo_targets.npz and tests/golden/solo_head_cfg.json by EXECUTING the reference's own code on the CPU
(developer tool; needs the upstream checkout, BOXINST_REFERENCE_ROOT, and scipy).  Nothing of the reference is copied:
``DiscoBoxSOLOv2Head.solov2_target_single`` and ``center_of_mass`` (discobox_head.py), ``BoxSOLOv2Head.solo_target_single``
(box_solov2_head.py), ``multi_apply``, ``py_sigmoid_focal_loss``, ``reduce_loss`` and ``weight_reduce_loss`` are taken out of their
files by AST and compiled in memory.  What stands in for the rest:
  BitmapMasks      a thin ndarray wrapper (indexing, iteration, to_ndarray);
  mmcv.imrescale   tests/solo_ref.py:rescale, the restated 2-of-4 rule.  THIS IS THE UNPINNED PART: neither OpenCV nor mmcv is
                   installed where this tool runs, so the rescaled masks of the fixture are what the rule says, not what OpenCV did;
  ndimage          scipy.ndimage (``ndimage.measurements.center_of_mass`` is scipy's own ``center_of_mass``);
  loss_cate        a closure that calls py_sigmoid_focal_loss the way FocalLoss does on the CPU (one-hot labels, reduction 'mean');
  torch.sqrt       correctly rounded in float32 (as on a device; see make_golden_box_head_loss.py).
The reference raises on an image without instances (``gt_labels_raw[0]``); such an image is recorded as all background, the library's rule.

Inputs and cases: tests/golden/solo_targets_cases.json.  Recorded per case: the exact moments and the rescaled masks at every factor;
per case and mode every target array (the GPU must equal them); ``loss_cate`` of seeded logits in float32 and float64 and the float64
gradients.  Recorded once, as the tests' tolerances (they allow 4x): ``tol_loss_cate`` / ``tol_grad_cate``, the reference's own
float32-against-float64 difference, relative (the gradient's to the largest float64 gradient), pooled over the cases and modes.

Checked before anything is written: tests/solo_ref.py reproduces every output of the reference, all equal; every moment is below 2^24
(the reference's float32 sums are exact there); the census of the case file holds (see ``census``)."""
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
from tests import solo_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEADS = dict(discobox='mmdet/models/dense_heads/discobox_head.py', boxlevelset='mmdet/models/dense_heads/box_solov2_head.py')
FILES = dict(misc='mmdet/core/utils/misc.py', focal='mmdet/models/losses/focal_loss.py', utils='mmdet/models/losses/utils.py')
SEED = 1313


def have_reference():
    return all(os.path.exists(os.path.join(REF, p)) for p in HEADS.values())


def _take(path, name, env, cls=None):
    """Compile one function (of class ``cls``) of the file into ``env``, decorators dropped."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = tree.body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    node.decorator_list = []
    m = ast.Module(body=[node], type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, 'exec'), env)
    return env[name]


class _IeeeSqrtTorch:
    """torch, with a correctly rounded float32 ``sqrt``."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def sqrt(x):
        return torch.sqrt(x.double()).float() if x.dtype == torch.float32 else torch.sqrt(x)


class BitmapMasks:
    """What the target functions use of mmdet's BitmapMasks."""

    def __init__(self, masks):
        self.masks = np.asarray(masks, np.uint8)

    def __getitem__(self, index):
        return BitmapMasks(self.masks[index].reshape(-1, *self.masks.shape[1:]))

    def __iter__(self):
        return iter(self.masks)

    def __len__(self):
        return len(self.masks)

    def to_ndarray(self):
        return self.masks


def _imrescale(img, scale):
    f = int(round(1.0 / scale))
    assert f % 2 == 0 and abs(1.0 / f - scale) < 1e-12, scale
    return R.rescale(img, f)


def load_reference(spec, mode):
    """An object that carries the reference's target function of ``mode``, ``multi_apply`` and ``loss_cate``."""
    from scipy import ndimage
    env = {'torch': _IeeeSqrtTorch(), 'np': np, 'F': F, 'mmcv': types.SimpleNamespace(imrescale=_imrescale),
           'ndimage': types.SimpleNamespace(measurements=types.SimpleNamespace(center_of_mass=ndimage.center_of_mass)),
           'partial': __import__('functools').partial, 'map': map}
    p = lambda k: os.path.join(REF, FILES[k])                                         # noqa: E731
    for key, name in (('misc', 'multi_apply'), ('utils', 'reduce_loss'), ('utils', 'weight_reduce_loss'), ('focal', 'py_sigmoid_focal_loss')):
        _take(p(key), name, env)
    head = os.path.join(REF, HEADS[mode])
    if mode == 'discobox':
        _take(head, 'center_of_mass', env)
    lc, C = spec['loss_cate'][mode], spec['num_classes']

    def loss_cate(pred, labels, avg_factor=None):
        onehot = F.one_hot(labels, num_classes=C + 1)[:, :C]
        return lc['loss_weight'] * env['py_sigmoid_focal_loss'](pred, onehot, None, gamma=lc['gamma'], alpha=lc['alpha'], reduction='mean',
                                                                 avg_factor=avg_factor)

    me = types.SimpleNamespace(num_classes=C, cate_out_channels=C, strides=list(spec['strides']), seg_num_grids=list(spec['num_grids']),
                               scale_ranges=tuple(tuple(r) for r in spec['scale_ranges']), sigma=spec['sigma'], loss_cate=loss_cate,
                               multi_apply=env['multi_apply'])
    name, cls = ('solov2_target_single', 'DiscoBoxSOLOv2Head') if mode == 'discobox' else ('solo_target_single', 'BoxSOLOv2Head')
    me.target_single = types.MethodType(_take(head, name, env, cls=cls), me)
    return me


def run_reference(spec, case, mode):
    """The reference's targets of ``case``: per (level, image) cate_label [S*S], ins_ind_label [S*S], the planes, grid_order (DiscoBox)."""
    me = load_reference(spec, mode)
    boxes, labels = R.gt_of(case)
    masks = R.masks_of(case)
    planes = R.level_planes(spec, mode)
    live = [b for b in range(len(boxes)) if boxes[b].shape[0]]
    if mode == 'discobox':
        res = me.multi_apply(me.target_single, [boxes[b] for b in live], [labels[b] for b in live], [BitmapMasks(masks[b]) for b in live],
                             mask_feat_size=tuple(spec['mask_feat_size']))
        ins, cate, ind, order = res
    else:
        sizes = [hw for _, hw in planes]
        res = me.multi_apply(me.target_single, [boxes[b] for b in live], [labels[b] for b in live], [BitmapMasks(masks[b]) for b in live],
                             [torch.zeros(3, *masks[b].shape[1:]) for b in live], [torch.zeros(1, *sizes[0]) for _ in live], featmap_sizes=sizes)
        ins, cate, ind = res[:3]
        ins = [[pl[sel] for pl, sel in zip(i, s)] for i, s in zip(ins, ind)]            # what `loss` selects (box_solov2_head.py:294-297)
        order = [[None] * len(spec['num_grids']) for _ in live]
    out = []
    for l, S in enumerate(spec['num_grids']):
        row = []
        for b in range(len(boxes)):
            if b in live:
                k = live.index(b)
                go = None if order[k][l] is None else np.asarray(order[k][l], np.int64).reshape(-1)
                row.append(dict(cate=cate[k][l].reshape(-1).numpy(), ind=ind[k][l].reshape(-1).numpy().astype(np.uint8), planes=ins[k][l].numpy(),
                                order=go))
            else:       # the library's rule for an image without instances
                row.append(dict(cate=np.full(S * S, spec['num_classes'], np.int64), ind=np.zeros(S * S, np.uint8),
                                planes=np.zeros((0, *planes[l][1]), np.uint8), order=None if mode != 'discobox' else np.zeros(0, np.int64)))
        out.append(row)
    return out


def restated(spec, case, mode):
    boxes, labels = R.gt_of(case)
    h, w = spec['mask_feat_size']
    return R.targets(mode, boxes, labels, R.masks_of(case), num_grids=spec['num_grids'], scale_ranges=spec['scale_ranges'], sigma=spec['sigma'],
                     num_classes=spec['num_classes'], canvas=(4 * h, 4 * w))


def rescaled_of(spec, case):
    """factor -> uint8 [G, h, w]: every instance's rescaled mask on the factor's plane, zeros outside the image's own part."""
    out = {}
    for mode in R.MODES:
        for f, (h, w) in R.level_planes(spec, mode):
            if f in out:
                continue
            planes = []
            for m in R.masks_of(case):
                p = np.zeros((m.shape[0], h, w), np.uint8)
                p[:, :m.shape[1] // f, :m.shape[2] // f] = R.rescale(m, f)
                planes.append(p)
            out[f] = np.concatenate(planes)
    return out


def restatement_agrees(spec, case, mode, ref, tg):
    """tests/solo_ref.py gives every output of the reference, all equal."""
    planes = R.level_planes(spec, mode)
    resc = rescaled_of(spec, case)
    at = 0
    for l, S in enumerate(spec['num_grids']):
        for b in range(spec['B']):
            r = ref[l][b]
            n = S * S
            if not (np.array_equal(tg['cate_labels'][at:at + n], r['cate']) and np.array_equal(tg['ins_ind_labels'][at:at + n], r['ind'])):
                print(f'{mode} level {l} image {b}: restated cate / ind labels differ')
                return False
            idx = tg['pair_inst'][l][b] if mode == 'discobox' else tg['sel_inst'][l][b]
            if not np.array_equal(resc[planes[l][0]][idx], r['planes']):
                print(f'{mode} level {l} image {b}: restated planes differ')
                return False
            if mode == 'discobox' and not np.array_equal(tg['grid_order'][l][b], r['order']):
                print(f'{mode} level {l} image {b}: restated grid_order differs')
                return False
            at += n
    return True


def census(spec, name, case, tgs):
    """What the case file promises is really in the fixture."""
    ok = True
    mom = np.concatenate([R.moments(m) for m in R.masks_of(case)])
    ok &= bool((mom < 2 ** 24).all())
    if name == 'mixed':
        d, bl = tgs['discobox'], tgs['boxlevelset']
        ok &= mom[1, 0] == 0 and 0 < mom[2, 0] < R.MIN_MASK_SUM
        ok &= any(2 in np.concatenate(p).tolist() for p in d['pair_inst']) and not any(2 in np.concatenate(p).tolist() for p in bl['pair_inst'])
        hit_levels = [l for l in range(len(spec['num_grids'])) if 0 in d['pair_inst'][l][0].tolist()]
        ok &= len(hit_levels) == 2                                                       # one box inside two scale ranges
        dup = any(len(set(o.tolist())) < len(o) for lv in d['grid_order'] for o in lv)   # two instances share a cell
        ok &= dup
        ok &= 6 not in d['pair_inst'][1][1].tolist() and 6 in d['pair_inst'][2][1].tolist()      # the reversed box: empty window at grid 6 only
        for f, want in ((4, (1, 2, 3)), (8, (2,)), (16, (2,))):
            sums = np.concatenate([R.sampled_sums(m, f).reshape(-1) for m in R.masks_of(case) if m.shape[0]])
            ok &= all(int((sums == s).sum()) > 0 for s in want)
    print(f'{name}: census {"holds" if ok else "FAILS"}; pairs per level (DiscoBox)', [sum(len(o) for o in lv) for lv in tgs['discobox']['grid_order']],
          'set cells (BoxLevelSet)', [sum(len(o) for o in lv) for lv in tgs['boxlevelset']['sel_inst']])
    return bool(ok)


def reference_loss(spec, mode, inputs, flat_labels, num_ins, dtype):
    me = load_reference(spec, mode)
    C = spec['num_classes']
    maps = [torch.from_numpy(m).to(dtype).requires_grad_(True) for m in inputs]
    flat = torch.cat([m.permute(0, 2, 3, 1).reshape(-1, C) for m in maps])
    n = torch.tensor(num_ins, dtype=torch.int32)                                          # flatten_ins_ind_labels.int().sum()
    loss = me.loss_cate(flat, torch.from_numpy(flat_labels), avg_factor=n + 1)
    return loss.detach(), [g.detach() for g in torch.autograd.grad(loss, maps)]


def case_arrays(spec, name, case, inputs):
    """({fixture key: array}, {tolerance: value}) of one case, or None where the restatement or the census fails."""
    out, tol, tgs = {}, {'tol_loss_cate': 0.0, 'tol_grad_cate': 0.0}, {}
    out[f'{name}_moments'] = np.concatenate([R.moments(m) for m in R.masks_of(case)])
    for f, planes in rescaled_of(spec, case).items():
        out[f'{name}_rescaled_f{f}'] = planes
    for mode in R.MODES:
        ref, tg = run_reference(spec, case, mode), restated(spec, case, mode)
        if not restatement_agrees(spec, case, mode, ref, tg):
            return None
        tgs[mode] = tg
        key = f'{name}_{mode}'
        for k in R.CELL_KEYS:
            out[f'{key}_{k}'] = tg[k]
        for k in ('grid_order', 'pair_inst', 'sel_inst'):
            out[f'{key}_{k}'] = np.concatenate([a for lv in tg[k] for a in lv]).astype(np.int64)
        out[f'{key}_pair_counts'] = np.array([[len(a) for a in lv] for lv in tg['grid_order']], np.int64)
        out[f'{key}_set_counts'] = np.array([[len(a) for a in lv] for lv in tg['sel_inst']], np.int64)
        for l in range(len(spec['num_grids'])):
            out[f'{key}_ins_labels{l}'] = np.concatenate([r['planes'] for r in ref[l]])
        out[f'{key}_num_ins'] = np.array(tg['num_ins'], np.int64)
        l32, _ = reference_loss(spec, mode, inputs, tg['cate_labels'], tg['num_ins'], torch.float32)
        l64, g64 = reference_loss(spec, mode, inputs, tg['cate_labels'], tg['num_ins'], torch.float64)
        _, g32 = reference_loss(spec, mode, inputs, tg['cate_labels'], tg['num_ins'], torch.float32)
        lc = spec['loss_cate'][mode]
        mine, mine_g = R.cate_loss(inputs, tg['cate_labels'], tg['num_ins'], lc['gamma'], lc['alpha'], lc['loss_weight'])
        if not (np.allclose(float(mine), float(l64), rtol=1e-12, atol=0) and
                all(np.allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-13 * float(b.abs().max())) for a, b in zip(mine_g, g64))):
            print(f'{key}: restated loss_cate differs')
            return None
        out[f'{key}_loss32'], out[f'{key}_loss64'] = l32.numpy(), l64.numpy()
        for l, g in enumerate(g64):
            out[f'{key}_grad_cate{l}'] = g.numpy()
        a32, a64 = torch.cat([g.reshape(-1) for g in g32]).double(), torch.cat([g.reshape(-1) for g in g64])
        tol['tol_loss_cate'] = max(tol['tol_loss_cate'], abs(float(l32) - float(l64)) / abs(float(l64)))
        tol['tol_grad_cate'] = max(tol['tol_grad_cate'], float((a32 - a64).abs().max() / a64.abs().max()))
    if not census(spec, name, case, tgs):
        return None
    return out, tol


def config_blocks():
    from boxinstseg_amd import load_config
    out = {}
    for d in ('discobox', 'boxlevelset'):
        folder = os.path.join(REF, 'configs', d)
        for f in sorted(os.listdir(folder)):
            if f.endswith('.py'):
                out[f'{d}/{f}'] = load_config(os.path.join(folder, f))['model']['bbox_head']
    return out


def main():
    spec = R.load_cases()
    inputs = R.make_cate_inputs(spec, SEED)
    out = {'seed': np.array(SEED)}
    for l, m in enumerate(inputs):
        out[f'in_cate{l}'] = m
    tols = {}
    for name, case in spec['cases'].items():
        got = case_arrays(spec, name, case, inputs)
        if got is None:
            raise SystemExit(f'case {name} rejected')
        out.update(got[0])
        for k, v in got[1].items():
            tols[k] = max(tols.get(k, 0.0), v)
    for k, v in tols.items():
        assert v > 0, k
        out[k] = np.array(v)
        print(f'{k} = {v:.3e}')
    path = os.path.join(HERE, 'solo_targets.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    with open(os.path.join(HERE, 'solo_head_cfg.json'), 'w') as fh:
        json.dump(config_blocks(), fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
