"""Regenerate tests/golden/roi_front.npz and roi_front_cases.json (developer tool; needs the upstream checkout, BOXINST_REFERENCE_ROOT).

The level case EXECUTES the reference's own statements on the CPU; nothing of the reference is copied.  The front of one level of
``DiscoBoxSOLOv2Head.corr_loss`` (discobox_head.py:1018-1057: from ``s_input = torch.sigmoid(s_input)`` to the ``queue_area_mask`` assignment)
and ``relu_and_l2_norm_feat`` are taken out of the file by AST and compiled in memory; the object loop behind it (:1056-1127) is the one
tests/golden/make_golden_corr.py extracts the same way.  What stands in for the rest: ``self.feat_roi_align`` and ``self.mask_roi_align`` are
tests/roi_ref.roi_align at 7 x 7 and 28 x 28 -- mmcv's op is not in the reference tree and never ran here, its arithmetic is restated and
unpinned; ``use_ind_teacher`` is False, so ``t_input is s_input``; ``save_corr_img`` is False.  The run happens in float64 (stored) and in
float32.

The fixture holds the inputs (floats rounded to float16, so exact in every format), the fp64 results, and for every toleranced quantity
``tol_<name>`` = 4 x the largest difference of the fp32 run against the fp64 run, relative to the largest fp64 magnitude of the quantity.
The op-level cases of tests/roi_ref.py (op_cases, mask_cases, fused_cases) have no reference statements to execute: their expectations are
computed by the tests from the restatement in fp64, and only their tolerances are measured here, the same way.

Checked before anything is written, else the case is refused: the fp32 and fp64 runs agree on everything exact; tests/roi_ref.py reproduces
the fp64 run; the margins of make_golden_corr.conditions hold for the kept objects; exactly the objects of ``census`` run."""
import ast
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import corr_ref as CR  # noqa: E402
from tests import roi_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/discobox_head.py'
FACTOR = 4.0

CASE = dict(C=8, L=8, num_class=3, B=2, hw=[24, 40], min_size=8, seed=51, ptr=[5, 5, 0],
            what='six objects over two images, object 2 with an all-zero target (dropped: the later objects read an earlier label), object 5 a single '
                 'pixel in the bottom-right corner; class 0 holds five entries that look like object 0, class 1 five that look like object 4, which '
                 'reads label 1 only through the shift (its own is 2): objects 0 and 4 run; the others share class 2, empty before the call',
            boxes=[[4, 3, 18, 17], [22, 2, 38, 12], None, [1, 4, 13, 22], [20, 6, 34, 20], [39, 23, 40, 24]],
            img_inds=[0, 0, 1, 1, 1, 0], kernel_labels=[0, 2, 2, 1, 2, 0], alike=[[0, 0], [4, 1]],
            census=dict(keep=[1, 1, 0, 1, 1, 1], labels=[0, 2, -1, 2, 1, 2], count=[5, 0, 0, 0, 5, 0], ran=[0, 4], ptr=[6, 6, 2]))


def _corr_generator():
    spec = importlib.util.spec_from_file_location('make_golden_corr', os.path.join(HERE, 'make_golden_corr.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def have_reference():
    return os.path.exists(os.path.join(REF, HEAD))


def build_inputs(case=CASE):
    """The arrays of the level case (every float exact in float16).  The two objects that run have 14 x 14 boxes and logits of 8 and -4 (not symmetric: sigmoid(8) + sigmoid(-8) is the 1 that a count of the loop thresholds at): their
    28 x 28 samples fall on quarter positions, so the pooled mask takes few values, none of them near a threshold of the loop."""
    rng = np.random.RandomState(case['seed'])
    (H, W), C, B, N = case['hw'], case['C'], case['B'], len(case['boxes'])
    target, s_input = np.zeros((N, H, W), np.uint8), np.zeros((N, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, b in enumerate(case['boxes']):
        if b is None:
            s_input[i] = R.half(-4 + rng.standard_normal((H, W)))
            continue
        x1, y1, x2, y2 = b
        target[i, y1:y2, x1:x2] = 1
        if (y2 - y1) > 2 and (x2 - x1) > 2:
            target[i, y1 + 1, x1 + 1] = 0                                    # a hole: the box is that of the non-zero pixels
        cy, cx, ry, rx = (y1 + y2 - 1) / 2, (x1 + x2 - 1) / 2, max((y2 - y1) * 0.42, 0.6), max((x2 - x1) * 0.42, 0.6)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        noise = 0.0 if any(i == a for a, _ in case['alike']) else 0.5
        s_input[i] = R.half(np.where(inside, 8.0, -4.0) + noise * rng.standard_normal((H, W)))
    s_feat = R.half(rng.standard_normal((B, C, H, W)))
    t_feat = R.half(s_feat + 0.1 * rng.standard_normal((B, C, H, W)))
    inp = dict(s_input=s_input, target=target, img_inds=np.asarray(case['img_inds'], np.int64), kernel_labels=np.asarray(case['kernel_labels'], np.int64),
               s_feat=s_feat, t_feat=t_feat)
    # the bank: five entries per class made from what the front gives the object they are to look like
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    si = t['s_input'].double()
    f = R.front(si, si, t['target'], t['img_inds'], t['kernel_labels'], t['s_feat'].double(), t['t_feat'].double())
    L, nc = case['L'], case['num_class']
    bank = dict(bank_feature=np.zeros((nc, L, C, 7, 7), np.float32), bank_mask=np.zeros((nc, L, 28, 28), np.float32),
                bank_box=np.zeros((nc, L, 4), np.float32), bank_ptr=np.asarray(case['ptr'], np.int32))
    for obj, cls in case['alike']:
        for s in range(5):
            feat = np.maximum(f['roi_t_feat'][obj].numpy() + 0.03 * rng.standard_normal((C, 7, 7)), 0.0)
            bank['bank_feature'][cls, s] = R.half(feat / (np.sqrt((feat ** 2).sum(0, keepdims=True) + 1e-6) + 1e-6))
            bank['bank_mask'][cls, s] = R.half(CR.snap(f['roi_s_mask'][obj].numpy()))
            bank['bank_box'][cls, s] = f['boxes'][obj].numpy()
    inp.update(bank)
    return inp


# ---- the reference, by AST ---------------------------------------------------------------------------------------------------------------
def load_front():
    """``front(self, s_input, t_input, img_inds, target, kernel_labels, s_feat, t_feat, use_ind_teacher)``: the statements :1018-1057, returning
    their local variables (None where the reference ``continue``s: no non-zero target)."""
    path = os.path.join(REF, HEAD)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    relu = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'relu_and_l2_norm_feat')
    head = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DiscoBoxSOLOv2Head')
    closs = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'corr_loss')
    outer = next(n for n in closs.body if isinstance(n, ast.For) and any(isinstance(m, ast.Name) and m.id == 'queue_area_mask' for m in ast.walk(n)))
    names = lambda n: {m.id for m in ast.walk(n) if isinstance(m, ast.Name)}                # noqa: E731
    first = next(i for i, n in enumerate(outer.body) if isinstance(n, ast.Assign) and 'sigmoid' in {m.attr for m in ast.walk(n) if isinstance(m, ast.Attribute)})
    last = next(i for i, n in enumerate(outer.body) if isinstance(n, ast.With) and 'queue_area_mask' in names(n))
    shell = ast.parse('def front(self, s_input, t_input, img_inds, target, kernel_labels, s_feat, t_feat, use_ind_teacher, img=None):\n'
                      '    for _once in (0,):\n        pass\n        return dict(locals())\n    return None\n').body[0]
    loop = shell.body[0]
    loop.body = list(outer.body[first:last + 1]) + [loop.body[1]]
    m = ast.Module(body=[relu, shell], type_ignores=[])
    ast.fix_missing_locations(m)
    env = {'torch': torch, 'nn': nn, 'F': F, 'np': np}
    exec(compile(m, path, 'exec'), env)
    return env


def run_front(env, inp, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
        s_feat = t['s_feat'].to(dtype).requires_grad_(True)
        me = types.SimpleNamespace(feat_roi_align=lambda x, rois: R.roi_align(x, rois, R.FEAT), mask_roi_align=lambda x, rois: R.roi_align(x, rois, R.MASK),
                                   save_corr_img=False, objbank_min_size=CASE['min_size'])
        s_input = t['s_input'].to(dtype)
        loc = env['front'](me, s_input, s_input, t['img_inds'], t['target'], t['kernel_labels'], s_feat, t['t_feat'].to(dtype), False)
        return loc, s_feat
    finally:
        torch.set_default_dtype(old)


def run_level(env, gen, cenv, inp, dtype, case=CASE):
    """The reference's front, then its object loop (make_golden_corr.run_reference) on what the front gave; everything in full-N form."""
    loc, s_feat = run_front(env, inp, dtype)
    keep = loc['mask'].numpy()
    N, (H, W), K = keep.shape[0], case['hw'], gen.CFG['max_retrieval_objs']
    arrays = dict(s_feat=loc['roi_s_feat'].detach().numpy(), s_mask=loc['roi_s_mask'].numpy(), t_feat=loc['roi_t_feat'].numpy(), t_mask=loc['roi_t_mask'].numpy(),
                  boxes=loc['boxes'].numpy(), labels=inp['kernel_labels'], bank_feature=inp['bank_feature'].astype(arrays_dtype(dtype)),
                  bank_mask=inp['bank_mask'].astype(arrays_dtype(dtype)), bank_box=inp['bank_box'].astype(arrays_dtype(dtype)), bank_ptr=inp['bank_ptr'])
    ccase = dict(C=case['C'], L=case['L'], num_class=case['num_class'], min_size=case['min_size'], out_hw=case['hw'],
                 bank=[dict(cls=c) for _, c in case['alike']])
    rec = gen.run_reference(cenv, ccase, arrays, dtype)
    g_roi = torch.from_numpy(rec['grad']).to(dtype)
    g_level = torch.autograd.grad(loc['roi_s_feat'], s_feat, grad_outputs=g_roi)[0] if int(rec['num_ins']) else torch.zeros_like(s_feat)

    def full(a, fill=0):
        out = np.full((N,) + a.shape[1:], fill, a.dtype)
        out[keep] = a
        return out

    labels = np.full(N, -1, np.int64)
    labels[keep] = inp['kernel_labels'][:int(keep.sum())]
    assert np.array_equal(loc['queue_area_mask'].numpy(), ((loc['boxes'][:, 2] - loc['boxes'][:, 0] > case['min_size']) &
                                                           (loc['boxes'][:, 3] - loc['boxes'][:, 1] > case['min_size'])).numpy())
    return dict(keep=keep.astype(np.uint8), labels=labels, boxes=full(loc['boxes'].double().numpy()), roi_s_feat=full(loc['roi_s_feat'].detach().double().numpy()),
                roi_t_feat=full(loc['roi_t_feat'].double().numpy()), roi_s_mask=full(loc['roi_s_mask'].double().numpy()),
                loss_sum=rec['loss_sum'], num_ins=rec['num_ins'], iiu=full(rec['iiu']), g_level=g_level.double().numpy(), count=full(rec['count']),
                ret_slot=full(rec['ret_slot'], -1), assign=full(rec['assign'], -1), after_feature=rec['after_feature'], after_mask=rec['after_mask'],
                after_box=rec['after_box'], after_ptr=rec['after_ptr'], _arrays=arrays, _rec=rec)


def arrays_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


EXACT = ('keep', 'labels', 'boxes', 'num_ins', 'count', 'ret_slot', 'assign', 'after_ptr')
LEVEL_TOL = ('roi_s_feat', 'roi_s_mask', 'loss_sum', 'iiu', 'g_level')


def rel(a32, a64):
    a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
    top = np.abs(a64).max() if a64.size else 0.0
    return float(np.abs(a32 - a64).max() / top) if top > 0 else 0.0


def level_arrays(env, gen, cenv):
    """({fixture key: array}, {tolerance name: fp32-against-fp64 difference}) of the level case; SystemExit where a check fails."""
    inp = build_inputs()
    r32, r64 = run_level(env, gen, cenv, inp, torch.float32), run_level(env, gen, cenv, inp, torch.float64)
    for k in EXACT:
        if not np.array_equal(r32[k], r64[k]):
            raise SystemExit(f'the fp32 and fp64 runs of the reference differ in {k}')
    for k in ('after_feature', 'after_mask', 'after_box'):
        if not np.allclose(r32[k], r64[k], rtol=0, atol=1e-4):          # the appended entries are the toleranced roi tensors
            raise SystemExit(f'the fp32 and fp64 runs of the reference differ in {k}')
    cs = CASE['census']
    ran = [i for i in range(len(CASE['boxes'])) if r64['count'][i] >= gen.CFG['min_objs']]
    if (r64['keep'].tolist(), r64['labels'].tolist(), r64['count'].tolist(), ran, r64['after_ptr'].tolist(), int(r64['num_ins'])) != \
            (cs['keep'], cs['labels'], cs['count'], cs['ran'], cs['ptr'], len(cs['ran'])):
        raise SystemExit(f"the census fails: keep {r64['keep'].tolist()} labels {r64['labels'].tolist()} count {r64['count'].tolist()} ran {ran} ptr {r64['after_ptr'].tolist()}")
    ccase = dict(min_size=CASE['min_size'], L=CASE['L'])
    kept = {k: np.asarray(v) for k, v in r64['_arrays'].items()}
    kept['labels'] = kept['labels'][:int(r64['keep'].sum())]
    if not gen.conditions(ccase, kept, r64['_rec']):
        raise SystemExit(f'a value of the loop is within {gen.MARGIN} of a discontinuity')
    mine, grad = restated(inp)
    same = all(np.array_equal(np.asarray(mine[k]), r64[k]) for k in ('labels', 'count', 'ret_slot')) and np.array_equal(mine['keep'].numpy(), r64['keep'].astype(bool))
    same &= mine['num_ins'] == int(r64['num_ins']) and np.array_equal(mine['boxes'].numpy(), r64['boxes'])
    same &= all(np.allclose(np.asarray(a), b, rtol=1e-9, atol=1e-12) for a, b in (
        (mine['roi_s_feat'].detach().numpy(), r64['roi_s_feat']), (mine['roi_t_feat'].numpy(), r64['roi_t_feat']), (mine['roi_s_mask'].numpy(), r64['roi_s_mask']),
        (mine['iiu'].numpy(), r64['iiu']), (float(mine['loss_sum']), float(r64['loss_sum'])), (grad.numpy(), r64['g_level'])))
    if not same:
        raise SystemExit('tests/roi_ref.py does not reproduce the reference')
    out = {k: (v.astype(np.float16) if v.dtype == np.float32 else v) for k, v in inp.items()}
    for k, v in inp.items():
        assert v.dtype != np.float32 or np.array_equal(out[k].astype(np.float32), v), k
    for k in EXACT + LEVEL_TOL + ('roi_t_feat',):
        out[f'level_{k}'] = np.asarray(r64[k])
    for k in ('after_feature', 'after_mask', 'after_box'):
        out[f'level_{k}'] = r64[k]                          # the bank of the fp64 run
    return out, {k: rel(r32[k], r64[k]) for k in LEVEL_TOL}


def restated(inp):
    t, bank = R.inputs_of({k: v for k, v in inp.items()}, dtype=torch.float64)
    t['s_feat'].requires_grad_(True)
    gen_cfg = dict(_corr_cfg(), min_size=CASE['min_size'])
    out = R.corr_level(t, bank, gen_cfg)
    grad = torch.autograd.grad(out['loss_sum'], t['s_feat'])[0] if out['num_ins'] else torch.zeros_like(t['s_feat'])
    return out, grad


def _corr_cfg():
    return CR.load_cases()['cfg']


def op_tolerances():
    """fp32 against fp64 of the restatement on the op-level cases: forward and gradient of the op, the mask path, the fused feature path."""
    tol = dict(fwd=0.0, bwd=0.0, mask=0.0, fused_fwd=0.0, fused_bwd=0.0)

    def both(fn, feat):
        res = []
        for dt in (torch.float32, torch.float64):
            x = feat.to(dt).requires_grad_(True)
            y = fn(x, dt)
            g = torch.sin(torch.arange(y.numel(), dtype=torch.float64)).view(y.shape).to(dt)
            res.append((y.detach().numpy(), torch.autograd.grad((y * g).sum(), x)[0].numpy()))
        return rel(res[0][0], res[1][0]), rel(res[0][1], res[1][1])

    for c in R.op_cases().values():
        f, b = both(lambda x, dt: R.roi_align(x, c['rois'].to(dt), c['size'], **c['kw']), c['feat'])
        tol['fwd'], tol['bwd'] = max(tol['fwd'], f), max(tol['bwd'], b)
    for c in R.mask_cases().values():
        N = c['logits'].shape[0]
        f, _ = both(lambda x, dt: R.roi_align(torch.sigmoid(x).unsqueeze(1), torch.cat([torch.arange(N).to(dt).view(N, 1), c['boxes'].to(dt)], 1), R.MASK), c['logits'])
        tol['mask'] = max(tol['mask'], f)
    for c in R.fused_cases().values():
        f, b = both(lambda x, dt: R.relu_and_l2_norm_feat(R.roi_align(x, c['rois'].to(dt), R.FEAT)), c['feat'])
        tol['fused_fwd'], tol['fused_bwd'] = max(tol['fused_fwd'], f), max(tol['fused_bwd'], b)
    return tol


def main():
    gen = _corr_generator()
    out, tol = level_arrays(load_front(), gen, gen.load_reference())
    tol.update(op_tolerances())
    for k, v in tol.items():
        assert v > 0, k
        out[f'tol_{k}'] = np.array(FACTOR * v)
        print(f'tol_{k} = {FACTOR} x {v:.3e}')
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), 'bytes')
    assert os.path.getsize(R.GOLDEN) < (1 << 20)
    with open(R.CASES, 'w') as fh:
        json.dump(dict(cfg=dict(_corr_cfg(), min_size=CASE['min_size']), factor=FACTOR, case=CASE), fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
