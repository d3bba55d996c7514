"""Regenerate tests/golden/corr.npz, corr_planes_<case>.npz, corr_cases.json and corr_cfg.json by EXECUTING the reference's own code on
the CPU (developer tool; needs the upstream checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied:
``relu_and_l2_norm_feat``, ``ObjectFactory``, ``ObjectElements``, ``ObjectQueues``, ``SemanticCorrSolver``, ``DiscoBoxSOLOv2Head.superres_T``
and the statements of the object loop of ``DiscoBoxSOLOv2Head.corr_loss`` (discobox_head.py:1056-1127: the ``queue_area_mask`` assignment and
the ``for idx in torch.arange(len(queue_area_mask))`` loop) are taken out of the file by AST and compiled in memory.  What stands in for the
rest: ``autocast`` is a null context; ``self`` is a namespace with the attributes the loop reads; ``self.qobj`` exists before the first
object, so the double relu_and_l2_norm_feat of the very first query of a run (ObjectFactory.create_one :40) does not happen -- the library
does not reproduce it.  The fp64 run is the same code with float64 inputs, float64 as the default dtype and ``Tensor.float`` redirected to
``Tensor.double``.

Per case (corr_cases.json says what each is made of) the fixture holds the inputs, rounded to float16 so that they are exact in every
format, and from the reference: the retrieved slots and counts, the assignments, num_ins, the bank and ptr afterwards (all exact); fp64
loss_sum, its gradient w.r.t. roi_s_feat and iiu in corr.npz, fp64 Cu and C in corr_planes_<case>.npz.  ``tol_*``: the reference's own
fp32-against-fp64 difference, relative to the largest fp64 magnitude of the quantity, the maximum over the cases; the tests allow 4x.

Checked in fp64 before anything is written (a discontinuity must not hide a failure), else the case is refused: every finite fg / bg /
appearance / ratio score at least 1e-3 (relative) away from its threshold; every A + B and 2 - A - B of a non-empty slot at least 1e-3 from
1; every m0 m1 and (1 - m0)(1 - m1) of a retrieved pair at least 1e-3 from 0.5; every row of C with a relative top-1 / top-2 gap of at
least 1e-3; fp32 and fp64 runs agree on everything exact; tests/corr_ref.py reproduces the fp64 run; the census of each case holds."""
import ast
import contextlib
import copy
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
from tests import corr_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/discobox_head.py'
CFG = dict(fg_iou_thresh=0.7, bg_iou_thresh=0.7, appear_thresh=0.7, ratio_range=[0.9, 1.2], max_retrieval_objs=5, min_objs=5, dist_kernel=9,
           corr_num_iter=10, corr_num_smooth_iter=1, corr_exp=1.0, corr_eps=0.05, gaussian_filter_size=3, low_score=0.3)
MARGIN = 1e-3
LEVELS = R.LEVELS                 # what the masks are snapped to, and why: tests/corr_ref.py

# kinds of entries: (mask radius, background floor, feature base, box)
SQ, WIDE, THIN = [8, 6, 28, 26], [4, 10, 34, 25], [10, 5, 30, 6]
KINDS = {'good': dict(), 'good_wide': dict(box=[6, 6, 28, 26]), 'small': dict(radius=5.0), 'softbg': dict(floor=0.44), 'otherfeat': dict(base=1),
         'ratio': dict(box=WIDE), 'thin': dict(box=THIN)}


def _e(kind, cls, slot=None, box=None, **kw):
    d = dict(kind=kind, cls=cls, **kw)
    if slot is not None:
        d['slot'] = slot
    if box is not None:
        d['box'] = box
    return d


SPEC = {
    'plain': dict(C=32, L=12, num_class=2, out_hw=[40, 56], min_size=8, seed=11, ptr=[6, 3],
                  what='six objects of two classes; class 0 holds five good entries, class 1 three: the three good objects of class 0 retrieve exactly five',
                  bank=[_e('good', 0, s) for s in range(5)] + [_e('good_wide', 1, s) for s in range(3)],
                  objects=[_e('good', 0), _e('good', 1), _e('good', 0, box=[30, 10, 52, 30]), _e('good', 0), _e('good', 1), _e('otherfeat', 0)],
                  census=dict(count=[5, 3, 5, 5, 4, 0], ran=[0, 2, 3])),
    'one_fails_each': dict(C=32, L=12, num_class=2, out_hw=[40, 56], min_size=8, seed=12, ptr=[11, 0],
                           what='slots that fail exactly one predicate each (1 fg, 3 bg, 5 appearance, 7 ratio), seven good ones (two beyond the fifth), a never-used class',
                           bank=[_e('good', 0, 0), _e('small', 0, 1), _e('good', 0, 2), _e('softbg', 0, 3), _e('good', 0, 4), _e('otherfeat', 0, 5),
                                 _e('good', 0, 6), _e('ratio', 0, 7), _e('good', 0, 8), _e('good', 0, 9), _e('good', 0, 10)],
                           objects=[_e('good', 0), _e('good', 1)],
                           census=dict(count=[5, 0], ran=[0], slots0=[0, 2, 4, 6, 8], fails={1: 0, 3: 1, 5: 2, 7: 3})),
    'in_call': dict(C=32, L=6, num_class=1, out_hw=[40, 56], min_size=8, seed=13, ptr=[5],
                    what='four good stored entries: object 0 finds four (it would have matched object 1), object 1 finds its fifth in object 0 (slot 5), '
                         'its append wraps ptr to slot 0, object 2 sees both',
                    bank=[_e('otherfeat', 0, 0)] + [_e('good', 0, s) for s in range(1, 5)],
                    objects=[_e('good', 0), _e('good', 0), _e('good', 0)],
                    census=dict(count=[4, 5, 5], ran=[1, 2], src1=[-1, -1, -1, -1, 0], src2=[1, -1, -1, -1, -1], ptr=[2])),
    'edges': dict(C=32, L=8, num_class=2, out_hw=[40, 56], min_size=8, seed=14, ptr=[5, 5],
                  what='a box 1 pixel high (below min_size: not appended; one 1 pixel WIDE and higher makes the reference raise at :1103, its squeeze() drops the width), a box touching the right and bottom border, one touching the top-left corner',
                  bank=[_e('thin', 0, s) for s in range(5)] + [_e('good', 1, s) for s in range(5)],
                  objects=[_e('thin', 0), _e('good', 1, box=[36, 18, 56, 40]), _e('good', 1, box=[0, 0, 20, 22])],
                  census=dict(count=[5, 5, 5], ran=[0, 1, 2], ptr=[5, 7])),
    'edges_empty': dict(C=32, L=8, num_class=2, out_hw=[40, 56], min_size=8, seed=15, ptr=[5, 5], what='N = 0', bank=[_e('good', 1, 0)], objects=[],
                        census=dict(count=[], ran=[])),
    'c256': dict(C=256, L=8, num_class=1, out_hw=[24, 40], min_size=8, seed=16, ptr=[5], what='one object at C = 256',
                 bank=[_e('good', 0, s) for s in range(5)], objects=[_e('good', 0, box=[9, 2, 29, 22])], census=dict(count=[5], ran=[0])),
}


def have_reference():
    return os.path.exists(os.path.join(REF, HEAD))


def build_inputs(case):
    """The float32 arrays of one case (every value exact in float16)."""
    rng = np.random.RandomState(case['seed'])
    C, L, nc = case['C'], case['L'], case['num_class']
    bases = [[np.abs(rng.standard_normal((C, R.FEAT, R.FEAT))) for _ in range(2)] for _ in range(nc)]

    def entry(e, jitter):
        k = dict(KINDS[e['kind']])
        box = e.get('box', k.get('box', SQ))
        m = R.blob(13.5 + jitter * rng.uniform(-0.4, 0.4), 13.5 + jitter * rng.uniform(-0.4, 0.4), k.get('radius', 9.0) + jitter * rng.uniform(-0.3, 0.3),
                   k.get('floor', 0.0))
        m = R.snap(m)
        return R.half(R.feature(bases[e['cls']][k.get('base', 0)], rng)), R.half(m), np.asarray(box, np.float32)

    out = dict(bank_feature=np.zeros((nc, L, C, 7, 7), np.float32), bank_mask=np.zeros((nc, L, 28, 28), np.float32),
               bank_box=np.zeros((nc, L, 4), np.float32), bank_ptr=np.asarray(case['ptr'], np.int32))
    for e in case['bank']:
        out['bank_feature'][e['cls'], e['slot']], out['bank_mask'][e['cls'], e['slot']], out['bank_box'][e['cls'], e['slot']] = entry(e, 1.0)
    N = len(case['objects'])
    out.update(s_feat=np.zeros((N, C, 7, 7), np.float32), s_mask=np.zeros((N, 28, 28), np.float32), t_feat=np.zeros((N, C, 7, 7), np.float32),
               t_mask=np.zeros((N, 28, 28), np.float32), boxes=np.zeros((N, 4), np.float32), labels=np.zeros((N,), np.int64))
    for i, e in enumerate(case['objects']):
        out['s_feat'][i], out['s_mask'][i], out['boxes'][i] = entry(e, 1.0)
        out['t_feat'][i], out['t_mask'][i], _ = entry(e, 1.0)
        out['labels'][i] = e['cls']
    return out


# ---- the reference, by AST ---------------------------------------------------------------------------------------------------------------
def load_reference():
    path = os.path.join(REF, HEAD)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    env = {'torch': torch, 'nn': nn, 'F': F, 'np': np, 'autocast': lambda **kw: contextlib.nullcontext()}
    want = ('relu_and_l2_norm_feat', 'ObjectFactory', 'ObjectElements', 'ObjectQueues', 'SemanticCorrSolver')
    nodes = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert len(nodes) == len(want)
    head = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DiscoBoxSOLOv2Head')
    sup = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'superres_T')
    closs = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'corr_loss')
    outer = next(n for n in closs.body if isinstance(n, ast.For) and any(isinstance(m, ast.Name) and m.id == 'queue_area_mask' for m in ast.walk(n)))
    area = next(n for n in ast.walk(outer) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id == 'queue_area_mask')
    loop = next(n for n in ast.walk(outer) if isinstance(n, ast.For) and n is not outer and
                any(isinstance(m, ast.Name) and m.id == 'queue_area_mask' for m in ast.walk(n.iter)))
    shell = ast.parse('def object_loop(self, roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, kernel_labels, min_x, max_x, min_y, max_y, iiu, mask, '
                      'corr_loss, num_ins):\n    pass\n    return corr_loss, num_ins\n').body[0]
    shell.body = [area, loop, shell.body[1]]
    for n in nodes + [sup]:
        n.decorator_list = []
    m = ast.Module(body=nodes + [sup, shell], type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, 'exec'), env)
    return env


@contextlib.contextmanager
def precision(dtype):
    old_default, old_float = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(dtype)
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.set_default_dtype(old_default)
        torch.Tensor.float = old_float


def run_reference(env, case, arrays, dtype):
    """The reference's loop over one case; returns what the fixture records (tensors of ``dtype``)."""
    with precision(dtype):
        t = {k: torch.from_numpy(v.copy()) for k, v in arrays.items()}
        f = {k: (v.to(dtype) if v.dtype == torch.float32 else v) for k, v in t.items()}
        C, L, nc, K = case['C'], case['L'], case['num_class'], CFG['max_retrieval_objs']
        N = f['s_feat'].shape[0]
        queues = env['ObjectQueues'](num_class=nc, len_queue=L, fg_iou_thresh=CFG['fg_iou_thresh'], bg_iou_thresh=CFG['bg_iou_thresh'],
                                     ratio_range=CFG['ratio_range'], appear_thresh=CFG['appear_thresh'], max_retrieval_objs=K)
        used = {e['cls'] for e in case['bank']}
        for c in sorted(used):
            q = env['ObjectElements'](size=L, img_size=0, feat_size=R.FEAT, mask_size=R.MASK, n_channel=C, device='cpu', category=c)
            q.mask[...], q.feature[...], q.box[...] = f['bank_mask'][c], f['bank_feature'][c], f['bank_box'][c]
            q.ptr = int(f['bank_ptr'][c])
            queues.queues[c] = q
        solver = env['SemanticCorrSolver'](CFG['corr_exp'], CFG['corr_eps'], CFG['gaussian_filter_size'], CFG['low_score'], CFG['corr_num_iter'],
                                           CFG['corr_num_smooth_iter'], dist_kernel=CFG['dist_kernel'])
        rec = dict(ret_slot=-np.ones((N, K), np.int64), count=np.zeros(N, np.int64), Cu=np.zeros((N, K, 49, 49)), C=np.zeros((N, K, 49, 49)),
                   assign=-np.ones((N, K, 49), np.int64))
        state = dict(i=-1, idx=None)
        real_get, real_item, real_solve = queues.get_similar_obj, env['ObjectElements'].__getitem__, solver.solve

        def getitem(self, idx):
            if torch.is_tensor(idx):
                state['idx'] = idx.clone()
            return real_item(self, idx)

        def get_similar(qobj):
            state['i'] += 1
            state['idx'] = None
            ret = real_get(qobj)
            if state['idx'] is not None:
                n = state['idx'].numel()
                rec['count'][state['i']] = n
                rec['ret_slot'][state['i'], :n] = state['idx'].numpy()
            return ret

        def solve(qobjs, kobjs, f0):
            Cu, Cm, fg, bg = real_solve(qobjs, kobjs, f0)
            n = Cu.shape[0]
            rec['Cu'][state['i'], :n], rec['C'][state['i'], :n] = Cu.detach().double().numpy(), Cm.detach().double().numpy()
            rec['assign'][state['i'], :n] = Cm.argmax(2).numpy()
            return Cu, Cm, fg, bg

        env['ObjectElements'].__getitem__ = getitem
        queues.get_similar_obj, solver.solve = get_similar, solve
        try:
            me = types.SimpleNamespace(object_queues=queues, semantic_corr_solver=solver, save_corr_img=False, corr_feat_height=R.FEAT,
                                       corr_feat_width=R.FEAT, corr_mask_height=R.MASK, corr_mask_width=R.MASK, objbank_min_size=case['min_size'],
                                       num_created_gpu_bank=0, num_gpu_bank=1 << 30, img_norm_cfg=None)
            me.superres_T = types.MethodType(env['superres_T'], me)
            me.qobj = env['ObjectFactory'].create_one(mask=torch.zeros(1, R.MASK, R.MASK), feature=torch.zeros(1, C, R.FEAT, R.FEAT), box=torch.zeros(1, 4),
                                                      img=None, category=0)
            H, W = case['out_hw']
            s_feat = f['s_feat'].clone().requires_grad_(True)
            b = f['boxes']
            iiu = torch.zeros(2 * N, H, W)
            loss, num_ins = env['object_loop'](me, s_feat, f['s_mask'], f['t_feat'], f['t_mask'], b, f['labels'], b[:, 0].long(), b[:, 2].long(),
                                               b[:, 1].long(), b[:, 3].long(), iiu, f['s_mask'], torch.zeros(()), 0)
            grad = torch.autograd.grad(loss, s_feat)[0] if num_ins else torch.zeros_like(s_feat)
        finally:
            env['ObjectElements'].__getitem__ = real_item
        rec.update(loss_sum=np.asarray(float(loss)), num_ins=np.asarray(num_ins, np.int64), grad=grad.double().numpy(),
                   iiu=iiu.reshape(N, 2, H, W).double().numpy())
        after = {k: f[k].clone() for k in ('bank_feature', 'bank_mask', 'bank_box')}
        ptr = f['bank_ptr'].clone()
        for c in range(nc):
            q = queues.queues[c]
            if q is not None:
                after['bank_feature'][c], after['bank_mask'][c], after['bank_box'][c], ptr[c] = q.feature, q.mask, q.box, q.ptr
        rec.update(after_feature=after['bank_feature'].float().numpy(), after_mask=after['bank_mask'].float().numpy(),
                   after_box=after['bank_box'].float().numpy(), after_ptr=ptr.numpy().astype(np.int32))
        return rec


EXACT = ('ret_slot', 'count', 'assign', 'num_ins', 'after_feature', 'after_mask', 'after_box', 'after_ptr')


def restated(case, arrays):
    inp = {k: torch.from_numpy(arrays[k].copy()) for k in R.INPUT_KEYS}
    inp = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in inp.items()}
    inp['s_feat'].requires_grad_(True)
    cfg = dict(CFG, min_size=case['min_size'])
    out = R.corr_objects(inp, cfg, case['out_hw'], record=True)
    grad = torch.autograd.grad(out['loss_sum'], inp['s_feat'])[0] if out['num_ins'] else torch.zeros_like(inp['s_feat'])
    return out, grad, inp


def conditions(case, arrays, r64):
    """The margins of the docstring, in fp64, over the bank as every object sees it."""
    inp = {k: torch.from_numpy(arrays[k].copy()) for k in R.INPUT_KEYS}
    inp = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in inp.items()}
    ok = True
    worst = dict(score=np.inf, count=np.inf, half=np.inf, gap=np.inf)
    bf, bm, bb, ptr = (inp[k] for k in R.INPUT_KEYS[6:])
    lo, hi = CFG['ratio_range']
    for i in range(inp['labels'].shape[0]):
        c = int(inp['labels'][i])
        live = bm[c].flatten(1).abs().sum(1) > 0
        sc = R.slot_scores(inp['s_mask'][i], inp['s_feat'][i], inp['boxes'][i], bm[c], bf[c], bb[c])
        for v, ths in zip(sc, ((CFG['fg_iou_thresh'],), (CFG['bg_iou_thresh'],), (CFG['appear_thresh'],), (lo, hi))):
            for th in ths:
                fin = torch.isfinite(v) & live
                ok &= bool(((v[fin] - th).abs() >= MARGIN * th).all())
                worst['score'] = min([worst['score']] + ((v[fin] - th).abs() / th).tolist())
        A = inp['s_mask'][i][None]
        ok &= bool((((A + bm[c][live]) - 1).abs() >= MARGIN).all()) and bool((((2 - A - bm[c][live]) - 1).abs() >= MARGIN).all())
        if bool(live.any()):
            worst['count'] = min(worst['count'], float(((A + bm[c][live]) - 1).abs().min()), float(((2 - A - bm[c][live]) - 1).abs().min()))
        n = int(r64['count'][i])
        if n >= CFG['min_objs']:
            m1 = bm[c][torch.from_numpy(r64['ret_slot'][i, :n])]
            a, b = inp['s_mask'][i].reshape(1, -1, 1), m1.reshape(n, 1, -1)
            ok &= bool(((a * b - 0.5).abs() >= MARGIN).all()) and bool((((1 - a) * (1 - b) - 0.5).abs() >= MARGIN).all())
            worst['half'] = min(worst['half'], float((a * b - 0.5).abs().min()), float(((1 - a) * (1 - b) - 0.5).abs().min()))
            top = torch.from_numpy(r64['C'][i, :n]).topk(2, dim=2).values
            worst['gap'] = min(worst['gap'], float(((top[..., 0] - top[..., 1]) / top[..., 0]).min()))
            ok &= bool((((top[..., 0] - top[..., 1]) / top[..., 0]) >= MARGIN).all())
        if (inp['boxes'][i][2] - inp['boxes'][i][0]) > case['min_size'] and (inp['boxes'][i][3] - inp['boxes'][i][1]) > case['min_size']:
            s = int(ptr[c])
            bf[c, s], bm[c, s], bb[c, s] = inp['t_feat'][i], inp['t_mask'][i], inp['boxes'][i]
            ptr[c] = (s + 1) % case['L']
    print('smallest margins:', {k: f'{v:.2e}' for k, v in worst.items()})
    return ok


def census(name, case, arrays, r64):
    cs = case['census']
    ran = [i for i in range(len(case['objects'])) if r64['count'][i] >= CFG['min_objs']]
    ok = r64['count'].tolist() == cs['count'] and ran == cs['ran'] and int(r64['num_ins']) == len(ran)
    if 'slots0' in cs:
        ok &= r64['ret_slot'][0].tolist() == cs['slots0']
        inp = {k: torch.from_numpy(arrays[k]).double() for k in R.INPUT_KEYS[:5] + R.INPUT_KEYS[6:9]}
        sc = torch.stack(R.slot_scores(inp['s_mask'][0], inp['s_feat'][0], inp['boxes'][0], inp['bank_mask'][0], inp['bank_feature'][0], inp['bank_box'][0]))
        lo, hi = CFG['ratio_range']
        good = torch.stack([sc[0] > CFG['fg_iou_thresh'], sc[1] > CFG['bg_iou_thresh'], sc[2] > CFG['appear_thresh'], (sc[3] >= lo) & (sc[3] <= hi)])
        for slot, which in cs['fails'].items():
            ok &= (~good[:, int(slot)]).nonzero().flatten().tolist() == [which]
    if 'ptr' in cs:
        ok &= r64['after_ptr'].tolist() == cs['ptr']
    print(f'{name}: census {"holds" if ok else "FAILS"}; counts {r64["count"].tolist()}, ran {ran}')
    return bool(ok)


def rel(a32, a64):
    a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
    top = np.abs(a64).max() if a64.size else 0.0
    return float(np.abs(a32 - a64).max() / top) if top > 0 else 0.0


def config_blocks():
    from boxinstseg_amd import load_config, parse_corr_cfg
    out = {}
    folder = os.path.join(REF, 'configs', 'discobox')
    for f in sorted(os.listdir(folder)):
        if f.endswith('.py'):
            out[f'discobox/{f}'] = parse_corr_cfg(load_config(os.path.join(folder, f))['model']['bbox_head'])
    return out


def case_arrays(env, name, case):
    """({fixture key: array}, {'Cu', 'C'} planes, {tolerance: value}) of one case; SystemExit where a check of the docstring fails."""
    out, tols = {}, {k: 0.0 for k in R.TOLERANCED}
    arrays = build_inputs(case)
    r32, r64 = run_reference(env, case, arrays, torch.float32), run_reference(env, case, arrays, torch.float64)
    for k in EXACT:
        if not np.array_equal(r32[k], r64[k]):
            raise SystemExit(f'case {name}: fp32 and fp64 runs of the reference differ in {k}')
    mine, grad, inp = restated(case, arrays)
    same = all(np.array_equal(np.asarray(mine[k]), r64[k]) for k in ('ret_slot', 'count', 'assign')) and mine['num_ins'] == int(r64['num_ins'])
    same &= all(np.allclose(a, b, rtol=1e-9, atol=1e-12) for a, b in ((mine['Cu'].numpy(), r64['Cu']), (mine['C'].numpy(), r64['C']), (grad.numpy(), r64['grad']),
                                                                  (mine['iiu'].numpy(), r64['iiu']), (float(mine['loss_sum']), float(r64['loss_sum']))))
    same &= all(np.array_equal(inp[a].float().numpy(), r64[b]) for a, b in (('bank_feature', 'after_feature'), ('bank_mask', 'after_mask'),
                                                                              ('bank_box', 'after_box'))) and np.array_equal(inp['bank_ptr'].numpy(), r64['after_ptr'])
    if not same:
        raise SystemExit(f'case {name}: tests/corr_ref.py does not reproduce the reference')
    if not conditions(case, arrays, r64):
        raise SystemExit(f'case {name}: a value is within {MARGIN} of a discontinuity')
    if not census(name, case, arrays, r64):
        raise SystemExit(f'case {name} rejected')
    for k, v in arrays.items():
        out[f'{name}_{k}'] = v.astype(np.float16) if v.dtype == np.float32 else v
        assert v.dtype != np.float32 or np.array_equal(out[f'{name}_{k}'].astype(np.float32), v), k
    for k in EXACT + ('loss_sum', 'grad', 'iiu'):
        v = r64[k]
        out[f'{name}_{k}'] = v.astype(np.float16) if k in ('after_feature', 'after_mask', 'after_box') else v
    out[f'{name}_iiu_zero'] = np.packbits(r64['iiu'] == 0)
    assert np.array_equal(r32['iiu'] == 0, r64['iiu'] == 0)
    if int(r64['num_ins']):
        for k in R.TOLERANCED:
            tols[k] = rel(r32[k], r64[k])
    return out, dict(Cu=r64['Cu'], C=r64['C']), tols


def main():
    env = load_reference()
    out, planes, tols = {}, {}, {k: 0.0 for k in R.TOLERANCED}
    for name, case in SPEC.items():
        got, planes[name], tol = case_arrays(env, name, case)
        out.update(got)
        for k, v in tol.items():
            tols[k] = max(tols[k], v)
    for k, v in tols.items():
        assert v > 0, k
        out[f'tol_{k}'] = np.array(v)
        print(f'tol_{k} = {v:.3e}')
    for path, data in [(R.GOLDEN, out)] + [(os.path.join(HERE, f'corr_planes_{n}.npz'), d) for n, d in planes.items()]:
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < (1 << 20)
    spec = copy.deepcopy(SPEC)
    with open(R.CASES, 'w') as fh:
        json.dump(dict(cfg=CFG, kinds=KINDS, cases=spec), fh, indent=1, sort_keys=True)
        fh.write('\n')
    with open(os.path.join(HERE, 'corr_cfg.json'), 'w') as fh:
        json.dump(config_blocks(), fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
