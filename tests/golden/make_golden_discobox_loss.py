#!/usr/bin/env python
"""Developer tool: writes tests/golden/discobox_loss.npz from the reference's own text (needs the reference checkout; never run by a test).

Taken out of mmdet/models/dense_heads/discobox_head.py by AST: ``MeanField``, ``dice_loss``, ``mil_loss`` (oracle/reference_extract.py) and the
statements of ``DiscoBoxSOLOv2Head.loss`` at :1271-1306 (the level loop and the mean of loss_ins) and :1335-1339 (loss_ts), and of ``corr_loss``
the head of its level loop (:1014-1029, the text of :1271-1286 again) with its tail :1127-1137.  They run on the CPU in fp32 and in fp64
(autocast is not entered; in the fp64 run ``Tensor.float()`` keeps fp64, the reference casts with it in eleven places).

The block is pinned behind the sigmoid: ``torch.sigmoid`` is the identity while the statements run, the inputs ARE the probabilities (folding
the sigmoid into the kernels is out of scope, and an fp32 / fp64 sigmoid would give the two runs different inputs).  ``iiu`` of a level is handed
to the tail where the object loop (:1059-1125, pinned by tests/golden/corr.npz) would have filled it.

Inputs follow tests/mf_decided.recipe (features, boxes, img_inds, inter_img_mask in the competing range), every float rounded to an fp16-exact
value.  A case is REFUSED when the fp32 and fp64 labels differ, or when tests/mf_decided.step_with_corners marks any pixel undecided in any
iteration of either leg (zero may not be left out: a device result may differ from the reference exactly there).

Per case the file holds the inputs, per-row pseudo-labels of both legs, ``live``, mil / ts / ts_corr rows, the three means, the gradient of
loss_ts w.r.t. s (fp64 values), and ``tol_*`` = the reference's own fp32-against-fp64 difference relative to the largest fp64 magnitude."""
import ast
import contextlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference_extract as RE  # noqa: E402
from tests import mf_decided as D  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'discobox_loss.npz')
LINES = dict(level_loop=1271, ins_mean=1302, ts_mean=1335, corr_level_loop=1014, corr_tail=1127)
GAMMA = 0.01
MF = dict(alpha0=2.0, theta0=0.5, theta1=30.0, theta2=20.0, base=0.1)
# name -> (rows, H, W, kernel size, iterations, rows per level, dead rows)
CASES = {
    'k3': (6, 20, 70, 3, 10, [2, 0, 4], [3]),
    'k3_short': (5, 12, 40, 3, 3, [5], []),
    # a 5x5 kernel cannot be pinned this way: exp(-acc) of 25 neighbours is 1e-9 .. 1e-13 against the + 1e-6, most in-target pixels sit within an
    # fp32 ulp of 0.5 and the fp32 and fp64 runs of the reference disagree on over a hundred labels (the refusal rule); 5x5 labels are held to
    # meanfield_forward and, through it, to tests/mf_decided.py
}


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def build_inputs(name):
    n, H, W, ks, iters, level_rows, dead = CASES[name]
    d = D.recipe(n, H, W, ks, with_inter=True)
    rng = np.random.default_rng(77 + n)
    target = d['t'].copy()
    for r in dead:
        target[r] = 0
    return dict(feats=f16(d['feats']), s=f16(d['x']), t=f16(rng.uniform(0, 1, size=(n, H, W))), target=target, img=np.asarray(d['img'], np.int64),
                inter=f16(d['inter'] * np.float32(D.INTER_COMPETING_HI / 20.0)), level_rows=np.asarray(level_rows, np.int64), ks=ks, iters=iters)


def load_reference():
    """The namespace of the extracted text with three functions made of the reference's statements."""
    path = os.path.join(RE.REFERENCE_ROOT, RE.DISCOBOX_FILE)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    head = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DiscoBoxSOLOv2Head')
    loss = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'loss')
    closs = next(n for n in head.body if isinstance(n, ast.FunctionDef) and n.name == 'corr_loss')
    at = lambda fn, line, kind: next(n for n in fn.body if isinstance(n, kind) and n.lineno == line)
    level_loop, ins_mean, ts_mean = at(loss, LINES['level_loop'], ast.For), at(loss, LINES['ins_mean'], ast.If), at(loss, LINES['ts_mean'], ast.If)
    assert ins_mean.end_lineno == 1306 and ts_mean.end_lineno == 1339 and level_loop.end_lineno == 1300
    cloop = at(closs, LINES['corr_level_loop'], ast.For)
    cut = next(i for i, n in enumerate(cloop.body) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id == 'pos_inds')
    tail = cloop.body[-2:]
    assert isinstance(tail[0], ast.Assign) and tail[0].lineno == LINES['corr_tail'] and isinstance(tail[1], ast.For) and tail[1].end_lineno == 1137
    hand = ast.parse('iiu = next_iiu(mask)').body
    shells = ast.parse(
        'def loss_block(self, s_ins_pred_list, t_ins_pred_list, img_ind_list, ins_labels, kernel_label_list, mean_fields, color_feats, use_ind_teacher,'
        ' use_loss_ts):\n    loss_ins = []\n    loss_ts = []\n    pass\n    return loss_ins, loss_ts\n'
        'def ts_block(self, loss_ts, corr_loss_ts, use_loss_ts, loss_ins):\n    pass\n    return loss_ts\n'
        'def corr_tail(self, s_ins_pred_list, t_ins_pred_list, img_ind_list, ins_labels, kernel_label_list, mean_fields, use_ind_teacher, next_iiu):\n'
        '    loss_ts = []\n    pass\n    return loss_ts\n').body
    fill = lambda fn, stmts: fn.body.__setitem__(slice(len(fn.body) - 2, len(fn.body) - 1), stmts)
    fill(shells[0], [level_loop, ins_mean])
    fill(shells[1], [ts_mean])
    fill(shells[2], [ast.For(target=cloop.target, iter=cloop.iter, body=cloop.body[:cut] + hand + tail, orelse=[])])
    env = dict(RE.load_discobox()._env)
    mod = ast.Module(body=shells, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, 'exec'), env)
    return env


@contextlib.contextmanager
def precision(dtype):
    """In the fp64 run ``.float()`` keeps fp64; ``torch.sigmoid`` is the identity in both (module docstring)."""
    real_float, real_sigmoid = torch.Tensor.float, torch.sigmoid
    if dtype == torch.float64:
        torch.Tensor.float = lambda self: self.double()
    torch.sigmoid = lambda x: x
    try:
        yield
    finally:
        torch.Tensor.float, torch.sigmoid = real_float, real_sigmoid


class Recorder:
    """A mean field that keeps the labels it returned, in call order."""

    def __init__(self, mf, store):
        self.mf, self.store, self.gamma = mf, store, mf.gamma

    def __call__(self, x, targets, inter=None):
        ret, valid = self.mf(x, targets, inter) if inter is not None else self.mf(x, targets)
        self.store.append(ret.squeeze(1).detach().clone())
        return ret, valid


def run_reference(env, a, dtype):
    n, H, W = a['s'].shape
    rows = [int(v) for v in a['level_rows']]
    first = np.cumsum([0] + rows)
    s = torch.tensor(a['s'], dtype=dtype, requires_grad=True)
    t = torch.tensor(a['t'], dtype=dtype)
    target, img = torch.tensor(a['target']), torch.tensor(a['img'])
    cut = lambda v: [v[first[l]:first[l + 1]] if rows[l] else None for l in range(len(rows))]
    s_list, t_list = cut(s), cut(t)
    img_list = [None if v is None else v.to(torch.float32) for v in cut(img)]
    labels = [target[first[l]:first[l + 1]] for l in range(len(rows))]
    klabels = [torch.zeros(r, dtype=torch.int64) for r in rows]
    me = types.SimpleNamespace(ins_loss_weight=1.0, ts_loss_weight=1.0)
    mil_rows = []
    real_mil = env['mil_loss']

    def mil(*args):
        out = real_mil(*args)
        mil_rows.append(out.detach().clone())
        return out
    env = dict(env, mil_loss=mil)
    # the three functions look names up in their own globals: rebuild them over the patched namespace
    fns = {k: types.FunctionType(env[k].__code__, env) for k in ('loss_block', 'ts_block', 'corr_tail')}
    with precision(dtype):
        color = torch.tensor(a['feats'], dtype=dtype)
        lab0, lab1 = [], []
        mfs = [env['MeanField'](c.unsqueeze(0), alpha0=MF['alpha0'], theta0=MF['theta0'], theta1=MF['theta1'], theta2=MF['theta2'], iter=int(a['iters']),
                                kernel_size=int(a['ks']), base=MF['base']) for c in color]
        loss_ins, ts_list = fns['loss_block'](me, s_list, t_list, img_list, labels, klabels, [Recorder(m, lab0) for m in mfs], color, True, True)
        inter = torch.tensor(a['inter'], dtype=dtype)
        levels = [inter[first[l]:first[l + 1]] for l in range(len(rows)) if rows[l]]

        def next_iiu(mask):
            v = levels.pop(0)[mask.bool()]
            return v.reshape(v.shape[0] * 2, H, W)
        corr_list = fns['corr_tail'](me, s_list, t_list, img_list, labels, klabels, [Recorder(m, lab1) for m in mfs], True, next_iiu)
        corr_mean = torch.cat(corr_list).mean()                                            # :1330
        mean_ts = torch.cat(ts_list).mean()
        loss_ts = fns['ts_block'](me, list(ts_list), corr_mean, True, loss_ins)
        (grad,) = torch.autograd.grad(loss_ts, s)
    # scatter to rows: level-major, inside a level image by image, the kept rows in order (the loops' order)
    live = (target.flatten(1).sum(1) != 0).numpy()
    order = []
    for l in range(len(rows)):
        kept = [r for r in range(first[l], first[l + 1]) if live[r]]
        order += [[r for r in kept if int(img[r]) == b] for b in range(color.shape[0]) if any(int(img[r]) == b for r in kept)]
    flat = [r for grp in order for r in grp]
    out = dict(live=live.astype(np.uint8), grad=grad.double().numpy(), mean_ins=float(loss_ins.detach()), mean_ts=float(mean_ts.detach()),
               mean_ts_corr=float(corr_mean.detach()), loss_ts=float(loss_ts.detach()))
    for key, vals, idx in (('pseudo', torch.cat(lab0), flat), ('pseudo_corr', torch.cat(lab1), flat), ('ts_rows', torch.cat(ts_list).detach(), flat),
                           ('ts_corr_rows', torch.cat(corr_list).detach(), flat), ('mil_rows', torch.cat(mil_rows), [r for r in range(n) if live[r]])):
        full = np.zeros((n,) + tuple(vals.shape[1:]), np.float64)
        full[idx] = vals.double().numpy()
        out[key] = full
    return out


def refuse(name, a, r32, r64):
    for key in ('pseudo', 'pseudo_corr'):
        if not np.array_equal(r32[key], r64[key]):
            raise SystemExit(f'{name}: REFUSED: {int((r32[key] != r64[key]).sum())} {key} labels differ between fp32 and fp64')
    from oracle import discobox_oracle as do
    Ko = np.stack([do.meanfield_kernel(a['feats'][b], int(a['ks']), MF['alpha0'], MF['theta0'], MF['theta1']) for b in range(a['feats'].shape[0])])
    x = ((a['t'] + a['s']) / np.float32(2)).astype(np.float32)
    for key, inter in (('pseudo', None), ('pseudo_corr', a['inter'])):
        states, undecided = D.trajectory_by_image(Ko, a['img'], x, a['target'], int(a['iters']), MF['base'], inter, GAMMA)
        bad = sum(int(u.sum()) for u in undecided)
        if bad:
            raise SystemExit(f'{name}: REFUSED: {bad} undecided pixels on the way to {key}')
        if not np.array_equal(states[-1], r64[key] != 0):
            raise SystemExit(f'{name}: REFUSED: the oracle trajectory and the reference disagree on {key}')
    if np.array_equal(r64['pseudo'], r64['pseudo_corr']) or not r64['pseudo'].any():
        raise SystemExit(f'{name}: REFUSED: the legs do not differ, or leg 0 is empty')


def rel(a32, a64):
    a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
    return float(np.abs(a32 - a64).max() / max(np.abs(a64).max(), 1e-300))


def main():
    if not RE.available():
        raise SystemExit('the reference checkout is not here')
    env = load_reference()
    out = {}
    for name in CASES:
        a = build_inputs(name)
        r32, r64 = run_reference(env, a, torch.float32), run_reference(env, a, torch.float64)
        refuse(name, a, r32, r64)
        for k, v in a.items():
            out[f'{name}/{k}'] = np.asarray(v)
        for k in ('live', 'pseudo', 'pseudo_corr'):
            out[f'{name}/{k}'] = r64[k].astype(np.uint8)
        for k in ('mil_rows', 'ts_rows', 'ts_corr_rows', 'grad'):
            out[f'{name}/{k}'] = r64[k]
            out[f'{name}/tol_{k}'] = np.float64(rel(r32[k], r64[k]))
        for k in ('mean_ins', 'mean_ts', 'mean_ts_corr', 'loss_ts'):
            out[f'{name}/{k}'] = np.float64(r64[k])
            out[f'{name}/tol_{k}'] = np.float64(rel(r32[k], r64[k]))
        print(name, {k.split('/')[1]: float(v) for k, v in out.items() if k.startswith(name + '/tol_')},
              'labels', int(r64['pseudo'].sum()), int(r64['pseudo_corr'].sum()), 'differ', int((r64['pseudo'] != r64['pseudo_corr']).sum()))
    out['gamma'], out['cases'] = np.float64(GAMMA), np.array(list(CASES))
    for k, v in MF.items():
        out[f'mf/{k}'] = np.float64(v)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
