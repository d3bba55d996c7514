"""The pseudo-label block of DiscoBoxSOLOv2Head.loss restated in torch, and the cases of tests/test_gpu_dbx_loss.py.

TEST INFRASTRUCTURE ONLY (numpy / torch on the CPU; imported by tests/test_host_dbx_loss.py, tests/test_gpu_dbx_loss.py and
tests/test_gpu_guarded_dbx_loss.py).

``terms(...)`` is discobox_head.py:1294-1300 and :1130-1137 for a row buffer, given the pseudo-labels: the enlarged target by
``F.max_pool2d``, ``dice_loss`` as the reference writes it, the gamma mix with the reference's fp32 constants.  In fp64 it is the value the
kernels are held to; its autograd is the gradient.

The inputs of every case are dyadic: s and t are multiples of 2^-6 in [0, 1].  Then s * e, (s e)^2 and their sums over a map of up to
2^16 pixels are exact in fp64 in any order, and the leg-0 dice row is ONE rounding of an exactly known fp64 value: the GPU test compares it
with no tolerance.  Leg 1 multiplies by fl32(0.01) and fl32(0.99), whose products are not dyadic; see TOL_ROW below.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
GAMMA = 0.01
# what fp32 formats allow, written down (no figure here comes from a run of the code under test):
# * a leg-1 row is a fp64 expression of fp64 sums rounded once to fp32 (2^-24 relative), of terms a1 = fl(fl(a0 g) + fl(a0 (1 - g))) that
#   the restatement forms with the same three fp32 roundings; the sums themselves differ only by their fp64 order (2^-53 per term).
#   1 - 2A/D lies in [0, 1], so the bound is absolute: 2^-23 leaves one fp32 ulp at 1 for the order of the fp64 sums.
TOL_ROW = 2.0 ** -23
# * a mean is a fp64 sum of at most 65535 such rows divided once and rounded once: the rows' own error plus one rounding.
TOL_MEAN = 2.0 ** -22
# * an element of the gradient is e (g0 (cb0 b0 + ca0 a0) + gamma g1 (cb1 b1 + ca1 a1)) with the four coefficients rounded from fp64 to
#   fp32 and at most 9 fp32 operations behind them: 13 roundings of 2^-24 each, relative to the largest term, bounded by the largest
#   gradient magnitude of the row times 4 (the terms of one element may cancel): 13 * 4 * 2^-24 < 2^-18 of the row's largest |gradient|.
TOL_GRAD_REL = 2.0 ** -18


def enlarged_of(target: torch.Tensor) -> torch.Tensor:
    """discobox_head.py:1294 / :1130."""
    return F.max_pool2d(target.float().unsqueeze(1), kernel_size=3, stride=1, padding=1).squeeze(1).byte()


def dice_loss(inp, target):
    """discobox_head.py:542-550."""
    inp = inp.contiguous().view(inp.size()[0], -1)
    target = target.contiguous().view(target.size()[0], -1).to(inp.dtype)
    a = torch.sum(inp * target, 1)
    b = torch.sum(inp * inp, 1) + 0.001
    c = torch.sum(target * target, 1) + 0.001
    return 1 - (2 * a) / (b + c)


def terms(s, target, pseudo, pseudo_corr=None, gamma=GAMMA, dtype=torch.float64):
    """(ts_rows, ts_corr_rows | None) for ALL rows (a dead row gives 1 - 0 / 0.002 = 1), differentiable w.r.t. ``s`` (any float dtype; the
    arithmetic runs in ``dtype``).  The gamma mix uses the reference's constants: a fp32 tensor times the python floats gamma and 1 - gamma
    multiplies by fl32(gamma) and fl32(1 - gamma); in fp32 the two products and the sum are rounded as the reference's are."""
    e = enlarged_of(target).to(dtype)
    a0 = s.to(dtype) * e
    ts = dice_loss(a0, pseudo.to(dtype))
    if pseudo_corr is None:
        return ts, None
    g, omg = float(f32(gamma)), float(f32(1.0 - gamma))
    if dtype == torch.float64:
        # the fp32 value of a1 (three roundings) carried in fp64, with the reference's gradient (the factor gamma on the first product)
        a1v = ((a0.detach().float() * f32(gamma)) + (a0.detach().float() * f32(1.0 - gamma))).double()
        a1 = a1v + (a0 - a0.detach()) * g
    else:
        a1 = a0 * g + a0.detach() * omg
    return ts, dice_loss(a1, pseudo_corr.to(dtype))


def live_of(target: torch.Tensor) -> torch.Tensor:
    """discobox_head.py:1281-1286: the rows the reference keeps."""
    return (target != 0).flatten(1).any(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (H, W, ks, iters, level_rows, iiu given per level, kind)
CASES = {
    'w13': (9, 13, 3, 10, [2, 2], [True, True], 'boxes'),                 # W below one word
    'w64': (6, 64, 3, 1, [4], [True], 'boxes'),                           # no partial word
    'w128': (6, 128, 5, 10, [2, 3], [True, True], 'boxes'),
    'w70': (7, 70, 3, 10, [3, 2], [True, True], 'boxes'),                 # partial last word
    'w129': (5, 129, 5, 1, [5], [True], 'boxes'),
    'w70_k5_it0': (7, 70, 5, 0, [3, 2], [True, True], 'boxes'),
    'w70_k3_it1': (7, 70, 3, 1, [3, 2], [True, True], 'boxes'),
    'edges': (8, 130, 3, 10, [6, 6], [True, True], 'edges'),              # single pixels at columns 0, 63, 64, W - 1 and lines 0, H - 1
    'r1': (9, 13, 3, 10, [1], [True], 'boxes'),
    'dead': (7, 70, 3, 10, [3, 4], [True, True], 'dead'),                 # dead rows first, in the middle and last
    'all_dead': (7, 70, 3, 10, [2, 2], [True, True], 'all_dead'),
    'level_gap': (9, 70, 3, 10, [2, 0, 2, 1], [True, False, False, True], 'boxes'),     # a level without rows; iiu null for a level with rows
    'many': (200, 304, 3, 10, [24, 16], [True, True], 'boxes'),           # 40 x 200 x 5 items > MF_MANY_ITEMS: four items per wave
}
EDGE_COLUMNS = (0, 63, 64, -1)
EDGE_LINES = (0, -1)


def _dyadic(rng, shape):
    return (rng.integers(0, 65, size=shape).astype(f32) / f32(64.0)).astype(f32)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of CASES[name] as read-only numpy arrays: feats [2,3,H,W], s / t [R,H,W] (dyadic), target uint8, img int64, inter per
    level ([N_l,2,H,W] in the competing range of tests/mf_decided.py, or None), level_rows, ks, iters, base."""
    H, W, ks, iters, level_rows, given, kind = CASES[name]
    R = sum(level_rows)
    rng = np.random.default_rng(H * 1000 + W + 7 * len(name))
    yy, xx = np.mgrid[0:H, 0:W]
    feats = np.stack([np.stack([np.sin(xx / (7.0 + b)) + 0.3 * np.cos(yy / 5.0), np.cos(xx / 9.0 + yy / 11.0), 0.5 * np.sin(yy / (4.0 + b))])
                      for b in range(2)])
    feats = (feats + 0.05 * rng.standard_normal(feats.shape)).astype(f32)
    s, t = _dyadic(rng, (R, H, W)), _dyadic(rng, (R, H, W))
    target = np.zeros((R, H, W), np.uint8)
    if kind == 'edges':
        spots = [(r, c) for r in EDGE_LINES for c in EDGE_COLUMNS] + [(H // 2, c) for c in EDGE_COLUMNS]
        for i in range(R):
            r, c = spots[i % len(spots)]
            target[i, r, c] = 1
    elif kind != 'all_dead':
        for i in range(R):
            r0, c0 = int(rng.integers(0, max(H // 2, 1))), int(rng.integers(0, max(W // 2, 1)))
            target[i, r0:r0 + int(rng.integers(2, H // 2 + 2)), c0:c0 + int(rng.integers(2, W // 2 + 2))] = 1
        target[0] = 1                                                      # one target covers the map: the dilation is clipped on all sides
        if kind == 'dead':
            for i in (0, R // 2, R - 1):
                target[i] = 0
    # high student / teacher scores inside the targets, so that the initial state is not empty and the iterations have something to move
    inside = target != 0
    s = np.where(inside & (rng.random(s.shape) < 0.7), np.maximum(s, f32(0.75)), s).astype(f32)
    t = np.where(inside & (rng.random(t.shape) < 0.7), np.maximum(t, f32(0.75)), t).astype(f32)
    img = rng.integers(0, 2, size=R).astype(np.int64)
    inter = [(rng.uniform(0, 0.1, size=(n, 2, H, W)).astype(f32) if g and n else None) for n, g in zip(level_rows, given)]
    d = dict(name=name, H=H, W=W, R=R, ks=ks, iters=iters, base=0.1, level_rows=list(level_rows), feats=feats, s=s, t=t, target=target, img=img,
             inter=inter)
    for v in [feats, s, t, target, img] + [x for x in inter if x is not None]:
        v.setflags(write=False)
    return d


def inter_cat(d):
    """The levels' inter_img_mask concatenated, zeros for a level whose pointer is null: what MeanField.forward gets in the reference."""
    parts = [(np.zeros((n, 2, d['H'], d['W']), f32) if x is None else x) for n, x in zip(d['level_rows'], d['inter']) if n]
    return np.concatenate(parts) if parts else np.zeros((0, 2, d['H'], d['W']), f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/golden/discobox_loss.npz (tests/golden/make_golden_discobox_loss.py: the reference's own statements in fp32 and fp64)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'discobox_loss.npz')
FIXTURE_CASES = ('k3', 'k3_short')
TOL_FACTOR = 4.0                 # the project's rule: 4 x the reference's own fp32-against-fp64 difference


@functools.lru_cache(maxsize=None)
def fixture(name):
    """Case ``name`` of the fixture as a dict of read-only numpy arrays (inputs, fp64 results, tol_*), plus gamma and the mean-field settings."""
    with np.load(FIXTURE) as z:
        d = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        d['gamma'] = float(z['gamma'])
        d['mf'] = {k.split('/', 1)[1]: float(z[k]) for k in z.files if k.startswith('mf/')}
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def within(got, want, tol, what):
    """|got - want| <= TOL_FACTOR * tol * max|want|: ``tol`` is the fixture's relative fp32-against-fp64 difference of that quantity."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, bound = float(np.abs(got - want).max()), TOL_FACTOR * float(tol) * float(np.abs(want).max())
    print(f'{what}: differs by {err:.3e}, bound {bound:.3e}')
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e}'
