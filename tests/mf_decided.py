"""Which MeanField labels are decided: the oracle's step, evaluated again at the two corners of what the device may compute differently.

TEST INFRASTRUCTURE ONLY (numpy; imported by tests/test_host_meanfield_decided.py, tests/test_gpu_meanfield_paths.py and the MeanField
comparisons of tests/test_gpu_discobox.py / tests/test_gpu_guarded_modules.py).

csrc/meanfield.hip follows the fp32 operation order of oracle/discobox_oracle.py::meanfield_step exactly; only two things may differ:

* the four level values -log(1 - x), -log(x) for x = lo / hi are computed on the host with logf, the oracle uses numpy's log.  On the
  build host the two differ by ONE ulp in two of the values in use (-log(hi) at base 0.1, -log(1 - lo) at base 0.3; see
  test_host_meanfield_decided.py::test_level_values_logf_against_numpy, which prints them).  Hence LEVEL_ULP = 1.
* expf on the device.  HIP documents expf at 1 ulp; doubled, EXP_ULP = 2.  The nudge is applied to exp(-acc) before inter * gamma is
  added (every later operation is a correctly rounded fp32 operation on both sides).

K >= 0, so acc is monotone in the levels, f = exp(-acc) is monotone in acc and r1 = f1 / (f0 + f1) is monotone in f0 (down) and f1 (up):
moving channel 0 one way and channel 1 the other way by the full amounts bounds every combination.  The two corners are therefore
  'low'  : channel 0 -> larger f0 (levels -LEVEL_ULP, exp +EXP_ULP), channel 1 -> smaller f1 (levels +LEVEL_ULP, exp -EXP_ULP)
  'high' : the opposite.
A pixel of the target where a corner decides differently from the middle is UNDECIDED: a device result may differ from the oracle there
and nowhere else.  (A margin on |r1 - 0.5| is the wrong yardstick: with a 5x5 kernel exp(-acc) is 1e-9..1e-13 against the +1e-6, most
in-target pixels sit within 1e-6 of 0.5 and are still perfectly robust, because the ulp of 1e-6 swallows any expf difference.)
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from oracle import discobox_oracle as do

f32 = np.float32
LEVEL_ULP = 1       # host logf against numpy log
EXP_ULP = 2         # HIP's documented 1 ulp of expf, doubled


def _nudge(a, ulps: int):
    """a moved by `ulps` fp32 steps (towards +inf if positive)."""
    a = np.asarray(a, f32)
    to = f32(np.inf) if ulps > 0 else f32(-np.inf)
    for _ in range(abs(int(ulps))):
        a = np.nextafter(a, to, dtype=f32)
    return a


def _step(K, state, targets, base, inter, gamma, level_ulps=(0, 0), exp_ulps=(0, 0)):
    """discobox_oracle.meanfield_step over all instances at once, with channel c's levels moved by level_ulps[c] and its exp(-acc) by
    exp_ulps[c] fp32 steps -> (decisions, r1).  Elementwise fp32 operations in the oracle's order: with (0, 0), (0, 0) bit for bit the oracle's."""
    n, H, W = state.shape
    ks = int(round(np.sqrt(K.shape[0])))
    half = ks // 2
    _, _, nl = do.state_levels(base)
    t = targets.astype(f32)
    f = []
    for c in range(2):
        hi, lo = _nudge(nl['hi'][c], level_ulps[c]), _nudge(nl['lo'][c], level_ulps[c])
        pad = np.zeros((n, H + 2 * half, W + 2 * half), f32)
        pad[:, half:half + H, half:half + W] = np.where(state, hi, lo).astype(f32)
        acc = np.zeros((n, H, W), f32)
        for k in range(ks * ks):
            dy, dx = k // ks - half, k % ks - half
            acc = (acc + (pad[:, half + dy:half + dy + H, half + dx:half + dx + W] * K[k]).astype(f32)).astype(f32)
        fc = _nudge(np.exp((-acc).astype(f32)).astype(f32), exp_ulps[c])
        if inter is not None:
            fc = (fc + (inter[:, c].astype(f32) * f32(gamma)).astype(f32)).astype(f32)
        f.append(fc)
    f[1] = (f[1] * t).astype(f32)
    f = [(v + f32(1e-6)).astype(f32) for v in f]
    r1 = (f[1] / (f[0] + f[1]).astype(f32)).astype(f32)
    return r1 > f32(0.5), r1


def step_with_corners(K, state, targets, base, inter=None, gamma=0.01):
    """One mean-field step -> (new_state [n,H,W] bool, undecided [n,H,W] bool).

    new_state is discobox_oracle.meanfield_step's (the middle evaluation); undecided marks the in-target pixels where one of the two
    corners (module docstring: levels +-LEVEL_ULP = 1 ulp because host logf and numpy log differ by that much, exp(-acc) +-EXP_ULP = 2 ulp
    because HIP documents expf at 1 ulp, doubled; channel 0 against channel 1) decides differently."""
    mid, _ = _step(K, state, targets, base, inter, gamma)
    low, _ = _step(K, state, targets, base, inter, gamma, (-LEVEL_ULP, +LEVEL_ULP), (+EXP_ULP, -EXP_ULP))
    high, _ = _step(K, state, targets, base, inter, gamma, (+LEVEL_ULP, -LEVEL_ULP), (-EXP_ULP, +EXP_ULP))
    undecided = ((low != mid) | (high != mid)) & (np.asarray(targets) != 0)
    return mid, undecided


def trajectory(K, x, t, iters, base, inter=None, gamma=0.01):
    """MeanField.forward along the oracle's (middle) states -> (states: iters + 1 bool arrays [n,H,W], undecided_per_step: iters bool arrays;
    undecided_per_step[k] belongs to the step states[k] -> states[k + 1])."""
    tf = np.asarray(t).astype(f32)
    states = [(np.asarray(x).astype(f32) * tf).astype(f32) > f32(0.5)]
    undecided = []
    for _ in range(iters):
        s, u = step_with_corners(K, states[-1], tf, base, inter, gamma)
        states.append(s); undecided.append(u)
    return states, undecided


def trajectory_by_image(Ko, img, x, t, iters, base, inter=None, gamma=0.01):
    """trajectory() for instances spread over several kernel planes: Ko [B,k*k,H,W], img [n] -> as trajectory()."""
    n = x.shape[0]
    states = [np.zeros(x.shape, bool) for _ in range(iters + 1)]
    undecided = [np.zeros(x.shape, bool) for _ in range(iters)]
    for b in range(Ko.shape[0]):
        m = np.asarray(img) == b
        if m.any():
            s, u = trajectory(Ko[b], x[m], t[m], iters, base, None if inter is None else inter[m], gamma)
            for k in range(iters + 1):
                states[k][m] = s[k]
            for k in range(iters):
                undecided[k][m] = u[k]
    assert n == 0 or len(states) == iters + 1
    return states, undecided


def assert_steps(run, t, states, undecided, tag=''):
    """One step at a time.  run(x [n,H,W] float32, iters) -> (ret, valid) as numpy arrays is the call under test.  From x = states[k] one
    step has to give states[k + 1] on every decided pixel and 0 outside the target; only undecided pixels may differ."""
    inside = np.asarray(t) != 0
    for k in range(len(undecided)):
        got, _ = run(states[k].astype(f32), 1)
        assert got.dtype == np.float32 and ((got == 0) | (got == 1)).all(), f'{tag}: step {k}: values other than 0 / 1'
        assert not got[~inside].any(), f'{tag}: step {k}: {int((got[~inside] != 0).sum())} labels set outside the target'
        wrong = ((got != 0) != states[k + 1]) & ~undecided[k]
        assert not wrong.any(), (f'{tag}: step {k}: {int(wrong.sum())} decided labels differ, the first at (instance, row, column) '
                                 f'{tuple(int(v) for v in np.argwhere(wrong)[0])}')


def assert_labels(run, x, t, states, undecided, tag=''):
    """The whole call.  Where the trajectory has no undecided pixel, ret and valid are the oracle's on every pixel; otherwise the full call
    cannot be pinned (an undecided pixel feeds the next step) and the steps are compared one at a time."""
    iters = len(undecided)
    if any(u.any() for u in undecided):
        assert_steps(run, t, states, undecided, tag)
        return
    got, valid = run(x, iters)
    assert got.dtype == np.float32
    bad = got != states[-1].astype(f32)
    assert not bad.any(), (f'{tag}: {int(bad.sum())} of {bad.size} labels differ, the first at (instance, row, column) '
                           f'{tuple(int(v) for v in np.argwhere(bad)[0])}')
    assert np.array_equal(valid, valid_of(states[-1])), f'{tag}: valid'


def valid_of(state):
    """MeanField.forward's `valid` (:633-636) of a final state, as the oracle computes it."""
    ret = state.astype(f32)
    count = ret.reshape(ret.shape[0], -1).sum(1).astype(f32)
    hw = ret.shape[1] * ret.shape[2]
    return ((count >= f32(hw * 0.05)) & (count <= f32(hw * 0.95))).astype(f32)


# -----------------------------------------------------------------------------------------------------------------------------------
# the inputs of the six cases (and of test_meanfield_vs_oracle / test_meanfield_guarded, whose recipe this is)
def recipe(n, H, W, ks, with_inter=False):
    """Features of two images, their oracle kernels, x, box targets (t[0] covers the map), img_inds and optionally inter_img_mask in
    uniform(0, 20), drawn from default_rng(H * 1000 + W) in the order test_meanfield_vs_oracle / test_meanfield_guarded draw them."""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    feats = []
    for b in range(2):
        f = np.stack([np.sin(xx / (7.0 + b)) + 0.3 * np.cos(yy / 5.0), np.cos(xx / 9.0 + yy / 11.0), 0.5 * np.sin(yy / (4.0 + b))])
        feats.append((f + 0.05 * rng.standard_normal(f.shape)).astype(np.float32))
    feats = np.stack(feats)
    Ko = np.stack([do.meanfield_kernel(feats[b], ks, 2.0, 0.5, 30.0) for b in range(2)])
    x = rng.uniform(0, 1, size=(n, H, W)).astype(np.float32)
    t = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        r0, c0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
        t[i, r0:r0 + int(rng.integers(4, H // 2 + 1)), c0:c0 + int(rng.integers(4, W // 2 + 1))] = 1
    t[0, :, :] = 1
    img = rng.integers(0, 2, size=n)
    inter = rng.uniform(0, 20, size=(n, 2, H, W)).astype(np.float32) if with_inter else None
    return dict(feats=feats, Ko=Ko, x=x, t=t, img=img, inter=inter)


def fuzz_recipe(seed):
    """The inputs of test_meanfield_fuzz[seed], drawn from default_rng(4000 + seed) in that test's order."""
    rng = np.random.default_rng(4000 + seed)
    H = int(rng.integers(2, 60)); W = int(rng.choice([1, 5, 63, 64, 65, 127, 128, 129, int(rng.integers(2, 200))]))
    ks = int(rng.choice([3, 3, 5])); iters = int(rng.integers(0, 12)); base = float(rng.choice([0.05, 0.1, 0.3, 0.45]))
    n = int(rng.integers(1, 9)); B = int(rng.integers(1, 3))
    yy, xx = np.mgrid[0:H, 0:W]
    feats = np.stack([np.stack([np.sin(xx / (5.0 + b)), np.cos(yy / 6.0 + xx / 9.0), 0.3 * np.sin(yy / 3.0)]) for b in range(B)])
    feats = (feats + 0.1 * rng.standard_normal(feats.shape)).astype(np.float32)
    Ko = np.stack([do.meanfield_kernel(feats[b], ks, 2.0, 0.5, 30.0) for b in range(B)])
    x = rng.uniform(0, 1, size=(n, H, W)).astype(np.float32)
    t = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            continue                                   # no target
        if kind == 1:
            t[i] = 1                                   # everything
        elif kind == 2:
            t[i, int(rng.integers(0, H)), :] = 1       # one row
        else:
            r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            t[i, r0:r0 + int(rng.integers(1, H + 1)), c0:c0 + int(rng.integers(1, W + 1))] = 1
    img = rng.integers(0, B, size=n)
    inter = rng.uniform(0, 20, size=(n, 2, H, W)).astype(np.float32) if rng.integers(0, 2) else None
    return dict(feats=feats, Ko=Ko, x=x, t=t, img=img, inter=inter, n=n, H=H, W=W, ks=ks, iters=iters, base=base, gamma=0.01)


# the parameter sets of the existing comparisons (H, W, n, ks, iters, base)
VS_ORACLE_PARAMS = [(100, 136, 12, 3, 10, 0.10), (200, 304, 6, 3, 10, 0.10), (64, 64, 3, 5, 3, 0.45), (37, 65, 4, 3, 0, 0.10), (50, 129, 5, 3, 1, 0.30)]
GUARDED_PARAMS = [(37, 65, 4, 3, 2, 0.10), (20, 128, 5, 5, 3, 0.45), (100, 136, 6, 3, 4, 0.10)]
FUZZ_SEEDS = list(range(10))


# inter_img_mask * gamma against exp(-acc): uniform(0, 20) * 0.01 is 0 .. 0.2 and swamps a 3x3 exp(-acc) almost everywhere, so the
# stencil stops moving the state after two steps.  The competing range is INTER_COMPETING_HI * 0.01 = 0 .. 1e-3, the size of exp(-acc)
# where about seven level * K products of ~1 meet (e^-7 ~ 1e-3): the stencil and the mask then both decide pixels at every step.
INTER_COMPETING_HI = 0.1

# name -> (N, H, W, ks, iters, base, inter): None, 'swamping' (uniform(0, 20), the existing tests' range) or 'competing'
CASES = {
    'k5_small': (3, 64, 64, 5, 3, 0.45, None),
    'k5_many_010': (300, 110, 37, 5, 3, 0.10, None),
    'k5_many_030': (300, 110, 37, 5, 3, 0.30, None),
    'k3_many_045': (70, 157, 130, 3, 4, 0.45, None),
    'k3_many_010_inter': (70, 157, 130, 3, 4, 0.10, 'swamping'),
    'k3_many_010_inter_competing': (70, 157, 130, 3, 4, 0.10, 'competing'),
    'k3_many_word': (130, 255, 64, 3, 3, 0.30, None),
    'k3_threshold': (129, 256, 64, 3, 2, 0.10, None),      # its first 128 instances are exactly MF_MANY_ITEMS items: one item per wave
}


FULL = ['k5_many_010', 'k3_many_045', 'k3_many_word']       # the shapes of full_case(): one, three and exactly one full segment per row


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of CASES[name] with the oracle's trajectory: computed once per session, shared, read-only."""
    n, H, W, ks, iters, base, kind = CASES[name]
    d = recipe(n, H, W, ks, with_inter=kind is not None)
    if kind == 'competing':
        d['inter'] = (d['inter'] * f32(INTER_COMPETING_HI / 20.0)).astype(f32)
    d.update(n=n, H=H, W=W, ks=ks, iters=iters, base=base, gamma=0.01)
    d['states'], d['undecided'] = trajectory_by_image(d['Ko'], d['img'], d['x'], d['t'], iters, base, d['inter'], 0.01)
    d['valid'] = valid_of(d['states'][-1])
    for v in list(d.values()) + d['states'] + d['undecided']:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def full_case(name):
    """The kernels and img_inds of CASES[name] with x = 1 and a target that covers every map.  An all-set state stays all-set: with every
    neighbour at `hi`, acc0 - acc1 = (-log(1 - hi) + log(hi)) * sum(K) >= 0.2 * K[centre] = 0.4 even at base 0.45, so f1 / f0 >= e^0.4 before
    the +1e-6 and r1 > 0.5 far from any rounding.  Every (instance, row, segment) word therefore has to be written with all its bits at every
    step: an item that a launch leaves out shows as zeros, whatever the boxes of recipe() happen to cover.  Two steps, so that both state
    buffers are read."""
    n, H, W, ks, _, base, _ = CASES[name]
    d = dict(case(name))
    d.update(x=np.ones((n, H, W), f32), t=np.ones((n, H, W), np.uint8), inter=None, iters=2)
    d['states'], d['undecided'] = trajectory_by_image(d['Ko'], d['img'], d['x'], d['t'], 2, base)
    d['valid'] = valid_of(d['states'][-1])
    for v in [d['x'], d['t']] + d['states'] + d['undecided']:
        v.setflags(write=False)
    return d


def hip_many_items():
    """kMfManyItems as csrc/meanfield.hip states and uses it."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'boxinstseg_amd/csrc/meanfield.hip')) as fh:
        code = fh.read()
    assert 'N * H * a.segs > bxi::kMfManyItems' in code
    found = re.search(r'constexpr int kMfManyItems = (\d+);', code)
    assert found, 'csrc/meanfield.hip does not give kMfManyItems as a plain number'
    return int(found.group(1))


def summary(t, states, undecided):
    """Per step: (in-target pixels, pixels the step changed, undecided pixels)."""
    inside = int((np.asarray(t) != 0).sum())
    return [(inside, int((states[k + 1] != states[k]).sum()), int(undecided[k].sum())) for k in range(len(undecided))]
