"""CPU: which MeanField labels the device has to reproduce exactly (tests/mf_decided.py; no kernel is launched here).

* the middle evaluation of step_with_corners is oracle/discobox_oracle.py::meanfield_step bit for bit;
* on the eight inputs of tests/test_gpu_meanfield_paths.py and on every parameter set of test_meanfield_vs_oracle, test_meanfield_fuzz and
  test_meanfield_guarded the share of undecided pixels per step is capped (printed with -s; measured: 0 everywhere), so those tests may
  and do ask for every label;
* the inputs are not vacuous: the stencil moves the state, the final state is neither empty nor the whole target, and with an
  inter_img_mask the state still moves after the first step;
* csrc/meanfield.hip's kMfManyItems is _lib.MF_MANY_ITEMS and the many-item inputs lie on the side of it they were made for;
* printed only: which level values differ between libm's logf and numpy's log on this host (the reason for the level nudge)."""
import ctypes

import numpy as np
import pytest

from oracle import discobox_oracle as do
from tests import mf_decided as M

f32 = np.float32
UNDECIDED_CAP = 1e-3        # share of the in-target pixels, per step


def _report(tag, rows):
    for k, (inside, moved, undecided) in enumerate(rows):
        print(f'{tag}: step {k}: {inside} in-target pixels, {moved} changed, {undecided} undecided')
        assert undecided <= UNDECIDED_CAP * inside, f'{tag}: step {k}: {undecided} of {inside} in-target pixels are undecided'


@pytest.mark.parametrize('ks,base,with_inter', [(3, 0.10, False), (3, 0.30, True), (5, 0.45, False), (5, 0.05, True)])
def test_middle_is_the_oracle_step(ks, base, with_inter):
    d = M.recipe(4, 23, 70, ks, with_inter=with_inter)
    K, t = d['Ko'][1], d['t'].astype(f32)
    inter = None if d['inter'] is None else (d['inter'] * f32(M.INTER_COMPETING_HI / 20.0)).astype(f32)
    state = (d['x'] * t).astype(f32) > f32(0.5)
    for k in range(3):
        want, margin = do.meanfield_step(K, state, t, base, inter, 0.01)
        got, r1 = M._step(K, state, t, base, inter, 0.01)
        assert np.array_equal(got, want)
        assert np.array_equal(np.abs(r1 - f32(0.5)).view(np.uint32), margin.view(np.uint32))       # bit for bit
        new, undecided = M.step_with_corners(K, state, t, base, inter, 0.01)
        assert np.array_equal(new, want) and undecided.shape == want.shape and not undecided[t == 0].any()
        assert k > 0 or (new != state).any()
        state = new


def test_corners_see_a_planted_tie():
    """A pixel whose two channels are equal up to the nudges is reported; one whose channels are far apart is not.  K = 0 makes exp(-acc) = 1
    for both channels, so r1 = (1 + 1e-6) / (2 + 2e-6) is 0.5 exactly in the middle and the corners fall on either side of it."""
    K = np.zeros((9, 4, 5), f32)
    state = np.zeros((1, 4, 5), bool)
    t = np.ones((1, 4, 5), f32); t[0, 0, 0] = 0
    new, undecided = M.step_with_corners(K, state, t, 0.1)
    assert not new.any() and undecided[0, 0, 0] == False and undecided[t != 0].all()               # noqa: E712
    inter = np.zeros((1, 2, 4, 5), f32); inter[0, 1] = 50.0                                    # f1 = 1.5 against f0 = 1: decided
    new, undecided = M.step_with_corners(K, state, t, 0.1, inter, 0.01)
    assert new[t != 0].all() and not new[0, 0, 0] and not undecided.any()


@pytest.mark.parametrize('name', list(M.CASES))
def test_cases_are_decided_and_not_vacuous(name):
    d = M.case(name)
    n, H, W, ks, iters, base, kind = M.CASES[name]
    rows = M.summary(d['t'], d['states'], d['undecided'])
    _report(name, rows)
    inside = rows[0][0]
    assert len(rows) == iters and len(set(d['img'].tolist())) == 2
    assert max(moved for _, moved, _ in rows) >= 0.01 * inside
    final, target = d['states'][-1], d['t'] != 0
    assert final.any() and not np.array_equal(final, target) and not final[~target].any()
    want = np.zeros_like(d['x']); wv = np.zeros(n, f32)
    for b in range(2):                             # the oracle's own forward, not only the helper's restatement of it
        m = d['img'] == b
        want[m], wv[m] = do.meanfield_forward(d['Ko'][b], d['x'][m], d['t'][m], iters, base, None if d['inter'] is None else d['inter'][m], 0.01)
    assert np.array_equal(final.astype(f32), want) and np.array_equal(d['valid'], wv)
    assert 0 < wv.sum() < n or name == 'k5_many_010'
    print(f'{name}: final state {int(final.sum())} of {inside} in-target pixels, valid for {int(d["valid"].sum())} of {n} instances')
    if kind is not None:                           # the stencil still moves the state against the mask
        assert max(moved for _, moved, _ in rows[1:]) >= 0.001 * inside
    if kind == 'competing':                        # and goes on doing so: the swamping range stops after two steps
        assert all(moved > 0 for _, moved, _ in rows)
        swamped = M.summary(d['t'], *[M.case('k3_many_010_inter')[k] for k in ('states', 'undecided')])
        assert swamped[-1][1] == 0 and all(a[1] > b[1] for a, b in zip(rows[1:], swamped[1:]))


@pytest.mark.parametrize('name', M.FULL)
def test_an_all_set_state_stays_all_set(name):
    d = M.full_case(name)
    _report(f'{name} full', M.summary(d['t'], d['states'], d['undecided']))
    assert len(d['states']) == 3 and all(s.all() for s in d['states']) and not any(u.any() for u in d['undecided'])
    assert not d['valid'].any()                    # the whole map is more than 0.95 of it


@pytest.mark.parametrize('H,W,n,ks,iters,base', M.VS_ORACLE_PARAMS)
def test_vs_oracle_parameter_sets_are_decided(H, W, n, ks, iters, base):
    d = M.recipe(n, H, W, ks)
    _report(f'vs_oracle {H}x{W}', M.summary(d['t'], *M.trajectory_by_image(d['Ko'], d['img'], d['x'], d['t'], iters, base)))


@pytest.mark.parametrize('seed', M.FUZZ_SEEDS)
def test_fuzz_parameter_sets_are_decided(seed):
    d = M.fuzz_recipe(seed)
    _report(f'fuzz {seed} ({d["H"]}x{d["W"]} ks{d["ks"]} it{d["iters"]} base{d["base"]})',
            M.summary(d['t'], *M.trajectory_by_image(d['Ko'], d['img'], d['x'], d['t'], d['iters'], d['base'], d['inter'], 0.01)))


@pytest.mark.parametrize('H,W,n,ks,iters,base', M.GUARDED_PARAMS)
def test_guarded_parameter_sets_are_decided(H, W, n, ks, iters, base):
    d = M.recipe(n, H, W, ks, with_inter=True)
    for use_inter in (False, True):
        _report(f'guarded {H}x{W} inter={use_inter}', M.summary(d['t'], *M.trajectory_by_image(d['Ko'], d['img'], d['x'], d['t'], iters, base,
                                                                                                 d['inter'] if use_inter else None, 0.01)))
    _report(f'guarded {H}x{W} module', M.summary(d['t'], *M.trajectory(d['Ko'][0], d['x'], d['t'], iters, base)))


def test_many_item_threshold_is_the_library_s():
    from boxinstseg_amd import _lib
    assert M.hip_many_items() == _lib.MF_MANY_ITEMS
    items = {name: n * H * ((W + 63) // 64) for name, (n, H, W, *_) in M.CASES.items()}
    assert items['k5_small'] <= _lib.MF_MANY_ITEMS
    assert [items[k] for k in ('k5_many_010', 'k5_many_030', 'k3_many_045', 'k3_many_010_inter', 'k3_many_010_inter_competing', 'k3_many_word',
                               'k3_threshold')] == [33000, 33000, 32970, 32970, 32970, 33150, _lib.MF_MANY_ITEMS + 256]
    assert all(v > _lib.MF_MANY_ITEMS for k, v in items.items() if k != 'k5_small')


def test_level_values_logf_against_numpy():
    """Information only (run with -s): the level values where libm's logf and numpy's log differ on this host."""
    try:
        libm = ctypes.CDLL('libm.so.6')
    except OSError as e:
        print(f'no libm.so.6 on this host ({e}): nothing compared')
        return
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    for base in (0.05, 0.1, 0.3, 0.45):
        lo, hi, nl = do.state_levels(base)
        for name, x in (('lo', lo), ('hi', hi)):
            for c, arg in enumerate((f32(f32(1.0) - x), x)):
                host, ref = f32(-libm.logf(ctypes.c_float(float(arg)))), nl[name][c]
                steps = int(np.int64(host.view(np.int32)) - np.int64(ref.view(np.int32)))
                what = '-log(1 - %s)' % name if c == 0 else '-log(%s)' % name
                print(f'base {base}: {what:13s} logf {float(host)!r} numpy {float(ref)!r}' + (f'  differ by {steps} ulp' if steps else ''))
