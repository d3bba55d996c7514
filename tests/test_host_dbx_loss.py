"""Host side of the DiscoBox pseudo-label block (boxinstseg_amd/discobox_loss.py, csrc/discobox_loss.hip).  No GPU needed.

* a census: every case of tests/dbx_loss_ref.py reaches the path it is named for (word counts, partial words, edge pixels, dead rows,
  the level table, the side of MF_MANY_ITEMS), and its competing inter_img_mask moves labels of the oracle's mean field;
* the torch restatement: its fp32 form is the reference's statement, and the fp64 form the tests hold the kernels to lies within the
  stated bounds of it; the dilation of a bit mask is F.max_pool2d's;
* parse_discobox_loss_cfg accepts the bbox_head block of every configs/discobox file unchanged (tests/golden/solo_head_cfg.json);
* the exports, the header's statements and the documents."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import dbx_loss_ref as R
from tests import mf_decided as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [n for n in R.CASES if n != 'many']


def test_census_of_the_cases():
    from boxinstseg_amd import _lib
    seen_w = set()
    for name in R.CASES:
        d = R.case(name)
        H, W, Rr = d['H'], d['W'], d['R']
        assert d['s'].shape == d['t'].shape == d['target'].shape == (Rr, H, W) and sum(d['level_rows']) == Rr
        for v in (d['s'], d['t']):                                         # dyadic: multiples of 2^-6 in [0, 1]
            assert v.dtype == np.float32 and np.array_equal(v * 64, np.round(v * 64)) and v.min() >= 0 and v.max() <= 1
        seen_w.add((W < 64, W % 64 == 0, W > 64))
        assert (Rr * H * ((W + 63) // 64) > _lib.MF_MANY_ITEMS) == (name == 'many')
    assert seen_w == {(True, False, False), (False, True, False), (False, True, True), (False, False, True)}
    assert {R.CASES[n][3] for n in R.CASES} == {0, 1, 10} and {R.CASES[n][2] for n in R.CASES} == {3, 5}
    e = R.case('edges')
    cols, lines = set(), set()
    for i in range(e['R']):
        r, c = np.flatnonzero(e['target'][i].any(1)), np.flatnonzero(e['target'][i].any(0))
        assert r.size == 1 and c.size == 1
        cols.add(int(c[0])); lines.add(int(r[0]))
    assert cols == {0, 63, 64, e['W'] - 1} and {0, e['H'] - 1} <= lines
    dead = R.case('dead')
    live = dead['target'].reshape(dead['R'], -1).any(1)
    assert not live[0] and not live[-1] and not live[dead['R'] // 2] and live.sum() == dead['R'] - 3
    assert not R.case('all_dead')['target'].any() and R.case('r1')['R'] == 1
    gap = R.case('level_gap')
    assert gap['level_rows'] == [2, 0, 2, 1] and [x is None for x in gap['inter']] == [False, True, True, False]


@pytest.mark.parametrize('name', ['w70', 'w13', 'level_gap'])
def test_the_competing_mask_moves_labels(name):
    """Leg 1 is not a copy of leg 0 on these inputs: the oracle's trajectories with and without inter_img_mask end differently, and leg 0
    ends with labels set."""
    from oracle import discobox_oracle as do
    d = R.case(name)
    Ko = np.stack([do.meanfield_kernel(d['feats'][b], d['ks'], 2.0, 0.5, 30.0) for b in range(2)])
    x = ((d['t'] + d['s']) * np.float32(0.5)).astype(np.float32)
    s0, _ = D.trajectory_by_image(Ko, d['img'], x, d['target'], d['iters'], d['base'])
    s1, _ = D.trajectory_by_image(Ko, d['img'], x, d['target'], d['iters'], d['base'], R.inter_cat(d), R.GAMMA)
    assert s0[-1].any() and (s0[-1] != s1[-1]).any()


@pytest.mark.parametrize('name', SMALL)
def test_restatement_fp32_against_fp64(name):
    d = R.case(name)
    rng = np.random.default_rng(3)
    target = torch.from_numpy(d['target'].copy())
    inside = target != 0
    pseudo = (torch.from_numpy(rng.random(d['s'].shape) < 0.5) & inside).to(torch.uint8)
    pseudo_corr = (torch.from_numpy(rng.random(d['s'].shape) < 0.5) & inside).to(torch.uint8)
    out = {}
    for dtype in (torch.float32, torch.float64):
        s = torch.from_numpy(d['s'].copy()).to(dtype).requires_grad_(True)
        ts, tsc = R.terms(s, target, pseudo, pseudo_corr, dtype=dtype)
        (g,) = torch.autograd.grad(ts.sum() + 2.0 * tsc.sum(), s)
        out[dtype] = (ts.detach().double(), tsc.detach().double(), g.double())
    a, b = out[torch.float32], out[torch.float64]
    # torch's fp32 sums over a map carry more than one rounding: the restatements agree to the sums' own error, far below any label flip
    assert float((a[0] - b[0]).abs().max()) <= 1e-5 and float((a[1] - b[1]).abs().max()) <= 1e-5
    assert float((a[2] - b[2]).abs().max()) <= 1e-5 * max(float(b[2].abs().max()), 1e-30)
    # the gradient of leg 1 carries the factor gamma, and nothing flows where the enlarged target is zero
    s = torch.from_numpy(d['s'].copy()).double().requires_grad_(True)
    _, tsc = R.terms(s, target, pseudo, pseudo_corr)
    (g1,) = torch.autograd.grad(tsc.sum(), s)
    e = R.enlarged_of(target)
    assert not bool(g1[e == 0].any())
    a0 = (s.detach() * e.double()).requires_grad_(True)
    plain = R.dice_loss(a0 * 1.0, pseudo_corr.double())
    (gp,) = torch.autograd.grad(plain.sum(), a0)
    scale = max(float(gp.abs().max()), 1e-30)
    assert float((g1 - float(np.float32(R.GAMMA)) * gp * e.double()).abs().max()) <= 1e-6 * scale     # a1 differs from a0 by fp32 roundings only


@pytest.mark.parametrize('name', R.FIXTURE_CASES)
def test_restatement_reproduces_the_fixture(name):
    """tests/golden/discobox_loss.npz holds what the reference's own statements give in fp64; the restatement, on the fixture's inputs and
    labels, gives the same rows, means and gradient (fp64 against fp64: only the order of sums differs), and its labels are the oracle's
    trajectory on x = (t + s) / 2 with no undecided pixel on the way."""
    from oracle import discobox_oracle as do
    f = R.fixture(name)
    target = torch.from_numpy(f['target'].copy())
    live = R.live_of(target)
    assert np.array_equal(live.numpy(), f['live'] != 0) and int(f['level_rows'].sum()) == target.shape[0]
    for v in (f['s'], f['t'], f['feats'], f['inter']):
        assert np.array_equal(v, v.astype(np.float16).astype(np.float32))                        # fp16-exact inputs
    s = torch.from_numpy(f['s'].copy()).double().requires_grad_(True)
    ts, tsc = R.terms(s, target, torch.from_numpy(f['pseudo'].copy()), torch.from_numpy(f['pseudo_corr'].copy()), gamma=f['gamma'])
    lv = live.double()
    n = max(int(live.sum()), 1)
    mean_ts, mean_tsc = (ts * lv).sum() / n, (tsc * lv).sum() / n
    (g,) = torch.autograd.grad(mean_ts + mean_tsc, s)
    # the one thing the fp64 restatement keeps in fp32 is the gamma mix (three fp32 roundings, as the fp32 reference has them): 2^-23 on leg 1
    assert float(((ts.detach() - torch.from_numpy(f['ts_rows'])) * lv).abs().max()) <= 1e-12
    assert float(((tsc.detach() - torch.from_numpy(f['ts_corr_rows'])) * lv).abs().max()) <= 2.0 ** -23
    assert abs(float(mean_ts) - float(f['mean_ts'])) <= 1e-12 and abs(float(mean_tsc) - float(f['mean_ts_corr'])) <= 2.0 ** -23
    assert abs(float(f['loss_ts']) - (float(f['mean_ts']) + float(f['mean_ts_corr']))) <= 1e-12
    assert float((g - torch.from_numpy(f['grad'])).abs().max()) <= 2.0 ** -23 * float(np.abs(f['grad']).max())
    assert not f['grad'][f['live'] == 0].any() and not f['pseudo'][f['live'] == 0].any()
    # labels: the oracle's trajectory, decided everywhere, the legs differ
    Ko = np.stack([do.meanfield_kernel(f['feats'][b], int(f['ks']), f['mf']['alpha0'], f['mf']['theta0'], f['mf']['theta1']) for b in range(f['feats'].shape[0])])
    x = ((f['t'] + f['s']) / np.float32(2)).astype(np.float32)
    for key, inter in (('pseudo', None), ('pseudo_corr', f['inter'])):
        states, undecided = D.trajectory_by_image(Ko, f['img'], x, f['target'], int(f['iters']), f['mf']['base'], inter, f['gamma'])
        assert not any(u.any() for u in undecided) and np.array_equal(states[-1], f[key] != 0), key
    assert (f['pseudo'] != f['pseudo_corr']).any() and f['pseudo'].any()
    for k in ('tol_ts_rows', 'tol_ts_corr_rows', 'tol_mean_ts', 'tol_mean_ts_corr', 'tol_grad', 'tol_mil_rows'):
        assert 0 < float(f[k]) < 1e-6, k


def test_dilation_of_bits_is_max_pool():
    rng = np.random.default_rng(11)
    t = torch.from_numpy((rng.random((5, 9, 70)) < 0.05).astype(np.uint8))
    want = R.enlarged_of(t).numpy().astype(bool)
    b = t.numpy().astype(bool)
    pad = np.zeros((5, 11, 72), bool)
    pad[:, 1:-1, 1:-1] = b
    got = np.zeros_like(b)
    for dy in range(3):
        for dx in range(3):
            got |= pad[:, dy:dy + 9, dx:dx + 70]
    assert np.array_equal(got, want)


def test_reference_loss_blocks_are_accepted():
    import boxinstseg_amd as B
    import importlib
    M = importlib.import_module('boxinstseg_amd.discobox_loss')           # the package attribute of that name is the function
    with open(os.path.join(ROOT, 'tests', 'golden', 'solo_head_cfg.json')) as fh:
        blocks = {k: v for k, v in json.load(fh).items() if k.startswith('discobox/')}
    assert len(blocks) == 4
    for fname, block in blocks.items():
        before = json.dumps(block, sort_keys=True)
        s = B.parse_discobox_loss_cfg(block)
        assert json.dumps(block, sort_keys=True) == before
        assert s == dict(w_ins=1.0, w_ts=1.0, w_corr=1.0, kernel=3, max_iter=10, alpha0=2.0, theta0=0.5, theta1=30.0, theta2=20.0, base=0.1), fname
        ns = types.SimpleNamespace(**block)
        assert B.parse_discobox_loss_cfg(ns) == s
        B.parse_solo_head_cfg(block); B.parse_corr_cfg(block)              # the three parsers discobox_loss runs on one block
    block = next(iter(blocks.values()))
    with pytest.raises(TypeError, match='loss_ts'):
        B.parse_discobox_loss_cfg({k: v for k, v in block.items() if k != 'loss_ts'})
    with pytest.raises(NotImplementedError, match='kernel'):
        B.parse_discobox_loss_cfg(dict(block, loss_ts=dict(block['loss_ts'], kernel=7)))
    with pytest.raises(RuntimeError, match='base'):
        B.parse_discobox_loss_cfg(dict(block, loss_ts=dict(block['loss_ts'], base=0.5)))
    for name in ('discobox_loss', 'discobox_pseudo_losses', 'live_means', 'parse_discobox_loss_cfg'):
        assert name in B.__all__ and getattr(B, name) is getattr(M, name) and name in B.__doc__


def test_header_source_and_documents_say_the_same():
    from boxinstseg_amd import _lib, build
    with open(os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_dbx.h')) as fh:
        header = fh.read()
    assert f'#define BXI_DBX_MAX_LEVELS {_lib.DBX_MAX_LEVELS}' in header and f'#define BXI_DBX_MAX_MEANS {_lib.DBX_MAX_MEANS}' in header
    assert 'discobox_loss.hip' in build.SOURCES and 'meanfield_device.hpp' in build.HEADERS
    with open(os.path.join(ROOT, 'boxinstseg_amd', 'csrc', 'discobox_loss.hip')) as fh:
        code = fh.read()
    with open(os.path.join(ROOT, 'boxinstseg_amd', 'csrc', 'meanfield.hip')) as fh:
        mf = fh.read()
    # ONE copy of the mean-field arithmetic: both translation units include it, neither restates it
    for text in (code, mf):
        assert '#include "meanfield_device.hpp"' in text and 'nl_hi0 : a.nl_lo0' not in text
    assert 'mf_eval_loaded<KS>' in code and 'atomic' not in code.replace('no atomics', '') and 'hipMemset' not in code and 'hipMalloc' not in code
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3q', 'discobox_loss', 'discobox_pseudo_losses', 'parse_discobox_loss_cfg', 'bxi_dbx_steps_f32', '0-dim'):
        assert word in integration, word
    with open(os.path.join(ROOT, 'README.md')) as fh:
        assert 'discobox_loss' in fh.read()
    with open(os.path.join(ROOT, 'DESIGN_NEXT_ROWS.md')) as fh:
        assert '3.13' in fh.read()
