"""Host side of the BoxLevelSet loss tests (no GPU): the restatement of tests/bls_loss_ref.py equals the reference's own statements
(tests/golden/box_solov2_loss.npz), the shared-per-(size, image) algebra of boxinstseg_amd/boxlevelset_loss.py equals the per-row
restatement in fp64, every case of tests/bls_cases.py reaches the path it is named for, no projection line of any case has a tie for its
largest logit, the ragged row order is what the module documents, and the trees of the cases that let the context build its own do not
hang on a rounding."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tree_filter_oracle as tfo
from tests import b2m_loss_ref as R2
from tests import bls_cases as K
from tests import bls_loss_ref as R


def _resize(x, size):
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False)


def shared_form(name, dtype=torch.float64):
    """The algebra of box_solov2_mask_losses in torch on the CPU: per size one resize of image and feature and one pair of trees per
    image, the image's rows of all the size's levels as channels of one tree filter, the means over the live rows -- no per-row copy."""
    d = K.inputs(name)
    sizes, group = K.groups_of(d['level_sizes'])
    B, L = d['B'], len(d['level_sizes'])
    preds = [torch.from_numpy(p).to(dtype).requires_grad_(True) for p in d['ins_preds']]
    lf = torch.from_numpy(d['lst_feat']).to(dtype).requires_grad_(True)
    img = torch.from_numpy(d['norm_img']).to(dtype)
    proj = [np.zeros(len(p)) for p in d['ins_preds']]
    levelset = [np.zeros(len(p)) for p in d['ins_preds']]
    all_proj, all_ls = [], []
    for g, size in enumerate(sizes):
        img_g, feat_g = _resize(img, size), _resize(lf, size)
        trees = d['trees'][g] if d['trees'] is not None else (R2.mst_trees(img_g), R2.mst_trees(feat_g))
        for b in range(B):
            rows = [(l, n) for l in range(L) if group[l] == g for n in range(len(d['tgt_of'][l]))
                    if d['img_of'][l][n] == b and d['tgt_of'][l][n] >= 0]
            if not rows:
                continue
            C = len(rows)
            p = torch.stack([torch.sigmoid(preds[l][n]) for l, n in rows])[:, None]
            T = torch.stack([torch.from_numpy(d['masks'][l][d['tgt_of'][l][n]]) for l, n in rows]).to(dtype)[:, None]
            pn = T.sum((1, 2, 3)).clamp(min=1)
            phi = torch.cat((p, 1 - p), 1) * T
            per_proj = R2.box_projection_loss(p, T, K.LOSS_BOXPRO_WEIGHT)
            per_img = R2.levelset_loss(phi, img_g[b:b + 1] * T, pn, K.LOSS_LEVELSET_WEIGHT) * R.W_IMG
            y = R2._TreeFilter.apply(p, img_g[b:b + 1].expand(C, -1, -1, -1), np.repeat(trees[0][b:b + 1], C, 0), True, None)
            z = R2._TreeFilter.apply(y, feat_g[b:b + 1].expand(C, -1, -1, -1), np.repeat(trees[1][b:b + 1], C, 0), False, None)
            per_ls = per_img + R2.levelset_loss(phi, torch.cat((y, z), 1) * T, pn, K.LOSS_LEVELSET_WEIGHT) * R.W_FEAT
            all_proj.append(per_proj)
            all_ls.append(per_ls)
            for k, (l, n) in enumerate(rows):
                proj[l][n], levelset[l][n] = float(per_proj[k].detach()), float(per_ls[k].detach())
    z = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy().astype(np.float64)
    if not all_proj:
        return dict(loss_boxpro=0.0, loss_levelset=0.0, proj=proj, levelset=levelset, grads=[z(p) for p in preds], lst_grad=z(lf))
    lb, ll = torch.cat(all_proj).mean(), torch.cat(all_ls).mean()
    (lb + ll).backward()
    return dict(loss_boxpro=float(lb.detach()), loss_levelset=float(ll.detach()), proj=proj, levelset=levelset, grads=[z(p) for p in preds], lst_grad=z(lf))


@pytest.mark.parametrize('name', list(K.CASES))
def test_shared_form_equals_the_per_row_restatement_in_fp64(name):
    """Sharing the resizes, the trees and the weights per (size, image), and filtering an image's rows as channels of one tree, changes
    nothing but the order of a few fp64 additions."""
    got, want = shared_form(name), K.reference(name, 'float64')
    for key in ('loss_boxpro', 'loss_levelset'):
        assert abs(got[key] - want[key]) <= 1e-10 * max(abs(want[key]), 1e-300), key
    for key in ('proj', 'levelset', 'grads'):
        for g, w in zip(got[key], want[key]):
            assert g.shape == w.shape and (g.size == 0 or np.abs(g - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-300)), key
    assert np.abs(got['lst_grad'] - want['lst_grad']).max() <= 1e-10 * max(np.abs(want['lst_grad']).max(), 1e-300)


def test_restatement_against_the_reference_fixture():
    """tests/golden/box_solov2_loss.npz holds what the reference's own statements :331-367 returned for case three_groups (executed by AST
    from its checkout, tests/golden/make_golden_box_solov2_loss.py; its tree filter is the oracle's, see the file's `provenance`).  The
    restatement in float32 runs the same torch operations on the same CPU: losses and gradients agree to a few fp32 roundings."""
    from tests.golden.make_golden_box_solov2_loss import checksum
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'box_solov2_loss.npz'))
    assert 'oracle/tree_filter_oracle.py' in str(g['provenance']) and str(g['case']) == 'three_groups'
    assert int(g['inputs_crc32']) == checksum(K.inputs('three_groups')), 'the fixture was made from other inputs'
    got = K.reference('three_groups', 'float32')
    items = [('loss_boxpro', got['loss_boxpro'], g['loss_boxpro']), ('loss_levelset', got['loss_levelset'], g['loss_levelset']),
             ('lst_grad', got['lst_grad'], g['lst_grad'])]
    for l in range(len(got['grads'])):
        items += [(f'proj_{l}', got['proj'][l], g[f'proj_{l}']), (f'levelset_{l}', got['levelset'][l], g[f'levelset_{l}']),
                  (f'grad_{l}', got['grads'][l], g[f'grad_{l}'])]
    for key, mine, want in items:
        mine, want = np.asarray(mine, np.float64), np.asarray(want, np.float64)
        assert mine.shape == want.shape, key
        if want.size:
            assert np.abs(mine - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-30), (key, np.abs(mine - want).max(), np.abs(want).max())


def test_restatement_holds_together():
    r32, r64 = K.reference('three_groups', 'float32'), K.reference('three_groups', 'float64')
    for key in ('loss_boxpro', 'loss_levelset'):
        assert abs(r32[key] - r64[key]) <= 1e-5 * abs(r64[key])
    z = K.reference('no_rows', 'float64')
    assert z['loss_boxpro'] == 0.0 and z['loss_levelset'] == 0.0
    a, b = K.reference('inert', 'float64'), K.inputs('inert')
    for l, r, _ in K.CASES['inert']['inert']:
        assert a['proj'][l][r] == 0 and a['levelset'][l][r] == 0 and not a['grads'][l][r].any()
    live = sum(int(((t >= 0) & (i >= 0)).sum()) for t, i in zip(b['tgt_of'], b['img_of']))
    assert abs(a['loss_boxpro'] - sum(p.sum() for p in a['proj']) / live) <= 1e-12          # the means run over the live rows


def test_census_every_case_reaches_the_path_it_is_named_for():
    from boxinstseg_amd import _lib
    assert K.CHUNK_PIXELS == _lib.BLS_CHUNK_PIXELS
    c = K.CASES
    t = K.inputs('three_groups')
    sizes, group = K.groups_of(t['level_sizes'])
    assert t['B'] == 2 and t['level_sizes'] == [(24, 40), (24, 40), (12, 20), (6, 10), (6, 10)] and len(sizes) == 3 and group == [0, 0, 1, 2, 2]
    assert t['counts'] == [[3, 2], [1, 0], [2, 2], [0, 0], [1, 3]] and t['lst_feat'].shape[1] == 5 and t['trees'] is None
    assert sum(t['counts'][3]) == 0 and t['counts'][1][1] == 0 and t['counts'][0][0] and t['counts'][1][0]      # image 0 of size 0: two input segments
    assert any(len(set(x.tolist())) < len(x) for x in t['tgt_of'] if len(x))                                     # rows share a ground truth
    assert all(K.inputs(k)['trees'] is not None for k in c if not c[k].get('own_trees'))
    o = K.inputs('odd')
    assert o['level_sizes'] == [(25, 37), (13, 19)] and all(w % 4 and w % 64 for _, w in o['level_sizes'])
    e = K.inputs('empty_target')
    used = {(l, int(g)) for l in range(2) for g in e['tgt_of'][l]}
    assert not e['masks'][0][0].any() and e['masks'][0][1].all() and (0, 0) in used and (0, 1) in used and (1, 1) in used
    assert all(np.abs(np.abs(p) - 30).max() < 0.01 for p in e['ins_preds'])
    assert float(torch.sigmoid(torch.tensor(np.float32(29.99)))) == 1.0                      # the scores saturate to exactly 1
    assert (e['ins_preds'][0][1] < 0).all() and (e['ins_preds'][1][0] > 0).all()             # all-ones target under all -30 / all +30: both 1e-5 clamps
    te = K.inputs('tree_edge')
    assert te['B'] == 1 and te['counts'] == [[2], [2]] and [h * w for h, w in te['level_sizes']] == [10200, 10302]     # kTfMaxV = 10200 (tree_filter.hip)
    m = K.inputs('many_rows')
    assert sum(sum(r) for r, s in zip(m['counts'], m['level_sizes']) if s == (8, 8)) == 70 > 64 and sum(m['counts'][2]) == 3
    assert all(min(r) > 0 for r in m['counts'][:2]) and len(K.groups_of(m['level_sizes'])[0]) == 2
    i = K.inputs('inert')
    assert sum(int((x < 0).sum()) for x in i['tgt_of']) == 2 and sum(int((x < 0).sum()) for x in i['img_of']) == 2
    assert all(np.array_equal(a, b) for a, b in zip(i['ins_preds'], t['ins_preds']))
    assert sum(map(sum, K.inputs('no_rows')['counts'])) == 0
    # the one dispatch boundary of the kernels: lines per chunk.  h = LPC - 1, LPC, LPC + 1; 1024 // w = 1 and 0; several chunks per row
    lpc = K.lines_per_chunk
    assert lpc(40) == 25 and t['level_sizes'][0][0] == lpc(40) - 1
    assert [h - lpc(w) for h, w in K.inputs('chunk_edge')['level_sizes']] == [0, 1]
    assert [1024 // w for _, w in K.inputs('wide')['level_sizes']] == [1, 0] and lpc(1025) == 1 and 1025 <= _lib.BLS_MAX_W
    assert [-(-h // lpc(w)) for h, w in te['level_sizes']] == [10, 11]
    assert all(len(K.groups_of(K.inputs(k)['level_sizes'])[0]) <= _lib.BLS_MAX_GROUPS and len(K.inputs(k)['level_sizes']) <= _lib.BLS_MAX_LEVELS for k in c)


@pytest.mark.parametrize('name', list(K.CASES))
def test_no_projection_line_has_a_tie_for_its_largest_logit(name):
    """Every line and every column of every row: the largest fp32 logit is unique, so the arg-max rules of the restatement (torch.max on the
    scores) and of the kernels (first index of the largest logit) name the same element, or elements whose scores are equal."""
    for x in K.inputs(name)['ins_preds']:
        for axis in (1, 2):
            if x.size:
                top = x.max(axis=axis, keepdims=True)
                assert ((x == top).sum(axis=axis) == 1).all()


def test_ragged_row_order():
    """(size group, image, level, cell): an image's rows of one size are contiguous although two levels keep them apart in the input."""
    from boxinstseg_amd.boxlevelset_loss import _Plan
    d = K.inputs('three_groups')
    sizes, group = K.groups_of(d['level_sizes'])
    ctx = types.SimpleNamespace(level_sizes=d['level_sizes'], B=2, sizes=sizes, group_of_level=group, img=[torch.zeros(1) for _ in sizes])
    plan = _Plan(ctx, [torch.from_numpy(p) for p in d['ins_preds']], [torch.from_numpy(m) for m in d['masks']], d['counts'])
    assert plan.segments == [(0, 0, 3, 0), (1, 0, 1, 0), (0, 3, 2, 1), (2, 0, 2, 0), (2, 2, 2, 1), (4, 0, 1, 0), (4, 1, 3, 1)]
    assert plan.blocks == [(0, 0, 0, 4), (0, 1, 4, 2), (1, 0, 6, 2), (1, 1, 8, 2), (2, 0, 10, 1), (2, 1, 11, 3)]
    assert plan.group_rows == [6, 4, 4] and plan.M == 14 and plan.pixels == 6 * 960 + 4 * 240 + 4 * 60
    assert plan.row_pixels(1, 8, 2) == (6 * 960 + 2 * 240, 6 * 960 + 4 * 240)
    with_pairs = [[(9, c) for c in per] for per in d['counts']]                              # SoloTargets.counts entries: (pairs, set cells)
    assert _Plan(ctx, [torch.from_numpy(p) for p in d['ins_preds']], [torch.from_numpy(m) for m in d['masks']], with_pairs).segments == plan.segments


def test_parse_cfg():
    from boxinstseg_amd import parse_box_solov2_loss_cfg
    cfg = dict(type='BoxSOLOv2Head', num_classes=80, in_channels=256, stacked_convs=4, seg_feat_channels=512, strides=[8, 8, 16, 32, 32],
               scale_ranges=((1, 96), (48, 192), (96, 384), (192, 768), (384, 2048)), sigma=0.2, num_grids=[40, 36, 24, 16, 12], ins_out_channels=256,
               loss_cate=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
               loss_boxpro=dict(type='BoxProjectionLoss', loss_weight=3.0), loss_levelset=dict(type='LevelsetLoss', loss_weight=1.0))
    kw = parse_box_solov2_loss_cfg(cfg)
    assert kw['loss_boxpro'] == 3.0 and kw['loss_levelset'] == 1.0 and kw['mode'] == 'boxlevelset' and kw['num_grids'] == [40, 36, 24, 16, 12]
    assert kw['gamma'] == 2.0 and kw['alpha'] == 0.25 and kw['loss_weight_cate'] == 1.0
    with pytest.raises(NotImplementedError, match='loss_boxpro.type'):
        parse_box_solov2_loss_cfg(dict(cfg, loss_boxpro=dict(type='DiceLoss')))
    with pytest.raises(NotImplementedError, match='loss_levelset.mode'):
        parse_box_solov2_loss_cfg(dict(cfg, loss_levelset=dict(type='LevelsetLoss', loss_weight=1.0, mode='x')))
    with pytest.raises(TypeError, match='loss_levelset'):
        parse_box_solov2_loss_cfg({k: v for k, v in cfg.items() if k != 'loss_levelset'})
    with pytest.raises(NotImplementedError, match='BoxSOLOv2Head'):
        parse_box_solov2_loss_cfg(dict(cfg, type='DiscoBoxSOLOv2Head'))


@pytest.mark.parametrize('name', [k for k in K.CASES if K.CASES[k].get('own_trees') and k != 'inert'])
def test_own_trees_do_not_hang_on_a_rounding(name):
    """For a case whose context builds its own trees: the MST of every size is the same when every edge weight moves by up to +-2 ulp."""
    d = K.inputs(name)
    rng = np.random.default_rng(3)
    for size in K.groups_of(d['level_sizes'])[0]:
        for src in (torch.from_numpy(d['norm_img']), torch.from_numpy(d['lst_feat'])):
            fm = _resize(src, size).numpy()
            H, W = size
            index = tfo.grid_edges(H, W)
            for b in range(fm.shape[0]):
                wgt = tfo.grid_weights(fm[b])
                want = tfo.mst_edges(index, wgt, H * W)
                ulp = np.spacing(np.abs(wgt))
                for shift in (np.full(wgt.shape, 2.0), np.full(wgt.shape, -2.0), rng.integers(-2, 3, wgt.shape).astype(np.float64)):
                    moved = (wgt.astype(np.float64) + shift * ulp).astype(np.float32)
                    assert np.array_equal(tfo.mst_edges(index, moved, H * W), want)
