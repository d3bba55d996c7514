"""CPU: the host side of the SOLOv2-style heads' training targets (no kernel is launched here).

* tests/solo_ref.py, the restatement the GPU tests lean on, reproduces what the reference's own code computed
  (tests/golden/solo_targets.npz, make_golden_solo_targets.py); with the reference present the fixture is regenerated live and compared;
* include/boxinst/boxinst_hip_solo.h, the library's exports and _lib.SOLO_SIGNATURES name the same entry points, and each is run by a
  named guarded test or is a size query;
* the bbox_head block of every configs/discobox and configs/boxlevelset file is accepted (tests/golden/solo_head_cfg.json);
* CPU tensors and bad arguments fail before any launch."""
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import solo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_solo_targets.py')
HEADER = os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_solo.h')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
SPEC = R.load_cases()
CASES = sorted(SPEC['cases'])


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def restated(name, mode):
    case = SPEC['cases'][name]
    boxes, labels = R.gt_of(case)
    h, w = SPEC['mask_feat_size']
    return R.targets(mode, boxes, labels, R.masks_of(case), num_grids=SPEC['num_grids'], scale_ranges=SPEC['scale_ranges'], sigma=SPEC['sigma'],
                     num_classes=SPEC['num_classes'], canvas=(4 * h, 4 * w))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_fixture(name, mode):
    g = np.load(R.GOLDEN)
    case = SPEC['cases'][name]
    masks = R.masks_of(case)
    tg = restated(name, mode)
    key = f'{name}_{mode}'
    assert np.array_equal(tg['moments'], g[f'{name}_moments']) and int(g[f'{name}_moments'].max()) < 2 ** 24
    for k in R.CELL_KEYS:
        assert np.array_equal(tg[k], g[f'{key}_{k}']) and tg[k].dtype == g[f'{key}_{k}'].dtype, k
    for k in ('grid_order', 'pair_inst', 'sel_inst'):
        assert np.array_equal(np.concatenate([a for lv in tg[k] for a in lv]), g[f'{key}_{k}']), k
    assert [[len(a) for a in lv] for lv in tg['grid_order']] == g[f'{key}_pair_counts'].tolist()
    assert [[len(a) for a in lv] for lv in tg['sel_inst']] == g[f'{key}_set_counts'].tolist()
    assert tg['num_ins'] == int(g[f'{key}_num_ins']) == int(g[f'{key}_set_counts'].sum())
    # the planes the reference stacked are the rescaled masks of the recorded instances
    planes = R.level_planes(SPEC, mode)
    for f, (h, w) in set(planes):
        want = g[f'{name}_rescaled_f{f}']
        at = 0
        for m in masks:
            got = np.zeros((m.shape[0], h, w), np.uint8)
            got[:, :m.shape[1] // f, :m.shape[2] // f] = R.rescale(m, f)
            assert np.array_equal(got, want[at:at + m.shape[0]])
            at += m.shape[0]
    for l, (f, _) in enumerate(planes):
        idx = np.concatenate(tg['pair_inst' if mode == 'discobox' else 'sel_inst'][l])
        assert np.array_equal(g[f'{name}_rescaled_f{f}'][idx], g[f'{key}_ins_labels{l}'])
    # loss_cate in float64, and the measured tolerances: present, positive, of the size of float32 rounding
    inputs = R.make_cate_inputs(SPEC, int(g['seed']))
    for l, m in enumerate(inputs):
        assert np.array_equal(m, g[f'in_cate{l}'])
    lc = SPEC['loss_cate'][mode]
    loss, grads = R.cate_loss(inputs, tg['cate_labels'], tg['num_ins'], lc['gamma'], lc['alpha'], lc['loss_weight'])
    assert np.allclose(float(loss), float(g[f'{key}_loss64']), rtol=1e-12, atol=0)
    for l, gr in enumerate(grads):
        want = g[f'{key}_grad_cate{l}']
        assert np.allclose(gr.numpy(), want, rtol=1e-10, atol=1e-13 * np.abs(want).max())
    for k in ('tol_loss_cate', 'tol_grad_cate'):
        assert 0 < float(g[k]) < 1e-5, k
    assert abs(float(g[f'{key}_loss32']) - float(g[f'{key}_loss64'])) / float(g[f'{key}_loss64']) <= float(g['tol_loss_cate'])


def test_restatement_rules_by_hand():
    # the rescale rule: 2 of the 4 sampled pixels make a 1, 1 of 4 does not
    m = np.zeros((8, 8), np.uint8)
    m[2:, 2:] = 1                       # f = 4 samples rows / cols 1, 2 and 5, 6: the corner sample sees one pixel, the edges two
    assert R.rescale(m, 4).tolist() == [[0, 1], [1, 1]] and R.sampled_sums(m, 4).tolist() == [[1, 2], [2, 4]]
    # floor division is the reference's operation, not floor(x * S): 0.5 // (1 / 40) is 19 in double
    assert int(0.5 // (1. / 40)) == 19 and int(torch.tensor(0.5) // (1. / 40)) == 19
    # one 12 x 12 mask in a 32 x 32 canvas, grid 4: DiscoBox takes it, BoxLevelSet needs 10 pixels
    boxes, labels = [torch.tensor([[8., 8., 20., 20.]])], [torch.tensor([3])]
    mk = np.zeros((1, 32, 32), np.uint8)
    mk[0, 10:13, 10:13] = 1
    kw = dict(num_grids=[4], scale_ranges=[(1, 64)], sigma=0.2, num_classes=5, canvas=(32, 32))
    d, b = R.targets('discobox', boxes, labels, [mk], **kw), R.targets('boxlevelset', boxes, labels, [mk], **kw)
    assert d['moments'].tolist() == [[9, 99, 99]] and d['grid_order'][0][0].tolist() == [5] and d['cate_labels'][5] == 3 and d['num_ins'] == 1
    assert b['num_ins'] == 0 and bool((b['cate_labels'] == 5).all()) and bool((b['cell_owner'] == -1).all())
    # an image without boxes: all background
    e = R.targets('discobox', [torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.int64)], [np.zeros((0, 32, 32), np.uint8)], **kw)
    assert bool((e['cate_labels'] == 5).all()) and e['num_ins'] == 0 and e['moments'].shape == (0, 3)


@pytest.mark.parametrize('name', CASES)
def test_fixture_is_what_the_reference_computes_now(name):
    """Live: the reference's code, loaded where it lies, gives the stored expectations again."""
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/models/dense_heads/discobox_head.py')):
        pytest.skip('the upstream checkout is not here')
    pytest.importorskip('scipy')
    spec = importlib.util.spec_from_file_location('make_golden_solo_targets', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(R.GOLDEN)
    inputs = [g[f'in_cate{l}'] for l in range(len(SPEC['num_grids']))]
    got = gen.case_arrays(SPEC, name, SPEC['cases'][name], inputs)
    assert got is not None, 'the restatement or the census failed'
    live, tol = got
    for key, want in live.items():
        assert key in g, key
        if want.dtype.kind != 'f':
            assert np.array_equal(g[key], want), key
        else:           # exp and log may differ by an ulp between builds of torch
            assert np.allclose(g[key], want, rtol=1e-5 if want.dtype == np.float32 else 1e-11, atol=1e-13), key
    for k, v in tol.items():
        assert v <= float(g[k]) * 1.5, k
    with open(R.CFG_JSON) as fh:
        assert json.load(fh) == json.loads(json.dumps(gen.config_blocks())), 'tests/golden/solo_head_cfg.json is not the bbox_head blocks of the reference any more'


def test_header_exports_and_signatures_agree():
    """(declarations, exports and ctypes signatures: tests/test_abi_families.py)"""
    from boxinstseg_amd import _lib, solo_targets
    lib = _lib.load()
    with open(HEADER) as fh:
        text = fh.read()
    for macro, value in (('BXI_SOLO_MODE_DISCOBOX', _lib.SOLO_MODES['discobox']), ('BXI_SOLO_MODE_BOXLEVELSET', _lib.SOLO_MODES['boxlevelset']),
                         ('BXI_SOLO_MAX_FACTORS', _lib.SOLO_MAX_FACTORS), ('BXI_SOLO_MAX_FACTOR', _lib.SOLO_MAX_FACTOR),
                         ('BXI_SOLO_RESCALE_MIN_ONES', _lib.SOLO_RESCALE_MIN_ONES), ('BXI_SOLO_MIN_MASK_SUM', _lib.SOLO_MIN_MASK_SUM),
                         ('BXI_SOLO_MAX_GRID', _lib.SOLO_MAX_GRID), ('BXI_SOLO_PAIRS_PER_INSTANCE', _lib.SOLO_PAIRS_PER_INSTANCE),
                         ('BXI_SOLO_STATUS_BAD_LABEL', _lib.SOLO_STATUS_BAD_LABEL)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', text).group(1)) == value, macro
    assert solo_targets.RESCALE_MIN_ONES == R.RESCALE_MIN_ONES == _lib.SOLO_RESCALE_MIN_ONES and R.MIN_MASK_SUM == _lib.SOLO_MIN_MASK_SUM
    assert lib.bxi_abi_version() == _lib.BXI_ABI_VERSION == 7                # additive: the version stays
    for word in ('UNPINNED', 'rounded once', 'all background', 'fmod-based', 'BXI_SOLO_RESCALE_MIN_ONES', 'LAST instance'):
        assert word in text, word
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3f', 'unpinned', 'rounded once', 'best_target_single', 'F.interpolate', 'F.conv2d', 'all-zero targets',
                 'bxi_solo_mask_pass_u8', 'bxi_solo_assign_f32', 'bxi_solo_cate_loss_f32'):
        assert word in integration, word


def test_reference_head_blocks_are_accepted():
    import boxinstseg_amd as B
    from boxinstseg_amd import solo_targets
    with open(R.CFG_JSON) as fh:
        stored = json.load(fh)
    assert len(stored) == 9
    for d in ('discobox', 'boxlevelset'):
        folder = os.path.join(REFERENCE, 'configs', d)
        if os.path.isdir(folder):
            assert sorted(k for k in stored if k.startswith(d + '/')) == sorted(f'{d}/{f}' for f in os.listdir(folder) if f.endswith('.py'))
    for fname, block in stored.items():
        s = B.parse_solo_head_cfg(block)
        assert s['mode'] == fname.split('/')[0] and s['num_classes'] == block['num_classes'] and s['num_grids'] == list(block['num_grids'])
        assert s['strides'] == list(block['strides']) and s['scale_ranges'] == tuple((float(a), float(b)) for a, b in block['scale_ranges'])
        assert s['sigma'] == block['sigma'] and (s['gamma'], s['alpha'], s['loss_weight_cate']) == (2.0, 0.25, 1.0)
        assert sorted(s) == sorted(solo_targets._FLAT_KEYS)
        ns = types.SimpleNamespace(**{k: (types.SimpleNamespace(**v) if isinstance(v, dict) else v) for k, v in block.items()})
        assert B.parse_solo_head_cfg(ns) == s
    block = next(iter(stored.values()))
    for key, bad, word in (('loss_cate', dict(type='QualityFocalLoss'), 'loss_cate.type'), ('type', 'SOLOv2Head', 'bbox_head.type'),
                           ('loss_cate', dict(type='FocalLoss', use_sigmoid=True, activated=True), 'loss_cate.activated'),
                           ('loss_cate', dict(type='FocalLoss', use_sigmoid=False), 'loss_cate.use_sigmoid'),
                           ('loss_cate', dict(type='FocalLoss', beta=1), 'loss_cate.beta')):
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            B.parse_solo_head_cfg(dict(block, **{key: bad}))
    for mode in R.MODES:
        s = B.parse_solo_head_cfg(R.head_cfg(SPEC, mode))
        assert s['mode'] == mode and s['gamma'] == SPEC['loss_cate'][mode]['gamma'] and s['num_grids'] == SPEC['num_grids']
    for name in ('solov2_targets', 'box_solov2_targets', 'solo_cate_loss', 'parse_solo_head_cfg'):
        assert name in B.__all__ and getattr(B, name) is getattr(solo_targets, name)


def test_cpu_tensors_and_bad_arguments_fail_loudly():
    import boxinstseg_amd as B
    case = SPEC['cases']['mixed']
    boxes, labels = R.gt_of(case)
    masks = [torch.from_numpy(m) for m in R.masks_of(case)]
    s = B.parse_solo_head_cfg(R.head_cfg(SPEC, 'discobox'))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **s)
    sb = B.parse_solo_head_cfg(R.head_cfg(SPEC, 'boxlevelset'))
    sizes = [hw for _, hw in R.level_planes(SPEC, 'boxlevelset')]
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box_solov2_targets(boxes, labels, masks, sizes, **sb)
    with pytest.raises(RuntimeError, match='DiscoBox'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **sb)
    with pytest.raises(RuntimeError, match='BoxLevelSet'):
        B.box_solov2_targets(boxes, labels, masks, sizes, **s)
    with pytest.raises(RuntimeError, match='gt_masks'):
        B.solov2_targets(boxes, labels, masks[:2], SPEC['mask_feat_size'], **s)
    with pytest.raises(TypeError, match='missing'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], num_grids=[4])
    with pytest.raises(TypeError, match='unknown'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], radius=3, **s)
    with pytest.raises(RuntimeError, match='levels'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **dict(s, strides=s['strides'][:3]))
    with pytest.raises(RuntimeError, match='num_grids'):
        B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **dict(s, num_grids=[8, 6, 5, 4, 65]))
    preds = [torch.from_numpy(p) for p in R.make_cate_inputs(SPEC, 1)]
    n = sum(SPEC['B'] * g * g for g in SPEC['num_grids'])
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_cate_loss(preds, torch.zeros(n, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match='tensor'):
        B.solo_cate_loss(preds, torch.zeros(n, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match='levels'):
        B.solo_cate_loss([], torch.zeros(n, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000                                           # a non-NULL value no call below dereferences: every one fails before its launch
    nan = float('nan')
    ia, fa, pa = _lib.int_array, _lib.float_array, _lib.ptr_array
    offs = ia([0, 2, 3])

    def mask_pass(masks=(X, X), off=offs, H=(32, 64), W=(64, 96), B=2, factors=(4, 8), oh=(16, 8), ow=(24, 12), nf=2, outs=(X, X), mom=X,
                  no_masks=False):
        return lib.bxi_solo_mask_pass_u8(None if no_masks else pa(masks), off, ia(H), ia(W), B, ia(factors), ia(oh), ia(ow), nf, pa(outs), mom, None)
    assert mask_pass(B=0) == 0 and mask_pass(off=ia([0, 0, 0])) == 0
    assert mask_pass(B=-1) == -2 and mask_pass(B=65) == -2 and mask_pass(off=ia([1, 2, 3])) == -2 and mask_pass(off=ia([0, 3, 2])) == -2
    assert mask_pass(H=(0, 64)) == -2 and mask_pass(oh=(7, 8)) == -2 and mask_pass(ow=(24, 11)) == -2 and mask_pass(oh=(16, 0)) == -2
    assert mask_pass(nf=5) == _lib.BXI_ERR_UNSUPPORTED and mask_pass(factors=(3, 8)) == _lib.BXI_ERR_UNSUPPORTED
    assert mask_pass(factors=(4, 6)) == _lib.BXI_ERR_UNSUPPORTED and mask_pass(factors=(4, 128)) == _lib.BXI_ERR_UNSUPPORTED
    assert mask_pass(H=(36, 64)) == _lib.BXI_ERR_UNSUPPORTED and mask_pass(W=(64, 100)) == _lib.BXI_ERR_UNSUPPORTED
    assert mask_pass(no_masks=True) == -1 and mask_pass(masks=(X, 0)) == -1 and mask_pass(outs=(X, 0)) == -1 and mask_pass(mom=None) == -1
    assert mask_pass(mom=X + 4) == -3

    def assign(mode=0, B=2, n=2, grids=(4, 3), rg=(1, 48, 24, 96), sigma=0.2, C=5, Hc=64, Wc=96, boxes=X, labels=X, mom=X, off=offs, **outs):
        o = dict(cate=X, ind=X, owner=X, sel=X, pc=X, pi=X, counts=X, num_ins=X, status=X)
        o.update(outs)
        return lib.bxi_solo_assign_f32(mode, B, n, ia(grids), fa(rg), sigma, C, Hc, Wc, boxes, labels, mom, off, o['cate'], o['ind'], o['owner'],
                                       o['sel'], o['pc'], o['pi'], o['counts'], o['num_ins'], o['status'], None)
    assert assign(B=0) == 0
    assert assign(n=0) == -2 and assign(n=9) == -2 and assign(B=65) == -2 and assign(B=-1) == -2 and assign(C=0) == -2 and assign(Hc=0) == -2
    assert assign(grids=(4, 0)) == -2 and assign(grids=(65, 3)) == -2 and assign(off=ia([1, 2, 3])) == -2
    assert assign(mode=2) == -3 and assign(sigma=nan) == -3 and assign(rg=(1, nan, 24, 96)) == -3
    for name in ('boxes', 'labels', 'mom', 'cate', 'ind', 'owner', 'sel', 'pc', 'pi', 'counts', 'num_ins', 'status'):
        assert assign(**{name: None}) == -1, name

    wb = lib.bxi_solo_cate_workspace_bytes
    assert wb(ia([4, 3]), 2, 0, 5) == 0 and wb(ia([4, 3]), 0, 2, 5) == 0 and wb(ia([4, 3]), 2, 2, 0) == 0 and wb(ia([4, 65]), 2, 2, 5) == 0
    assert wb(None, 2, 2, 5) == 0 and wb(ia([4, 3]), 2, 2, 5) == 8 * 2 and wb(ia([40]), 1, 2, 80) == 8 * ((2 * 80 * 1600 + 1023) // 1024)

    def loss(preds=(X, X), grids=(4, 3), n=2, B=2, C=5, labels=X, num_ins=X, gamma=2.0, alpha=0.25, lw=1.0, grads=(X, X), out=X, ws=X, nbytes=1 << 30):
        return lib.bxi_solo_cate_loss_f32(pa(preds), ia(grids), n, B, C, labels, num_ins, gamma, alpha, lw, pa(grads), out, ws, nbytes, None)
    assert loss(B=0) == 0
    assert loss(n=0) == -2 and loss(B=65) == -2 and loss(C=0) == -2 and loss(grids=(4, 65)) == -2
    assert loss(gamma=nan) == -3 and loss(gamma=-1.0) == -3 and loss(alpha=nan) == -3 and loss(lw=nan) == -3
    for name in ('labels', 'num_ins', 'out'):
        assert loss(**{name: None}) == -1, name
    assert loss(preds=(X, 0)) == -1 and loss(grads=(0, X)) == -1
    assert loss(ws=None) == -5 and loss(nbytes=7) == -5 and loss(ws=X + 2) == -5

    def rescale(grids=(4, 3), n=2, B=2, C=5, unit=(X, X), up=X, out=(X, X)):
        return lib.bxi_solo_cate_grad_rescale_f32(ia(grids), n, B, C, pa(unit), up, pa(out), None)
    assert rescale(B=0) == 0
    assert rescale(n=0) == -2 and rescale(C=0) == -2 and rescale(up=None) == -1 and rescale(unit=(X, 0)) == -1 and rescale(out=(0, X)) == -1
