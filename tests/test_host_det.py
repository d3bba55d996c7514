"""CPU: the host side of CondInst's test-time detections (no kernel is launched here).

* tests/box_nms_ref.py, the restatement the GPU tests lean on, reproduces what the reference's own code computed
  (tests/golden/det_nms.npz, make_golden_det.py); with the reference present the fixture is regenerated live and compared;
* include/boxinst/boxinst_hip_det.h, the library's exports and _lib.DET_SIGNATURES name the same entry points, and each is run by a
  named guarded test or is a size query;
* CPU tensors and bad arguments fail before any launch;
* the test_cfg of the reference's BoxInst config, as load_config reads it, is accepted."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import box_nms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'det_nms.npz')
CFG_JSON = os.path.join(ROOT, 'tests', 'golden', 'det_test_cfg.json')
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_det.py')
HEADER = os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_det.h')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def stored_inputs(g):
    return {k: [g[f'in_{k}{lv}'] for lv in range(len(R.DET_SIZES))] for k in ('cls', 'bbox', 'ctr', 'params')}


@pytest.mark.parametrize('name', sorted(R.DET_CASES))
def test_restatement_reproduces_the_reference(name):
    g = np.load(GOLDEN)
    inp = stored_inputs(g)
    made = R.det_inputs(int(g['seed']))
    for k in inp:
        for a, b in zip(inp[k], made[k]):
            assert np.array_equal(a, b), f'the stored {k} are not the inputs of the recipe'
    rescale, cfg = R.DET_CASES[name]
    tol = float(g[f'{name}_tol'])
    assert 0 < tol < 1e-6
    got32 = R.get_bboxes(inp, R.DET_STRIDES, R.det_img_dims(), cfg, rescale, np.float32)
    got64 = R.get_bboxes(inp, R.DET_STRIDES, R.det_img_dims(), cfg, rescale, np.float64)
    for b in range(R.DET_B):
        k = f'{name}{b}'
        for got in (got32, got64):
            c = got[b]['cand']
            assert np.array_equal(c['boxes'], g[f'{k}_cand_boxes']) and c['boxes'].dtype == np.float32
            assert np.array_equal(c['labels'], g[f'{k}_cand_labels'])
            assert np.abs(c['scores'].astype(np.float64) - g[f'{k}_cand_scores64']).max(initial=0) <= 4 * tol
            assert np.array_equal(got[b]['dets'][:, :4].astype(np.float32), g[f'{k}_dets32'][:, :4])
            assert np.abs(got[b]['dets'][:, 4] - g[f'{k}_scores64']).max(initial=0) <= 4 * tol
            assert np.array_equal(got[b]['labels'], g[f'{k}_labels']) and np.array_equal(got[b]['params'], g[f'{k}_params'])
            assert np.array_equal(got[b]['coors'], g[f'{k}_coors']) and np.array_equal(got[b]['level_inds'], g[f'{k}_level_inds'])
        assert np.abs(g[f'{k}_cand_scores32'].astype(np.float64) - g[f'{k}_cand_scores64']).max(initial=0) <= tol
        # the margin the GPU tests rely on
        labels = None if cfg['class_agnostic'] else g[f'{k}_cand_labels']
        assert R.iou_margin(g[f'{k}_cand_boxes'], labels, cfg['iou_threshold']) > 1e-4
        # deviation (b): comparing labels and mmcv's class-offset trick keep the same boxes here, in either form of the threshold test
        if len(g[f'{k}_cand_labels']):
            want = got32[b]['keep'].tolist()
            for form in ('mul', 'div'):
                _, keep = R.batched_nms_mmcv_style(g[f'{k}_cand_boxes'], g[f'{k}_cand_scores32'], g[f'{k}_cand_labels'],
                                                   dict(type='nms', iou_threshold=cfg['iou_threshold'], class_agnostic=cfg['class_agnostic']), form=form)
                assert keep.tolist()[:cfg['max_per_img']] == want, form
    assert len(g[f'{name}{R.DET_EMPTY_IMAGE}_labels']) == 0 and g[f'{name}{R.DET_EMPTY_IMAGE}_dets32'].shape == (0, 5)
    if name == 'cut':
        assert [len(g[f'cut{b}_labels']) for b in (0, 2)] == [7, 7] and min(len(g[f'lv3{b}_labels']) for b in (0, 2)) > 7


def test_default_recipe_ignores_the_new_parameters():
    a, b = R.det_inputs(3), R.det_inputs(3, R.DET_SIZES, R.DET_STRIDES, R.DET_B, {})
    assert all(np.array_equal(x, y) for k in a for x, y in zip(a[k], b[k]))


EDGE_CFG = dict(nms_pre=1000, score_thr=0.05, iou_threshold=0.5, max_per_img=100, class_agnostic=False)


def test_edge_recipe_reaches_the_late_tiles():
    """The configs' level sizes: 20267 locations are 317 row tiles, more than one trip of the sum over the earlier tiles' counts."""
    from boxinstseg_amd import _lib
    tile, threads = _lib.DET_ROW_TILE, 4 * _lib.DET_ROW_TILE
    off = R.level_offsets(R.EDGE_SIZES)
    M_all = int(off[-1])
    assert M_all == 20267 and (M_all + tile - 1) // tile == 317 and M_all - 316 * tile == 43 and R.EDGE_ROWS[-1] == M_all - 1
    assert [m // tile for m in R.EDGE_ROWS] == [0, 0, 1, 255, 256, 256, 257, 316] and threads == 256
    seed, inp = R.edge_inputs_with_margin(1, EDGE_CFG)
    assert [m.shape for m in inp['cls']] == [(R.EDGE_B, R.DET_C, h, w) for h, w in R.EDGE_SIZES]
    sel = R.select(inp, EDGE_CFG['nms_pre'], np.float64)
    assert sel.shape == (R.EDGE_B, 3267) and (3267 + tile - 1) // tile == 52
    # the cut of the top 1000 falls among the background's scores, far below every candidate's location
    loc_score = R.location_scores(inp, np.float64)[0]
    cand_locs = np.unique(R.candidates(inp, R.EDGE_STRIDES, R.edge_img_dims(), False, 0.05, None, np.float64)[0]['pos'])
    for lv in range(2):
        cut = np.sort(loc_score[off[lv]:off[lv + 1]])[::-1][EDGE_CFG['nms_pre'] - 1]
        mine = cand_locs[(cand_locs >= off[lv]) & (cand_locs < off[lv + 1])]
        assert len(mine) and loc_score[mine].min() > 2 * cut and set(mine.tolist()) <= set(sel[0].tolist())
    pts, lvl = R.points_of(R.EDGE_SIZES, R.EDGE_STRIDES)
    for name, rows in (('every location', None), ('the per-level top 1000', sel)):
        for rescale in (False, True):
            c64 = R.candidates(inp, R.EDGE_STRIDES, R.edge_img_dims(), rescale, 0.05, rows, np.float64)
            c32 = R.candidates(inp, R.EDGE_STRIDES, R.edge_img_dims(), rescale, 0.05, rows, np.float32)
            assert all(np.array_equal(a['pos'], b['pos']) and np.array_equal(a['labels'], b['labels']) for a, b in zip(c32, c64))
        c = c64[0]
        loc = c['pos'] if rows is None else rows[0][c['pos']]
        tiles = sorted(set((c['pos'] // tile).tolist()))
        twice = int((np.bincount(c['pos']) == 2).sum())
        print(f'seed {seed}, {name}: candidates per image {[len(x["labels"]) for x in c64]}, in row tiles {tiles}, on levels '
              f'{np.bincount(lvl[loc], minlength=5).tolist()}, locations with two classes: {twice}')
        assert len(c64[1]['labels']) == 0 and len(c['labels']) > min(R.EDGE_CAPS) and len(c['labels']) <= max(R.EDGE_CAPS)
        assert (np.bincount(lvl[loc], minlength=5) > 0).all() and twice >= 1
        assert set(R.EDGE_ROWS) <= set(loc.tolist())
        if rows is None:
            assert min(tiles) < threads and max(tiles) >= threads + 1 and tiles[-1] == 316
        # no class score is within fp32 reach of the threshold
        s = R.sigmoid(R.flatten_levels(inp['cls'])[0], np.float64)
        assert np.abs(s - 0.05).min() > 1e-3
        assert R.iou_margin(c['boxes'], c['labels'], EDGE_CFG['iou_threshold']) > 1e-4
    scores = np.sort(c64[0]['scores'])
    assert np.diff(scores).min() > 1e-4                                                # a shuffled linspace: the order is not fp32's to decide
    for nms_pre in (1000, -1):
        out = R.get_bboxes(inp, R.EDGE_STRIDES, R.edge_img_dims(), dict(EDGE_CFG, nms_pre=nms_pre), False, np.float64)
        print(f'nms_pre {nms_pre}: detections per image {[len(o["labels"]) for o in out]}')
        assert 0 < len(out[0]['labels']) < len(c64[0]['labels']) and len(out[1]['labels']) == 0


def test_greedy_nms_by_hand():
    # A suppresses B, B would suppress C, A does not suppress C: C is kept
    boxes = np.array([[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]], np.float32)
    assert R.greedy_nms(boxes, np.array([0.9, 0.8, 0.7], np.float32), None, 0.4) == [0, 2]
    assert R.greedy_nms(boxes, np.array([0.9, 0.8, 0.7], np.float32), np.array([0, 1, 0]), 0.4) == [0, 1, 2]
    assert R.greedy_nms(boxes, np.array([0.7, 0.8, 0.9], np.float32), None, 0.4) == [2, 0]
    assert R.greedy_nms(boxes, np.array([0.9, 0.8, 0.7], np.float32), None, 0.4, max_num=1) == [0]
    # ties by index, NaN first, -0 == +0
    assert R.sort_order(np.array([0.5, np.nan, 0.5, 0.7, -0.0, 0.0, np.nan], np.float32)).tolist() == [1, 6, 3, 0, 2, 4, 5]
    # offset = 1: two 1-pixel boxes side by side share an edge, so they do not overlap at offset 0 and do at offset 1
    b = np.array([[0, 0, 1, 1], [1, 0, 2, 1]], np.float32)
    assert R.greedy_nms(b, np.array([0.9, 0.8], np.float32), None, 0.3) == [0, 1]
    assert R.greedy_nms(b, np.array([0.9, 0.8], np.float32), None, 0.3, offset=1) == [0]     # inter 1*2 = 2, union 4 + 4 - 2 = 6


@pytest.mark.parametrize('name', sorted(R.DET_CASES))
def test_fixture_is_what_the_reference_computes_now(name):
    """Live: the reference's code, loaded where it lies, gives the stored expectations again."""
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/models/dense_heads/condinst_head.py')):
        pytest.skip('the upstream checkout is not here')
    spec = importlib.util.spec_from_file_location('make_golden_det', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(GOLDEN)
    inp = stored_inputs(g)
    live = gen.reference_case(name, inp)
    assert live and gen.margins_ok(inp, name, live) and gen.restatement_agrees(inp, name, live)
    for key, want in live.items():
        assert key in g, key
        if key.endswith(('_cand_boxes', '_params', '_coors')) or want.dtype.kind != 'f':     # decoded, gathered or integer: bit-equal
            assert np.array_equal(g[key], want), key
            continue
        if key.endswith('_dets32'):
            assert np.array_equal(g[key][:, :4], want[:, :4]), key
        # scores pass through exp, which may differ by an ulp between builds of torch
        assert np.allclose(g[key], want, rtol=0, atol=1e-6 if want.dtype == np.float32 else 1e-12), key


def _header_text():
    with open(HEADER) as fh:
        return fh.read()


def test_header_exports_and_signatures_agree():
    """(declarations, exports and ctypes signatures: tests/test_abi_families.py)"""
    from boxinstseg_amd import _lib, box_nms
    lib = _lib.load()
    text = _header_text()
    for macro, value in (('BXI_DET_MAX_LEVELS', _lib.DET_MAX_LEVELS), ('BXI_DET_SORT_MAX', _lib.DET_SORT_MAX), ('BXI_DET_NMS_ROUND', _lib.DET_NMS_ROUND),
                         ('BXI_DET_KEEP_TILE', _lib.DET_KEEP_TILE), ('BXI_DET_ROW_TILE', _lib.DET_ROW_TILE),
                         ('BXI_DET_STATUS_OVER_CAP', _lib.DET_STATUS_OVER_CAP), ('BXI_DET_STATUS_OVER_SORT', _lib.DET_STATUS_OVER_SORT),
                         ('BXI_DET_STATUS_BAD_ORDER', _lib.DET_STATUS_BAD_ORDER)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', text).group(1)) == value, macro
    assert (box_nms.SORT_MAX, box_nms.NMS_ROUND, box_nms.KEEP_TILE) == (_lib.DET_SORT_MAX, _lib.DET_NMS_ROUND, _lib.DET_KEEP_TILE)
    assert lib.bxi_abi_version() == _lib.BXI_ABI_VERSION == 7                # additive: the version stays
    # struct bxi_det_level: four pointers and three ints
    assert [f[0] for f in _lib.DetLevel._fields_] == ['cls', 'bbox', 'ctr', 'params', 'H', 'W', 'stride']
    assert re.search(r'typedef struct \{ const float \*cls, \*bbox, \*ctr, \*params; int H, W, stride; \} bxi_det_level;', text)
    for word in ('inter > iou_thr * (Sa + Sb - inter)', 'max coordinate + 1'):   # the two documented deviations
        assert word in text
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    assert 'Level 3d' in integration and 'max coordinate + 1' in integration


def test_reference_test_cfg_is_accepted():
    import boxinstseg_amd as B
    from boxinstseg_amd import box_nms
    with open(CFG_JSON) as fh:
        stored = json.load(fh)
    path = os.path.join(REFERENCE, 'configs/boxinst/boxinst_r50_fpn_1x_coco.py')
    if os.path.exists(path):
        assert B.load_config(path)['model']['test_cfg'] == stored, 'tests/golden/det_test_cfg.json is not the config block of the reference any more'
    want = dict(nms_pre=2000, score_thr=0.05, iou_threshold=0.5, max_per_img=2000, class_agnostic=False, nms_max_num=-1)
    assert box_nms.parse_test_cfg(stored) == want
    import types
    ns = types.SimpleNamespace(**{k: (types.SimpleNamespace(**v) if isinstance(v, dict) else v) for k, v in stored.items()})
    assert box_nms.parse_test_cfg(ns) == want
    with pytest.raises(NotImplementedError, match='soft_nms'):
        box_nms.parse_test_cfg(dict(stored, nms=dict(type='soft_nms', iou_threshold=0.5)))
    with pytest.raises(TypeError):
        box_nms.parse_test_cfg(dict(score_thr=0.05))
    assert B.condinst_get_bboxes is box_nms.condinst_get_bboxes and B.nms is box_nms.nms and B.batched_nms is box_nms.batched_nms
    assert B.nms_with_others is box_nms.nms_with_others
    for name in ('nms', 'batched_nms', 'nms_with_others', 'condinst_get_bboxes'):
        assert name in B.__all__ and name in B.__doc__


def test_cpu_tensors_fail_loudly():
    import boxinstseg_amd as B
    boxes, scores, idxs = torch.rand(5, 4), torch.rand(5), torch.zeros(5, dtype=torch.long)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.nms(boxes, scores, 0.5)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.batched_nms(boxes, scores, idxs, dict(type='nms', iou_threshold=0.5))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.nms_with_others(boxes, torch.rand(5, 3), 0.05, dict(type='nms', iou_threshold=0.5))
    g = np.load(GOLDEN)
    inp = {k: [torch.from_numpy(a) for a in v] for k, v in stored_inputs(g).items()}
    metas = [dict(img_shape=s, scale_factor=np.array(f, np.float32)) for s, f in zip(R.DET_IMG_SHAPES, R.DET_SCALES)]
    cfg = dict(nms_pre=40, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.condinst_get_bboxes(inp['cls'], inp['bbox'], inp['ctr'], inp['params'], metas, cfg, R.DET_STRIDES)
    with pytest.raises(NotImplementedError):
        B.condinst_get_bboxes(inp['cls'], inp['bbox'], inp['ctr'], inp['params'], metas, dict(cfg, nms=dict(type='soft_nms', iou_threshold=0.5)),
                              R.DET_STRIDES)


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000                                           # a non-NULL value no call below dereferences: every one fails before its launch
    big = 1 << 40

    def levels(n=2, H=4, W=5, stride=8, cls=X, params=X):
        arr = (_lib.DetLevel * max(n, 1))()
        for i in range(n):
            arr[i] = _lib.DetLevel(cls, X, X, params, H, W, stride)
        return arr

    def score(lv=None, n=2, B=2, C=3, out=X, **kw):
        return lib.bxi_det_location_score_f32(levels(n, **kw) if lv is None else lv, n, B, C, out, None)
    assert score(B=0, out=None) == 0
    assert score(n=0) == -2 and score(n=9) == -2 and score(B=-1) == -2 and score(B=65) == -2 and score(C=0) == -2
    assert score(H=0) == -2 and score(stride=0) == -2 and score(H=40000, W=40000) == -2
    assert score(out=None) == -1 and score(cls=None) == -1
    assert lib.bxi_det_location_score_f32(None, 2, 2, 3, X, None) == -1

    cw = lib.bxi_det_candidates_workspace_bytes
    assert cw(0, 10) == 0 and cw(65, 10) == 0 and cw(2, -1) == 0
    assert cw(2, 0) == 8 and cw(2, 64) == 8 and cw(2, 65) == 16 and cw(3, 1000) == 4 * 3 * 16
    dims = _lib.float_array([8, 8, 1, 1, 1, 1] * 2)

    def cand(sel=X, M=10, dims_=dims, thr=0.05, cap=16, boxes=X, scores=X, labels=X, pos=X, count=X, ws=X, nbytes=big, B=2, C=3, **kw):
        return lib.bxi_det_candidates_f32(levels(2, **kw), 2, B, C, sel, M, dims_, 0, thr, cap, boxes, scores, labels, pos, count, ws, nbytes, None)
    assert cand(B=0) == 0
    assert cand(M=-1) == -2 and cand(cap=-1) == -2 and cand(H=0) == -2
    assert cand(thr=float('nan')) == -3
    for name in ('dims_', 'boxes', 'scores', 'labels', 'pos', 'count'):
        assert cand(**{name: None}) == -1, name
    assert cand(ws=None) == -5 and cand(nbytes=cw(2, 10) - 1) == -5 and cand(ws=X + 2) == -5
    assert cand(sel=None, nbytes=cw(2, 40) - 1) == -5                       # sel NULL: M is M_all = 2 * 4 * 5

    nw = lib.bxi_box_nms_workspace_bytes
    assert nw(0, 8, 8) == 0 and nw(2, 0, 1) == 0 and nw(2, 8, 0) == 0 and nw(65535, 8, 1 << 20) == 0 and nw(65536, 8, 8) == 0
    assert nw(2, 100, 100) == 4 * 2 * 100 and nw(3, 5000, 100) == 4 * 3 * 5000
    assert nw(2, 5000, 5000) == 4 * (2 * 5000 + 2 * (5000 - _lib.DET_KEEP_TILE) * 6)
    # max_keep is max_num also where that is above cap: the stride of keep grows, the spill does not
    assert nw(2, 8, 9) == 4 * 2 * 8 and nw(2, 100, 2000) == 4 * 2 * 100 and nw(2, 3000, 5000) == 4 * (2 * 3000 + 2 * (3000 - _lib.DET_KEEP_TILE) * 6)

    def nms(boxes=X, scores=X, labels=X, count=X, order=None, P=2, cap=100, thr=0.5, offset=0, max_num=-1, keep=X, n_keep=X, status=X, ws=X, nbytes=big):
        return lib.bxi_box_nms_f32(boxes, scores, labels, count, order, P, cap, thr, offset, max_num, keep, n_keep, status, ws, nbytes, None)
    assert nms(P=0) == 0
    assert nms(P=-1) == -2 and nms(P=65536) == -2 and nms(cap=0) == -2 and nms(P=60000, cap=60000) == -2
    assert nms(offset=2) == -3 and nms(offset=-1) == -3 and nms(thr=float('nan')) == -3
    for name in ('boxes', 'scores', 'count', 'keep', 'n_keep', 'status'):
        assert nms(**{name: None}) == -1, name
    assert nms(P=60000, cap=8, max_num=1 << 20) == -2                        # P * max_keep >= 2^31
    assert nms(ws=None) == -5 and nms(nbytes=nw(2, 100, 100) - 1) == -5 and nms(ws=X + 1) == -5
    assert nms(cap=5000, order=X, ws=None) == -5                             # max_keep = cap > the LDS tile: the spill needs the workspace

    def gather(P=4, sel=X, M=10, cb=X, cs=X, cl=X, cp=X, cap=16, keep=X, nk=X, max_keep=8, dets=X, dl=X, dp=X, dc=X, dli=X, B=2, **kw):
        return lib.bxi_det_gather_f32(levels(2, **kw), 2, B, 3, P, sel, M, cb, cs, cl, cp, cap, keep, nk, max_keep, dets, dl, dp, dc, dli, None)
    assert gather(B=0) == 0 and gather(max_keep=0) == 0
    assert gather(P=-1) == -2 and gather(cap=0) == -2 and gather(M=-1) == -2 and gather(max_keep=-1) == -2
    for name in ('cb', 'cs', 'cl', 'cp', 'keep', 'nk', 'dets', 'dl', 'dp', 'dc', 'dli'):
        assert gather(**{name: None}) == -1, name
    assert gather(params=None) == -1 and gather(cls=None) == -1
