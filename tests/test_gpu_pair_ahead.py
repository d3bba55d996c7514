"""The tile wave's split pair loop (fused_eval.hip, math_tile: phase A = S, log2 S, 1 / S of every pair ahead of the wait for the
predicate words, parked in the wave's LDS and in registers; phase B = weights and multiply-adds behind it) on the smallest shapes at
which it can go wrong: ragged column tiles narrower than the dilation, rows that do not fill a 4-row tile, boxes of one cell, a tile that
takes the log-space path next to tiles that take the split loop, waves that walk several tiles, poisoned outputs and scratch.

Everything against the C oracle (losses 1e-4 relative, gradient 1e-4 of max|grad|, every line: tests/helpers.py), and bit for bit between
the three forms with 4-row tiles: the single launch (eval1_kernel<D, 4, false>, which runs the split loop at dilation 2) and the two launches and the
targets-ready launch (pair_kernel<D, 4>, eval1_kernel<D, 4, true>: one switch each in fused_eval.hip, the un-split loop where it measured
faster) -- the terms and their order are the same, so the bits are, whichever way a switch stands."""
import ctypes as C

import numpy as np
import pytest
import torch

from boxinstseg_amd import synthetic
from oracle import c_oracle
from tests.guarded import poisoned_empty
from tests.helpers import expected_grad_logit_first, grad_check_all_lines, grad_report, hip_loss, oracle_path, rel, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-4
R = 4           # the split loop is built for 4-row tiles


def _batch(h, w, boxes, extra_inds=(), seed=0):
    """One image of h x w cells (stride 4) with the given GT boxes (pixels), one instance per box plus one per entry of `extra_inds`."""
    boxes = np.asarray(boxes, np.float32)
    d = synthetic.make_batch(B=1, H=4 * h, W=4 * w, boxes_per_img=len(boxes), seed=seed, min_box=8, max_box=4 * min(h, w))
    d['gt_bboxes'] = [boxes]
    rng = np.random.default_rng(1000 + seed)
    extra = (2.0 * rng.standard_normal((len(extra_inds), 1, h, w))).astype(np.float32)
    d['gt_inds'] = np.concatenate([d['gt_inds'], np.asarray(extra_inds, np.int64)])
    d['mask_logits'] = np.concatenate([d['mask_logits'], extra], axis=0)
    d['N'] = len(d['gt_inds'])
    return d


def _cells(d, box):
    """(r0, r1, c0, c1): the half-open cell rectangle whose samples lie in the GT box."""
    bm = c_oracle.box_bitmask(np.asarray(box, np.float32), d['H'], d['W'], d['stride']) > 0
    rows, cols = np.nonzero(bm.any(1))[0], np.nonzero(bm.any(0))[0]
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def _hull_cols(d, box, dil):
    _, _, c0, c1 = _cells(d, box)
    return max(c0 - dil, 0), min(c1 + dil, d['w'])


def _tiles(d, box, dil):
    r0, r1, _, _ = _cells(d, box)
    h0, h1 = _hull_cols(d, box, dil)
    tw = 64 - 2 * dil
    return ((r1 - 1) // R - r0 // R + 1) * ((h1 - h0 + tw - 1) // tw)


# map A: 12 x 72 cells.  map B: 9 x 130 cells (rows not a multiple of 4).  Cell c has its sample at pixel 4 c + 2.
def _map_a():
    boxes = [[0, 0, 287, 47],          # touches all four borders: 72 columns = 60 + 12 (dilation 2) = 62 + 10 (dilation 1)
             [121, 21, 123, 23],       # one cell: (5, 30)
             [161, 5, 163, 41],        # one column (40), rows 1..9: narrower than the dilation
             [9, 9, 235, 31],          # cells 2..58: hull [0, 61) at dilation 2 -> tiles of 60 and ONE column
             [5, 1, 247, 39]]          # cells 1..61: hull [0, 63) at dilation 1 -> tiles of 62 and ONE column
    return _batch(12, 72, boxes, extra_inds=[3, 1], seed=41)       # two instances share box 3, two share the one-cell box


def _map_b():
    boxes = [[0, 0, 519, 35],          # all four borders: 130 columns = 60 + 60 + 10 = 62 + 62 + 6
             [9, 2, 475, 30],          # cells 2..118: hull [0, 121) at dilation 2 -> 60 + 60 + 1
             [5, 6, 495, 35],          # cells 1..123: hull [0, 125) at dilation 1 -> 62 + 62 + 1
             [301, 13, 303, 15],       # one cell: (3, 75)
             [401, 0, 403, 35]]        # one column (100), every row
    return _batch(9, 130, boxes, extra_inds=[1], seed=42)


def test_the_maps_have_the_tile_geometry_the_tests_are_about():
    """(no GPU work: the geometry the cases below rely on, computed the way the kernels compute it)"""
    a, b = _map_a(), _map_b()
    assert (a['h'], a['w'], b['h'], b['w']) == (12, 72, 9, 130)
    for d, i2, i1, n2, n1 in ((a, 3, 4, 2, 2), (b, 1, 2, 3, 3)):
        bx = d['gt_bboxes'][0]
        assert _cells(d, bx[0]) == (0, d['h'], 0, d['w'])
        h0, h1 = _hull_cols(d, bx[i2], 2)
        assert h0 == 0 and (h1 - h0) % 60 == 1 and (h1 - h0 + 59) // 60 == n2          # a last tile of one column < dilation 2
        h0, h1 = _hull_cols(d, bx[i1], 1)
        assert h0 == 0 and (h1 - h0) % 62 == 1 and (h1 - h0 + 61) // 62 == n1
    r0, r1, c0, c1 = _cells(a, a['gt_bboxes'][0][1])
    assert (r1 - r0, c1 - c0) == (1, 1)
    r0, r1, c0, c1 = _cells(a, a['gt_bboxes'][0][2])
    assert c1 - c0 == 1 and r1 - r0 > 4
    r0, r1, c0, c1 = _cells(b, b['gt_bboxes'][0][3])
    assert (r1 - r0, c1 - c0) == (1, 1)


def _against_oracle(d, got, ref, what):
    lp, lw, grad = got
    assert rel(lp, ref['loss_prj']) <= TOL, (what, lp, ref['loss_prj'])
    assert rel(lw, ref['loss_pairwise']) <= TOL or abs(lw - ref['loss_pairwise']) < 1e-7, (what, lw, ref['loss_pairwise'])
    err, ties = grad_report(grad, ref['grad'], d['mask_logits'][:, 0])
    assert err <= TOL, f'{what}: grad err {err:.3e} ({ties} ambiguous arg-max lines excluded)'
    err = grad_check_all_lines(grad, expected_grad_logit_first(d, ref, 1.0))
    assert err <= TOL, f'{what}: grad err {err:.3e} over every line'


def _with_targets(d, dev, **kw):
    from boxinstseg_amd import boxinst_mask_loss, functional as Fh
    Fh.DEBUG_KEEP_LAST = True
    t = to_dev(d, dev)
    tg = Fh.prepare_targets(t['imgs'], d['img_metas'], t['gt_bboxes'], out_stride=d['stride'], **kw)
    assert tg is not None
    x = t['logits'].clone().requires_grad_(True)
    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], out_stride=d['stride'], targets=tg,
                            warmup_factor=1.0, **kw)
    (out['loss_prj'] + out['loss_pairwise']).backward()
    torch.cuda.synchronize()
    assert tuple(Fh.last_eval_status()) == (0, R)
    return float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), x.grad.cpu().numpy()[:, 0]


def _three_forms(d, dev, dil):
    """(single launch, two launches, targets ready) with 4-row tiles, each checked to have launched the kernel it is named for."""
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    res = []
    for form, ready, want in ((_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4, False, {'eval1'}),
                              (_lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4, False, {'prep', 'pair'}),
                              (_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4, True, {'eval1_ready'})):
        names = []
        cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
        lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
        try:
            with Fh.eval_flags(form):
                res.append(_with_targets(d, dev, pairwise_dilation=dil) if ready else hip_loss(d, dev, pairwise_dilation=dil))
        finally:
            lib.bxi_dev_set_launch_hook(None, None)
        assert want <= set(names), (form, ready, names)
        assert tuple(Fh.last_eval_status()) == (0, R)
    return res


_REF = {}


def _ref(name, d, dil):
    """The oracle's answer, computed once per (map, dilation) and shared."""
    key = (name, dil)
    if key not in _REF:
        _REF[key] = oracle_path(d, want_targets=False, size=3, dil=dil)
    return _REF[key]


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('name', ['map_12x72', 'map_9x130'])
def test_tile_geometry_three_forms_against_the_oracle_and_each_other(dev, name, dil):
    d = _map_a() if name == 'map_12x72' else _map_b()
    ref = _ref(name, d, dil)
    one, two, ready = _three_forms(d, dev, dil)
    for what, got in (('single launch', one), ('two launches', two), ('targets ready', ready)):
        _against_oracle(d, got, ref, what)
    for what, got in (('two launches', two), ('targets ready', ready)):
        assert got[0] == one[0] and got[1] == one[1], (what, got[:2], one[:2])
        assert np.array_equal(got[2], one[2]), what


@pytest.mark.parametrize('dil', [1, 2])
def test_a_log_space_tile_between_tiles_of_the_split_loop(dev, dil):
    """Logits of +40 and -40 inside ONE column tile of the instance that spans the map: that wave takes slow_tile (whose LDS is the same
    bytes the split loop parks its terms in), its neighbours in the same workgroup take the split loop."""
    d = _map_b()
    d['mask_logits'] = d['mask_logits'].copy()
    d['mask_logits'][0, 0, 0, 5] = 40.0           # rows 0 and 1: the tile of rows 0..3, columns 0..59 / 61 of instance 0 only (the next row
    d['mask_logits'][0, 0, 1, 6] = -40.0          # tile's halo starts at row 4 - dilation >= 2)
    assert (np.abs(d['mask_logits']) > 34).sum() == 2
    ref = oracle_path(d, want_targets=False, size=3, dil=dil)
    one, two, ready = _three_forms(d, dev, dil)
    for what, got in (('single launch', one), ('two launches', two), ('targets ready', ready)):
        _against_oracle(d, got, ref, what)
        assert got[0] == one[0] and got[1] == one[1] and np.array_equal(got[2], one[2]), what


def test_a_wave_that_walks_several_tiles(dev):
    """80 instances on 16 x 64 maps, two launches, 4-row tiles, on a stream restricted to 8 CUs: 64 tile workgroups = 256 tile waves for
    more than 320 tiles, so a quarter of the waves park the terms of a second tile in the LDS and the registers that held the first one's.
    Against the oracle; a second evaluation must give the same bits."""
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    d = synthetic.make_batch(B=2, H=64, W=256, boxes_per_img=40, seed=43, min_box=40, max_box=250)
    assert (d['N'], d['h'], d['w']) == (80, 16, 64)
    tiles = sum(_tiles(d, np.concatenate(d['gt_bboxes'])[g], 2) for g in d['gt_inds'])
    assert tiles >= 64 * 4 + 64, tiles             # 64 waves or more take a second tile
    ref = oracle_path(d, want_targets=False, size=3, dil=2)
    lib = _lib.load()
    hip = C.CDLL('libamdhip64.so')
    stream = C.c_void_p()
    mask = (C.c_uint32 * 8)(0xff, 0, 0, 0, 0, 0, 0, 0)
    assert hip.hipExtStreamCreateWithCUMask(C.byref(stream), 8, mask) == 0
    try:
        ext = torch.cuda.ExternalStream(stream.value, device=dev)
        t = to_dev(d, dev)
        torch.cuda.synchronize()
        Fh.DEBUG_KEEP_LAST = True
        res = []
        for _ in range(2):
            names = []
            cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
            lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
            try:
                with torch.cuda.stream(ext), Fh.eval_flags(_lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4):
                    x = t['logits'].clone().requires_grad_(True)
                    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], out_stride=d['stride'],
                                            warmup_factor=1.0)
                    (out['loss_prj'] + out['loss_pairwise']).backward()
            finally:
                lib.bxi_dev_set_launch_hook(None, None)
            torch.cuda.synchronize()
            assert 'prep' in names and 'pair' in names, names
            assert tuple(Fh.last_eval_status()) == (0, R)
            res.append((float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), x.grad.cpu().numpy()[:, 0]))
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(stream)
    _against_oracle(d, res[0], ref, 'first evaluation')
    assert res[1][0] == res[0][0] and res[1][1] == res[0][1] and np.array_equal(res[1][2], res[0][2])


def test_a_wave_of_the_single_launch_that_walks_several_tiles(dev):
    """The same in the kernel that runs the split loop whatever the switches of the others: 120 instances with boxes of half the image and
    more on 64 x 256 maps, ONE launch with 4-row tiles -- more than 4096 + 256 tiles for the 4096 tile waves of a full device (the stream
    workgroups' waves among them), so hundreds of waves take a second tile.  Against the oracle; evaluated twice, identical bits."""
    from boxinstseg_amd import _lib, functional as Fh
    d = synthetic.make_batch(B=2, H=256, W=1024, boxes_per_img=60, seed=44, min_box=1000, max_box=1024)
    assert (d['N'], d['h'], d['w']) == (120, 64, 256)
    tiles = sum(_tiles(d, np.concatenate(d['gt_bboxes'])[g], 2) for g in d['gt_inds'])
    assert tiles >= 4096 + 256, tiles
    ref = oracle_path(d, want_targets=False, size=3, dil=2)
    lib = _lib.load()
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        with Fh.eval_flags(_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4):
            res = [hip_loss(d, dev), hip_loss(d, dev)]
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert names.count('eval1') >= 2 and 'pair' not in names, names
    assert tuple(Fh.last_eval_status()) == (0, R)
    _against_oracle(d, res[0], ref, 'first evaluation')
    assert res[1][0] == res[0][0] and res[1][1] == res[0][1] and np.array_equal(res[1][2], res[0][2])


@pytest.mark.parametrize('dil', [1, 2])
def test_poisoned_outputs_and_scratch_change_nothing(dev, dil):
    """The first case again with every torch.empty buffer the evaluation is handed (losses, gradient, loss state, scratch) filled with a
    NaN pattern beforehand, on a workspace of its own (zeroed, as the ABI asks of an evaluation's workspace): what a tile wave parks is
    its own, so the bits are those of the clean run."""
    from boxinstseg_amd import functional as Fh
    d = _map_a()
    ref = _ref('map_12x72', d, dil)
    clean = _three_forms(d, dev, dil)
    Fh.reset_eval_state()
    with poisoned_empty():
        dirty = _three_forms(d, dev, dil)
    for c, g in zip(clean, dirty):
        _against_oracle(d, g, ref, 'poisoned')
        assert g[0] == c[0] and g[1] == c[1] and np.array_equal(g[2], c[2])
