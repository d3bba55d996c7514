"""CPU: the host side of BoxLevelSet's mask predictions (no kernel is launched here).

* tests/box_solo_masks_ref.py reproduces tests/golden/box_solo_masks.npz (the reference's own statements, executed by
  tests/golden/make_golden_box_solo_masks.py) in fp64: rows, grad_feat and every grad_kernel map;
* resize-then-multiply (the order of the kernels) equals multiply-then-resize to 1e-12 in fp64, and the weight rule of
  include/boxinst/boxinst_hip_dconvl.h equals F.interpolate to 1e-12 in fp64 on the cases' sizes;
* every argument error of box_solov2_ins_preds, box_solov2_set_cells and box_solov2_get_seg_single_kernels is raised, shapes before the
  device; bxi_solo_dconvl_forward_f32 / _backward_f32 validate their arguments before anything touches a device, in the stated order;
* the header's limits are those of _lib, the build lists the source and the header;
* the level sizes of every configs/boxlevelset pipeline (tests/golden/box_solo_masks_cfg.json: scales, Pad divisor, strides) lie inside
  the support set;
* the documents name the feature."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import box_solo_masks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'box_solo_masks.npz')
X = 0x1000                                                                    # a pointer nothing dereferences


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_reproduces_the_golden(golden, name):
    case = R.make_case(**R.CASES[name])
    assert np.array_equal(golden[f'{name}/feat'], case['feat'])
    for l in range(5):
        assert np.array_equal(golden[f'{name}/map{l}'], case['maps'][l]) and np.array_equal(golden[f'{name}/labels{l}'], case['labels'][l])
        assert np.array_equal(golden[f'{name}/g{l}'], case['g'][l])
    rows, gfeat, gmaps = R.run_ref(case, torch.float64)
    for l in range(5):
        assert rows[l].shape == (sum(case['counts'][l]),) + case['sizes'][l]
        assert np.array_equal(golden[f'{name}/rows{l}'], rows[l]) and np.array_equal(golden[f'{name}/gmap{l}'], gmaps[l]), l
    assert np.array_equal(golden[f'{name}/gfeat'], gfeat)
    for what in ('rows', 'gfeat', 'gmap'):
        assert 0 < float(golden[f'{name}/tol_{what}']) < 1e-5, what


@pytest.mark.parametrize('name', list(R.CASES) + list(R.EXACT_CASES))
def test_the_two_orders_agree_in_fp64(name):
    case = R.make_case(**{**R.CASES, **R.EXACT_CASES}[name])
    a, b = R.run_ref(case, torch.float64), R.run_ref(case, torch.float64, R.resized_first)
    top = max(1.0, float(np.abs(R.flat(a[0])).max()))
    assert np.abs(R.flat(a[0]) - R.flat(b[0])).max() <= 1e-12 * top
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * max(1.0, float(np.abs(a[1]).max()))
    assert np.abs(R.flat(a[2]) - R.flat(b[2])).max() <= 1e-12 * max(1.0, float(np.abs(R.flat(a[2])).max()))
    if name in R.EXACT_CASES:                                                 # integers and weights 1, 1/2: equal, and exact in fp32 too
        assert np.array_equal(R.flat(a[0]), R.flat(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(R.flat(a[2]), R.flat(b[2]))
        c = R.run_ref(case, torch.float32, R.resized_first)
        assert np.array_equal(R.flat(a[0]), R.flat(c[0])) and np.array_equal(a[1], c[1]) and np.array_equal(R.flat(a[2]), R.flat(c[2]))
        assert float(np.abs(a[1]).max()) < 2 ** 24 and float(np.abs(R.flat(a[2])).max()) < 2 ** 24


def test_the_weight_rule_is_interpolate():
    rng = torch.Generator().manual_seed(3)
    for spec in R.CASES.values():
        x = torch.randn(2, 3, spec['H'], spec['W'], generator=rng, dtype=torch.float64)
        for oh, ow in spec['sizes']:
            want = F.interpolate(x, size=(oh, ow), mode='bilinear')
            assert (R.resize_by_taps(x, oh, ow) - want).abs().max() <= 1e-12
    i0, i1, l0, l1 = R.taps(16, 8)                                            # ratio 2: taps 2d, 2d + 1, weights 1/2
    assert i0.tolist() == list(range(0, 16, 2)) and i1.tolist() == list(range(1, 16, 2)) and bool((l0 == 0.5).all()) and bool((l1 == 0.5).all())
    i0, i1, l0, l1 = R.taps(13, 14)                                           # up-size: the first and the last tap are clamped
    assert i0[0] == 0 and l1[0] == 0 and i0[-1] == 12 and i1[-1] == 12


def test_the_adjoints_candidate_range_holds_every_tap():
    """csrc/solo_dconv_level.hip visits, for a source index, the outputs of tap_range() and lets taps_of() decide.  Both restated here in
    numpy fp32 (one rounding per operation, as the kernel's __f*_rn): over every in <= 40 and every out of the support set, no output that
    taps an index lies outside that index's range."""
    f32 = np.float32
    for n_in in range(1, 41):
        for n_out in range(-(-n_in // 8), 2 * n_in + 1):
            scale, inv = f32(n_in) / f32(n_out), f32(n_out) / f32(n_in)
            dst = np.arange(n_out, dtype=np.float32)
            src = np.maximum(scale * (dst + f32(0.5)) - f32(0.5), f32(0))
            i0 = np.minimum(src.astype(np.int64), n_in - 1)
            i1 = np.minimum(i0 + 1, n_in - 1)
            at = np.arange(n_in, dtype=np.float32)
            lo = np.maximum(np.floor((at - f32(0.5)) * inv - f32(0.5)).astype(np.int64), 0)
            hi = np.minimum(np.ceil((at + f32(1.5)) * inv - f32(0.5)).astype(np.int64), n_out - 1)
            o = np.arange(n_out)
            for idx in (i0, i1):
                assert bool(((lo[idx] <= o) & (o <= hi[idx])).all()), (n_in, n_out)
            entries = np.bincount(i0, minlength=n_in) + np.bincount(i1, minlength=n_in)
            assert int(entries.max()) <= 7 and int(entries.sum()) == 2 * n_out, (n_in, n_out)      # an index is tapped a few times at most
            assert int((hi - lo).max()) <= 2 * int(np.ceil(inv)) + 3, (n_in, n_out)


def _cpu_args(case):
    feat, maps, _, _ = R.to_torch(case, torch.float32)
    return maps, feat, R.cells_of(case), case['sizes']


def test_ins_preds_argument_errors():
    import boxinstseg_amd as B
    case = R.make_case(**R.CASES['ratios124'])
    maps, feat, cells, sizes = _cpu_args(case)
    with pytest.raises(RuntimeError, match='CUDA'):                           # everything right but the device: there is no fallback
        B.box_solov2_ins_preds(maps, feat, cells, sizes)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match='fp32 only'):
            B.box_solov2_ins_preds(maps, feat.to(dtype), cells, sizes)
        with pytest.raises(RuntimeError, match='fp32 only'):
            B.box_solov2_ins_preds(maps[:4] + [maps[4].to(dtype)], feat, cells, sizes)
    with pytest.raises(TypeError, match='tensor'):
        B.box_solov2_ins_preds(maps[:4] + [None], feat, cells, sizes)
    with pytest.raises(RuntimeError, match=r'\[B,E,h,w\]'):
        B.box_solov2_ins_preds(maps, feat[0], cells, sizes)
    with pytest.raises(RuntimeError, match='levels'):
        B.box_solov2_ins_preds([], feat, [], [])
    with pytest.raises(RuntimeError, match='levels'):
        B.box_solov2_ins_preds(maps * 2, feat, cells * 2, sizes * 2)
    with pytest.raises(RuntimeError, match=r'\[level\]\[image\]'):
        B.box_solov2_ins_preds(maps, feat, cells[:4], sizes)
    with pytest.raises(RuntimeError, match=r'\[level\]\[image\]'):
        B.box_solov2_ins_preds(maps, feat, [c[:1] for c in cells], sizes)
    with pytest.raises(RuntimeError, match='pairs'):
        B.box_solov2_ins_preds(maps, feat, cells, sizes[:4])
    with pytest.raises(RuntimeError, match='pairs'):
        B.box_solov2_ins_preds(maps, feat, cells, [(16, 24, 1)] + sizes[1:])
    with pytest.raises(RuntimeError, match='positive'):
        B.box_solov2_ins_preds(maps, feat, cells, [(0, 24)] + sizes[1:])
    with pytest.raises(RuntimeError, match=r'kernel_preds\[1\]'):
        B.box_solov2_ins_preds([maps[0], maps[1][:, :5]] + maps[2:], feat, cells, sizes)
    with pytest.raises(RuntimeError, match=r'kernel_preds\[0\]'):
        B.box_solov2_ins_preds([maps[0][:1]] + maps[1:], feat, cells, sizes)
    with pytest.raises(RuntimeError, match=r'kernel_preds\[2\]'):
        B.box_solov2_ins_preds(maps[:2] + [maps[2][:, :, :, :2]] + maps[3:], feat, cells, sizes)
    with pytest.raises(RuntimeError, match=r'cells\[0\]\[1\] must be an int64 vector'):
        B.box_solov2_ins_preds(maps, feat, [[cells[0][0], cells[0][1].int()]] + cells[1:], sizes)
    with pytest.raises(RuntimeError, match='int64 vector'):
        B.box_solov2_ins_preds(maps, feat, [[cells[0][0], cells[0][1].view(1, -1)]] + cells[1:], sizes)
    with pytest.raises(RuntimeError, match='status'):
        B.box_solov2_ins_preds(maps, feat, cells, sizes, status=torch.zeros(1))
    # outside the support set: said before a device is asked for, naming the header
    for bad in ((1, 24), (16, 2), (33, 24), (16, 49)):
        with pytest.raises(NotImplementedError, match='boxinst_hip_dconvl.h'):
            B.box_solov2_ins_preds(maps, feat, cells, sizes[:4] + [bad])
    for edge in ((2, 3), (32, 48)):                                           # 16 / 2 = 8, 24 / 3 = 8; 2 x: the limits themselves are inside
        with pytest.raises(RuntimeError, match='CUDA'):
            B.box_solov2_ins_preds(maps, feat, cells, sizes[:4] + [edge])


def test_set_cells_and_get_seg_argument_errors():
    import boxinstseg_amd as B
    for bad in (types.SimpleNamespace(mode='discobox'), object()):
        with pytest.raises(RuntimeError, match='boxlevelset'):
            B.box_solov2_set_cells(bad)
    # on CPU tensors the selection itself runs: nonzero of the labels, cut to the counts
    lab = [torch.tensor([0, 1, 0, 1, 1, 0, 0, 0], dtype=torch.bool), torch.tensor([1, 0], dtype=torch.bool)]
    t = types.SimpleNamespace(mode='boxlevelset', B=2, num_grids=[2, 1], ins_ind_labels=lab, counts=[[(0, 2), (0, 1)], [(0, 1), (0, 0)]])
    got = B.box_solov2_set_cells(t)
    assert [[c.tolist() for c in row] for row in got] == [[[1, 3], [0]], [[0], []]] and all(c.dtype == torch.int64 for row in got for c in row)
    meta, cfg = dict(img_shape=(20, 28, 3), ori_shape=(20, 28, 3)), dict(score_thr=0.1)
    cate, feat, kern = torch.rand(5, 2), torch.rand(1, 4, 5, 7), torch.rand(5, 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box_solov2_get_seg_single_kernels(cate, feat, kern, (5, 7), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='cate_preds'):
        B.box_solov2_get_seg_single_kernels(cate[:4], feat, kern, (5, 7), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='cate_preds'):
        B.box_solov2_get_seg_single_kernels(cate, feat, kern[0], (5, 7), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='mask_feat'):
        B.box_solov2_get_seg_single_kernels(cate, feat[:, :3], kern, (5, 7), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='mask_feat'):
        B.box_solov2_get_seg_single_kernels(cate, feat[0], kern, (5, 7), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='seg_num_grids'):
        B.box_solov2_get_seg_single_kernels(cate, feat, kern, (5, 7), meta, cfg, [2, 2], [8, 16])
    with pytest.raises(RuntimeError, match='seg_num_grids'):
        B.box_solov2_get_seg_single_kernels(cate, feat, kern, (5, 7), meta, cfg, [2, 1], [8])


def _callers():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    d = dict(feat=X, B=2, E=5, H=8, W=12, maps=[X, X, X], grids=[3, 2, 2], sizes=[8, 12, 4, 6, 4, 6], L=3, cells=X, counts=[2, 1, 0, 1, 1, 0], N=5,
             out=X, status=X, gout=X, gfeat=X, gmaps=[X, X, X], ws=X)

    def arrays(a):
        return [None if a[k] is None else f(a[k]) for k, f in (('maps', lambda m: _lib.ptr_array([p or 0 for p in m])), ('grids', _lib.int_array),
                                                               ('sizes', _lib.int_array), ('counts', _lib.int_array))]

    def size(which, **k):
        a = {**d, **k}
        _, _, sizes, counts = arrays(a)
        return getattr(lib, f'bxi_solo_dconvl_{which}_workspace_bytes')(a['B'], a['E'], a['H'], a['W'], sizes, counts, a['L'])

    def fwd(**k):
        a = {**d, 'bytes': size('forward'), **k}
        maps, grids, sizes, counts = arrays(a)
        return lib.bxi_solo_dconvl_forward_f32(a['feat'], a['B'], a['E'], a['H'], a['W'], maps, grids, sizes, a['L'], a['cells'], counts, a['N'], a['out'],
                                               a['status'], a['ws'], a['bytes'], None)

    def bwd(**k):
        a = {**d, 'bytes': size('backward'), **k}
        maps, grids, sizes, counts = arrays(a)
        gmaps = None if a['gmaps'] is None else _lib.ptr_array([m or 0 for m in a['gmaps']])
        return lib.bxi_solo_dconvl_backward_f32(a['feat'], a['B'], a['E'], a['H'], a['W'], maps, grids, sizes, a['L'], a['cells'], counts, a['N'], a['gout'],
                                                a['gfeat'], gmaps, a['status'], a['ws'], a['bytes'], None)
    return lib, fwd, bwd, size


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib, fwd, bwd, size = _callers()
    # forward: the resized feature of the one resampled group (2 x 5 x 4 x 6 floats), then the product's own workspace for its 2 rows;
    # backward: the feature gradient of both groups, the resized feature, the product's largest backward workspace
    sub_f = max(lib.bxi_solo_dconv_forward_workspace_bytes(3, 2, 5), lib.bxi_solo_dconv_forward_workspace_bytes(2, 2, 5))
    sub_b = max(lib.bxi_solo_dconv_backward_workspace_bytes(3, 2, 5, 8, 12), lib.bxi_solo_dconv_backward_workspace_bytes(2, 2, 5, 4, 6))
    assert size('forward') == 4 * 240 + sub_f and size('backward') == 4 * (960 + 240 + 240) + sub_b
    assert size('forward', counts=[0] * 6) == 0 and size('backward', counts=[0] * 6) == 0
    assert size('forward', counts=[2, 1, 0, 0, 0, 0]) == lib.bxi_solo_dconv_forward_workspace_bytes(3, 2, 5)          # no resampled group with rows
    for bad in (dict(B=0), dict(B=65), dict(E=0), dict(E=1025), dict(H=0), dict(L=0), dict(L=9), dict(sizes=[8, 12, 0, 6, 4, 6]), dict(counts=[2, 1, 0, -1, 1, 0]),
                dict(sizes=None), dict(counts=None), dict(sizes=[8, 12, 4, 1, 4, 6]), dict(sizes=[8, 12, 17, 6, 4, 6])):
        assert size('forward', **bad) == 0 and size('backward', **bad) == 0, bad
    for call in (fwd, bwd):
        for key in ('maps', 'grids', 'sizes', 'counts'):                      # the host arrays first
            assert call(**{key: None}) == -1 and call(**{key: None}, E=0) == -1, key
        assert call(B=0) == -2 and call(B=_lib.BXI_MAX_IMAGES + 1, counts=[0] * 195) == -2 and call(L=0) == -2 and call(E=0) == -2 and call(E=1025) == -2
        assert call(L=9, maps=[X] * 9, grids=[2] * 9, sizes=[8, 12] * 9, counts=[0] * 18) == -2
        assert call(H=0) == -2 and call(W=0) == -2 and call(N=-1) == -2 and call(N=4) == -2 and call(counts=[2, 1, 0, -1, 1, 2]) == -2
        assert call(grids=[3, 0, 2]) == -2 and call(sizes=[8, 12, 0, 6, 4, 6]) == -2 and call(sizes=[8, 12, 4, -1, 4, 6]) == -2
        assert call(E=1024, H=1024, W=1024) == -2
        # the support set: per axis in <= 8 out and out <= 2 in; answered before a device pointer or the workspace is looked at
        for bad in ([8, 12, 4, 1, 4, 6], [8, 12, 17, 6, 4, 6], [8, 12, 4, 6, 4, 25]):
            assert call(sizes=bad) == _lib.BXI_ERR_UNSUPPORTED and call(sizes=bad, out=None, gout=None, ws=None) == _lib.BXI_ERR_UNSUPPORTED, bad
        for good in ([8, 12, 1, 2, 4, 6], [8, 12, 16, 24, 4, 6]):
            assert call(sizes=good, ws=None) == -5, good
        for key in ('status', 'cells'):
            assert call(**{key: None}) == -1, key
        assert call(maps=[X, None, X]) == -1 and call(feat=None) == -1
        assert call(ws=None) == -5 and call(bytes=0) == -5 and call(ws=X + 8) == -5
    assert fwd(out=None) == -1 and fwd(bytes=size('forward') - 1) == -5 and bwd(bytes=size('backward') - 1) == -5
    assert bwd(gout=None) == -1 and bwd(gmaps=[X, None, X]) == -1
    assert bwd(feat=None, gmaps=None, ws=None) == -5                           # grad_feat alone does not read the feature
    # N == 0 touches nothing forward; with both gradients NULL the backward checks and returns
    zero = dict(N=0, counts=[0] * 6)
    assert fwd(**zero, feat=None, cells=None, out=None, status=None, maps=[None] * 3, ws=None, bytes=0) == 0
    assert fwd(**zero, E=0) == -2 and fwd(**zero, sizes=[8, 12, 4, 1, 4, 6]) == _lib.BXI_ERR_UNSUPPORTED
    assert bwd(gfeat=None, gmaps=None, gout=None, ws=None, bytes=0) == 0 and bwd(**zero, gfeat=None, gmaps=None, ws=None, bytes=0) == 0
    assert bwd(gfeat=None, gmaps=None, sizes=[8, 12, 4, 1, 4, 6]) == _lib.BXI_ERR_UNSUPPORTED


def test_header_table_and_build_agree():
    from boxinstseg_amd import _lib, build
    assert sorted(_lib.DCONVL_SIGNATURES) == ['bxi_solo_dconvl_backward_f32', 'bxi_solo_dconvl_backward_workspace_bytes',
                                              'bxi_solo_dconvl_forward_f32', 'bxi_solo_dconvl_forward_workspace_bytes']
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_dconvl.h')) as fh:
        text = fh.read()
    for name in ('DCONVL_MAX_DOWN', 'DCONVL_MAX_UP'):
        assert re.search(r'#define BXI_' + name + r' (\d+)', text).group(1) == str(getattr(_lib, name)), name
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_dconv.h')) as fh:
        base = fh.read()
    for name in ('DCONV_MAX_LEVELS', 'DCONV_MAX_E'):                          # B, L and E are bounded as in boxinst_hip_dconv.h
        assert re.search(r'#define BXI_' + name + r' (\d+)', base).group(1) == str(getattr(_lib, name)), name
    for word in ('fp32 only', 'BXI_ERR_UNSUPPORTED', 'DEVIATION', 'size group', 'no float atomics', 'BXI_DCONV_STATUS_BAD_CELL', 'align_corners=False'):
        assert word in text, word
    assert 'solo_dconv_level.hip' in build.SOURCES and any(h.endswith('boxinst_hip_dconvl.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, p)) for p in build.SOURCES + build.HEADERS)
    # no float atomics and no memset, here and in the product it runs (comments aside)
    for src in ('solo_dconv_level.hip', 'solo_dconv.hip', 'solo_dconv_device.hpp'):
        with open(os.path.join(build.CSRC, src)) as fh:
            code = '\n'.join(line.split('//')[0] for line in fh.read().splitlines())
        assert 'atomic' not in code.lower() and 'memset' not in code.lower(), src


def test_every_config_pipeline_is_inside_the_support_set():
    """Images are resized inside a scale and padded to the Pad divisor; the mask feature is a quarter of the padded size and level l is
    2 x ceil(padded / stride_l) (the reference's featmap_sizes[i] * 2)."""
    from boxinstseg_amd import box_solo_masks as M
    with open(os.path.join(ROOT, 'tests', 'golden', 'box_solo_masks_cfg.json')) as fh:
        cfgs = json.load(fh)
    assert len(cfgs) == 5
    seen = set()
    for name, c in cfgs.items():
        assert c['strides'] == [8, 8, 16, 32, 32] and c['size_divisors'] == [32], name
        div = c['size_divisors'][0]
        for long_side, short_side in c['img_scales']:
            top = -(-max(long_side, short_side) // div) * div
            for ph in range(div, top + 1, div):
                for pw in (div, ph, top):
                    h, w = ph // 4, pw // 4
                    sizes = [(2 * -(-ph // s), 2 * -(-pw // s)) for s in c['strides']]
                    M._supported(h, w, sizes)                                 # raises NotImplementedError outside
                    seen.update((h // oh, w // ow) for oh, ow in sizes)
    assert seen == {(1, 1), (2, 2), (4, 4)}                                   # the three size groups of the issue: ratios 1, 2 and 4


def test_exports_and_documents():
    import boxinstseg_amd as B
    from boxinstseg_amd import box_solo_masks
    for name in ('box_solov2_ins_preds', 'box_solov2_set_cells', 'box_solov2_get_seg_single_kernels'):
        assert name in B.__all__ and getattr(B, name) is getattr(box_solo_masks, name) and name in B.__doc__, name
    assert 'DEVIATION' in box_solo_masks.__doc__ and 'solo_dconv_level' in box_solo_masks.__doc__
    for rel, words in (('README.md', ('box_solov2_ins_preds', 'solo_dconv_level')),
                       ('DESIGN_NEXT_ROWS.md', ('solo_dconv_level', 'box_solov2_ins_preds')),
                       ('INTEGRATION.md', ('Level 3n', 'box_solov2_ins_preds', 'box_solov2_set_cells', 'box_solov2_get_seg_single_kernels',
                                           'boxinst_hip_dconvl.h')),
                       ('profiles/NOTES.md', ('R27-1', 'box_solo_masks_bench')), ('tools/README.md', ('box_solo_masks_bench.py',))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)
    with open(os.path.join(ROOT, 'DESIGN_NEXT_ROWS.md')) as fh:
        assert "Not built: `BoxSOLOv2Head.forward`'s grouped convolution" not in fh.read()
