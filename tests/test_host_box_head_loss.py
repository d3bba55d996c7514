"""CPU: the host side of the box head's training step (no kernel is launched here).

* tests/fcos_ref.py, the restatement the GPU tests lean on, reproduces what the reference's own code computed
  (tests/golden/box_head_loss.npz, make_golden_box_head_loss.py); with the reference present the fixture is regenerated live and compared;
* include/boxinst/boxinst_hip_fcos.h, the library's exports and _lib.FCOS_SIGNATURES name the same entry points, and each is run by a
  named guarded test or is a size query;
* the bbox_head block of every configs/boxinst file is accepted, an unsupported loss type raises;
* CPU tensors and bad arguments fail before any launch."""
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import fcos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_JSON = os.path.join(ROOT, 'tests', 'golden', 'box_head_cfg.json')
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_box_head_loss.py')
HEADER = os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_fcos.h')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
SPEC = R.load_cases()
MAPS = ('cls', 'bbox', 'ctr')


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def stored_inputs(g):
    return {k: [g[f'in_{k}{lv}'] for lv in range(len(SPEC['levels']))] for k in MAPS}


def settings(name):
    from boxinstseg_amd import parse_box_head_cfg
    return parse_box_head_cfg(R.head_cfg(SPEC, name))


def restated_targets(name, dtype):
    s = settings(name)
    boxes, labels = R.gt_of(SPEC, dtype)
    return R.targets(SPEC['levels'], s['strides'], boxes, labels, s['regress_ranges'], s['center_sampling'], s['center_sample_radius'],
                     s['norm_on_bbox'], s['num_classes'], dtype)


@pytest.mark.parametrize('name', sorted(SPEC['cases']))
def test_restatement_reproduces_the_reference(name):
    g = np.load(R.GOLDEN)
    inp = stored_inputs(g)
    made = R.make_inputs(SPEC, int(g['seed']))
    for k in MAPS:
        for a, b in zip(inp[k], made[k]):
            assert np.array_equal(a, b), f'the stored {k} are not the inputs of the recipe'
    assert any((m == 0).any() for m in inp['bbox']), 'exact zeros among the distances, as after a relu'
    tg32 = restated_targets(name, torch.float32)
    for k in R.TARGET_KEYS:
        assert np.array_equal(tg32[k].numpy(), g[f'{name}_{k}']) and tg32[k].numpy().dtype == g[f'{name}_{k}'].dtype, k
    tg64 = restated_targets(name, torch.float64)
    assert np.array_equal(tg64['stats'].numpy(), g[f'{name}_stats64'])
    got = R.losses_and_grads(inp, tg64, settings(name), torch.float64)
    assert np.allclose(got[0].numpy(), g[f'{name}_losses64'], rtol=1e-12, atol=0)
    for k, grads in zip(MAPS, got[1:]):
        for lv, gr in enumerate(grads):
            want = g[f'{name}_grad_{k}{lv}']
            assert np.allclose(gr.numpy(), want, rtol=1e-10, atol=1e-13 * np.abs(want).max()), (k, lv)
    # the measured tolerances: present, positive, of the size of float32 rounding, and they hold for the float32 run they were measured on
    for k in ('tol_stats', 'tol_losses', 'tol_grad_cls', 'tol_grad_bbox', 'tol_grad_ctr'):
        assert 0 < float(g[k]) < 1e-5, k
    l32, l64 = g[f'{name}_losses32'].astype(np.float64), g[f'{name}_losses64']
    assert (np.abs(l32 - l64) / np.abs(l64)).max() <= float(g['tol_losses'])
    # the census the issue states
    sizes = [h * w for h, w in SPEC['levels']]
    gi, at, counts = g[f'{name}_gt_inds'], 0, []
    for n in sizes:
        counts.append(int((gi[at:at + n] >= 0).sum()))
        img1 = gi[at + n:at + 2 * n]
        assert set(img1[img1 >= 0].tolist()) <= {5}, 'the equal-area tie goes to the first box of image 1'
        at += 2 * n
    assert counts == SPEC['positives_image0']['center_sampling' if SPEC['cases'][name]['center_sampling'] else 'inside_box']
    assert int((g[f'{name}_img_inds'][gi >= 0] == 1).sum()) == SPEC['positives_image1']


def test_restatement_rules_by_hand():
    # two boxes of equal area over the same point: the lower index wins; a point outside every box is background and carries box 0's distances
    boxes = [torch.tensor([[0., 0., 16., 8.], [0., 0., 8., 16.]])]
    labels = [torch.tensor([3, 1])]
    tg = R.targets([(2, 2)], [8], boxes, labels, [(-1, 1e8)], False, 1.5, False, 5)
    assert tg['labels'].tolist() == [3, 3, 1, 5] and tg['gt_inds'].tolist() == [0, 0, 1, -1]
    assert tg['bbox_targets'][3].tolist() == [12., 12., 4., -4.] and float(tg['ctr_targets'][3]) == 0.0
    assert tg['points'].tolist() == [[4., 4.], [12., 4.], [4., 12.], [12., 12.]]
    # an image without boxes: background, zeros, -1
    tg = R.targets([(1, 2)], [8], [torch.zeros(0, 4), boxes[0]], [torch.zeros(0, dtype=torch.int64), labels[0]], [(-1, 1e8)], False, 1.5, True, 5)
    assert tg['labels'].tolist() == [5, 5, 3, 3] and tg['gt_inds'].tolist() == [-1, -1, 0, 0] and tg['img_inds'].tolist() == [0, 0, 1, 1]
    assert bool((tg['bbox_targets'][:2] == 0).all()) and tg['bbox_targets'][2].tolist() == [0.5, 0.5, 1.5, 0.5]


@pytest.mark.parametrize('name', sorted(SPEC['cases']))
def test_fixture_is_what_the_reference_computes_now(name):
    """Live: the reference's code, loaded where it lies, gives the stored expectations again."""
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/models/dense_heads/condinst_head.py')):
        pytest.skip('the upstream checkout is not here')
    spec = importlib.util.spec_from_file_location('make_golden_box_head_loss', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(R.GOLDEN)
    inp = stored_inputs(g)
    assert gen.tie_margin(SPEC, inp, name) > 1.0
    live, tol = gen.reference_case(SPEC, inp, name)
    assert live and gen.restatement_agrees(SPEC, inp, name, live)
    for key, want in live.items():
        assert key in g, key
        if want.dtype.kind != 'f' or key.endswith(('_points', '_bbox_targets', '_ctr_targets')):      # targets: bit-equal
            assert np.array_equal(g[key], want), key
        else:   # losses and gradients pass through exp and log, which may differ by an ulp between builds of torch
            assert np.allclose(g[key], want, rtol=1e-5 if want.dtype == np.float32 else 1e-11, atol=1e-13), key
    for k, v in tol.items():
        assert v <= float(g[k]) * 1.5, k          # the stored tolerance is the largest over the cases (exp / log may move by an ulp)
    with open(CFG_JSON) as fh:
        assert json.load(fh) == gen.config_blocks(), 'tests/golden/box_head_cfg.json is not the bbox_head blocks of the reference any more'


def test_header_exports_and_signatures_agree():
    """(declarations, exports and ctypes signatures: tests/test_abi_families.py)"""
    from boxinstseg_amd import _lib, box_head_loss
    lib = _lib.load()
    with open(HEADER) as fh:
        text = fh.read()
    for macro, value in (('BXI_FCOS_GT_CHUNK', _lib.FCOS_GT_CHUNK), ('BXI_FCOS_LOC_TILE', _lib.FCOS_LOC_TILE), ('BXI_FCOS_ELEM_TILE', _lib.FCOS_ELEM_TILE),
                         ('BXI_FCOS_STATUS_BAD_LABEL', _lib.FCOS_STATUS_BAD_LABEL), ('BXI_FCOS_BBOX_GIOU', _lib.FCOS_BBOX_KINDS['giou']),
                         ('BXI_FCOS_BBOX_IOU_LOG', _lib.FCOS_BBOX_KINDS['iou_log']), ('BXI_FCOS_BBOX_IOU_LINEAR', _lib.FCOS_BBOX_KINDS['iou_linear']),
                         ('BXI_FCOS_BBOX_IOU_SQUARE', _lib.FCOS_BBOX_KINDS['iou_square'])):
        assert int(re.search(r'#define ' + macro + r' (\d+)', text).group(1)) == value, macro
    assert box_head_loss.GT_CHUNK == _lib.FCOS_GT_CHUNK
    assert lib.bxi_abi_version() == _lib.BXI_ABI_VERSION == 7                # additive: the version stays
    assert [f[0] for f in _lib.FcosLevel._fields_] == ['H', 'W', 'stride'] and [f[0] for f in _lib.FcosGrads._fields_] == ['cls', 'bbox', 'ctr']
    assert re.search(r'typedef struct \{ int H, W, stride; \} bxi_fcos_level;', text)
    assert re.search(r'typedef struct \{ float \*cls, \*bbox, \*ctr; \} bxi_fcos_grads;', text)
    for word in ('LOWEST box index', 'not enough values to unpack', 'restated, unpinned', 'BXI_ERR_UNSUPPORTED', 'mixed units'):
        assert word in text, word
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3e', 'not enough values to unpack', 'lowest box index', 'unpinned', 'DIoULoss', 'bxi_fcos_grad_rescale_f32'):
        assert word in integration, word


def test_reference_head_blocks_are_accepted():
    import boxinstseg_amd as B
    from boxinstseg_amd import box_head_loss
    with open(CFG_JSON) as fh:
        stored = json.load(fh)
    assert len(stored) == 7
    d = os.path.join(REFERENCE, 'configs', 'boxinst')
    if os.path.isdir(d):
        assert sorted(stored) == sorted(f for f in os.listdir(d) if f.endswith('.py'))
    for fname, block in stored.items():
        s = B.parse_box_head_cfg(block)
        assert s == dict(num_classes=20 if 'voc' in fname else 80, strides=[8, 16, 32, 64, 128],
                         regress_ranges=((-1.0, 64.0), (64.0, 128.0), (128.0, 256.0), (256.0, 512.0), (512.0, 1e8)), center_sampling=True,
                         center_sample_radius=1.5, norm_on_bbox=True, gamma=2.0, alpha=0.25, loss_weight_cls=1.0, bbox_loss_kind='giou', eps=1e-6,
                         loss_weight_bbox=1.0, loss_weight_centerness=1.0), fname
        ns = types.SimpleNamespace(**{k: (types.SimpleNamespace(**v) if isinstance(v, dict) else v) for k, v in block.items()})
        assert B.parse_box_head_cfg(ns) == s
    block = stored['boxinst_r50_fpn_1x_coco.py']
    for key, bad, word in (('loss_bbox', dict(type='DIoULoss', loss_weight=1.0), 'loss_bbox.type'), ('loss_bbox', dict(type='CIoULoss'), 'loss_bbox.type'),
                           ('loss_bbox', dict(type='BoundedIoULoss'), 'loss_bbox.type'), ('loss_cls', dict(type='QualityFocalLoss'), 'loss_cls.type'),
                           ('loss_cls', dict(type='FocalLoss', use_sigmoid=True, activated=True), 'loss_cls.activated'),
                           ('loss_centerness', dict(type='CrossEntropyLoss', use_sigmoid=False), 'loss_centerness'),
                           ('loss_centerness', dict(type='MSELoss'), 'loss_centerness.type'),
                           ('loss_bbox', dict(type='IoULoss', mode='cubic'), 'loss_bbox.mode'), ('loss_bbox', dict(type='GIoULoss', beta=1), 'loss_bbox.beta'),
                           ('type', 'FCOSHead', 'bbox_head.type')):
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            B.parse_box_head_cfg(dict(block, **{key: bad}))
    assert B.parse_box_head_cfg(dict(block, loss_bbox=dict(type='IoULoss', linear=True)))['bbox_loss_kind'] == 'iou_linear'
    assert B.parse_box_head_cfg(dict(block, loss_bbox=dict(type='IoULoss', mode='square', eps=1e-5)))['eps'] == 1e-5
    assert B.condinst_box_loss is box_head_loss.condinst_box_loss and B.condinst_box_targets is box_head_loss.condinst_box_targets
    for name in ('condinst_box_loss', 'condinst_box_targets', 'parse_box_head_cfg'):
        assert name in B.__all__ and name in B.__doc__


def test_reduce_mean_without_a_process_group_is_the_tensor_itself():
    from boxinstseg_amd import dist
    t = torch.tensor([3.0, 1.5])
    assert dist.reduce_mean(t) is t


def test_cpu_tensors_fail_loudly():
    import boxinstseg_amd as B
    g = np.load(R.GOLDEN)
    inp = {k: [torch.from_numpy(a) for a in v] for k, v in stored_inputs(g).items()}
    boxes, labels = R.gt_of(SPEC)
    cfg = R.head_cfg(SPEC, 'cs_norm_giou')
    with pytest.raises(RuntimeError, match='CUDA'):
        B.condinst_box_loss(inp['cls'], inp['bbox'], inp['ctr'], boxes, labels, None, cfg)
    s = settings('cs_norm_giou')
    with pytest.raises(RuntimeError, match='CUDA'):
        B.condinst_box_targets(SPEC['levels'], s['strides'], boxes, labels, regress_ranges=s['regress_ranges'], center_sampling=True,
                               center_sample_radius=1.5, norm_on_bbox=True, num_classes=5, B=2)
    with pytest.raises(RuntimeError, match='images'):
        B.condinst_box_targets(SPEC['levels'], s['strides'], boxes, labels, regress_ranges=s['regress_ranges'], center_sampling=True,
                               center_sample_radius=1.5, norm_on_bbox=True, num_classes=5, B=3)
    with pytest.raises(NotImplementedError, match='loss_bbox.type'):
        B.condinst_box_loss(inp['cls'], inp['bbox'], inp['ctr'], boxes, labels, None, dict(cfg, loss_bbox=dict(type='DIoULoss')))
    with pytest.raises(RuntimeError, match='levels'):
        B.condinst_box_loss(inp['cls'], inp['bbox'][:2], inp['ctr'], boxes, labels, None, cfg)


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000                                           # a non-NULL value no call below dereferences: every one fails before its launch
    big = 1 << 40
    nan = float('nan')

    def fl(n=2, H=3, W=5, stride=8):
        arr = (_lib.FcosLevel * max(n, 1))()
        for i in range(n):
            arr[i] = _lib.FcosLevel(H, W, stride)
        return arr

    wb = lib.bxi_fcos_workspace_bytes
    assert wb(fl(), 2, 0, 3) == 0 and wb(fl(), 2, 65, 3) == 0 and wb(fl(), 0, 2, 3) == 0 and wb(fl(), 9, 2, 3) == 0 and wb(fl(), 2, 2, 0) == 0
    assert wb(fl(H=0), 2, 2, 3) == 0 and wb(None, 2, 2, 3) == 0 and wb(fl(H=40000, W=40000), 2, 2, 3) == 0
    # two levels of 15 locations, B = 2, C = 3: 2 * 2 location workgroups, and one flat workgroup per level (90 logits each)
    assert wb(fl(), 2, 2, 3) == 16 * (4 + 2)
    assert wb(fl(n=1, H=20, W=20), 1, 3, 80) == 16 * (3 * 2 + (3 * 80 * 400 + 1023) // 1024)

    ranges = _lib.float_array([-1, 64, 64, 1e8])
    offs = _lib.int_array([0, 2, 3])

    def targets(lv=None, n=2, B=2, rg=ranges, cs=1, radius=1.5, C=5, boxes=X, labels=X, off=offs, ws=X, nbytes=big, **outs):
        o = dict(labels_=X, bt=X, gi=X, pts=X, li=X, ii=X, ct=X, stats=X, status=X)
        o.update(outs)
        return lib.bxi_fcos_targets_f32(fl(n) if lv is None else lv, n, B, rg, cs, radius, 1, C, boxes, labels, off, o['labels_'], o['bt'], o['gi'],
                                        o['pts'], o['li'], o['ii'], o['ct'], o['stats'], o['status'], ws, nbytes, None)
    assert targets(B=0) == 0
    assert targets(n=0) == -2 and targets(n=9) == -2 and targets(B=-1) == -2 and targets(B=65) == -2 and targets(C=0) == -2
    assert targets(lv=fl(H=0)) == -2 and targets(lv=fl(stride=0)) == -2 and targets(lv=fl(H=40000, W=40000)) == -2
    assert targets(off=_lib.int_array([1, 2, 3])) == -2 and targets(off=_lib.int_array([0, 3, 2])) == -2
    assert targets(radius=nan) == -3 and targets(radius=-1.0) == -3
    assert targets(rg=_lib.float_array([-1, nan, 64, 1e8])) == -3
    for name in ('rg', 'off', 'boxes', 'labels', 'labels_', 'bt', 'gi', 'pts', 'li', 'ii', 'ct', 'stats', 'status'):
        assert targets(**{name: None}) == -1, name
    assert lib.bxi_fcos_targets_f32(None, 2, 2, ranges, 1, 1.5, 1, 5, X, X, offs, X, X, X, X, X, X, X, X, X, X, big, None) == -1
    assert targets(ws=None) == -5 and targets(nbytes=16 * 4 - 1) == -5 and targets(ws=X + 2) == -5

    def dl(n=2, H=3, W=5, stride=8, cls=X):
        arr = (_lib.DetLevel * max(n, 1))()
        for i in range(n):
            arr[i] = _lib.DetLevel(cls, X, X, None, H, W, stride)
        return arr

    def gr(n=2, cls=X):
        arr = (_lib.FcosGrads * max(n, 1))()
        for i in range(n):
            arr[i] = _lib.FcosGrads(cls, X, X)
        return arr

    def loss(lv=None, n=2, B=2, C=3, labels=X, bt=X, ct=X, norm=X, gamma=2.0, alpha=0.25, lw=(1.0, 1.0, 1.0), kind=0, eps=1e-6, grads=None,
             losses=X, ws=X, nbytes=big, no_grads=False):
        return lib.bxi_fcos_loss_f32(dl(n) if lv is None else lv, n, B, C, labels, bt, ct, norm, gamma, alpha, lw[0], lw[1], lw[2], kind, eps,
                                     None if no_grads else (gr(n) if grads is None else grads), losses, ws, nbytes, None)
    assert loss(B=0) == 0
    assert loss(n=0) == -2 and loss(n=9) == -2 and loss(B=65) == -2 and loss(B=-1) == -2 and loss(C=0) == -2
    assert loss(lv=dl(H=0)) == -2 and loss(lv=dl(H=30000, W=30000), C=80) == -2
    assert loss(gamma=nan) == -3 and loss(gamma=-1.0) == -3 and loss(alpha=nan) == -3 and loss(eps=nan) == -3 and loss(eps=0.0) == -3
    assert loss(lw=(nan, 1.0, 1.0)) == -3 and loss(lw=(1.0, nan, 1.0)) == -3 and loss(lw=(1.0, 1.0, nan)) == -3
    assert loss(kind=4) == _lib.BXI_ERR_UNSUPPORTED and loss(kind=-1) == _lib.BXI_ERR_UNSUPPORTED
    for name in ('labels', 'bt', 'ct', 'norm', 'losses'):
        assert loss(**{name: None}) == -1, name
    assert loss(no_grads=True) == -1 and loss(lv=dl(cls=None)) == -1 and loss(grads=gr(cls=None)) == -1
    assert lib.bxi_fcos_loss_f32(None, 2, 2, 3, X, X, X, X, 2.0, 0.25, 1.0, 1.0, 1.0, 0, 1e-6, gr(), X, X, big, None) == -1
    assert loss(ws=None) == -5 and loss(nbytes=wb(fl(), 2, 2, 3) - 1) == -5 and loss(ws=X + 1) == -5

    def rescale(lv=None, n=2, B=2, C=3, unit=None, up=X, out=None, no_unit=False, no_out=False):
        return lib.bxi_fcos_grad_rescale_f32(fl(n) if lv is None else lv, n, B, C, None if no_unit else (gr(n) if unit is None else unit), up,
                                             None if no_out else (gr(n) if out is None else out), None)
    assert rescale(B=0) == 0
    assert rescale(n=0) == -2 and rescale(B=65) == -2 and rescale(C=0) == -2 and rescale(lv=fl(W=0)) == -2
    assert rescale(up=None) == -1 and rescale(no_unit=True) == -1 and rescale(no_out=True) == -1 and rescale(unit=gr(cls=None)) == -1
    assert rescale(out=gr(cls=None)) == -1
