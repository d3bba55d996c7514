"""CPU: the host side of RoIAlign and of the front of one level of DiscoBox's corr_loss (no kernel is launched here).

* tests/roi_ref.py, the restatement the GPU tests lean on, reproduces what the reference's own statements computed (tests/golden/roi_front.npz,
  make_golden_roi.py); with the reference present the case is regenerated live and compared;
* the restated RoIAlign -- mmcv's op never ran here, its arithmetic is unpinned -- equals a second statement built from F.grid_sample, and
  obeys rules checked by hand;
* the limits of include/boxinst/boxinst_hip_roi.h are those of _lib, and INTEGRATION.md names the feature (the header against
  _lib.ROI_SIGNATURES, the exports and the guarded tests: tests/test_abi_families.py);
* bad arguments, CPU tensors and pool_mode='max' fail before any launch."""
import importlib
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import roi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_roi.py')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
SPEC = R.load_cases()
LEVEL_KEYS = ('roi_s_feat', 'roi_t_feat', 'roi_s_mask', 'iiu')


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def test_restatement_reproduces_the_fixture():
    g = np.load(R.GOLDEN)
    inp, bank = R.inputs_of(g, dtype=torch.float64)
    inp['s_feat'].requires_grad_(True)
    out = R.corr_level(inp, bank, SPEC['cfg'])
    cs = SPEC['case']['census']
    assert out['keep'].tolist() == [bool(k) for k in cs['keep']] == g['level_keep'].astype(bool).tolist()
    assert out['labels'].tolist() == cs['labels'] == g['level_labels'].tolist() and out['count'].tolist() == cs['count'] == g['level_count'].tolist()
    assert np.array_equal(out['boxes'].numpy(), g['level_boxes']) and np.array_equal(out['ret_slot'].numpy(), g['level_ret_slot'])
    assert out['num_ins'] == int(g['level_num_ins']) == len(cs['ran']) and bank['bank_ptr'].tolist() == cs['ptr'] == g['level_after_ptr'].tolist()
    grad = torch.autograd.grad(out['loss_sum'], inp['s_feat'])[0]
    for k in LEVEL_KEYS:
        assert np.allclose(out[k].detach().numpy(), g[f'level_{k}'], rtol=1e-9, atol=1e-12), k
    assert np.allclose(float(out['loss_sum']), float(g['level_loss_sum']), rtol=1e-9) and np.allclose(grad.numpy(), g['level_g_level'], rtol=1e-9, atol=1e-12)
    for mine, key in ((bank['bank_feature'], 'after_feature'), (bank['bank_mask'], 'after_mask'), (bank['bank_box'], 'after_box')):
        assert np.allclose(mine.numpy(), g[f'level_{key}'], rtol=1e-9, atol=1e-12), key
    # the quirk is in the case: with its own label object 4 (label 2, an empty class) would not have run
    own = R.target_boxes(inp['target'], inp['kernel_labels'], own_labels=True)[2].tolist()
    assert own == [0, 2, -1, 1, 2, 0] and own != cs['labels']
    for k in [n for n in g.files if n.startswith('tol_')]:
        assert 0 < float(g[k]) < 1e-3, k                                   # measured, positive, of the size of float32 rounding


def test_fixture_is_what_the_reference_computes_now():
    """Live: the reference's statements, loaded where they lie, give the stored expectations again."""
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/models/dense_heads/discobox_head.py')):
        pytest.skip('the upstream checkout is not here')
    spec = importlib.util.spec_from_file_location('make_golden_roi', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert json.loads(json.dumps(gen.CASE)) == SPEC['case'] and gen.FACTOR == SPEC['factor']
    g = np.load(R.GOLDEN)
    corr = gen._corr_generator()
    live, tol = gen.level_arrays(gen.load_front(), corr, corr.load_reference())
    assert sorted(live) == sorted(k for k in g.files if not k.startswith('tol_'))
    for key, want in live.items():
        if want.dtype.kind != 'f' or want.dtype == np.float16:
            assert np.array_equal(g[key], want), key
        else:               # exp and log may differ by an ulp between builds of torch
            assert np.allclose(g[key], want, rtol=1e-11, atol=1e-13), key
    for k, v in tol.items():
        assert gen.FACTOR * v <= float(g[f'tol_{k}']) * 1.5, k


IN_CANVAS = torch.tensor([[0, 2, 3, 9, 10], [1, 0, 0, 20, 12], [0, 4, 1, 5, 2], [1, 3, 0, 18, 12], [0, 2, 3, 9, 10], [1, 0, 2, 15, 11.], [0, 1.3, 2.2, 11.7, 9.1]],
                         dtype=torch.float64)


@pytest.mark.parametrize('size', [7, 28, (5, 3)])
def test_restatement_equals_the_grid_sample_form(size):
    torch.manual_seed(3)
    feat = torch.randn(2, 5, 12, 20, dtype=torch.float64, requires_grad=True)
    a, b = R.roi_align(feat, IN_CANVAS, size), R.roi_align_grid_sample(feat, IN_CANVAS, size)
    assert torch.allclose(a, b, rtol=1e-9, atol=1e-12)
    g = torch.randn_like(a)
    ga, gb = torch.autograd.grad((a * g).sum(), feat)[0], torch.autograd.grad((b * g).sum(), feat)[0]
    assert torch.allclose(ga, gb, rtol=1e-9, atol=1e-12)


def test_restatement_rules_by_hand():
    torch.manual_seed(4)
    H, W = 12, 20
    for dt in (torch.float64, torch.float32):
        feat = torch.randn(2, 5, H, W, dtype=dt)
        # aligned: the 7 x 7 output of (2, 3, 9, 10) has unit bins and every sample on a pixel centre
        assert torch.equal(R.roi_align(feat, torch.tensor([[0, 2, 3, 9, 10.]]), 7)[0], feat[0, :, 3:10, 2:9])
    rois = torch.tensor([[0, 1.5, 2.25, 13.0, 9.5], [1, 0, 0, 20, 12], [1, 6, 3, 7, 4]], dtype=torch.float64)
    const = torch.full((2, 3, H, W), 3.25, dtype=torch.float64)
    assert torch.allclose(R.roi_align(const, rois, 7), torch.full((3, 3, 7, 7), 3.25, dtype=torch.float64), rtol=1e-13)
    # a ramp gives the ramp at the bin centres while every sample stays in [0, H-1] x [0, W-1]: the mean of a bin's samples is its centre
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    ramp = (0.5 * ys - 0.25 * xs + 2.0)[None, None].repeat(2, 1, 1, 1).requires_grad_(True)
    box = torch.tensor([[1, 2.5, 1.5, 16.0, 10.25]], dtype=torch.float64)
    out = R.roi_align(ramp, box, (7, 5))
    cy = (1.5 - 0.5) + (torch.arange(7, dtype=torch.float64) + 0.5) * (10.25 - 1.5) / 7
    cx = (2.5 - 0.5) + (torch.arange(5, dtype=torch.float64) + 0.5) * (16.0 - 2.5) / 5
    assert torch.allclose(out[0, 0], 0.5 * cy[:, None] - 0.25 * cx[None, :] + 2.0, rtol=1e-12)
    g = torch.randn(1, 1, 7, 5, dtype=torch.float64)
    gin = torch.autograd.grad((out * g).sum(), ramp)[0]
    assert float(gin.sum()) == pytest.approx(float(g.sum()), rel=1e-12) and float(gin[0].abs().max()) == 0.0     # the weights of a sample add up to 1
    # a sample beyond -1 or H contributes 0; one AT -1 or H is clamped to the border and counts
    ones = torch.ones(1, 1, H, W, dtype=torch.float64)
    lo = R.roi_align(ones, torch.tensor([[0, -6, -6, 1, 1.]], dtype=torch.float64), 7, sampling_ratio=1)[0, 0]      # samples at -6 .. 0
    want = torch.zeros(7, 7, dtype=torch.float64)
    want[5:, 5:] = 1.0
    assert torch.equal(lo, want)
    hi = R.roi_align(ones, torch.tensor([[0, W - 1, H - 1, W + 6, H + 6.]], dtype=torch.float64), 7, sampling_ratio=1)[0, 0]   # samples at H-1 .. H+5
    want = torch.zeros(7, 7, dtype=torch.float64)
    want[:2, :2] = 1.0
    assert torch.equal(hi, want)
    # aligned=False clamps rw and rh to 1: two bins of 0.5 over [3, 4], not of 0.1 over [3, 3.2]
    xramp = xs[None, None].clone()
    out = R.roi_align(xramp, torch.tensor([[0, 3, 3, 3.2, 3.4]], dtype=torch.float64), 2, sampling_ratio=1, aligned=False)
    assert torch.allclose(out[0, 0], torch.tensor([[3.25, 3.75], [3.25, 3.75]], dtype=torch.float64), rtol=1e-13)
    # relu_and_l2_norm_feat: all channels <= 0 gives 0; one positive channel p gives p / (sqrt(p^2 + 1e-6) + 1e-6)
    f = torch.tensor([-1.0, 0.0, -3.0], dtype=torch.float64).view(1, 3, 1, 1)
    assert float(R.relu_and_l2_norm_feat(f).abs().max()) == 0.0
    f = torch.tensor([-1.0, 2.0, -3.0], dtype=torch.float64).view(1, 3, 1, 1)
    assert float(R.relu_and_l2_norm_feat(f)[0, 1]) == pytest.approx(2.0 / ((4.0 + 1e-6) ** 0.5 + 1e-6), rel=1e-14)


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[roi]."""
    from boxinstseg_amd import _lib
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_roi.h')) as fh:
        code = fh.read()
    for macro, value in (('BXI_ROI_MAX_POOL', _lib.ROI_MAX_POOL), ('BXI_ROI_MAX_SAMPLING', _lib.ROI_MAX_SAMPLING), ('BXI_ROI_MAX_SIDE', _lib.ROI_MAX_SIDE),
                         ('BXI_ROI_FUSED_MAX_C', _lib.ROI_FUSED_MAX_C), ('BXI_ROI_FEAT', _lib.ROI_FEAT), ('BXI_ROI_SIGMOID', _lib.ROI_SIGMOID)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', code).group(1)) == value, macro
    assert (R.FEAT, R.MASK) == (_lib.ROI_FEAT, _lib.CORR_MASK) == (_lib.CORR_FEAT, 28)
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3h', 'corr_level', 'unpinned', 'own_labels', "pool_mode='max'", 'img_roi_align', 'bxi_roi_feat_norm_forward_f32', 'BXI_ERR_UNSUPPORTED'):
        assert word in integration, word


def test_exports_and_pool_mode_max():
    import boxinstseg_amd as B
    mod = importlib.import_module('boxinstseg_amd.roi_align')
    for name in ('roi_align', 'RoIAlign', 'relu_and_l2_norm_feat', 'roi_feat_norm', 'sigmoid_roi_masks', 'target_boxes', 'corr_level'):
        assert name in B.__all__ and getattr(B, name) is getattr(mod, name) and name in B.__doc__
    x, r = torch.zeros(1, 1, 4, 4), torch.zeros(1, 5)
    with pytest.raises(NotImplementedError, match='max'):
        B.roi_align(x, r, 7, pool_mode='max')
    with pytest.raises(NotImplementedError, match='max'):
        B.RoIAlign(7, pool_mode='max')
    m = B.RoIAlign((7, 5), spatial_scale=0.25, sampling_ratio=2, aligned=False, use_torchvision=True)       # mmcv's constructor; use_torchvision is ignored
    assert (m.output_size, m.spatial_scale, m.sampling_ratio, m.pool_mode, m.aligned) == ((7, 5), 0.25, 2, 'avg', False) and 'RoIAlign(' in repr(m)
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())


def test_cpu_tensors_and_bad_arguments_fail_loudly():
    import boxinstseg_amd as B
    x, r = torch.zeros(2, 3, 8, 8), torch.zeros(4, 5)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.roi_align(x, r, 7)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.RoIAlign(7)(x, r)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.roi_feat_norm(x, r)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.relu_and_l2_norm_feat(x)
    with pytest.raises(RuntimeError, match=r'\[B,C,H,W\]'):
        B.roi_align(x[0], r, 7)
    for bad in (torch.zeros(4, 4), torch.zeros(5), torch.zeros(4, 5, 1)):
        with pytest.raises(RuntimeError, match=r'\[K,5\]'):
            B.roi_align(x, bad, 7)
    with pytest.raises(ValueError, match='output_size'):
        B.roi_align(x, r, 65)
    with pytest.raises(ValueError, match='output_size'):
        B.roi_align(x, r, (7, 0))
    with pytest.raises(ValueError, match='sampling_ratio'):
        B.roi_align(x, r, 7, sampling_ratio=-1)
    with pytest.raises(ValueError, match='spatial_scale'):
        B.roi_align(x, r, 7, spatial_scale=float('nan'))
    t, lab = torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.target_boxes(t, lab)
    with pytest.raises(RuntimeError, match='uint8'):
        B.target_boxes(t.float(), lab)
    with pytest.raises(RuntimeError, match='kernel_labels'):
        B.target_boxes(t, lab[:2])
    with pytest.raises(RuntimeError, match='boxes'):
        B.sigmoid_roi_masks(torch.zeros(3, 8, 8), torch.zeros(3, 5))
    kw = dict(num_class=2, len_queue=4, fg_iou_thresh=0.7, bg_iou_thresh=0.7, ratio_range=[0.9, 1.2], appear_thresh=0.7, max_retrieval_objs=5)
    bank, solver = B.ObjectBank(**kw), B.SemanticCorrSolver(1.0, 0.05, 3, 0.3, 10, 1, 9)
    s = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.corr_level(s, s, t, lab, lab, x, x, bank, solver, 4)
    with pytest.raises(RuntimeError, match='same'):
        B.corr_level(s, s[:2], t, lab, lab, x, x, bank, solver, 4)
    with pytest.raises(RuntimeError, match='img_inds'):
        B.corr_level(s, s, t, lab[:2], lab, x, x, bank, solver, 4)
    with pytest.raises(RuntimeError, match='s_feat'):
        B.corr_level(s, s, t, lab, lab, x, x[:, :2], bank, solver, 4)
    assert bank.feature is None                                              # nothing was allocated on the way


def test_abi_validation_without_device():
    """Every call fails before its launch: X is a non-NULL value that nothing dereferences."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X, nan = 0x1000, float('nan')
    fwd = lambda **k: lib.bxi_roi_align_forward_f32(k.get('inp', X), k.get('rois', X), 2, k.get('C', 5), k.get('H', 12), 20, k.get('K', 3), k.get('PH', 7), 7,  # noqa: E731
                                                    k.get('scale', 1.0), k.get('sr', 0), 1, k.get('flags', 0), k.get('out', X), None)
    assert fwd(PH=0) == -2 and fwd(PH=65) == -2 and fwd(H=0) == -2 and fwd(H=16385) == -2 and fwd(K=-1) == -2 and fwd(C=-1) == -2
    assert fwd(K=1 << 28) == -2                                                                   # K * C * PH * PW past 2^31
    assert fwd(scale=nan) == -3 and fwd(sr=-1) == -3 and fwd(sr=65) == -3 and fwd(flags=2) == -3
    assert fwd(rois=None) == -1 and fwd(out=None) == -1 and fwd(inp=None) == -1
    assert fwd(K=0, rois=None, out=None) == 0 and fwd(C=0, inp=None, out=None) == 0              # no-ops: nothing is touched
    bwd = lambda **k: lib.bxi_roi_align_backward_f32(k.get('g', X), X, 2, k.get('C', 5), 12, k.get('W', 20), 3, 7, k.get('PW', 7), k.get('scale', 1.0),  # noqa: E731
                                                     k.get('sr', 0), 1, k.get('gin', X), None)
    assert bwd(PW=0) == -2 and bwd(W=0) == -2 and bwd(W=1 << 20) == -2 and bwd(scale=nan) == -3 and bwd(sr=100) == -3
    assert bwd(gin=None) == -1 and bwd(g=None) == -1 and bwd(C=0, gin=None) == 0
    tb = lambda **k: lib.bxi_roi_target_boxes_u8(k.get('t', X), X, k.get('N', 3), k.get('H', 8), k.get('W', 8), 0, X, k.get('keep', X), X, None)  # noqa: E731
    assert tb(N=-1) == -2 and tb(H=0) == -2 and tb(H=65536, W=65536) == -2 and tb(t=None) == -1 and tb(keep=None) == -1 and tb(N=0, t=None) == 0
    q = lib.bxi_roi_feat_norm_workspace_bytes
    assert q(4, 32) == 4 * 49 * 4 + 4 * 32 * 49 * 4 and q(4, 32) % 16 == 0 and q(0, 32) == 16
    assert q(3, 5) == (3 * 49 * 4 + 15) // 16 * 16 + (3 * 5 * 49 * 4 + 15) // 16 * 16           # both arrays start on 16 bytes
    assert q(-1, 32) == 0 and q(4, 0) == 0 and q(4, _lib.ROI_FUSED_MAX_C + 1) == 0 and q(4, _lib.ROI_FUSED_MAX_C) > 0
    need = q(3, 32)
    ff = lambda **k: lib.bxi_roi_feat_norm_forward_f32(X, k.get('rois', X), 2, k.get('C', 32), 12, 20, 3, 1.0, k.get('sr', 0), 1, X, k.get('ws', X),  # noqa: E731
                                                       k.get('bytes', need), None)
    assert ff(C=0) == -2 and ff(C=_lib.ROI_FUSED_MAX_C + 1) == _lib.BXI_ERR_UNSUPPORTED and ff(sr=-2) == -3
    assert ff(ws=None) == -5 and ff(bytes=need - 1) == -5 and ff(ws=X + 4) == -5 and ff(ws=0x1000, rois=None) == -1
    fb = lambda **k: lib.bxi_roi_feat_norm_backward_f32(X, k.get('g', X), X, 2, k.get('C', 32), 12, 20, 3, 1.0, 0, 1, k.get('gin', X), k.get('ws', X),  # noqa: E731
                                                        k.get('bytes', need), None)
    assert fb(C=0) == -2 and fb(C=_lib.ROI_FUSED_MAX_C + 1) == _lib.BXI_ERR_UNSUPPORTED and fb(ws=None) == -5 and fb(bytes=16) == -5 and fb(ws=X + 8) == -5
    assert fb(gin=None) == -1 and fb(g=None) == -1
