"""HIP path vs CPU oracle on the same seeded inputs (run on a real MI355X: -m gpu).

Tolerances (north_star): losses within 1e-4 relative, gradient within 1e-4 * max|grad| of the fp32
oracle; the op-level kernels are also checked in fp64 (1e-10)."""
import numpy as np
import pytest
import torch

from boxinstseg_amd import synthetic
from tests.helpers import expected_grad_logit_first, grad_check_all_lines, grad_report, hip_loss, oracle_path, rel, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-4


# ---------------------------------------------------------------------------------------------
# op level: pairwise_nlog forward / backward  (mmdet.ops.pairwise)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,tol', [(np.float32, 2e-6), (np.float64, 1e-12)])
@pytest.mark.parametrize('shape,size,dil', [((3, 13, 17), 3, 2), ((2, 40, 24), 3, 1), ((2, 21, 33), 5, 2),
                                            ((1, 5, 3), 3, 3), ((4, 64, 64), 3, 2), ((2, 30, 70), 3, 4), ((1, 37, 150), 3, 6),
                                            ((1, 19, 130), 3, 2), ((2, 16, 64), 3, 8)])
def test_pairwise_op(dev, dtype, tol, shape, size, dil):
    from boxinstseg_amd import pairwise_nlog
    from oracle import c_oracle
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(shape) * 4).astype(dtype)
    want = c_oracle.pairwise_nlog_fwd(x, size, dil)
    gp = rng.standard_normal(want.shape).astype(dtype)
    want_g = c_oracle.pairwise_nlog_bwd(x, want, gp, size, dil)
    xt = torch.from_numpy(x[:, None]).to(dev).requires_grad_(True)
    out = pairwise_nlog(xt, size, dil)
    out.backward(torch.from_numpy(gp).to(dev))
    got = out.detach().cpu().numpy()
    got_g = xt.grad.cpu().numpy()[:, 0]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())
    assert np.abs(got_g - want_g).max() <= 10 * tol * max(1.0, np.abs(want_g).max())


@pytest.mark.parametrize('case', ['f32_3_2', 'f64_3_2', 'f32_5_1', 'f64_3_1'])
def test_pairwise_op_vs_reference_kernels_fixture(dev, case):
    """HIP op against what the reference's OWN pairwise.cu kernels produced (run on the CPU, tests/golden/pairwise_refk.npz)."""
    import os
    from boxinstseg_amd import pairwise_nlog
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'pairwise_refk.npz'))
    x, size, dil = g[f'{case}_logits'], int(g[f'{case}_size']), int(g[f'{case}_dil'])
    tol = 2e-6 if x.dtype == np.float32 else 1e-12
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = pairwise_nlog(xt, size, dil)
    out.backward(torch.from_numpy(g[f'{case}_gp']).to(dev))
    want, want_g = g[f'{case}_pairwise'], g[f'{case}_grad']
    assert np.abs(out.detach().cpu().numpy() - want).max() <= tol * max(1.0, np.abs(want).max())
    assert np.abs(xt.grad.cpu().numpy() - want_g).max() <= 10 * tol * max(1.0, np.abs(want_g).max())


def test_pairwise_op_vs_reference_kernels_live_full_size(dev):
    """BASELINE configs[1] size (32 x 200 x 256, window 3, dilation 2): the reference kernels run on this host's CPU where
    oracle/_ref is built (make -C oracle ref, from the reference tree); elsewhere the C oracle.  Either must reproduce the
    reference kernels' outputs bit for bit (their sha256, tests/golden/ref_kernels_live.npz)."""
    import hashlib
    import os
    from boxinstseg_amd import pairwise_nlog
    from oracle import c_oracle, pairwise_ref as pr
    rng = np.random.default_rng(5)
    x = (2.5 * rng.standard_normal((32, 1, 200, 256))).astype(np.float32)
    if pr.available():
        want = pr.forward(x, 3, 2)
    else:
        want = c_oracle.pairwise_nlog_fwd(x[:, 0], 3, 2)
    gp = rng.random(want.shape).astype(np.float32)
    if pr.available():
        want_g = pr.backward(x, want, gp, 3, 2)
    else:
        want_g = c_oracle.pairwise_nlog_bwd(x[:, 0], want, gp, 3, 2)[:, None]
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'ref_kernels_live.npz'))
    assert hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest() == str(g['pw_full_fwd_sha256'])
    assert hashlib.sha256(np.ascontiguousarray(want_g).tobytes()).hexdigest() == str(g['pw_full_bwd_sha256'])
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = pairwise_nlog(xt, 3, 2)
    out.backward(torch.from_numpy(gp).to(dev))
    assert np.abs(out.detach().cpu().numpy() - want).max() <= 2e-6 * max(1.0, np.abs(want).max())
    assert np.abs(xt.grad.cpu().numpy() - want_g).max() <= 2e-5 * max(1.0, np.abs(want_g).max())


def test_pairwise_op_extreme_logits(dev):
    """|x| up to 200: log-space evaluation must not overflow (pairwise.cu:27-50)."""
    from boxinstseg_amd import pairwise_nlog
    from oracle import c_oracle
    vals = np.array([0, 1e-3, -1e-3, 3, -3, 30, -30, 100, -100, 200, -200], np.float32)
    x = np.tile(vals, (1, 11, 1)).astype(np.float32)
    x = x + x.transpose(0, 2, 1) * 0.5
    want = c_oracle.pairwise_nlog_fwd(x, 3, 1)
    got = pairwise_nlog(torch.from_numpy(x[:, None]).to(dev), 3, 1).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_pairwise_op_backward_mixed_saturation(dev):
    """The size-3 backward picks its body per 16x64 tile: probabilities where every |logit| of the tile + halo <= 34, log space
    (pairwise.cu:38-58 to the letter) otherwise.  A map with a few large logits makes both run in one launch, next to each other."""
    from boxinstseg_amd import pairwise_nlog
    from oracle import c_oracle
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((2, 40, 150)) * 6).astype(np.float32)
    x[0, 3, 5] = 60.0; x[0, 30, 140] = -200.0; x[1, 17, 70] = 34.5; x[1, 18, 70] = -33.9
    want = c_oracle.pairwise_nlog_fwd(x, 3, 2)
    gp = rng.standard_normal(want.shape).astype(np.float32)
    want_g = c_oracle.pairwise_nlog_bwd(x, want, gp, 3, 2)
    xt = torch.from_numpy(x[:, None]).to(dev).requires_grad_(True)
    out = pairwise_nlog(xt, 3, 2)
    out.backward(torch.from_numpy(gp).to(dev))
    assert np.isfinite(xt.grad.cpu().numpy()).all()
    assert np.abs(out.detach().cpu().numpy() - want).max() <= 2e-6 * max(1.0, np.abs(want).max())
    assert np.abs(xt.grad.cpu().numpy()[:, 0] - want_g).max() <= 2e-5 * max(1.0, np.abs(want_g).max())


@pytest.mark.parametrize('shape', [(1, 200, 256), (3, 200, 256), (1, 16, 64), (5, 40, 192), (31, 56, 128)])
def test_pairwise_op_backward_covers_every_tile(dev, shape):
    """The f32 size-3 backward deals its 16x64 tiles to the workgroups in an XCD-aware order; the order has to be a bijection for
    EVERY tile count (round 3's skipped tiles whenever the count was not a multiple of 8: 52 tiles per 200x256 map times an odd
    N).  The output buffer of the C ABI call is pre-filled with NaN, so a tile nobody wrote cannot pass."""
    from boxinstseg_amd import _lib
    from oracle import c_oracle
    rng = np.random.default_rng(17)
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    want = c_oracle.pairwise_nlog_fwd(x, 3, 2)
    gp = rng.standard_normal(want.shape).astype(np.float32)
    want_g = c_oracle.pairwise_nlog_bwd(x, want, gp, 3, 2)
    xt = torch.from_numpy(x[:, None]).to(dev)
    pw = torch.from_numpy(want).to(dev)
    gpt = torch.from_numpy(gp).to(dev)
    g = torch.full_like(xt, float('nan'))
    lib = _lib.load()
    rc = lib.bxi_pairwise_nlog_backward_f32(xt.data_ptr(), pw.data_ptr(), gpt.data_ptr(), shape[0], shape[1], shape[2], 3, 2, g.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = g.cpu().numpy()[:, 0]
    assert np.isfinite(got).all(), 'tiles left unwritten: %d elements' % int((~np.isfinite(got)).sum())
    assert np.abs(got - want_g).max() <= 2e-5 * max(1.0, np.abs(want_g).max())


@pytest.mark.parametrize('shape,dil', [((2, 37, 132), 1), ((2, 37, 132), 2), ((2, 37, 132), 3), ((2, 37, 132), 4), ((3, 45, 68), 4), ((1, 23, 200), 3),
                                       ((5, 2, 8), 1), ((4, 3, 4), 2), ((2, 5, 64), 4), ((1, 20, 64), 2), ((7, 41, 256), 2), ((2, 100, 320), 1),
                                       ((3, 2, 8), 4), ((2, 3, 4), 4), ((3, 3, 8), 3), ((2, 1, 8), 1)])          # H <= dilation; H = 1 leaves the pair kernel
def test_pairwise_op_pair_backward_shapes(dev, shape, dil):
    """The f32 size-3 backward for W % 4 == 0 evaluates every unordered pair once (pairwise3_bwd_pair_kernel): the share of the later pixel travels
    by DPP / through LDS inside a 16- or 20-row x 64-column tile, pairs across a tile border are evaluated as edge items.  Every dilation the
    kernel is built for, maps narrower / shorter than a tile, ragged last tiles in both directions, 16- and 20-row tile forms, against the oracle
    (pairwise.cu:106-149); the output is pre-filled with NaN."""
    from boxinstseg_amd import _lib
    from oracle import c_oracle
    rng = np.random.default_rng(23)
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    want = c_oracle.pairwise_nlog_fwd(x, 3, dil)
    gp = rng.standard_normal(want.shape).astype(np.float32)
    want_g = c_oracle.pairwise_nlog_bwd(x, want, gp, 3, dil)
    xt = torch.from_numpy(x[:, None]).to(dev)
    pw = torch.from_numpy(want).to(dev)
    gpt = torch.from_numpy(gp).to(dev)
    g = torch.full_like(xt, float('nan'))
    lib = _lib.load()
    rc = lib.bxi_pairwise_nlog_backward_f32(xt.data_ptr(), pw.data_ptr(), gpt.data_ptr(), shape[0], shape[1], shape[2], 3, dil, g.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = g.cpu().numpy()[:, 0]
    assert np.isfinite(got).all(), 'pixels left unwritten: %d' % int((~np.isfinite(got)).sum())
    assert np.abs(got - want_g).max() <= 2e-5 * max(1.0, np.abs(want_g).max())


def test_pairwise_op_backward_ignores_gradient_of_padded_taps(dev):
    """pairwise.cu:118-121 skips a tap that leaves the map: whatever the upstream gradient holds there (inf, NaN) must not reach g_logits.
    The pair kernel reads those positions through in-bounds addresses and forces their sum to 0 by a select, not by a multiplication."""
    from boxinstseg_amd import pairwise_nlog_backward, pairwise_nlog_forward
    from oracle import c_oracle
    rng = np.random.default_rng(29)
    x = (rng.standard_normal((2, 24, 72)) * 2).astype(np.float32)
    pw = c_oracle.pairwise_nlog_fwd(x, 3, 2)
    gp = rng.standard_normal(pw.shape).astype(np.float32)
    want_g = c_oracle.pairwise_nlog_bwd(x, pw, gp, 3, 2)
    bad = gp.copy()
    H, W = x.shape[1:]
    for k in range(8):
        kk = k if k < 4 else k + 1
        dy, dx = (kk // 3 - 1) * 2, (kk % 3 - 1) * 2
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        out = (rr + dy < 0) | (rr + dy >= H) | (cc + dx < 0) | (cc + dx >= W)
        bad[:, k][:, out] = np.where(rng.random(out.sum()) < 0.5, np.inf, np.nan)
    xt = torch.from_numpy(x[:, None]).to(dev)
    got = pairwise_nlog_backward(3, 2, xt, pairwise_nlog_forward(3, 2, xt), torch.from_numpy(bad).to(dev)).cpu().numpy()[:, 0]
    assert np.isfinite(got).all()
    assert np.abs(got - want_g).max() <= 2e-5 * max(1.0, np.abs(want_g).max())


def test_pairwise_op_errors(dev):
    from boxinstseg_amd import pairwise_nlog, pairwise_nlog_forward
    with pytest.raises(RuntimeError, match='CUDA'):
        pairwise_nlog_forward(3, 2, torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match='contiguous'):
        pairwise_nlog_forward(3, 2, torch.zeros(1, 1, 4, 8, device=dev)[..., ::2])
    with pytest.raises(RuntimeError):
        pairwise_nlog_forward(4, 2, torch.zeros(1, 1, 4, 4, device=dev))     # even window
    assert pairwise_nlog(torch.zeros(0, 1, 4, 4, device=dev), 3, 2).shape == (0, 8, 4, 4)


# ---------------------------------------------------------------------------------------------
# target side
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['cfg1', 'ragged', 'bgr', 'stride8', 'exact_pixels'])
def test_color_affinity(dev, case):
    from boxinstseg_amd import color_affinity
    stride = 4
    if case == 'cfg1':
        d = synthetic.cfg1(0)
    elif case == 'ragged':
        d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=2, seed=3, img_shapes=[(96, 131), (70, 160)],
                                 ori_shapes=[(48, 66), (210, 480)], min_box=16, max_box=64)
    elif case == 'bgr':
        d = synthetic.make_batch(B=1, H=64, W=64, boxes_per_img=1, seed=4, min_box=16, max_box=32)
        d['img_metas'][0]['img_norm_cfg'] = dict(mean=np.array([103.53, 116.28, 123.675], np.float32),
                                                 std=np.array([1.0, 1.0, 1.0], np.float32), to_rgb=False)
    elif case == 'exact_pixels':              # de-normalised values within an ulp of an integer
        d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=1, seed=6, min_box=16, max_box=64, pixel_offset=0.0)
    else:
        stride = 8
        d = synthetic.make_batch(B=1, H=128, W=192, boxes_per_img=1, seed=5, stride=8, min_box=16, max_box=64)
    ref = oracle_path(d)
    sim, bits, _ = color_affinity(torch.from_numpy(d['imgs']).to(dev), d['img_metas'], out_stride=stride)
    sim = sim.cpu().numpy()
    bits = bits.cpu().numpy()
    assert np.abs(sim - ref['sim']).max() <= 2e-6
    # the thresholded bits: EVERY disagreement must sit on the threshold itself (the oracle's similarity within 4e-6 of 0.3, where
    # one ulp of expf decides); anywhere else a single flipped bit fails the test
    ambiguous = 0
    for k in range(8):
        mism = (((bits >> k) & 1) != (ref['sim'][:, k] >= 0.3)).astype(bool)
        near = np.abs(ref['sim'][:, k] - 0.3) <= 4e-6
        assert not (mism & ~near).any(), f'direction {k}: {(mism & ~near).sum()} threshold flips away from the threshold'
        ambiguous += int((mism & near).sum())
    assert ambiguous <= 2, f'{ambiguous} disagreements on the threshold itself'


def test_box_bitmasks(dev):
    from boxinstseg_amd import box_bitmasks
    from oracle import c_oracle
    boxes = [np.array([[10.7, 3.2, 50.9, 40.1], [-3.0, -2.0, 20.0, 10.0], [60.0, 60.0, 200.0, 200.0],
                       [5.0, 5.0, 5.9, 5.9], [30.0, 2.0, 10.0, 60.0]], np.float32),
             np.zeros((0, 4), np.float32),
             np.array([[0.0, 0.0, 95.0, 63.0]], np.float32)]
    H, W = 64, 96
    for stride, start in ((4, 2), (1, 0)):
        got = box_bitmasks([torch.from_numpy(b).to(dev) for b in boxes], H, W, stride, start).cpu().numpy()
        allb = np.concatenate(boxes)
        assert got.shape[0] == len(allb)
        for g, box in enumerate(allb):
            full = np.zeros((H, W), np.float32)
            full[int(box[1]):int(box[3]) + 1, int(box[0]):int(box[2]) + 1] = 1.0     # condinst_head.py:1429-1430
            assert np.array_equal(got[g], full[start::stride, start::stride]), (g, stride)
            if stride == 4:
                assert np.array_equal(got[g], c_oracle.box_bitmask(box, H, W, 4))


# ---------------------------------------------------------------------------------------------
# fused loss
# ---------------------------------------------------------------------------------------------
def Fh_status_rows():
    from boxinstseg_amd import functional as Fh
    return Fh.last_eval_status()[1]


def _check(d, dev, warmup=1.0, up=None, tol=TOL):
    g = (1.0, 1.0) if up is None else up
    ref = oracle_path(d, warmup=warmup, g_prj=g[0], g_pw=g[1], want_targets=False)
    lp, lw, grad = hip_loss(d, dev, warmup=warmup, up=up)
    assert rel(lp, ref['loss_prj']) <= tol, (lp, ref['loss_prj'])
    assert rel(lw, ref['loss_pairwise']) <= tol or abs(lw - ref['loss_pairwise']) < 1e-7, (lw, ref['loss_pairwise'])
    err, ties = grad_report(grad, ref['grad'], d['mask_logits'][:, 0])
    assert err <= tol, f'grad err {err:.3e} ({ties} ambiguous arg-max lines excluded)'
    raw = float(np.abs(grad - ref['grad']).max() / np.abs(ref['grad']).max())
    assert raw <= tol or ties > 0, f'raw grad err {raw:.3e} with no ambiguous arg-max line'
    _check_all_lines(d, ref, grad, g[0], tol)
    return lp, lw


def _check_all_lines(d, ref, grad, g_prj=1.0, tol=TOL):
    """What grad_report leaves out is checked as well: every pixel against the oracle's gradient with each line's projection mass at the
    first index of the largest logit (tests/helpers.py:expected_grad_logit_first), no line excluded."""
    err = grad_check_all_lines(grad, expected_grad_logit_first(d, ref, g_prj))
    assert err <= tol, f'grad err {err:.3e} over every line, against the first index of the largest logit'


def test_loss_cfg1(dev):
    _check(synthetic.cfg1(0), dev)


def test_loss_cfg1_warmup_and_upstream(dev):
    _check(synthetic.cfg1(1), dev, warmup=0.37)
    _check(synthetic.cfg1(2), dev, up=(0.5, 3.0))
    _check(synthetic.cfg1(2), dev, up=(512.0, 512.0))      # Fp16OptimizerHook loss_scale


def test_loss_ragged_two_per_box(dev):
    d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=3, inst_per_box=2, seed=7,
                             img_shapes=[(96, 131), (70, 160)], ori_shapes=[(48, 66), (210, 480)],
                             min_box=16, max_box=80)
    _check(d, dev)


def test_loss_wide_map(dev):
    """w > 256 exercises the multi-chunk column loop; h not a multiple of the tile height."""
    d = synthetic.make_batch(B=1, H=76, W=1344, boxes_per_img=3, seed=8, min_box=24, max_box=400)
    _check(d, dev)


def test_loss_extreme_logits(dev):
    """saturated logits take the log-space branch of the fused kernel (methodology rule: force the branch)."""
    d = synthetic.cfg1(3)
    d['mask_logits'] = (d['mask_logits'] * 40.0).astype(np.float32)
    ref = oracle_path(d, want_targets=False)
    lp, lw, grad = hip_loss(d, dev)
    assert np.isfinite([lp, lw]).all() and np.isfinite(grad).all()
    assert rel(lw, ref['loss_pairwise']) <= TOL and rel(lp, ref['loss_prj']) <= TOL
    _check_all_lines(d, ref, grad)          # (511 of its 512 lines have tied fp32 sigmoids: grad_report would compare one line)


def test_loss_zero_instances_and_empty_image(dev):
    from boxinstseg_amd import boxinst_mask_loss
    d = synthetic.cfg1(0)
    t = to_dev(d, dev)
    empty = torch.zeros((0, 1, d['h'], d['w']), device=dev, requires_grad=True)
    out = boxinst_mask_loss(empty, torch.zeros(0, dtype=torch.long, device=dev), t['gt_bboxes'], imgs=t['imgs'],
                            img_metas=d['img_metas'])
    assert float(out['loss_prj']) == 0.0 and float(out['loss_pairwise']) == 0.0
    (out['loss_prj'] + out['loss_pairwise']).backward()
    # an image with no GT boxes (the reference raises at condinst_head.py:1440)
    d2 = synthetic.make_batch(B=2, H=64, W=64, boxes_per_img=2, seed=9, min_box=16, max_box=40)
    d2['gt_bboxes'][0] = np.zeros((0, 4), np.float32)
    d2['gt_inds'] = np.array([0, 1, 1], np.int64)
    d2['mask_logits'] = d2['mask_logits'][:3]
    _check(d2, dev)


@pytest.mark.parametrize('batch', [
    dict(B=2, H=96, W=160, boxes_per_img=3, seed=12, img_shapes=[(96, 131), (70, 160)], ori_shapes=[(48, 66), (210, 480)], min_box=16, max_box=80),
    # 70 instances on 24x40 maps: stage1_kernel's work list (build_work_list) carries its total across chunks of 64 instances
    dict(B=2, H=96, W=160, boxes_per_img=5, inst_per_box=7, seed=12, min_box=16, max_box=80),
], ids=['n6_padded_images', 'n70_two_chunks'])
def test_loss_from_precomputed_bits(dev, batch):
    """bxi_boxinst_loss_fwd_bwd_f32 (affinity bits given) == bxi_boxinst_eval_f32 (bits derived from Lab)."""
    from boxinstseg_amd import boxinst_mask_loss, color_affinity
    d = synthetic.make_batch(**batch)
    t = to_dev(d, dev)
    _, bits, _ = color_affinity(t['imgs'], d['img_metas'], want_similarity=False)
    outs = []
    for kw in (dict(affinity_bits=bits), dict(imgs=t['imgs'], img_metas=d['img_metas'])):
        x = t['logits'].clone().requires_grad_(True)
        o = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], **kw)
        (o['loss_prj'] + o['loss_pairwise']).backward()
        outs.append((o['loss_prj'].item(), o['loss_pairwise'].item(), x.grad.clone()))
    assert outs[0][0] == outs[1][0]                                        # same leader arithmetic
    assert abs(outs[0][1] - outs[1][1]) <= 1e-6 * abs(outs[1][1])          # different pair order (ordered / unordered pairs)
    scale = outs[1][2].abs().max()                                         # two template instantiations: <= a few ulp
    assert (outs[0][2] - outs[1][2]).abs().max() <= 2e-6 * scale


def test_deterministic(dev):
    d = synthetic.cfg1(5)
    a = hip_loss(d, dev)
    b = hip_loss(d, dev)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.fixture(params=[0, 2], ids=['form_auto', 'form_two_launches'])
def eval_form(request):
    """bxi_boxinst_eval_f32 as the library chooses it (the single launch where it applies) and forced to two launches."""
    from boxinstseg_amd import functional as Fh
    with Fh.eval_flags(request.param):          # BXI_EVAL_* flags of every evaluation inside the test (per call, no library state)
        yield request.param


def test_single_launch_and_two_launch_forms_agree_bit_for_bit(dev):
    """The evaluation as ONE launch (back-half workgroups waiting, inside the launch, for front-half workgroups that precede them
    in the grid; tagged records) and as two launches (a kernel boundary instead) must give the same bits: integer loss
    accumulators, dice sums in index order, a gradient of at most two float additions onto a zero per element."""
    from boxinstseg_amd import functional as Fh
    cases = [synthetic.cfg1(3), synthetic.cfg2(1),
             synthetic.make_batch(B=3, H=160, W=224, boxes_per_img=3, seed=5, min_box=12, max_box=120, img_shapes=[[150, 200], [160, 224], [121, 183]]),
             synthetic.make_batch(B=1, H=1056, W=96, boxes_per_img=2, seed=6, min_box=16, max_box=90),          # tall: many bands
             synthetic.make_batch(B=2, H=128, W=1088, boxes_per_img=2, seed=7, min_box=16, max_box=300),        # wide: several chunks
             synthetic.make_batch(B=2, H=256, W=256, boxes_per_img=40, seed=8, min_box=8, max_box=60)]          # 80 instances
    from boxinstseg_amd import _lib
    for d in cases:
        for dil in (1, 2, 3):
            res = []
            # the single launch wherever it is built, with / without the stream workgroups staying on (BXI_EVAL_SHARED_DEVICE), and two launches
            for form in (_lib.EVAL_SINGLE_LAUNCH, _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_SHARED_DEVICE, _lib.EVAL_TWO_LAUNCHES):
                with Fh.eval_flags(form):                         # (dilation 3: the single launch is not built -- two launches whatever is asked)
                    res.append(hip_loss(d, dev, pairwise_dilation=dil))
            a, a2, b = res
            assert a[0] == a2[0] and a[1] == a2[1] and np.array_equal(a[2], a2[2]), dil
            assert a[0] == b[0] and a[1] == b[1], (dil, a[:2], b[:2])
            assert np.array_equal(a[2], b[2]), dil


def test_stream_with_a_cu_mask_takes_the_two_launch_form(dev):
    """The single-launch form sizes its grid for the whole device; on a stream restricted to a few CUs (hipExtStreamCreateWithCUMask)
    its stream workgroups would hold every slot while waiting for workgroups that cannot start.  The library asks the stream for its
    mask and takes the two-launch form there (no waiter depends on a workgroup that still needs a slot): same bits, status 0."""
    import ctypes as C
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    lib = _lib.load()
    hip = C.CDLL('libamdhip64.so')
    stream = C.c_void_p()
    mask = (C.c_uint32 * 8)(0xffffffff, 0, 0, 0, 0, 0, 0, 0)             # 32 of the 256 CUs
    assert hip.hipExtStreamCreateWithCUMask(C.byref(stream), 8, mask) == 0
    try:
        d = synthetic.cfg2(2)
        quiet = hip_loss(d, dev)
        names = []
        cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
        ext = torch.cuda.ExternalStream(stream.value, device=dev)
        t = to_dev(d, dev)
        torch.cuda.synchronize()
        Fh.DEBUG_KEEP_LAST = True
        lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
        try:
            with torch.cuda.stream(ext), Fh.eval_flags(0):       # (a second stream: this module would say SHARED_DEVICE; here the library's own choice is the test)
                x = t['logits'].clone().requires_grad_(True)
                out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'])
                (out['loss_prj'] + out['loss_pairwise']).backward()
        finally:
            lib.bxi_dev_set_launch_hook(None, None)
        torch.cuda.synchronize()
        assert 'eval1' not in names and 'prep' in names and 'pair' in names, names
        assert Fh.last_eval_status()[0] == 0
        assert float(out['loss_prj']) == quiet[0] and float(out['loss_pairwise']) == quiet[1]
        assert np.array_equal(x.grad.cpu().numpy()[:, 0], quiet[2])
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(stream)


def test_wait_timeouts_are_loud(dev, eval_form):
    """The second launch's bounded waits (tile waves for the predicate bytes / the normaliser, the finisher for everybody) never run
    out in practice; when they do -- forced here through the test hook -- the evaluation must not hand back plausible numbers: both
    losses are NaN (mmdet's CheckInvalidLossHook fires, mmdet/core/hook/checkloss_hook.py:20-24), the status word is set and the
    gradient is poisoned.  (The reference surfaces launch failures through AT_CUDA_CHECK, pairwise.cu:173,200.)"""
    import math
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    d = synthetic.cfg1(0)
    good = hip_loss(d, dev)
    with Fh.eval_flags(eval_form | _lib.EVAL_WAITS_GIVE_UP):
        Fh.DEBUG_KEEP_LAST = True
        t = to_dev(d, dev)
        x = t['logits'].clone().requires_grad_(True)
        out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'])
        (out['loss_prj'] + out['loss_pairwise']).backward()
        torch.cuda.synchronize()
        assert math.isnan(float(out['loss_prj'])) and math.isnan(float(out['loss_pairwise']))
        status, _ = Fh.last_eval_status()
        assert status != 0
        assert bool(torch.isnan(x.grad).all())
    Fh.reset_eval_state(drop_workspaces=False)                 # the ABI: zero the workspace after a faulted evaluation
    again = hip_loss(d, dev)                                   # and nothing sticks
    assert again[0] == good[0] and again[1] == good[1] and np.array_equal(again[2], good[2])


def test_two_streams_next_to_a_kernel_that_fills_the_gpu(dev, eval_form):
    """Two evaluations in flight on two streams while a third stream keeps every CU busy with matrix products: the in-kernel waits of
    the second launch (tile waves for earlier workgroups of their own grid) must still be met -- a time-out would turn the losses
    into NaN -- and the results must be those of the quiet, serial runs, bit for bit."""
    from boxinstseg_amd import boxinst_mask_loss
    ds = [synthetic.cfg1(7), synthetic.make_batch(B=2, H=192, W=256, boxes_per_img=4, seed=41, min_box=24, max_box=150)]
    quiet = [hip_loss(d, dev) for d in ds]
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    hog = torch.randn(4096, 4096, device=dev)
    ts = [to_dev(d, dev) for d in ds]
    xs = [t['logits'].clone().requires_grad_(True) for t in ts]
    torch.cuda.synchronize()
    outs = []
    for rep in range(6):
        with torch.cuda.stream(streams[2]):
            for _ in range(4):
                hog = (hog @ hog).clamp_(-1.0, 1.0)
        outs = []
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                xs[k].grad = None
                o = boxinst_mask_loss(xs[k], ts[k]['gt_inds'], ts[k]['gt_bboxes'], imgs=ts[k]['imgs'], img_metas=ds[k]['img_metas'],
                                      out_stride=ds[k]['stride'])
                (o['loss_prj'] + o['loss_pairwise']).backward()
                outs.append(o)
        torch.cuda.synchronize()
        for k in (0, 1):
            assert float(outs[k]['loss_prj']) == quiet[k][0] and float(outs[k]['loss_pairwise']) == quiet[k][1], (rep, k)
            assert np.array_equal(xs[k].grad.cpu().numpy()[:, 0], quiet[k][2]), (rep, k)


def test_loss_cfg2_full_size(dev):
    """The headline configuration against the C oracle (a few seconds of CPU)."""
    lp, lw = _check(synthetic.cfg2(0), dev)
    assert 0.1 < lp < 2.0 and 0.05 < lw < 2.0


@pytest.mark.parametrize('cfg', ['cfg1', 'cfg2'])
def test_loss_vs_fp64_oracle(dev, cfg):
    """SURVEY 8(d) parity gate, second half: <= 1e-5 against the fp64 oracle on cfg-1 and cfg-2 (f32 kernels: observed ~1e-6).
    At the headline size the comparison is exact in the discrete parts as well: no colour-threshold flip, no row / column whose
    arg-max is ambiguous in fp32 (nothing excluded from the gradient comparison)."""
    from tests.helpers import oracle_path_f64
    d = synthetic.cfg1(0) if cfg == 'cfg1' else synthetic.cfg2(0)
    ref = oracle_path_f64(d)
    lp, lw, grad = hip_loss(d, dev)
    assert rel(lp, ref['loss_prj']) <= 1e-5 and rel(lw, ref['loss_pairwise']) <= 1e-5, (lp, lw, ref['loss_prj'], ref['loss_pairwise'])
    err, ties = grad_report(grad, ref['grad'], d['mask_logits'][:, 0])
    raw = float(np.abs(grad - ref['grad']).max() / np.abs(ref['grad']).max())
    assert err <= 1e-5, f'grad err {err:.3e}'
    if cfg == 'cfg2':
        assert ties == 0 and raw <= 1e-5, f'{ties} ambiguous arg-max lines, raw grad err {raw:.3e}'
        from boxinstseg_amd import color_affinity
        sim, bits, _ = color_affinity(torch.from_numpy(d['imgs']).to(dev), d['img_metas'])
        want_bits = np.zeros(bits.shape, np.uint8)
        for k in range(8):
            want_bits |= ((ref['sim'][:, k] >= 0.3).astype(np.uint8) << k)
        flips = int(np.unpackbits((bits.cpu().numpy() ^ want_bits)[..., None], axis=-1).sum())
        assert flips == 0, f'{flips} colour-threshold flips of {want_bits.size * 8} at the headline size'


def coco_batch(seed):
    """What one rank of the reference's training hands the loss (configs/boxinst/boxinst_r50_fpn_1x_coco.py:65,99-105,125): two images of
    different orientation, img_shape (800, 1199) and (1333, 750), on the canvas Pad(size_divisor=32) makes of them -- 1344 x 1216, logits
    336 x 304 --, ori_shape (427, 640) and (640, 360) (18 and 20 bottom rows removed), 7 and 23 boxes, 128 instances split 40 / 88, box 6 of
    image 0 without any instance, box 10 with 16 and more."""
    d = synthetic.make_batch(B=2, H=1344, W=1216, boxes_per_img=23, seed=seed,
                             img_shapes=[(800, 1199), (1333, 750)], ori_shapes=[(427, 640), (640, 360)])
    rng = np.random.default_rng(1000 + seed)
    d['gt_bboxes'][0] = d['gt_bboxes'][0][:7].copy()            # 7 + 23 boxes
    gi0 = rng.integers(0, 6, size=40)                            # box 6 of image 0: no instance
    gi1 = np.concatenate([np.full(16, 10), 7 + rng.integers(0, 23, size=72)])
    gt_inds = np.concatenate([np.sort(gi0), np.sort(gi1)]).astype(np.int64)
    allb = np.concatenate(d['gt_bboxes'], 0)
    logits = (2.0 * rng.standard_normal((128, 1, 336, 304))).astype(np.float32)
    ys, xs = (np.arange(336) * 4 + 2)[:, None], (np.arange(304) * 4 + 2)[None, :]
    for n in range(128):
        x1, y1, x2, y2 = [int(v) for v in allb[gt_inds[n]]]
        logits[n, 0] += np.where((ys >= y1) & (ys <= y2) & (xs >= x1) & (xs <= x2), 2.0, -2.0).astype(np.float32)
    d.update(gt_inds=gt_inds, mask_logits=logits, N=128, G=30)
    return d


def test_loss_coco_like_batch(dev):
    """The batch real training supplies, evaluated whole (coco_batch(0)): warm-up mid-ramp (0.37), upstream gradients (0.5, 3.0).
      - against the C oracle at TOL under the rule of _check, and against the fp64 oracle at 1e-5 as test_loss_vs_fp64_oracle does;
      - every shipped form under the bit-equality rules of test_loss_fuzz_forms_and_targets_ahead, status 0 everywhere;
      - once more with logits and imgs inside guard bands at lead = 1 (tests/guarded.py): the scalar logit stream and the generic pooling
        launches at full COCO size, bands intact, inputs unchanged.
    What the comparison leaves out is a condition on the INPUTS, fixed from the oracle and the logits alone (counted on the CPU for seed 0;
    the HIP output has no say in it):
      - colour threshold: of the 1 634 304 oracle similarities of this batch NONE lies within 4e-6 of the threshold (seeds 1-6 have 2-8, seed 7
        none), so the HIP bits must equal `ref['sim'] >= 0.3` with a Hamming distance of 0 and no exclusion;
      - ambiguous arg-max: grad_report (tie_eps 2.5e-7, from the logits) finds 3 of the 81 920 rows and columns (0.004 %); the test asserts
        ties == 3, so the exclusion cannot grow unnoticed."""
    import ctypes as C
    from boxinstseg_amd import _lib, boxinst_mask_loss, color_affinity, functional as Fh
    from tests import guarded as G
    from tests.helpers import oracle_path_f64
    lib = _lib.load()
    d = coco_batch(0)
    assert d['N'] == 128 and [len(b) for b in d['gt_bboxes']] == [7, 23] and (d['h'], d['w']) == (336, 304)
    assert [Fh.rows_removed(10, m['img_shape'], m['ori_shape']) for m in d['img_metas']] == [18, 20]
    cnt = np.bincount(d['gt_inds'], minlength=30)
    assert cnt[:7].sum() == 40 and cnt[7:].sum() == 88 and cnt[6] == 0 and cnt[10] >= 16
    warm, up = 0.37, (0.5, 3.0)
    ref = oracle_path(d, warmup=warm, g_prj=up[0], g_pw=up[1], want_targets=True)
    assert int((np.abs(ref['sim'] - 0.3) <= 4e-6).sum()) == 0, 'the batch has similarities on the threshold: recount and restate the docstring'

    def against(got, r, tol, what):
        lp, lw, grad = got
        assert rel(lp, r['loss_prj']) <= tol and rel(lw, r['loss_pairwise']) <= tol, (what, lp, lw, r['loss_prj'], r['loss_pairwise'])
        err, ties = grad_report(grad, r['grad'], d['mask_logits'][:, 0])
        assert ties == 3, f'{what}: {ties} ambiguous arg-max lines (3 counted for this batch)'
        assert err <= tol, f'{what}: grad err {err:.3e}'

    want = hip_loss(d, dev, warmup=warm, up=up)
    rows = Fh.last_eval_status()[1]
    print(f'coco-like batch: losses {want[0]:.6f} / {want[1]:.6f} (C oracle {ref["loss_prj"]:.6f} / {ref["loss_pairwise"]:.6f}), {rows}-row tiles')
    against(want, ref, TOL, 'default form vs the C oracle')
    against(want, oracle_path_f64(d, warmup=warm, g_prj=up[0], g_pw=up[1]), 1e-5, 'default form vs the fp64 oracle')
    # the colour predicates: exact
    _, bits, _ = color_affinity(torch.from_numpy(d['imgs']).to(dev), d['img_metas'], want_similarity=False)
    want_bits = np.zeros(bits.shape, np.uint8)
    for k in range(8):
        want_bits |= ((ref['sim'][:, k] >= 0.3).astype(np.uint8) << k)
    flips = int(np.unpackbits((bits.cpu().numpy() ^ want_bits)[..., None], axis=-1).sum())
    assert flips == 0, f'{flips} colour-threshold flips of {want_bits.size * 8}'
    # every shipped form: the default's bits where the tile height is the default's, within TOL of it otherwise
    forms = [_lib.EVAL_SINGLE_LAUNCH, _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_SHARED_DEVICE, _lib.EVAL_TWO_LAUNCHES,
             _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8, _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4, 'targets_ahead']
    for form in forms:
        if form == 'targets_ahead':
            got = _loss_with_targets(d, dev, warmup=warm, up=up)
        else:
            with Fh.eval_flags(form):
                got = hip_loss(d, dev, warmup=warm, up=up)
        assert Fh.last_eval_status()[0] == 0, form
        if Fh.last_eval_status()[1] == rows:
            assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), (form, got[:2], want[:2])
        else:
            assert got[0] == want[0] and rel(got[1], want[1]) <= TOL, (form, got[:2], want[:2])
            assert np.abs(got[2] - want[2]).max() <= TOL * np.abs(want[2]).max(), form
            against(got, ref, TOL, f'form {form} vs the C oracle')
    # the inputs as views at lead 1: 4- but not 16-byte aligned -> scalar logit stream, generic pooling launches
    gl = G.embed(torch.from_numpy(d['mask_logits']).to(dev), 1, G.plane_band(d['h'], d['w'], 2))
    gi = G.embed(torch.from_numpy(d['imgs']).to(dev), 1, G.plane_band(d['H'], d['W'], 0))
    t = to_dev(d, dev)
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    Fh.DEBUG_KEEP_LAST = True
    x = gl.t.detach().requires_grad_(True)
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        with G.poisoned_empty():
            out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=gi.t, img_metas=d['img_metas'], warmup_factor=warm)
            (up[0] * out['loss_prj'] + up[1] * out['loss_pairwise']).backward()
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    torch.cuda.synchronize()
    assert x.data_ptr() == gl.ptr() and x.data_ptr() % 16 == 4 and gi.ptr() % 16 == 4
    assert 'pack_lab4' in names and 'pool_rgb' in names, names             # the generic pooling path
    assert Fh.last_eval_status()[0] == 0
    G.check_bands(gl, gi)
    G.check_unchanged(gl, gi)
    assert x.grad.shape == x.shape
    got = (float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), x.grad.cpu().numpy()[:, 0])
    against(got, ref, TOL, 'misaligned logits and images vs the C oracle')


def test_loss_cfg2_two_per_box(dev):
    _check(synthetic.cfg2(1, inst_per_box=2), dev)


def test_loss_cfg2_four_per_box(dev):
    """The shape real training runs: configs/boxinst/boxinst_r50_fpn_1x_coco.py:65 (topk_per_img=64) x :125 (samples_per_gpu=2) -> up to 128
    instances per evaluation (condinst_head.py:1190-1225), at the full 2 x 800 x 1024 canvas.  Default flags: two launches there, the
    first with its pool workgroups ahead of the stream workgroups (the launch exceeds the execution slots), the second with 8-row tiles
    at three workgroups per CU.  Losses and gradient within 1e-4 of the C oracle, status 0; the other form built for this size -- the targets made
    ahead and ONE launch with 8-row tiles (the default with targets from 96 instances on) -- gives the same bits; the 8-row single launch with the
    image side in it left the library with ABI 7: asking for it runs two launches."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    d = synthetic.cfg2(3, inst_per_box=4)
    assert d['N'] == 128
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        _check(d, dev)
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert 'prep' in names and 'pair' in names and 'eval1' not in names, names
    assert Fh.last_eval_status() == (0, 8)
    # the forms differ in where work runs, not in what is computed -- except the tile height, which changes the order of the float
    # additions inside a tile (4-row tiles: against the oracle)
    base = hip_loss(d, dev)
    names.clear()
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        other = _loss_with_targets(d, dev)
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert 'eval1_ready' in names and 'pair' not in names, names
    assert Fh.last_eval_status() == (0, 8)
    assert base[0] == other[0] and base[1] == other[1] and np.array_equal(base[2], other[2])
    names.clear()
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        with Fh.eval_flags(_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_8):
            other = hip_loss(d, dev)
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert 'prep' in names and 'pair' in names and 'eval1' not in names, names       # (not built without targets: two launches)
    assert base[0] == other[0] and base[1] == other[1] and np.array_equal(base[2], other[2])
    with Fh.eval_flags(_lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4):
        _check(d, dev)
        assert Fh.last_eval_status() == (0, 4)


# ---------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------
def test_head_loss_and_targets(dev):
    from boxinstseg_amd import CondInstMaskHead
    d = synthetic.cfg1(0)
    ref = oracle_path(d, warmup=0.0002)
    t = to_dev(d, dev)
    head = CondInstMaskHead(in_channels=16, boxinst_enabled=True, topk_per_img=64, max_proposals=-1).to(dev)
    head._iter.fill_(1.0)                                     # the counter is device state only (as after load_state_dict)
    logits = t['logits'].clone().requires_grad_(True)
    out = head.loss(t['imgs'], d['img_metas'], logits, t['gt_inds'], t['gt_bboxes'], None, None)
    assert set(out) == {'loss_prj', 'loss_pairwise'}
    assert float(head._iter) == 2.0
    assert rel(float(out['loss_prj']), ref['loss_prj']) <= TOL
    assert rel(float(out['loss_pairwise']), ref['loss_pairwise']) <= TOL
    sims, bms, full = head.get_targets(t['gt_bboxes'], None, t['imgs'], d['img_metas'])
    assert sims[0].shape == (4, 8, 64, 64) and bms[0].shape == (4, 64, 64) and full[0].shape == (4, 256, 256)
    assert np.abs(sims[0][0].cpu().numpy() - ref['sim'][0]).max() <= 2e-6
    assert np.array_equal(bms[0].cpu().numpy(), ref['bitmask'])
    with pytest.raises(RuntimeError, match='CUDA'):
        head.loss(t['imgs'].cpu(), d['img_metas'], logits.detach().cpu(), t['gt_inds'].cpu(),
                  [b.cpu() for b in t['gt_bboxes']], None, None)


def test_iteration_counter_is_advanced_by_the_evaluation(dev):
    """`self._iter += 1` (condinst_head.py:1297) rides in the evaluation's last launch: the buffer advances by exactly one per loss()
    call in every form of the evaluation (single launch, two launches, no instances, head-fused, no_grad, re-entrant backward counts
    once); the warm-up factor is evaluated on the device from it (no host copy), external writes simply count, a re-entrant backward
    uses the FIRST evaluation's factor although the counter has moved on, and the launch count of a call drops by one."""
    import ctypes as C
    from boxinstseg_amd import CondInstMaskHead, _lib, functional as Fh
    d = synthetic.cfg1(0)
    t = to_dev(d, dev)
    head = CondInstMaskHead(in_channels=16, boxinst_enabled=True, topk_per_img=64, max_proposals=-1, pairwise_warmup=100).to(dev)
    lib = _lib.load()
    expect = 0.0
    for form in (0, 2):
        with Fh.eval_flags(form):
            for grad in (True, False):
                x = t['logits'].clone().requires_grad_(grad)
                with torch.set_grad_enabled(grad):
                    out = head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
                expect += 1.0
                assert float(head._iter) == expect
                if grad:                                    # two backward passes through one node: still one iteration
                    (out['loss_prj'] + out['loss_pairwise']).backward(retain_graph=True)
                    g1 = x.grad.clone(); x.grad = None
                    (out['loss_prj'] + out['loss_pairwise']).backward()
                    assert float(head._iter) == expect
                    # the second pass evaluated again, with the counter one further -- and still the first pass's warm-up factor
                    assert float((x.grad - g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    # warm-up factor = the reference's min(_iter / warmup, 1) with the incremented value
    x = t['logits'].clone()
    with torch.no_grad():
        a = head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
    expect += 1.0
    head.set_iter(100 * 7)                                   # factor 1 from here on
    with torch.no_grad():
        b = head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
    assert float(head._iter) == 701.0
    assert rel(float(a['loss_pairwise']), float(b['loss_pairwise']) * expect / 100.0) <= 1e-6
    # no instances: the zero-loss launch counts
    with torch.no_grad():
        head.loss(t['imgs'], d['img_metas'], x[:0], t['gt_inds'][:0], t['gt_bboxes'], None, None)
    assert float(head._iter) == 702.0
    # an external in-place write simply counts: there is no host copy to fall out of step
    head._iter.fill_(5.0)
    with torch.no_grad():
        c = head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
    assert float(head._iter) == 6.0
    assert rel(float(c['loss_pairwise']), float(b['loss_pairwise']) * 6.0 / 100.0) <= 1e-6
    # a refused call counts nothing
    with pytest.raises(RuntimeError):
        head.loss(t['imgs'], d['img_metas'], x[:, :, :-1].contiguous(), t['gt_inds'], t['gt_bboxes'], None, None)
    with torch.no_grad():
        head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
    assert float(head._iter) == 7.0
    # one launch per call at this size, counted through the launch hook
    calls = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: calls.append(name))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        with torch.no_grad():
            head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    torch.cuda.synchronize()
    assert len(calls) // 2 <= 2 and float(head._iter) == 8.0


def test_head_composed_window5(dev):
    """pairwise_size=5 goes through the op-level kernels + torch glue; compare with the oracle."""
    from boxinstseg_amd import CondInstMaskHead
    d = synthetic.make_batch(B=1, H=64, W=96, boxes_per_img=2, seed=11, min_box=16, max_box=48)
    ref = oracle_path(d, size=5, dil=1)
    t = to_dev(d, dev)
    head = CondInstMaskHead(in_channels=16, boxinst_enabled=True, pairwise_size=5, pairwise_dilation=1,
                            pairwise_warmup=1, max_proposals=-1).to(dev)
    logits = t['logits'].clone().requires_grad_(True)
    out = head.loss(t['imgs'], d['img_metas'], logits, t['gt_inds'], t['gt_bboxes'], None, None)
    (out['loss_prj'] + out['loss_pairwise']).backward()
    assert rel(float(out['loss_prj']), ref['loss_prj']) <= TOL
    assert rel(float(out['loss_pairwise']), ref['loss_pairwise']) <= TOL
    err, _ = grad_report(logits.grad.cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
    assert err <= TOL


# ---------------------------------------------------------------------------------------------
# shape / parameter coverage of the fused path (loops that the headline shape never enters)
# ---------------------------------------------------------------------------------------------
def _check_cfg(d, dev, tol=TOL, **kw):
    """oracle vs HIP with non-default loss parameters (dilation, threshold, stride...)."""
    ref = oracle_path(d, want_targets=False, size=3, dil=kw.get('pairwise_dilation', 2),
                      thresh=kw.get('pairwise_color_thresh', 0.3),
                      bottom_pixels_removed=kw.get('bottom_pixels_removed', 10))
    lp, lw, grad = hip_loss(d, dev, **kw)
    assert rel(lp, ref['loss_prj']) <= tol, (lp, ref['loss_prj'])
    assert rel(lw, ref['loss_pairwise']) <= tol or abs(lw - ref['loss_pairwise']) < 1e-7, (lw, ref['loss_pairwise'])
    err, ties = grad_report(grad, ref['grad'], d['mask_logits'][:, 0])
    assert err <= tol, f'grad err {err:.3e} ({ties} ambiguous arg-max lines excluded)'
    _check_all_lines(d, ref, grad, 1.0, tol)


def test_loss_many_instances(dev):
    """N = 300 > 256 (leader / final loops over instance chunks), 20 per box, three images."""
    d = synthetic.make_batch(B=3, H=64, W=96, boxes_per_img=5, inst_per_box=20, seed=21, min_box=12, max_box=60)
    assert d['N'] == 300
    _check_cfg(d, dev)


def test_loss_many_boxes_per_image(dev):
    """140 GT boxes in two images (70 each), one instance per box: the predicate waves take rectangles 64 at a time with lane = rectangle --
    chunk 0 with the Lab records, entries 64..127 in the same round trip, 128.. by a load of their own -- for the instances' table (the
    evaluation that computes its own image side) and for the GT boxes' table (bxi_boxinst_targets_f32: per-box counts by one LDS add per lane).
    Against the C oracle, and the targets-ahead pair bit for bit against the un-split evaluation, in the default and the two-launch form; the
    finisher polls 64 x 8 arrival words, two per thread."""
    from boxinstseg_amd import functional as Fh
    d = synthetic.make_batch(B=2, H=128, W=256, boxes_per_img=70, inst_per_box=1, seed=812, min_box=16, max_box=90)
    assert d['N'] == 140 and d['G'] == 140
    _check_cfg(d, dev)
    for form in (0, 2):
        with Fh.eval_flags(form):
            want = hip_loss(d, dev)
            got = _loss_with_targets(d, dev)
        assert Fh.last_eval_status()[0] == 0
        assert got[0] == want[0] and got[1] == want[1], (form, got[:2], want[:2])
        assert np.array_equal(got[2], want[2]), form


@pytest.mark.parametrize('form', ['single_launch', 'single_launch_shared_device', 'two_launches', 'two_launches_8_row_tiles', 'two_launches_4_row_tiles'])
def test_loss_every_form_against_the_oracle(dev, form):
    """Each form of the evaluation (the BXI_EVAL_* flags of the call) against the C oracle: the single launch also where the library
    would not choose it (300 instances: the stream workgroups alone exceed the GPU), two launches, and the tile heights no default takes."""
    from boxinstseg_amd import _lib, functional as Fh
    flags = {'single_launch': _lib.EVAL_SINGLE_LAUNCH, 'single_launch_shared_device': _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_SHARED_DEVICE,
             'two_launches': _lib.EVAL_TWO_LAUNCHES, 'two_launches_8_row_tiles': _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8,
             'two_launches_4_row_tiles': _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4}[form]
    with Fh.eval_flags(flags):
        _check(synthetic.cfg1(4), dev)
        _check_cfg(synthetic.make_batch(B=3, H=64, W=96, boxes_per_img=5, inst_per_box=20, seed=21, min_box=12, max_box=60), dev)
        _check_cfg(synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=3, seed=26, min_box=16, max_box=90), dev, pairwise_dilation=3)
        _check_cfg(synthetic.make_batch(B=1, H=1088, W=1344, boxes_per_img=3, seed=22, min_box=200, max_box=900), dev)
        rows = Fh_status_rows()
        assert rows == (8 if flags & _lib.EVAL_TILE_ROWS_8 else 4)


def test_loss_tall_and_wide_map(dev):
    """h = 272 > 256 rows and w = 336 > 256 columns: second chunk of every row / column loop."""
    d = synthetic.make_batch(B=1, H=1088, W=1344, boxes_per_img=3, seed=22, min_box=200, max_box=900)
    _check_cfg(d, dev)


@pytest.mark.parametrize('dil', [1, 3, 4])
def test_loss_other_dilations(dev, dil):
    d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=3, seed=23 + dil, min_box=16, max_box=90)
    _check_cfg(d, dev, pairwise_dilation=dil)


def test_loss_unaligned_width_scalar_path(dev):
    """w = 51 (not a multiple of 4): the non-vector load/store path of every kernel."""
    d = synthetic.make_batch(B=2, H=72, W=204, boxes_per_img=2, seed=27, min_box=16, max_box=120)
    assert d['w'] == 51
    _check_cfg(d, dev)


def test_loss_stride8_generic_pool(dev):
    d = synthetic.make_batch(B=1, H=128, W=192, boxes_per_img=2, seed=28, stride=8, min_box=24, max_box=100)
    _check_cfg(d, dev)


@pytest.mark.parametrize('thresh', [0.0, -1.0, 0.999, 1.5, 0.05])
def test_loss_threshold_extremes(dev, thresh):
    """thresh <= 0: every pair (padded ones too) weighs 1; thresh > 1: none; the bisection's edge cases."""
    d = synthetic.make_batch(B=1, H=64, W=64, boxes_per_img=2, seed=29, min_box=16, max_box=50)
    _check_cfg(d, dev, pairwise_color_thresh=thresh)


def test_loss_bottom_rows_removed_variants(dev):
    d = synthetic.make_batch(B=2, H=96, W=128, boxes_per_img=2, seed=30, img_shapes=[(90, 128), (96, 100)],
                             ori_shapes=[(30, 43), (960, 1000)], min_box=16, max_box=90)
    _check_cfg(d, dev, bottom_pixels_removed=10)     # 30 rows removed in image 0, 1 in image 1
    _check_cfg(d, dev, bottom_pixels_removed=0)


def test_loss_box_edge_cases(dev):
    """boxes touching / leaving the canvas, degenerate and inverted boxes, invalid gt index."""
    d = synthetic.make_batch(B=1, H=64, W=96, boxes_per_img=6, seed=31, min_box=16, max_box=40)
    d['gt_bboxes'][0] = np.array([[0.0, 0.0, 95.0, 63.0], [-5.0, -7.0, 20.0, 30.0], [80.0, 50.0, 200.0, 100.0],
                                  [40.0, 40.0, 40.5, 40.5], [60.0, 30.0, 50.0, 20.0], [10.2, 5.9, 33.3, 41.7]], np.float32)
    _check_cfg(d, dev)


def _fuzz_case(seed):
    rng = np.random.default_rng(9000 + seed)
    stride = int(rng.choice([4, 4, 4, 8]))
    B = int(rng.integers(1, 4))
    H = int(rng.integers(3, 14)) * 16 + int(rng.choice([0, 0, stride, 2 * stride]))
    W = int(rng.integers(3, 20)) * 16 + int(rng.choice([0, 0, stride, 3 * stride]))
    shapes = [(int(rng.integers(H // 2, H + 1)), int(rng.integers(W // 2, W + 1))) for _ in range(B)]
    d = synthetic.make_batch(B=B, H=H, W=W, boxes_per_img=int(rng.integers(0, 7)), inst_per_box=int(rng.integers(1, 4)),
                             stride=stride, seed=100 + seed, img_shapes=shapes, min_box=8.0, max_box=float(max(H, W)),
                             logit_scale=float(rng.choice([0.5, 2.0, 6.0])))
    kw = dict(pairwise_dilation=int(rng.integers(1, 4)), pairwise_color_thresh=float(rng.choice([0.1, 0.3, 0.5, 0.8])),
              bottom_pixels_removed=int(rng.integers(0, 40)))
    warm = float(rng.choice([1.0, 0.37]))
    up = (float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0)))
    return d, kw, warm, up


@pytest.mark.parametrize('seed', list(range(100, 112)))
def test_loss_fuzz_forms_and_targets_ahead(dev, seed):
    """The same seeded shapes as test_loss_fuzz through every OTHER form of the evaluation -- two launches, two launches with 8-row tiles, and the
    targets-ahead split (bxi_boxinst_targets_f32 + BXI_EVAL_TARGETS_READY, also through the generic pooling path of stride 8) --: each must give the
    default form's bits when its tile height is the default's (8-row tiles: within 1e-4 of it), with status 0."""
    from boxinstseg_amd import _lib, functional as Fh
    d, kw, warm, up = _fuzz_case(seed)
    if d['N'] == 0:
        return
    want = hip_loss(d, dev, warmup=warm, up=up, **kw)
    rows = Fh.last_eval_status()[1]
    for form in (_lib.EVAL_TWO_LAUNCHES, _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8):
        with Fh.eval_flags(form):
            got = hip_loss(d, dev, warmup=warm, up=up, **kw)
        if Fh.last_eval_status()[1] == rows:
            assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), (form, got[:2], want[:2])
        else:
            assert got[0] == want[0] and rel(got[1], want[1]) <= TOL, (form, got[:2], want[:2])
            assert np.abs(got[2] - want[2]).max() <= TOL * np.abs(want[2]).max()
    got = _loss_with_targets(d, dev, warmup=warm, up=up, **kw)
    assert Fh.last_eval_status()[0] == 0
    if Fh.last_eval_status()[1] == rows:
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), (got[:2], want[:2])
    else:
        assert got[0] == want[0] and rel(got[1], want[1]) <= TOL and np.abs(got[2] - want[2]).max() <= TOL * np.abs(want[2]).max()


@pytest.mark.parametrize('seed', list(range(24)))
def test_loss_fuzz(dev, seed):
    """Seeded sweep over shapes and parameters nobody hand-picked: canvas sizes that are / are not multiples of the
    tile sizes, ragged image shapes, 1-3 images, 0-6 boxes per image, 1-3 instances per box, strides 4 / 8,
    dilations 1-3, random threshold / warm-up / rows removed / upstream gradients."""
    rng = np.random.default_rng(9000 + seed)
    stride = int(rng.choice([4, 4, 4, 8]))
    B = int(rng.integers(1, 4))
    H = int(rng.integers(3, 14)) * 16 + int(rng.choice([0, 0, stride, 2 * stride]))
    W = int(rng.integers(3, 20)) * 16 + int(rng.choice([0, 0, stride, 3 * stride]))
    shapes = [(int(rng.integers(H // 2, H + 1)), int(rng.integers(W // 2, W + 1))) for _ in range(B)]
    d = synthetic.make_batch(B=B, H=H, W=W, boxes_per_img=int(rng.integers(0, 7)), inst_per_box=int(rng.integers(1, 4)),
                             stride=stride, seed=100 + seed, img_shapes=shapes, min_box=8.0, max_box=float(max(H, W)),
                             logit_scale=float(rng.choice([0.5, 2.0, 6.0])))
    kw = dict(pairwise_dilation=int(rng.integers(1, 4)), pairwise_color_thresh=float(rng.choice([0.1, 0.3, 0.5, 0.8])),
              bottom_pixels_removed=int(rng.integers(0, 40)))
    warm = float(rng.choice([1.0, 0.37]))
    up = (float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0)))
    ref = oracle_path(d, warmup=warm, g_prj=up[0], g_pw=up[1], want_targets=False, size=3, dil=kw['pairwise_dilation'],
                      thresh=kw['pairwise_color_thresh'], bottom_pixels_removed=kw['bottom_pixels_removed'])
    lp, lw, grad = hip_loss(d, dev, warmup=warm, up=up, **kw)
    if d['N'] == 0:
        assert lp == 0.0 and lw == 0.0 and grad.size == 0
        return
    assert rel(lp, ref['loss_prj']) <= TOL, (lp, ref['loss_prj'])
    assert rel(lw, ref['loss_pairwise']) <= TOL or abs(lw - ref['loss_pairwise']) < 1e-7, (lw, ref['loss_pairwise'])
    err, ties = grad_report(grad, ref['grad'], d['mask_logits'][:, 0])
    assert err <= TOL, f'grad err {err:.3e} ({ties} ambiguous arg-max lines excluded); cfg {B}x{H}x{W} s{stride} {kw}'
    _check_all_lines(d, ref, grad, up[0])


def test_many_shapes_in_one_process_without_resets(dev):
    """Forty evaluations of changing canvases, instance counts, strides and dilations back to back, with no reset in between (the suite's
    fixture resets after every test; tools/extended_fuzz.py, which found this, does not).  Every canvas gets a workspace of its own
    (one LAYOUT per workspace: include/boxinst_hip.h, section 3): with one workspace for all shapes, a small tag met an old payload word
    of the same value at an address where the new layout keeps a tag (a predicate word is 16 * tag + bits) -- intermittent wrong
    results with status 0, and through a stale table entry out-of-bounds tile coordinates."""
    _check(synthetic.cfg2(7), dev)
    for seed in range(24, 64):
        test_loss_fuzz(dev, seed)
    _check(synthetic.cfg1(8), dev)


def test_one_workspace_serves_every_instance_count_of_its_canvas(dev):
    """At the C ABI: ONE workspace, sized for 24 instances of a 2 x 128 x 192 canvas and zeroed once, serves 48 evaluations whose
    instance count changes every time (8 / 16 / 24 / 3).  The layout is a function of the canvas and the workspace's size alone, so
    every kind of record keeps its address while N moves and the tags -- 1 .. 48 here, crossing 16, 32: the values old predicate words
    of tags 1, 2 carry -- stay safe.  Every evaluation: status 0, losses and gradient within 1e-4 of the oracle."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    ds = [synthetic.make_batch(B=2, H=128, W=192, boxes_per_img=4, inst_per_box=k, seed=300 + k, min_box=16, max_box=120) for k in (1, 2, 3)]
    small = synthetic.make_batch(B=2, H=128, W=192, boxes_per_img=4, inst_per_box=1, seed=310, min_box=16, max_box=120)
    small['gt_inds'] = small['gt_inds'][:3].copy(); small['mask_logits'] = small['mask_logits'][:3].copy(); small['N'] = 3
    ds.append(small)
    refs = [oracle_path(d, want_targets=False) for d in ds]
    ws = torch.zeros(lib.bxi_boxinst_eval_workspace_bytes(2, 128, 192, 4, 24), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for k in range(48):
        d, ref = ds[k % 4], refs[k % 4]
        t = to_dev(d, dev)
        batch = Fh._Batch(t['imgs'], d['img_metas'], 10)
        inst = Fh._Inst(t['logits'], t['gt_inds'], t['gt_bboxes'], d['H'], d['W'], d['stride'])
        losses, grad = torch.zeros(2, device=dev), torch.empty_like(inst.logits)
        state = torch.empty(lib.bxi_boxinst_loss_state_bytes(inst.N, inst.h, inst.w), dtype=torch.uint8, device=dev)
        rc = lib.bxi_boxinst_eval_f32(C.byref(batch.struct), C.byref(inst.struct), 3, 2, 0.3, 1.0, None, None, losses.data_ptr(), grad.data_ptr(),
                                      state.data_ptr(), ws.data_ptr(), ws.numel(), 1 if k % 3 else 2, st)
        assert rc == 0, _lib.status_string(rc)
        torch.cuda.synchronize()
        off = lib.bxi_boxinst_loss_state_status_offset(inst.N, inst.h, inst.w)
        assert state[off:off + 4].view(torch.int32).item() == 0, k
        got = losses.cpu().numpy()
        assert rel(float(got[0]), ref['loss_prj']) <= TOL and rel(float(got[1]), ref['loss_pairwise']) <= TOL, (k, got, ref['loss_prj'], ref['loss_pairwise'])
        err, _ = grad_report(grad.cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
        assert err <= TOL, (k, err)


def test_workspace_epoch_advances_once_per_evaluation_and_follows_the_workspace_across_streams(dev):
    """The evaluation's tag is `epoch + 1`, the epoch word 0 of the workspace: read by a SCALAR load (constant cache) by every wave, written
    by a PLAIN store of the finisher (csrc/fused_eval.hip: with_tag).  That is only right if every later kernel -- on whatever stream /
    hardware queue the caller serialises it behind -- sees the store: 30 evaluations alternating between three streams (each waits for
    the previous one's event) and between the two forms on ONE workspace; after evaluation k the word holds k, and every evaluation is
    within 1e-4 of the oracle with status 0.  (A stale epoch would make an evaluation accept the previous one's records.)"""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    ds = [synthetic.make_batch(B=2, H=128, W=192, boxes_per_img=4, inst_per_box=2, seed=520 + k, min_box=16, max_box=120) for k in range(3)]
    refs = [oracle_path(d, want_targets=False) for d in ds]
    ws = torch.zeros(lib.bxi_boxinst_eval_workspace_bytes(2, 128, 192, 4, 16), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    sets = []
    for d in ds:
        t = to_dev(d, dev)
        batch = Fh._Batch(t['imgs'], d['img_metas'], 10)
        inst = Fh._Inst(t['logits'], t['gt_inds'], t['gt_bboxes'], d['H'], d['W'], d['stride'])
        sets.append(dict(t=t, batch=batch, inst=inst, losses=torch.zeros(2, device=dev), grad=torch.empty_like(inst.logits),
                         state=torch.empty(lib.bxi_boxinst_loss_state_bytes(inst.N, inst.h, inst.w), dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    prev = None
    for k in range(30):
        b, ref, s = sets[k % 3], refs[k % 3], streams[(k * 2) % 3 if k % 5 else k % 3]
        if prev is not None:
            s.wait_event(prev)                                   # the caller's serialisation: the only ordering between the streams
        rc = lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, 0.3, 1.0, None, None, b['losses'].data_ptr(),
                                      b['grad'].data_ptr(), b['state'].data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.EVAL_SHARED_DEVICE | (_lib.EVAL_TWO_LAUNCHES if k % 4 == 3 else 0), s.cuda_stream)
        assert rc == 0, _lib.status_string(rc)
        prev = torch.cuda.Event()
        prev.record(s)
        if k % 3 == 2 or k == 29:                                # (checked every third evaluation: the others run back to back across streams)
            torch.cuda.synchronize()
            assert int(ws[:4].view(torch.int32).item()) == k + 1, (k, int(ws[:4].view(torch.int32).item()))
            inst = b['inst']
            off = lib.bxi_boxinst_loss_state_status_offset(inst.N, inst.h, inst.w)
            assert b['state'][off:off + 4].view(torch.int32).item() == 0, k
            got = b['losses'].cpu().numpy()
            assert rel(float(got[0]), ref['loss_prj']) <= TOL and rel(float(got[1]), ref['loss_pairwise']) <= TOL, (k, got)
            err, _ = grad_report(b['grad'].cpu().numpy()[:, 0], ref['grad'], ds[k % 3]['mask_logits'][:, 0])
            assert err <= TOL, (k, err)
    # ... and back to back on ONE stream with no host synchronisation in between (what a training loop does): 40 more, both forms
    s = streams[0]
    for k in range(30, 70):
        b = sets[k % 3]
        rc = lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, 0.3, 1.0, None, None, b['losses'].data_ptr(),
                                      b['grad'].data_ptr(), b['state'].data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.EVAL_TWO_LAUNCHES if k % 4 == 3 else 0, s.cuda_stream)
        assert rc == 0, _lib.status_string(rc)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 70
    for j in range(3):
        inst = sets[j]['inst']
        off = lib.bxi_boxinst_loss_state_status_offset(inst.N, inst.h, inst.w)
        assert sets[j]['state'][off:off + 4].view(torch.int32).item() == 0, j
        got = sets[j]['losses'].cpu().numpy()
        assert rel(float(got[0]), refs[j]['loss_prj']) <= TOL and rel(float(got[1]), refs[j]['loss_pairwise']) <= TOL, (j, got)


# ---------------------------------------------------------------------------------------------
# targets ahead of the evaluation (bxi_boxinst_targets_f32 + BXI_EVAL_TARGETS_READY)
# ---------------------------------------------------------------------------------------------
def _loss_with_targets(d, dev, stream=None, warmup=1.0, up=None, **kw):
    from boxinstseg_amd import boxinst_mask_loss, functional as Fh
    Fh.DEBUG_KEEP_LAST = True
    t = to_dev(d, dev)
    tg = Fh.prepare_targets(t['imgs'], d['img_metas'], t['gt_bboxes'], out_stride=d['stride'], stream=stream,
                            **{k: v for k, v in kw.items() if k in ('pairwise_dilation', 'pairwise_color_thresh', 'bottom_pixels_removed')})
    assert tg is not None
    x = t['logits'].clone().requires_grad_(True)
    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], out_stride=d['stride'], targets=tg,
                            warmup_factor=warmup, **kw)
    if up is None:
        (out['loss_prj'] + out['loss_pairwise']).backward()
    else:
        (up[0] * out['loss_prj'] + up[1] * out['loss_pairwise']).backward()
    torch.cuda.synchronize()
    return float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), x.grad.cpu().numpy()[:, 0]


@pytest.mark.parametrize('form', [0, 2], ids=['form_auto', 'form_two_launches'])
def test_targets_ahead_give_the_fused_evaluation_bit_for_bit(dev, form):
    """bxi_boxinst_targets_f32 (Lab, predicate words, per-box pair counts into the workspace; condinst_head.py:1298-1299 computes the same
    targets from imgs + gt_bboxes alone) followed by the evaluation with BXI_EVAL_TARGETS_READY -- only the logit stream, leaders, tiles and
    finisher are launched, sum W is a gather over gt_inds -- must give the bits of the evaluation that computes the image side itself:
    cfg-1, cfg-2 (32 and 128 instances), a ragged batch with two instances per box, an image without boxes, dilations 1 and 3, and with
    the targets computed on a side stream."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    ragged = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=3, inst_per_box=2, seed=7, img_shapes=[(96, 131), (70, 160)],
                                  ori_shapes=[(48, 66), (210, 480)], min_box=16, max_box=80)
    empty = synthetic.make_batch(B=2, H=64, W=64, boxes_per_img=2, seed=9, min_box=16, max_box=40)
    empty['gt_bboxes'][0] = np.zeros((0, 4), np.float32)
    empty['gt_inds'] = np.array([0, 1, 1], np.int64)
    empty['mask_logits'] = empty['mask_logits'][:3]
    side = torch.cuda.Stream(device=dev)
    cases = [(synthetic.cfg1(3), {}, None), (synthetic.cfg2(1), {}, None), (synthetic.cfg2(2, inst_per_box=4), {}, side), (ragged, {}, side), (empty, {}, None),
             (ragged, dict(pairwise_dilation=1), None), (synthetic.cfg1(5), dict(pairwise_dilation=3, pairwise_color_thresh=0.5), None)]
    for d, kw, stream in cases:
        with Fh.eval_flags(form):
            want = hip_loss(d, dev, **kw)
            names = []
            cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
            lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
            try:
                got = _loss_with_targets(d, dev, stream=stream, **kw)
            finally:
                lib.bxi_dev_set_launch_hook(None, None)
        assert 'targets_pool' in names and 'targets_pred' in names, names
        assert ('eval1_ready' in names) or ('prep_ready' in names and 'pair_tiles' in names), names      # no image role was launched by the evaluation
        assert Fh.last_eval_status()[0] == 0
        assert got[0] == want[0] and got[1] == want[1], (d['N'], kw, got[:2], want[:2])
        assert np.array_equal(got[2], want[2]), (d['N'], kw)


def test_targets_through_the_module_api_and_stale_targets_are_ignored(dev):
    """CondInstMaskHead.prepare_targets(imgs, img_metas, gt_bboxes) at the top of an iteration, loss() later: same bits as loss() alone; targets
    prepared for ANOTHER batch are not used (the evaluation computes its own); the iteration counter ramps as without them."""
    from boxinstseg_amd import CondInstMaskHead
    d, d2 = synthetic.cfg1(0), synthetic.cfg1(1)
    t, t2 = to_dev(d, dev), to_dev(d2, dev)
    outs = []
    for prepare in (None, 'own', 'other'):
        head = CondInstMaskHead(in_channels=16, boxinst_enabled=True, topk_per_img=64, max_proposals=-1).to(dev)
        head._iter.fill_(4321.0)
        if prepare == 'own':
            assert head.prepare_targets(t['imgs'], d['img_metas'], t['gt_bboxes'], stream=torch.cuda.Stream(device=dev))
        elif prepare == 'other':
            assert head.prepare_targets(t2['imgs'], d2['img_metas'], t2['gt_bboxes'])
        x = t['logits'].clone().requires_grad_(True)
        out = head.loss(t['imgs'], d['img_metas'], x, t['gt_inds'], t['gt_bboxes'], None, None)
        (out['loss_prj'] + out['loss_pairwise']).backward()
        torch.cuda.synchronize()
        assert float(head._iter) == 4322.0
        outs.append((float(out['loss_prj']), float(out['loss_pairwise']), x.grad.cpu().numpy()))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1] == outs[0][1] and np.array_equal(o[2], outs[0][2])
    # targets whose rotating workspace a LATER prepare_targets took (three calls, two workspaces per canvas) are not used either
    from boxinstseg_amd import boxinst_mask_loss, functional as Fh
    first = Fh.prepare_targets(t['imgs'], d['img_metas'], t['gt_bboxes'])
    for _ in range(2):
        assert Fh.prepare_targets(t2['imgs'], d2['img_metas'], t2['gt_bboxes']) is not None
    assert not first.matches(t['imgs'], t['gt_bboxes'], dict(out_stride=4, bottom_pixels_removed=10, pairwise_size=3, pairwise_dilation=2, pairwise_color_thresh=0.3))
    x = t['logits'].clone().requires_grad_(True)
    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], targets=first)
    (out['loss_prj'] + out['loss_pairwise']).backward()
    torch.cuda.synchronize()
    want = hip_loss(d, dev)                       # (warm-up factor 1, as the direct call above)
    assert float(out['loss_prj']) == want[0] and float(out['loss_pairwise']) == want[1] and np.array_equal(x.grad.cpu().numpy()[:, 0], want[2])


def test_targets_that_do_not_belong_to_the_evaluation_are_loud(dev):
    """At the C ABI: BXI_EVAL_TARGETS_READY on a workspace whose targets were computed for another threshold, or were overwritten by an
    evaluation that computed its own, or were never computed, or were computed for other BOXES of the same counts: the digest kept with the
    targets (or the box rectangles recorded with them) does not match -> NaN losses, status != 0, never a plausible number.  After bxi_boxinst_targets_f32 with the right arguments: the fused evaluation's bits, twice (targets serve
    several evaluations)."""
    import ctypes as C
    import math
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    d = synthetic.make_batch(B=2, H=128, W=192, boxes_per_img=4, inst_per_box=2, seed=77, min_box=16, max_box=120)
    b = _abi_eval_setup(d, dev, lib, Fh, 0)
    b['inst'].struct.iter_counter = 0
    st = torch.cuda.current_stream(dev).cuda_stream
    off = lib.bxi_boxinst_loss_state_status_offset(b['inst'].N, b['inst'].h, b['inst'].w)
    boxes = b['inst']

    def ev(flags, thresh=0.3):
        rc = lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, thresh, 1.0, None, None, b['losses'].data_ptr(),
                                      b['grad'].data_ptr(), b['state'].data_ptr(), b['ws'].data_ptr(), b['ws'].numel(), flags, st)
        assert rc == 0, _lib.status_string(rc)
        torch.cuda.synchronize()
        return b['losses'].cpu().numpy().copy(), b['grad'].cpu().numpy().copy(), int(b['state'][off:off + 4].view(torch.int32).item())

    def targets(thresh=0.3):
        rc = lib.bxi_boxinst_targets_f32(C.byref(b['batch'].struct), boxes.struct.boxes_per_img_host, boxes.struct.gt_count_host, d['stride'], 3, 2, thresh,
                                         b['ws'].data_ptr(), b['ws'].numel(), st)
        assert rc == 0, _lib.status_string(rc)

    want = ev(0)
    assert want[2] == 0
    for form in (0, _lib.EVAL_TWO_LAUNCHES):
        got = ev(_lib.EVAL_TARGETS_READY | form)                    # never computed (the fused evaluation above cleared the digest)
        assert got[2] != 0 and math.isnan(got[0][0]) and math.isnan(got[0][1]), got
        b['ws'].zero_()
        targets(0.5)
        got = ev(_lib.EVAL_TARGETS_READY | form)                    # another threshold
        assert got[2] != 0 and math.isnan(got[0][0])
        b['ws'].zero_()
        targets()
        for _ in range(2):
            got = ev(_lib.EVAL_TARGETS_READY | form)
            assert got[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # targets of OTHER BOXES with the same geometry and the same box counts (round-5 advice: the host-side digest cannot see device data):
        # the evaluation maps its own boxes to cells again and compares them with the rectangles the targets were counted in
        keep = [bx.clone() for bx in b['t']['gt_bboxes']]
        for bx in b['t']['gt_bboxes']:
            bx[0, 0] += 24.0; bx[0, 2] += 24.0                      # one box moved by six cells, in place: same pointers, same counts
        got = ev(_lib.EVAL_TARGETS_READY | form)
        assert got[2] != 0 and math.isnan(got[0][0]) and math.isnan(got[0][1]), got
        for bx, k_ in zip(b['t']['gt_bboxes'], keep):
            bx.copy_(k_)
        b['ws'].zero_()
        targets()
        got = ev(_lib.EVAL_TARGETS_READY | form)
        assert got[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        ev(form)                                                    # computes its own targets: the prepared ones are gone
        got = ev(_lib.EVAL_TARGETS_READY | form)
        assert got[2] != 0 and math.isnan(got[0][0])
        b['ws'].zero_()
    # refusals: a threshold <= 0 (every pair weighs 1: nothing of the image is needed ahead), contradicting flags
    assert lib.bxi_boxinst_targets_f32(C.byref(b['batch'].struct), boxes.struct.boxes_per_img_host, boxes.struct.gt_count_host, d['stride'], 3, 2, 0.0,
                                       b['ws'].data_ptr(), b['ws'].numel(), st) == _lib.BXI_ERR_UNSUPPORTED
    assert lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, 0.3, 1.0, None, None, b['losses'].data_ptr(),
                                    b['grad'].data_ptr(), b['state'].data_ptr(), b['ws'].data_ptr(), b['ws'].numel(),
                                    _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TWO_LAUNCHES, st) == -3


def test_tag_counter_wraps_by_zeroing_the_workspace(dev):
    """The evaluation's tag is 28 bits.  The evaluation that draws the last value (2^28 - 1) ends by returning the workspace to the all-zero
    state on the device (finisher, after every other wave has arrived with its stores drained), so records of 2^28 evaluations ago can
    never pass for fresh ones and no caller has to count: the epoch word is preset to 2^28 - 4 on a zeroed workspace, then eight evaluations
    of alternating instance counts and forms -- every one within 1e-4 of the oracle with status 0, the epoch word reading 2^28 - 3,
    2^28 - 2, 0 (wrapped: all of the workspace zero), 1, 2, ..."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    ds = [synthetic.make_batch(B=2, H=128, W=192, boxes_per_img=4, inst_per_box=k, seed=600 + k, min_box=16, max_box=120) for k in (3, 1, 2)]
    refs = [oracle_path(d, want_targets=False) for d in ds]
    ws = torch.zeros(lib.bxi_boxinst_eval_workspace_bytes(2, 128, 192, 4, 24), dtype=torch.uint8, device=dev)
    top = (1 << 28) - 1
    ws[:4].view(torch.int32).fill_(top - 3)
    st = torch.cuda.current_stream(dev).cuda_stream
    forms = [0, _lib.EVAL_TWO_LAUNCHES, 0, _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8, 0, _lib.EVAL_TWO_LAUNCHES, 0, _lib.EVAL_SINGLE_LAUNCH]
    expect_epoch = [top - 2, top - 1, 0, 1, 2, 3, 4, 5]
    for k in range(8):
        d, ref = ds[k % 3], refs[k % 3]
        t = to_dev(d, dev)
        batch = Fh._Batch(t['imgs'], d['img_metas'], 10)
        inst = Fh._Inst(t['logits'], t['gt_inds'], t['gt_bboxes'], d['H'], d['W'], d['stride'])
        losses, grad = torch.zeros(2, device=dev), torch.empty_like(inst.logits)
        state = torch.empty(lib.bxi_boxinst_loss_state_bytes(inst.N, inst.h, inst.w), dtype=torch.uint8, device=dev)
        rc = lib.bxi_boxinst_eval_f32(C.byref(batch.struct), C.byref(inst.struct), 3, 2, 0.3, 1.0, None, None, losses.data_ptr(), grad.data_ptr(),
                                      state.data_ptr(), ws.data_ptr(), ws.numel(), forms[k], st)
        assert rc == 0, _lib.status_string(rc)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == expect_epoch[k], (k, int(ws[:4].view(torch.int32).item()))
        if expect_epoch[k] == 0:
            assert int(ws.view(torch.int32).ne(0).sum().item()) == 0, 'the wrap leaves the workspace all zero'
        off = lib.bxi_boxinst_loss_state_status_offset(inst.N, inst.h, inst.w)
        assert state[off:off + 4].view(torch.int32).item() == 0, k
        got = losses.cpu().numpy()
        assert rel(float(got[0]), ref['loss_prj']) <= TOL and rel(float(got[1]), ref['loss_pairwise']) <= TOL, (k, got, ref['loss_prj'], ref['loss_pairwise'])
        err, _ = grad_report(grad.cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
        assert err <= TOL, (k, err)


# ---------------------------------------------------------------------------------------------
# hipGraph replay, shared devices, fall-back after a fault
# ---------------------------------------------------------------------------------------------
def _abi_eval_setup(d, dev, lib, Fh, iter_value):
    """One evaluation's buffers at the C ABI, all persistent (what a captured graph refers to)."""
    t = to_dev(d, dev)
    batch = Fh._Batch(t['imgs'], d['img_metas'], 10)
    inst = Fh._Inst(t['logits'], t['gt_inds'], t['gt_bboxes'], d['H'], d['W'], d['stride'])
    N, h, w = inst.N, inst.h, inst.w
    it = torch.full((1,), float(iter_value), device=dev)
    inst.struct.iter_counter = it.data_ptr()
    bufs = dict(t=t, batch=batch, inst=inst, it=it, losses=torch.zeros(2, device=dev), grad=torch.empty_like(inst.logits),
                state=torch.empty(lib.bxi_boxinst_loss_state_bytes(N, h, w), dtype=torch.uint8, device=dev),
                ws=torch.zeros(lib.bxi_boxinst_eval_workspace_bytes(d['B'], d['H'], d['W'], d['stride'], N), dtype=torch.uint8, device=dev))
    return bufs


@pytest.mark.parametrize('flags', [1, 2], ids=['single_launch', 'two_launches'])
@pytest.mark.parametrize('size', ['cfg1', 'medium'])
def test_hipgraph_replay_with_changed_inputs(dev, flags, size):
    """ONE evaluation captured into a hipGraph and replayed with the CONTENTS of imgs, mask_logits, the box tensors and gt_inds
    overwritten in place between replays -- the reason to replay in training.  Nothing a replay must renew may be a kernel argument:
    the evaluation's tag is drawn on the device from the workspace's epoch word (a by-value tag would make the second replay accept
    the first replay's records: stale predicates, stale losses), and the warm-up factor comes from the device counter
    (condinst_head.py:1297,1330-1331: state that changes per call).  Every replay: status 0, losses and gradient within 1e-4 of the
    oracle FOR THAT REPLAY'S inputs and iteration."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    mk = (lambda s: synthetic.cfg1(s)) if size == 'cfg1' else \
         (lambda s: synthetic.make_batch(B=2, H=320, W=512, boxes_per_img=5, seed=40 + s, min_box=24, max_box=200))
    ds = [mk(s) for s in range(5)]
    W_IT = 8.0                                               # pairwise_warmup: the ramp is still moving over these replays
    b = _abi_eval_setup(ds[0], dev, lib, Fh, iter_value=2.0)
    off = lib.bxi_boxinst_loss_state_status_offset(b['inst'].N, b['inst'].h, b['inst'].w)
    stream = torch.cuda.Stream(device=dev)

    def call(st):
        rc = lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, 0.3, -W_IT, None, None,
                                      b['losses'].data_ptr(), b['grad'].data_ptr(), b['state'].data_ptr(), b['ws'].data_ptr(),
                                      b['ws'].numel(), flags, st)
        assert rc == 0, _lib.status_string(rc)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call(stream.cuda_stream)                              # one eager evaluation first (iteration 3)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            call(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert float(b['it']) == 3.0                              # capturing runs nothing
    for k, d in enumerate(ds[1:] + ds[:1]):
        # overwrite the inputs IN PLACE (same shapes, same counts per image: those are the graph's frozen arguments)
        b['t']['imgs'].copy_(torch.from_numpy(d['imgs']))
        b['t']['logits'].copy_(torch.from_numpy(d['mask_logits']))
        b['t']['gt_inds'].copy_(torch.from_numpy(d['gt_inds']))
        for dst, src in zip(b['t']['gt_bboxes'], d['gt_bboxes']):
            assert dst.shape == src.shape
            dst.copy_(torch.from_numpy(src))
        b['losses'].fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it_now = 3.0 + k + 1.0
        assert float(b['it']) == it_now
        ref = oracle_path(d, warmup=min(it_now / W_IT, 1.0), want_targets=False)
        status = b['state'][off:off + 8].view(torch.int32).cpu().tolist()
        assert status[0] == 0, f'replay {k}: status {status[0]}'
        got = b['losses'].cpu().numpy()
        assert rel(float(got[0]), ref['loss_prj']) <= TOL and rel(float(got[1]), ref['loss_pairwise']) <= TOL, (k, got, ref['loss_prj'], ref['loss_pairwise'])
        err, _ = grad_report(b['grad'].cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
        assert err <= TOL, (k, err)


@pytest.mark.parametrize('flags', [1, 2, 0], ids=['single_launch', 'two_launches', 'mixed'])
def test_hipgraph_with_three_evaluations_on_one_workspace(dev, flags):
    """THREE evaluations (three input sets, ONE workspace) captured into ONE hipGraph: consecutive kernel nodes of a graph, each of which
    must see the epoch word the node before it wrote (the tag is read by a scalar load -- csrc/fused_eval.hip: with_tag -- so this is
    a statement about what a graph launch invalidates between its nodes).  Replayed four times with the inputs of all three overwritten
    in place in between: every evaluation within 1e-4 of the oracle for that replay's inputs, status 0, and the epoch word counts
    every evaluation."""
    import ctypes as C
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    mk = lambda s: synthetic.make_batch(B=2, H=256, W=384, boxes_per_img=4, seed=140 + s, min_box=24, max_box=160)
    ds = [mk(s) for s in range(6)]
    bs = [_abi_eval_setup(ds[j], dev, lib, Fh, iter_value=0.0) for j in range(3)]
    ws = bs[0]['ws']                                          # (same shapes: the first set's workspace serves all three)
    stream = torch.cuda.Stream(device=dev)
    form = lambda j: flags if flags else (1 if j != 1 else 2)

    def call(j, st):
        b = bs[j]
        rc = lib.bxi_boxinst_eval_f32(C.byref(b['batch'].struct), C.byref(b['inst'].struct), 3, 2, 0.3, 1.0, None, None,
                                      b['losses'].data_ptr(), b['grad'].data_ptr(), b['state'].data_ptr(), ws.data_ptr(), ws.numel(), form(j), st)
        assert rc == 0, _lib.status_string(rc)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call(0, stream.cuda_stream)                           # one eager evaluation first
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(3):
                call(j, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 1
    for k in range(4):
        cur = [ds[(k + j) % 6] for j in range(3)]
        for b, d in zip(bs, cur):
            b['t']['imgs'].copy_(torch.from_numpy(d['imgs']))
            b['t']['logits'].copy_(torch.from_numpy(d['mask_logits']))
            b['t']['gt_inds'].copy_(torch.from_numpy(d['gt_inds']))
            for dst, src in zip(b['t']['gt_bboxes'], d['gt_bboxes']):
                assert dst.shape == src.shape
                dst.copy_(torch.from_numpy(src))
            b['losses'].fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 1 + 3 * (k + 1)
        for j, (b, d) in enumerate(zip(bs, cur)):
            ref = oracle_path(d, want_targets=False)
            off = lib.bxi_boxinst_loss_state_status_offset(b['inst'].N, b['inst'].h, b['inst'].w)
            assert b['state'][off:off + 4].view(torch.int32).item() == 0, (k, j)
            got = b['losses'].cpu().numpy()
            assert rel(float(got[0]), ref['loss_prj']) <= TOL and rel(float(got[1]), ref['loss_pairwise']) <= TOL, (k, j, got, ref['loss_prj'], ref['loss_pairwise'])
            err, _ = grad_report(b['grad'].cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
            assert err <= TOL, (k, j, err)


def test_evaluation_next_to_a_kernel_holding_a_quarter_of_the_cus(dev):
    """What an RCCL all-reduce does during DDP's backward: a second stream keeps a fixed share of the compute units busy (here a
    CU-masked stream: 64 of the 256 CUs running matrix products back to back) while evaluations run in the form the library chooses
    on a device it believes it has to itself -- the single launch whose stream workgroups stay on.  They must finish with status 0 and
    the quiet run's bits, with a bounded slowdown (the launch needs 1024 slots and finds 768: its pool workgroups take two rounds)."""
    import ctypes as C
    import time
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    lib = _lib.load()
    hip = C.CDLL('libamdhip64.so')
    hstream = C.c_void_p()
    mask = (C.c_uint32 * 8)(0xffffffff, 0xffffffff, 0, 0, 0, 0, 0, 0)                  # 64 of the 256 CUs
    assert hip.hipExtStreamCreateWithCUMask(C.byref(hstream), 8, mask) == 0
    try:
        d = synthetic.cfg2(3)
        quiet = hip_loss(d, dev)
        t = to_dev(d, dev)
        hog_stream = torch.cuda.ExternalStream(hstream.value, device=dev)
        hog = torch.randn(4096, 4096, device=dev)
        work = torch.cuda.Stream(device=dev)
        names = []
        cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
        Fh.DEBUG_KEEP_LAST = True
        torch.cuda.synchronize()
        with torch.cuda.stream(hog_stream):
            for _ in range(40):                                                         # ~tens of ms on 64 CUs
                hog = (hog @ hog).clamp_(-1.0, 1.0)
        lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
        t0 = time.perf_counter()
        try:
            with torch.cuda.stream(work), Fh.eval_flags(0):
                for rep in range(20):
                    x = t['logits'].clone().requires_grad_(True)
                    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'])
                    (out['loss_prj'] + out['loss_pairwise']).backward()
                work.synchronize()
        finally:
            lib.bxi_dev_set_launch_hook(None, None)
        busy = not hog_stream.query()                                                   # the hog was still running when the work ended
        el = time.perf_counter() - t0
        torch.cuda.synchronize()
        assert 'eval1' in names, names
        assert Fh.last_eval_status()[0] == 0
        assert float(out['loss_prj']) == quiet[0] and float(out['loss_pairwise']) == quiet[1]
        assert np.array_equal(x.grad.cpu().numpy()[:, 0], quiet[2])
        assert el < 0.5, f'{el * 1e3:.1f} ms for 20 evaluations next to the hog (bounded waits are ~0.1 s each when they run out)'
        assert busy, 'the hog finished before the evaluations did: the test did not overlap them'
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(hstream)


def _two_process_worker(rank, seed_base, n, q):
    import numpy as np, torch
    from boxinstseg_amd import synthetic as syn, functional as Fh
    from tests.helpers import hip_loss
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    d = syn.cfg2(seed_base + rank)
    first = hip_loss(d, dev)
    ok = True
    for _ in range(n):
        again = hip_loss(d, dev)                   # asserts status 0 inside
        ok = ok and again[0] == first[0] and again[1] == first[1] and np.array_equal(again[2], first[2])
    q.put((rank, ok, first[0], first[1]))


def test_two_processes_share_one_device(dev):
    """Two PROCESSES evaluating on cuda:0 at the same time (what MPS-style sharing or a co-located job does): neither sees the other
    through any host-side bookkeeping.  Every evaluation of both must report status 0 and reproduce its own first result bit for
    bit; the losses must be the oracle's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_process_worker, args=(r, 50, 60, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, lp, lw in res:
        assert ok, f'process {rank}: results changed between evaluations'
        ref = oracle_path(synthetic.cfg2(50 + rank), want_targets=False)
        assert rel(lp, ref['loss_prj']) <= TOL and rel(lw, ref['loss_pairwise']) <= TOL


def test_fault_is_noticed_where_losses_reach_the_host_and_the_next_evaluations_take_two_launches(dev):
    """A bounded wait that runs out gives NaN losses (loud).  Where the losses reach the host anyway (dist.to_host / the key guard of
    dist.parse_losses) the fault is noticed, the workspaces are zeroed again and from then on this thread's evaluations take the
    two-launch form -- every wait of which is for an earlier workgroup of its grid -- instead of poisoning every iteration."""
    import ctypes as C
    import math
    import warnings
    from boxinstseg_amd import _lib, boxinst_mask_loss, dist as bdist, functional as Fh
    lib = _lib.load()
    d = synthetic.cfg2(4)
    good = hip_loss(d, dev)
    t = to_dev(d, dev)
    with Fh.eval_flags(_lib.EVAL_WAITS_GIVE_UP):
        out = boxinst_mask_loss(t['logits'], t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        vals = bdist.to_host(out)
    assert math.isnan(vals['loss_prj']) and math.isnan(vals['loss_pairwise'])
    assert any('two-launch' in str(x.message) for x in w)
    assert Fh.eval_launch_flags() & _lib.EVAL_TWO_LAUNCHES
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        again = hip_loss(d, dev)
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert 'prep' in names and 'pair' in names and 'eval1' not in names, names
    assert again[0] == good[0] and again[1] == good[1] and np.array_equal(again[2], good[2])
    # ... and a fault while ALREADY in the two-launch form takes the last step down: the path without any in-kernel wait
    # (colour-affinity bits, then bxi_boxinst_loss_fwd_bwd_f32 / _backward_f32: launches ordered by the stream alone)
    with warnings.catch_warnings(record=True) as w2:
        warnings.simplefilter('always')
        Fh.note_fault('forced by the test')
    assert any('without in-kernel waits' in str(x.message) for x in w2)
    names.clear()
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        ref = oracle_path(d, want_targets=False)
        x = t['logits'].clone().requires_grad_(True)
        out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'])
        (out['loss_prj'] + out['loss_pairwise']).backward()
        torch.cuda.synchronize()
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    assert not ({'eval1', 'prep', 'pair'} & set(names)) and 'box' in names and 'stage1' in names, names
    assert rel(float(out['loss_prj']), ref['loss_prj']) <= TOL and rel(float(out['loss_pairwise']), ref['loss_pairwise']) <= TOL
    err, _ = grad_report(x.grad.cpu().numpy()[:, 0], ref['grad'], d['mask_logits'][:, 0])
    assert err <= TOL, err
    # the module's counter still counts and ramps on that path (on the host, as the reference: condinst_head.py:1297,1330-1331)
    from boxinstseg_amd import CondInstMaskHead
    head = CondInstMaskHead(in_channels=16, boxinst_enabled=True, topk_per_img=64, max_proposals=-1, pairwise_warmup=100).to(dev)
    head.set_iter(49)
    with torch.no_grad():
        o2 = head.loss(t['imgs'], d['img_metas'], t['logits'], t['gt_inds'], t['gt_bboxes'], None, None)
    assert float(head._iter) == 50.0 and rel(float(o2['loss_pairwise']), 0.5 * ref['loss_pairwise']) <= TOL
