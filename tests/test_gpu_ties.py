"""Projection arg-max on TIED lines (run on a real MI355X: -m gpu).

The projection term sends each row's and each column's gradient to one pixel; every arg-max in the library documents "the first index of
the largest value wins".  The parity tests exclude lines whose two largest sigmoids agree to a few ulp (tests/helpers.py:grad_report), so a
merge that let the LAST index win would pass them.  Here every line is checked, on inputs built to be tied (tests/test_host_ties.py:
constant, nine-level, planted pairs across every merge boundary, bf16- / fp16-rounded and saturated logits) at the shapes that cross each
structure of the kernels, against tests/helpers.py:expected_grad_logit_first -- the C oracle's gradient with each line's projection mass
moved to the first index of the largest logit.

Which test reaches which arg-max:
  fused_eval.hip    stream waves + leaders, every launch form and tile height    test_boxinst_loss_on_tied_lines, test_upstream_factors_...
  mask_loss.hip     precomputed-bits path                                        the same two tests (their `bits` part)
  meanfield.hip     bxi_mil_loss / bxi_projection_loss                           test_mil_loss_on_tied_lines, test_box_projection_loss_on_tied_lines
  dynamic_head_device.hpp  head-fused partials                                   test_head_fused_loss_on_maps_the_head_ties
Tolerances are the existing ones of the modules these paths are tested in (named at each use); equalities need none."""
import copy

import numpy as np
import pytest
import torch

from oracle import discobox_oracle as do
from oracle import levelset_oracle as lo
from tests.helpers import expected_grad_logit_first, grad_check_all_lines, hip_loss, oracle_path, rel, to_dev
from tests.test_gpu_parity import TOL, _loss_with_targets          # TOL = 1e-4: losses relative, gradient over max|gradient|
from tests.test_host_ties import KINDS, SHAPES, tie_logits, tied_lines

pytestmark = pytest.mark.gpu


def _bits_loss(d, dev, warmup=1.0, up=None):
    """boxinst_mask_loss from precomputed affinity bits -> (loss_prj, loss_pairwise, grad [N,h,w])."""
    from boxinstseg_amd import boxinst_mask_loss, color_affinity
    t = to_dev(d, dev)
    _, bits, _ = color_affinity(t['imgs'], d['img_metas'], out_stride=d['stride'], want_similarity=False)
    x = t['logits'].clone().requires_grad_(True)
    out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], affinity_bits=bits, out_stride=d['stride'], warmup_factor=warmup)
    g = (1.0, 1.0) if up is None else up
    (g[0] * out['loss_prj'] + g[1] * out['loss_pairwise']).backward()
    torch.cuda.synchronize()
    return float(out['loss_prj'].detach()), float(out['loss_pairwise'].detach()), x.grad.cpu().numpy()[:, 0]


def _pairwise_support(d, dil=2):
    """[N,h,w] bool: the pixels a pairwise gradient can reach at all.  A pair weighs (similarity >= threshold) * bitmask of its first pixel
    (condinst_head.py:1324-1325) and sends gradient to both of its pixels: the box itself and its eight neighbours at the dilation.
    Everywhere else the pairwise part is 0 by construction, in the oracle and in any kernel, whatever the logits."""
    from tests.helpers import instance_bitmasks
    bm = instance_bitmasks(d) > 0
    sup = bm.copy()
    h, w = bm.shape[1:]
    for dy in (-dil, 0, dil):
        for dx in (-dil, 0, dil):
            ys, yd = (slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0)))
            xs, xd = (slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0)))
            sup[:, yd, xd] |= bm[:, ys, xs]
    return sup


def _prj_positions(got, pairwise, scale, support):
    """The pixels that hold projection mass: where `got` minus the oracle's pairwise part (g_prj = 0) is not zero.  Outside the support
    of the pairwise part (_pairwise_support: the oracle's is exactly 0 there, asserted) that is exact -- any non-zero bit counts; inside
    it two fp32 evaluations of the pairwise part differ in their last bits everywhere (and where a saturated pair's gradient underflows,
    one gives 0 and the other 1e-45), so 'not zero' is 'beyond TOL * max|gradient|', the bound the two evaluations are held to."""
    assert not pairwise[~support].any()
    return np.where(support, np.abs(got - pairwise) > TOL * scale, got != 0.0)


def _against(what, got, ref, want):
    lp, lw, grad = got
    err = grad_check_all_lines(grad, want)
    print(f'{what}: loss_prj {lp:.7f} ({ref["loss_prj"]:.7f})  loss_pairwise {lw:.7f} ({ref["loss_pairwise"]:.7f})  all-lines grad err {err:.3e}')
    assert rel(lp, ref['loss_prj']) <= TOL, (what, lp, ref['loss_prj'])
    assert rel(lw, ref['loss_pairwise']) <= TOL or abs(lw - ref['loss_pairwise']) < 1e-7, (what, lw, ref['loss_pairwise'])
    assert err <= TOL, f'{what}: grad err {err:.3e} over every line'


def _forms_agree(d, dev, want, rows, pairwise, scale, support, warmup=1.0, up=None):
    from boxinstseg_amd import _lib, functional as Fh
    pos = _prj_positions(want[2], pairwise, scale, support)
    forms = [_lib.EVAL_SINGLE_LAUNCH, _lib.EVAL_TWO_LAUNCHES, _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8,
             _lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4, 'targets_ahead']
    for form in forms:
        if form == 'targets_ahead':
            got = _loss_with_targets(d, dev, warmup=warmup, up=up)
        else:
            with Fh.eval_flags(form):
                got = hip_loss(d, dev, warmup=warmup, up=up)
        assert Fh.last_eval_status()[0] == 0, form
        if Fh.last_eval_status()[1] == rows:
            assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), (form, got[:2], want[:2])
        else:
            assert got[0] == want[0] and rel(got[1], want[1]) <= TOL, (form, got[:2], want[:2])
            assert np.abs(got[2] - want[2]).max() <= TOL * np.abs(want[2]).max(), form
            moved = int((_prj_positions(got[2], pairwise, scale, support) != pos).sum())
            assert moved == 0, f'form {form}: {moved} projection positions differ from the default form'
    return pos


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_boxinst_loss_on_tied_lines(dev, shape, kind):
    """boxinst_mask_loss from images (fused_eval.hip) and from precomputed bits (mask_loss.hip), every tie input at every shape:
      - losses within TOL of the C oracle, gradient within TOL of expected_grad_logit_first on EVERY pixel, status 0;
      - single launch, two launches, 8- and 4-row tiles, targets ahead: the default form's bits where the tile height is the default's,
        otherwise within TOL of it with the same set of projection positions;
      - the bits path: the same expectation, and the projection positions of the images path."""
    from boxinstseg_amd import functional as Fh
    d = SHAPES[shape]()
    d['mask_logits'] = tie_logits(kind, d)
    ref = oracle_path(d, want_targets=False)
    pairwise = oracle_path(d, g_prj=0.0, want_targets=False)['grad']
    want = expected_grad_logit_first(d, ref)
    scale = float(np.abs(want).max())
    got = hip_loss(d, dev)
    rows = Fh.last_eval_status()[1]
    _against(f'{shape} {kind} images', got, ref, want)
    support = _pairwise_support(d)
    pos = _forms_agree(d, dev, got, rows, pairwise, scale, support)
    bits = _bits_loss(d, dev)
    _against(f'{shape} {kind} bits', bits, ref, want)
    moved = int((_prj_positions(bits[2], pairwise, scale, support) != pos).sum())
    assert moved == 0, f'{moved} projection positions of the bits path differ from the images path'


@pytest.mark.parametrize('shape,kind,warmup,up', [('scalar_w51', 'nine_levels', 1.0, (0.5, 3.0)), ('odd_19x40', 'planted', 0.37, None),
                                                  ('two_chunks_272x336', 'constant', 0.37, (0.5, 3.0))])
def test_upstream_factors_and_warmup_on_tied_lines(dev, shape, kind, warmup, up):
    """Non-unit upstream factors send the gradient through the rescale kernel, which takes the projection mass off and re-adds it at the
    STORED arg positions (the constant map: all of them outside the box hull, the sparse loop); a warm-up factor scales the pairwise
    part only.  Same expectation, every form, and the bits path (whose backward applies the factors itself)."""
    from boxinstseg_amd import functional as Fh
    d = SHAPES[shape]()
    d['mask_logits'] = tie_logits(kind, d)
    g = (1.0, 1.0) if up is None else up
    ref = oracle_path(d, warmup=warmup, g_prj=g[0], g_pw=g[1], want_targets=False)
    pairwise = oracle_path(d, warmup=warmup, g_prj=0.0, g_pw=g[1], want_targets=False)['grad']
    want = expected_grad_logit_first(d, ref, g_prj=g[0])
    scale = float(np.abs(want).max())
    got = hip_loss(d, dev, warmup=warmup, up=up)
    rows = Fh.last_eval_status()[1]
    _against(f'{shape} {kind} images', got, ref, want)
    support = _pairwise_support(d)
    pos = _forms_agree(d, dev, got, rows, pairwise, scale, support, warmup=warmup, up=up)
    bits = _bits_loss(d, dev, warmup=warmup, up=up)
    _against(f'{shape} {kind} bits', bits, ref, want)
    assert int((_prj_positions(bits[2], pairwise, scale, support) != pos).sum()) == 0


# ---------------------------------------------------------------------------------------------
# the head-fused evaluation (dynamic_head_device.hpp): ties the head itself produces
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['zero_weights_and_a_bias', 'block_constant_features'])
@pytest.mark.parametrize('C', [8, 16])
def test_head_fused_loss_on_maps_the_head_ties(dev, case, C):
    """CondInstMaskHead.forward_loss with the head inside the evaluation's first launch, on maps with tied lines that the head really
    produces: all-zero weights with a bias (a freshly initialised controller: a constant map), and block-constant features with the
    relative coordinates off (constant blocks of logits, bilinear ramps between them).
      - the logits equal the composed head in fp64 to 1e-5 (the bound of test_dynamic_head_shapes_outside_the_hip_build_run_composed);
      - they carry ties: every line of the constant map, and most lines of the block-constant one;
      - losses and the gradients w.r.t. params and feat equal the un-fused forward() + loss() on the same tensors, within the tolerances
        of test_head_fused_into_the_loss_evaluation (logits 2e-6, losses 1e-5, gradients 2e-4 of their maximum).  The un-fused path is
        the one test_boxinst_loss_on_tied_lines pins to the first index; a head partial that let another index win moves a line's mass
        to another pixel, hence (block-constant case: other bilinear taps, other ReLU gates) to other feature pixels."""
    from boxinstseg_amd import CondInstMaskHead, synthetic
    d = synthetic.cfg1(1)
    imgs = torch.from_numpy(d['imgs']).to(dev)
    B, H, W = imgs.shape[0], imgs.shape[2], imgs.shape[3]
    boxes = [torch.from_numpy(b).to(dev) for b in d['gt_bboxes']]
    gt_inds = torch.from_numpy(d['gt_inds']).to(dev)
    n = gt_inds.numel()
    img_inds = torch.zeros(n, dtype=torch.long, device=dev)
    no_rel = case == 'block_constant_features'
    torch.manual_seed(40 + C)
    head = CondInstMaskHead(in_channels=C, boxinst_enabled=True, disable_rel_coors=no_rel, max_proposals=-1, topk_per_img=64).to(dev)
    head.set_iter(5000)
    coors = torch.rand(n, 2, device=dev) * torch.tensor([W, H], device=dev)
    lvl = torch.randint(0, 5, (n,), device=dev)
    if no_rel:
        coarse = torch.randn(B, C, H // 64, W // 64, device=dev)
        feat = coarse.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).contiguous()          # 8 x 8 feature pixels per block
        params = 0.3 * torch.randn(n, head.num_gen_params, device=dev)
    else:
        feat = torch.randn(B, C, H // 8, W // 8, device=dev)
        params = torch.zeros(n, head.num_gen_params, device=dev)
        nw = sum(head.dy_weights)
        params[:, nw:-1] = 0.5                                       # hidden biases: the last layer's weights then have a gradient
        params[:, -1] = torch.linspace(-1.0, 1.5, n, device=dev)     # the output bias: one constant map per instance
    assert feat.shape == (B, C, H // 8, W // 8)

    def run(fused):
        h2 = copy.deepcopy(head)
        f = feat.clone().requires_grad_(True); p = params.clone().requires_grad_(True)
        if fused:
            logits, losses = h2.forward_loss(f, p, coors, lvl, img_inds, imgs, d['img_metas'], gt_inds, boxes, fuse_head=True)
        else:
            logits = h2(f, p, coors, lvl, img_inds)
            losses = h2.loss(imgs, d['img_metas'], logits, gt_inds, boxes, None, None)
        (losses['loss_prj'] + 2.0 * losses['loss_pairwise']).backward()
        return logits.detach(), losses['loss_prj'].detach(), losses['loss_pairwise'].detach(), f.grad, p.grad

    a, b = run(True), run(False)
    cpu = copy.deepcopy(head).cpu().double()
    want = cpu._composed_forward(feat.cpu().double(), params.cpu().double(), coors.cpu().double(), lvl.cpu(), img_inds.cpu())
    for got in (a[0], b[0]):
        assert got.shape == want.shape
        assert (got.cpu().double() - want).abs().max() <= 1e-5 * max(1.0, float(want.abs().max()))
    for got in (a[0], b[0]):
        tc, tr = tied_lines(got.cpu().numpy()[:, 0])
        print(f'{case} C={C}: {int(tc.sum())} of {tc.size} columns and {int(tr.sum())} of {tr.size} rows tied')
        if no_rel:
            assert tc.mean() > 0.5 and tr.mean() > 0.5
        else:
            assert tc.all() and tr.all()
    assert (a[0] - b[0]).abs().max() <= 2e-6 * max(1.0, float(b[0].abs().max()))
    for i in (1, 2):
        assert abs(float(a[i]) - float(b[i])) <= 1e-5 * max(abs(float(b[i])), 1e-6), (i, float(a[i]), float(b[i]))
    for i in (3, 4):
        if float(b[i].abs().max()) == 0.0:                       # zero weights: no gradient reaches the features
            assert float(a[i].abs().max()) == 0.0
            continue
        assert (a[i] - b[i]).abs().max() <= 2e-4 * float(b[i].abs().max()), (i, float((a[i] - b[i]).abs().max()), float(b[i].abs().max()))


# ---------------------------------------------------------------------------------------------
# mil_loss / BoxProjectionLoss (meanfield.hip): probabilities with exact ties
# ---------------------------------------------------------------------------------------------
MIL_SIZES = [(200, 304), (64, 520), (9, 7), (33, 71), (2, 3)]
MIL_KINDS = ['zero_one', 'constant_half', 'five_levels', 'planted', 'all_zero']


def _mil_input(kind, H, W, n=6):
    rng = np.random.default_rng(H * 1000 + W + len(kind))
    if kind == 'zero_one':
        x = (rng.random((n, H, W)) < 0.3).astype(np.float32)
        x[0, :, W // 2:] = 0.0; x[0, H // 2:, :] = 0.0              # all-zero lines next to 0/1 lines
    elif kind == 'constant_half':
        x = np.full((n, H, W), 0.5, np.float32)
    elif kind == 'five_levels':
        x = (rng.integers(0, 5, size=(n, H, W)) * 0.25).astype(np.float32)
    elif kind == 'all_zero':
        x = np.zeros((n, H, W), np.float32)
    elif kind == 'planted':                # a tie-free base below 0.9; 0.95 twice per line, either side of a multiple of 4 / 16 / 64 / 256 / 320
        x = (rng.random((n, H, W)) * 0.9).astype(np.float32)
        for i in range(n):
            L = W if i % 2 == 0 else H
            pairs = [(0, L - 1)] + [(b - 1, b) for b in (4, 16, 64, 256, 320) if b < L]
            if L < 2:
                continue
            for k in range(H if i % 2 == 0 else W):
                p, q = pairs[(k + i) % len(pairs)]
                if i % 2 == 0:
                    x[i, k, p] = x[i, k, q] = 0.95              # every row tied
                else:
                    x[i, p, k] = x[i, q, k] = 0.95              # every column tied
    else:
        raise ValueError(kind)
    t = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        r0, c0 = int(rng.integers(0, max(H // 2, 1))), int(rng.integers(0, max(W // 2, 1)))
        t[i, r0:r0 + int(rng.integers(1, H // 2 + 2)), c0:c0 + int(rng.integers(1, W // 2 + 2))] = 1
    return x, t


@pytest.mark.parametrize('kind', MIL_KINDS)
@pytest.mark.parametrize('H,W', MIL_SIZES)
def test_mil_loss_on_tied_lines(built, dev, H, W, kind):
    """DiscoBox mil_loss against oracle/discobox_oracle.py:mil_loss (np.argmax: the first index), 2e-6 absolute as in
    tests/test_gpu_discobox.py, with per-instance upstream gradients."""
    from boxinstseg_amd import dice_loss, mil_loss
    x, t = _mil_input(kind, H, W)
    gl = np.linspace(0.5, 2.0, x.shape[0]).astype(np.float32)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    l = mil_loss(dice_loss, xd, xd, torch.from_numpy(t).to(dev))
    (l * torch.from_numpy(gl).to(dev)).sum().backward()
    lw, gw = do.mil_loss(x, t)
    gw = gw * gl[:, None, None]
    got = xd.grad.cpu().numpy()
    print(f'{H}x{W} {kind}: loss err {np.abs(l.detach().cpu().numpy() - lw).max():.2e}  grad err {np.abs(got - gw).max():.2e}')
    assert np.abs(l.detach().cpu().numpy() - lw).max() < 2e-6
    assert np.abs(got - gw).max() < 2e-6


@pytest.mark.parametrize('kind', MIL_KINDS)
@pytest.mark.parametrize('H,W', MIL_SIZES)
def test_box_projection_loss_on_tied_lines(built, dev, H, W, kind):
    """Box2Mask BoxProjectionLoss against oracle/levelset_oracle.py:box_projection_loss (np.argmax), TOL = 1e-4 of the largest
    magnitude as in tests/test_gpu_levelset.py."""
    from boxinstseg_amd import BoxProjectionLoss
    x, t = _mil_input(kind, H, W)
    box = t.astype(np.float32) * np.linspace(0.3, 1.0, x.shape[0]).astype(np.float32)[:, None, None]
    sd = torch.from_numpy(x[:, None]).to(dev).requires_grad_(True)
    l = BoxProjectionLoss(loss_weight=1.3)(sd, torch.from_numpy(box[:, None]).to(dev))
    l.sum().backward()
    lw, gw = lo.box_projection_loss(x, box, 1.3)
    got = sd.grad.cpu().numpy()[:, 0]
    close = lambda a, w: np.abs(np.asarray(a, np.float64) - w).max() <= 1e-4 * max(np.abs(w).max(), 1e-12)
    print(f'{H}x{W} {kind}: loss err {np.abs(l.detach().cpu().numpy() - lw).max():.2e}  grad err {np.abs(got - gw).max():.2e} of {np.abs(gw).max():.2e}')
    assert close(l.detach().cpu().numpy(), lw) and close(got, gw)


# ---------------------------------------------------------------------------------------------
# reduced-precision tensors at the Python surface
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('path', ['images', 'bits'])
def test_boxinst_loss_takes_half_logits(dev, path, dtype):
    """fp16 / bf16 logits (mixed precision hands the loss such tensors; their line maxima tie): the evaluation is the one of
    x.float() -- same loss bits --, the gradient comes back in the input's type and is the fp32 gradient rounded once."""
    from boxinstseg_amd import boxinst_mask_loss, color_affinity
    d = SHAPES['odd_19x40']()
    t = to_dev(d, dev)
    x16 = t['logits'].to(dtype)
    kw = dict(imgs=t['imgs'], img_metas=d['img_metas'])
    if path == 'bits':
        kw = dict(affinity_bits=color_affinity(t['imgs'], d['img_metas'], want_similarity=False)[1])
    res = []
    for x in (x16.clone().requires_grad_(True), x16.float().requires_grad_(True)):
        out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], **kw)
        (0.5 * out['loss_prj'] + 3.0 * out['loss_pairwise']).backward()
        res.append((out['loss_prj'].detach(), out['loss_pairwise'].detach(), x.grad))
    torch.cuda.synchronize()
    half, full = res
    assert torch.equal(half[0], full[0]) and torch.equal(half[1], full[1])
    assert half[2].dtype == dtype and full[2].dtype == torch.float32
    assert float(full[2].abs().max()) > 0
    assert torch.equal(half[2], full[2].to(dtype))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('which', ['mil_loss', 'BoxProjectionLoss'])
def test_projection_losses_take_half_scores(built, dev, which, dtype):
    """The same for the scores of mil_loss and BoxProjectionLoss (sigmoid outputs under autocast)."""
    from boxinstseg_amd import BoxProjectionLoss, dice_loss, mil_loss
    x, t = _mil_input('five_levels', 33, 71)
    x = x + np.random.default_rng(3).random(x.shape).astype(np.float32) * 0.2          # rounding to the half type makes the ties
    x16 = torch.from_numpy(x).to(dev).to(dtype)
    tt = torch.from_numpy(t).to(dev)
    res = []
    for x_in in (x16.clone(), x16.float()):
        if which == 'mil_loss':
            xx = x_in.requires_grad_(True)
            l = mil_loss(dice_loss, xx, xx, tt)
        else:
            xx = x_in[:, None].contiguous().requires_grad_(True)
            l = BoxProjectionLoss(loss_weight=1.3)(xx, tt[:, None].float())
        (l * torch.linspace(0.5, 2.0, l.numel(), device=dev)).sum().backward()
        res.append((l.detach(), xx.grad))
    half, full = res
    assert torch.equal(half[0].float(), full[0])
    assert half[1].dtype == dtype and full[1].dtype == torch.float32
    assert float(full[1].abs().max()) > 0
    assert torch.equal(half[1], full[1].to(dtype))
