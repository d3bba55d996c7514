"""GPU: the dynamic mask head bit for bit on exactly representable cases (tests/dyn_exact.py).

On these inputs every partial sum of the forward and of the backward is exact in fp32 in ANY order -- tests/test_host_dyn_exact.py
establishes that for each case used here -- so the kernels owe the fp64 result, rounded (without loss) to fp32, in every element:
no tolerance, no forgiven group.  A border or halo pixel of d feat, the gradient of a nearly dead unit, a slot's contribution
dropped at a tile seam, a ReLU gate open at exactly 0: each is a differing element.  Every call runs under poisoned_empty().

Equality is equality of values, as torch.equal has it (the sign of a zero is not order-free), except that where a NaN is expected a
NaN is demanded."""
import copy

import numpy as np
import pytest
import torch

from tests import dyn_exact as X
from tests import guarded as GD

pytestmark = pytest.mark.gpu
BAND_BITS = 0x49800000          # 2^20 as fp32: a finite, dyadic guard band (see test_guard_band_that_can_see)


def _ids(cases):
    return [X.spec_name(a, k).replace(' ', '-') for a, k in cases]


def _run(dev, c, *, general=None, dtype=torch.float32, feat=None, params=None, g=None, band_bits=None):
    """One forward and backward of case `c` (optionally with some inputs replaced) -> dict of numpy arrays: logits (fp32), d_feat and
    d_params in `dtype` widened to fp32.  With `band_bits` the features and the parameters sit between guard bands of that pattern."""
    from boxinstseg_amd import dynamic as dyn
    general = (not X.is_tuned(c)) if general is None else general
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    f = t(c['feat'] if feat is None else feat, dtype)
    p = t(c['params'] if params is None else params, dtype)
    guards = []
    if band_bits is not None:
        guards = [GD.embed(f, lead=1, band=GD.plane_band(c['H'], c['W']), poison=band_bits), GD.embed(p, lead=3, band=1024, poison=band_bits)]
        f, p = guards[0].t.detach(), guards[1].t.detach()
    f.requires_grad_(True); p.requires_grad_(True)
    coors, lvl, img, soi = t(c['coors']), t(c['lvl'], torch.int64), t(c['img'], torch.int64), torch.tensor(X.SOI, device=dev)
    with GD.poisoned_empty():
        if general:
            y = dyn.dynamic_mask_forward_generic(f, p, coors, lvl, img, soi, c['layers'], c['channels'], in_stride=X.IN_STRIDE,
                                                 out_stride=X.IN_STRIDE // c['factor'], disable_rel_coors=not c['rel'])
        else:
            y = dyn.dynamic_mask_forward(f, p, coors, lvl, img, soi, in_stride=X.IN_STRIDE, out_stride=X.IN_STRIDE // c['factor'],
                                         disable_rel_coors=not c['rel'])
        assert y.shape == (c['N'], 1, c['factor'] * c['H'], c['factor'] * c['W']) and y.dtype == torch.float32
        y.backward(t(c['g'] if g is None else g))
    assert f.grad.dtype == dtype and p.grad.dtype == dtype
    if guards:
        GD.check_unchanged(*guards)
        GD.check_bands(*guards)
    return dict(logits=y.detach().cpu().numpy(), d_feat=f.grad.float().cpu().numpy(), d_params=p.grad.float().cpu().numpy())


def _slots(dev, c):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return cus, X.slots_for(cus, c['B'], c['H'], c['W'], c['N'], c['factor'])


def _assert_exact(dev, c, got, want):
    """Every element of logits, d feat and d params; on a failure the index, both values and the tile and slot it belongs to."""
    slots = _slots(dev, c)[1] if X.is_tuned(c) else None
    msgs = [X.first_difference(c, what, got[what], w) if what == 'logits' else X.first_difference(c, what, got[what], w, slots)
            for what, w in zip(('logits', 'd_feat', 'd_params'), want)]
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


def _assert_empty_images_get_plus_zero(c, d_feat):
    for b in range(c['B']):
        if not (c['img'] == b).any():
            assert not d_feat[b].view(np.uint32).any(), f'{X.name_of(c)}: d feat of image {b}, which has no instance, is not +0 everywhere'


@pytest.mark.parametrize('case', X.TUNED, ids=_ids(X.TUNED))
def test_tuned_kernels_all_sixteen_instantiations(dev, case):
    """C in {8, 16} x relative coordinates x factor in {1, 2, 4, 8 (the run-time path, with dyadic weights)} at 2 x C x 17 x 37: two
    forward tiles of 14 x 32 (8 x 32 at factors 4 and 8: three by two) and three by two backward tiles of 8 x 32, none of them full."""
    c, want = X.case_and_expected(*case[0], **case[1])
    got = _run(dev, c)
    _assert_exact(dev, c, got, want)
    _assert_empty_images_get_plus_zero(c, got['d_feat'])


@pytest.mark.parametrize('case', X.SLOTS, ids=_ids(X.SLOTS))
def test_slot_counts(dev, case):
    """The backward walks `slots` workgroups per (image, tile), each every slots-th instance of its image; the reducer sums `slots`
    feature partials.  The shapes were chosen for 256 compute units, where the host code gives 8, 6, 3 and 1 slots at factor 2 (and 8
    with five instances per slot at N = 40) and 4 / 8 at factors 4 and 8; on another count the formula gives other numbers, the
    expectation is the same and the count is printed."""
    c, want = X.case_and_expected(*case[0], **case[1])
    cus, slots = _slots(dev, c)
    per_image = np.bincount(c['img'], minlength=c['B'])
    print(f'{X.name_of(c)}: {slots} slots per (image, tile) on {cus} compute units; instances per image {per_image.tolist()}')
    got = _run(dev, c)
    _assert_exact(dev, c, got, want)
    _assert_empty_images_get_plus_zero(c, got['d_feat'])


@pytest.mark.parametrize('case', X.EDGES, ids=_ids(X.EDGES))
def test_map_edges(dev, case):
    """A single row or column, the replicate pad folding onto the same pixel (H or W of 1 and 2), tiles that end exactly on the map
    edge (8, 32, 64) or one pixel past it (9, 33), 15 x 64 (one forward tile of 14 rows and a second of one)."""
    c, want = X.case_and_expected(*case[0], **case[1])
    got = _run(dev, c)
    _assert_exact(dev, c, got, want)
    _assert_empty_images_get_plus_zero(c, got['d_feat'])


@pytest.mark.parametrize('case', X.GENERIC, ids=_ids(X.GENERIC))
def test_generic_kernels(dev, case):
    """csrc/dynamic_head_generic.hip through its own entry (the shipped 3 x 8 on 16 shape included) against
    CondInstMaskHead._composed_forward in fp64."""
    c = X.dyadic_case(*case[0], **case[1])
    want = [a.astype(np.float32) for a in X.expected(c, torch.float64, general=True)]
    got = _run(dev, c, general=True)
    _assert_exact(dev, c, got, want)
    _assert_empty_images_get_plus_zero(c, got['d_feat'])


@pytest.mark.parametrize('shape', X.FUSED, ids=[f'C{s[0]}-rel{s[1]}-N{s[5]}' for s in X.FUSED])
def test_head_fused_evaluation(dev, shape):
    """The copy of the tile forward inside the evaluation's first launch: the logits forward_loss(fuse_head=True) returns equal the fp64
    logits and those of forward(), and the fused form was taken (the logits hang on the head-fused node)."""
    from boxinstseg_amd import CondInstMaskHead
    C, rel, B, H, W, N = shape
    d, gt_inds, c = X.fused_batch(*shape)
    want = X.expected(c, torch.float64)[0].astype(np.float32)
    imgs = torch.from_numpy(d['imgs']).to(dev)
    boxes = [torch.from_numpy(b).to(dev) for b in d['gt_bboxes']]
    head = CondInstMaskHead(in_channels=C, boxinst_enabled=True, disable_rel_coors=not rel, max_proposals=-1, topk_per_img=64).to(dev)
    head.set_iter(5000)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    f, p = t(c['feat']).requires_grad_(True), t(c['params']).requires_grad_(True)
    coors, lvl, img = t(c['coors']), t(c['lvl'], torch.int64), t(c['img'], torch.int64)
    with GD.poisoned_empty():
        fused, _ = copy.deepcopy(head).forward_loss(f, p, coors, lvl, img, imgs, d['img_metas'], t(gt_inds, torch.int64), boxes, fuse_head=True)
        plain = head(f, p, coors, lvl, img)
    assert type(fused.grad_fn).__name__ == 'HeadBoxInstLossBackward', type(fused.grad_fn).__name__
    assert type(plain.grad_fn).__name__ == 'DynamicMaskHeadBackward', type(plain.grad_fn).__name__
    for name, got in (('head-fused', fused), ('forward()', plain)):
        m = X.first_difference(c, 'logits', got.detach().cpu().numpy(), want)
        assert not m, f'{name}: {m}'
    assert torch.equal(fused.detach(), plain.detach())


@pytest.mark.parametrize('case', [X.SLOTS[4], X.SLOTS[6], X.GENERIC[4]], ids=_ids([X.SLOTS[4], X.SLOTS[6], X.GENERIC[4]]))
def test_run_to_run(dev, case):
    c = X.dyadic_case(*case[0], **case[1])
    a, b = _run(dev, c), _run(dev, c)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('case', [X.TUNED[1], X.TUNED[14], X.GENERIC[1]], ids=_ids([X.TUNED[1], X.TUNED[14], X.GENERIC[1]]))
def test_half_precision_at_the_surface(dev, case, dtype):
    """fp16 / bf16 features and parameters (the dyadic values are exact in both): the logits equal the fp32 run of the same inputs, both
    gradients come back in the input's dtype and equal the fp32 gradients rounded once."""
    c = X.dyadic_case(*case[0], **case[1])
    full, half = _run(dev, c), _run(dev, c, dtype=dtype)
    once = lambda a: torch.from_numpy(a).to(dtype).float().numpy()
    _assert_exact(dev, c, half, (full['logits'], once(full['d_feat']), once(full['d_params'])))


@pytest.mark.parametrize('case', [X.TUNED[1], X.TUNED[6], X.GENERIC[1]], ids=_ids([X.TUNED[1], X.TUNED[6], X.GENERIC[1]]))
def test_guard_band_that_can_see(dev, case):
    """Every hidden unit goes through fmaxf(acc, 0.f), which returns 0 for a NaN operand: a stray read of a feature or of a first- or
    second-layer parameter from a NaN band is flushed and never reaches an output.  Here the bands around the features and the
    parameters hold 2^20 -- finite and dyadic --, so that a stray read changes an output by an exact, visible amount."""
    c, want = X.case_and_expected(*case[0], **case[1])
    if not X.is_tuned(c):
        want = [a.astype(np.float32) for a in X.expected(c, torch.float64, general=True)]
    _assert_exact(dev, c, _run(dev, c, band_bits=BAND_BITS), want)


# ---- non-finite inputs, pinned as they are -----------------------------------------------------------------------------------
NAN_CASE = X.NAN


def test_nan_feature_is_flushed_by_the_first_relu(dev):
    """A deviation from the reference: F.relu propagates a NaN, fmaxf(acc, 0.f) returns 0.  A NaN in one feature
    pixel of image 0 therefore zeroes the first hidden layer of that pixel for every instance of image 0 -- the logits equal the
    restatement with exactly that --, leaves the instances of the other images untouched, and d feat stays finite."""
    c, _ = X.case_and_expected(*NAN_CASE[0], **NAN_CASE[1])
    assert (c['img'] == 0).any() and (c['img'] == 1).any()
    r_, c_ = 13, 31                                         # the last row and column of a forward tile: in the halo of three more
    feat = c['feat'].copy()
    feat[0, 3, r_, c_] = np.nan
    clean, got = _run(dev, c), _run(dev, c, feat=feat)
    want = X.restate(c, torch.float64, zero_h1_at=(0, r_, c_))['logits'].numpy().astype(np.float32)
    assert not np.array_equal(want, clean['logits'])        # the pixel matters
    m = X.first_difference(c, 'logits', got['logits'], want)
    assert not m, m
    others = c['img'] != 0
    assert np.array_equal(got['logits'][others], clean['logits'][others]) and np.array_equal(got['d_params'][others], clean['d_params'][others])
    assert np.isfinite(got['d_feat']).all()


def test_nan_last_layer_parameter_stays_in_its_instance(dev):
    c, _ = X.case_and_expected(*NAN_CASE[0], **NAN_CASE[1])
    wsz, bsz = X.param_sizes(c['C'] + 2, 3, 8)
    params = c['params'].copy()
    params[2, wsz[0] + wsz[1] + 5] = np.nan                 # a last-layer weight of instance 2
    params[4, sum(wsz) + bsz[0] + bsz[1]] = np.nan          # the last-layer bias of instance 4
    clean, got = _run(dev, c), _run(dev, c, params=params)
    hit = np.zeros(c['N'], bool)
    hit[[2, 4]] = True
    assert np.isnan(got['logits'][hit]).all()
    assert np.array_equal(got['logits'][~hit], clean['logits'][~hit])


def test_nan_upstream_gradient_stays_in_its_instance(dev):
    c, _ = X.case_and_expected(*NAN_CASE[0], **NAN_CASE[1])
    g = c['g'].copy()
    g[3, 0, 11, 40] = np.nan
    clean, got = _run(dev, c), _run(dev, c, g=g)
    wsz, bsz = X.param_sizes(c['C'] + 2, 3, 8)
    assert np.isnan(got['d_params'][3, sum(wsz) + bsz[0] + bsz[1]])          # d b2 = sum of d y
    keep = np.arange(c['N']) != 3
    assert np.array_equal(got['d_params'][keep], clean['d_params'][keep])
    assert np.array_equal(got['logits'], clean['logits'])
