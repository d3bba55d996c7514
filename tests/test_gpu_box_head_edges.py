"""GPU: the box head's training step (csrc/fcos_loss.hip, csrc/focal_device.hpp) at the configs' level sizes and on its tile, chunk and
image-count edges.  The cases are tests/fcos_edges.py's; tests/test_host_box_head_edges.py shows what each of them reaches.

Targets take no tolerance: every key is bit-equal to the float32 restatement (tests/fcos_ref.py), boxes off the pixel grid included.
Losses and gradients are compared with the restatement's float64 run on the float32 targets, within 4x what the restatement's own
float32 run differs from it on the same inputs (floored at 2^-24: the results are stored as float32); the figures are printed."""
import numpy as np
import pytest
import torch

from tests import fcos_edges as E
from tests import fcos_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

MAPS = ('cls', 'bbox', 'ctr')
FLOOR = 2.0 ** -24
BAND = 4096


def lib_targets(dev, case, s):
    import boxinstseg_amd as B
    return B.condinst_box_targets(case['sizes'], s['strides'], [b.to(dev) for b in case['boxes']], [t.to(dev) for t in case['labels']],
                                  regress_ranges=s['regress_ranges'], center_sampling=s['center_sampling'],
                                  center_sample_radius=s['center_sample_radius'], norm_on_bbox=s['norm_on_bbox'], num_classes=s['num_classes'],
                                  B=case['B'])


def assert_targets(tg, want):
    for k in R.TARGET_KEYS:
        assert G.same(getattr(tg, k).cpu(), want[k]), k
    stats = tg.stats.cpu()
    n_pos, ctr_sum = E.stats_of(want)
    print('stats', stats.tolist(), 'want', (n_pos, ctr_sum))
    assert float(stats[0]) == n_pos
    assert G.same(stats[1:], torch.tensor([ctr_sum], dtype=torch.float32))
    assert tg.status.cpu().tolist() == [0]


# ---- A -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.COMBOS)
def test_targets_at_the_configs_level_sizes(dev, name):
    """81 tiles per image, 324 workgroups (two trips of the finish kernel), 70 boxes off the pixel grid in image 0 (two chunks), an image
    without boxes and one with a single box over the canvas.  The centerness sum is exact in fp64 in any order (host test), so stats[1]
    has one rounding and is compared bit for bit."""
    assert_targets(lib_targets(dev, E.config_case(), E.config_settings(name)), E.config_want(name))


# ---- B -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_on_bbox', [True, False])
def test_targets_on_the_tile_edges(dev, norm_on_bbox):
    """Levels of 256, 257, 255, 512 and 511 locations in one call, every location positive with distances of its own."""
    c, s = E.tile_case(), E.tile_settings(norm_on_bbox)
    want = E.ref_targets(c, s)
    tg = lib_targets(dev, c, s)
    assert_targets(tg, want)
    assert int(tg.stats[0]) == 2 * sum(h * w for h, w in E.SIZES_TILE)


@pytest.mark.parametrize('arrangement', E.CHUNK_ARRANGEMENTS)
def test_box_chunks_at_a_multi_tile_level(dev, arrangement):
    c, s = E.chunk_case(arrangement), E.chunk_settings()
    tg = lib_targets(dev, c, s)
    assert_targets(tg, E.ref_targets(c, s))
    assert int(tg.stats[0]) == E.CHUNK_SIZE[0] * E.CHUNK_SIZE[1]


def test_targets_of_the_largest_batch(dev):
    """B = BXI_MAX_IMAGES: the last entry of the offset table; image 63's positives carry the indices that follow images 0's and 31's."""
    c, s = E.many_images_case(), E.many_images_settings()
    tg = lib_targets(dev, c, s)
    assert_targets(tg, E.ref_targets(c, s))
    last = tg.gt_inds[(tg.img_inds == E.MAX_IMAGES - 1) & (tg.gt_inds >= 0)]
    assert set(last.cpu().tolist()) == {5, 6}


# ---- C -----------------------------------------------------------------------------------------------------------------------
def run_loss(dev, m_np, case, s, upstream=(1.0, 1.0, 1.0)):
    import boxinstseg_amd as B
    m = {k: [torch.from_numpy(a).to(dev).requires_grad_(True) for a in m_np[k]] for k in MAPS}
    out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], [b.to(dev) for b in case['boxes']], [t.to(dev) for t in case['labels']], None, s)[0]
    (upstream[0] * out['loss_cls'] + upstream[1] * out['loss_bbox'] + upstream[2] * out['loss_centerness']).backward()
    vals = torch.stack([out['loss_cls'], out['loss_bbox'], out['loss_centerness']]).detach().cpu()
    return vals, {k: [t.grad.cpu() for t in m[k]] for k in MAPS}


@pytest.mark.parametrize('name', E.LOSS_CASES)
def test_losses_and_gradients_over_many_tiles(dev, name):
    """324 per-location and 398 focal workgroups: 722 partials, three trips of the finish kernel; saturated logits on both kinds of element
    at the tile and image edges of the two large levels.

    Measured on an MI355X (relative error of loss_cls / loss_bbox / loss_centerness, then of the cls / bbox / ctr gradients against the
    largest float64 gradient of the kind; in brackets what was allowed: 4x the restatement's own float32-against-float64 figure,
    floored at 2^-24 before the factor):
      cs_norm_giou    losses 3.2e-9 / 1.2e-7 / 5.0e-9 (2.4e-7 / 2.4e-7 / 3.1e-7), gradients 3.7e-7 / 2.2e-5 / 9.8e-8 (2.3e-6 / 8.7e-5 / 3.9e-7)
      box_pix_ioulog  losses 2.0e-8 / 5.2e-8 / 4.5e-8 (2.4e-7 / 2.4e-7 / 2.4e-7), gradients 3.3e-7 / 3.4e-4 / 1.0e-7 (2.0e-6 / 1.3e-3 / 4.6e-7)
    The distance gradients' figures are large on both sides: the seeded distances hold exact zeros, so some positives predict an almost
    flat box (0.03 pixels high under a target of 100); its IoU is tiny, that location carries both the largest gradient and the largest
    error, and the float32 restatement itself is good to 3e-4 there."""
    case, s, lc = E.config_case(), E.config_settings(name), E.loss_case(name)
    tg = E.config_want(name)
    l64, *g64 = R.losses_and_grads(lc['maps'], tg, s, torch.float64)
    l32, *g32 = R.losses_and_grads(lc['maps'], tg, s, torch.float32)
    tol_loss = [4 * max(abs(float(a) - float(b)) / abs(float(b)), FLOOR) for a, b in zip(l32, l64)]
    gmax = [max(float(g.abs().max()) for g in part) for part in g64]
    tol_grad = [4 * max(max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64)) / gm, FLOOR) for p32, p64, gm in zip(g32, g64, gmax)]
    vals, grads = run_loss(dev, lc['maps'], case, s)
    vals2, grads2 = run_loss(dev, lc['maps'], case, s)
    assert G.same(vals, vals2) and all(G.same(a, b) for k in MAPS for a, b in zip(grads[k], grads2[k]))      # two runs: bit-identical
    assert bool(torch.isfinite(vals).all()) and all(bool(torch.isfinite(g).all()) for k in MAPS for g in grads[k])
    err_loss = [abs(float(v) - float(w)) / abs(float(w)) for v, w in zip(vals, l64)]
    err_grad = [max(float((g.double() - w).abs().max()) for g, w in zip(grads[k], p64)) / gm for k, p64, gm in zip(MAPS, g64, gmax)]
    print(f'{name}: losses {vals.tolist()} vs float64 {l64.tolist()}; relative error {", ".join(f"{e:.3e}" for e in err_loss)} (allowed '
          f'{", ".join(f"{t:.3e}" for t in tol_loss)}); gradient error cls / bbox / ctr {", ".join(f"{e:.3e}" for e in err_grad)} (allowed '
          f'{", ".join(f"{t:.3e}" for t in tol_grad)})')
    assert all(float(w) > 0 for w in l64) and all(gm > 0 for gm in gmax)
    assert all(e <= t for e, t in zip(err_loss, tol_loss)), (err_loss, tol_loss)
    assert all(e <= t for e, t in zip(err_grad, tol_grad)), (err_grad, tol_grad)
    # background locations and the image without boxes: exact zeros
    bg = (tg['gt_inds'] < 0)
    assert bool(bg[tg['img_inds'] == 2].all())
    for k in ('bbox', 'ctr'):
        flat = R.flatten_maps(grads[k])
        assert bool((flat[bg] == 0).all()) and bool((flat[~bg] != 0).any()), k
        assert all(bool((g[2] == 0).all()) for g in grads[k])
    # upstream gradients: one fp32 multiply on both sides
    _, scaled = run_loss(dev, lc['maps'], case, s, E.UPSTREAM)
    for k, u in zip(MAPS, E.UPSTREAM):
        for a, b in zip(scaled[k], grads[k]):
            assert G.same(a, b * u), k


@pytest.mark.parametrize('name', E.LOSS_CASES)
def test_prediction_equal_to_the_target_over_many_tiles(dev, name):
    case, s, lc = E.config_case(), E.config_settings(name), E.loss_case(name)
    tg = lib_targets(dev, case, s)
    m = dict(lc['maps'], bbox=E.maps_from_targets(tg.bbox_targets.cpu().numpy(), E.SIZES_A, case['B']))
    vals, grads = run_loss(dev, m, case, s)
    assert float(vals[1]) == 0.0 and float(vals[0]) > 0 and float(vals[2]) > 0              # IoU = GIoU = 1 on every positive
    assert all(bool(torch.isfinite(g).all()) for k in MAPS for g in grads[k])


def _levels(sizes, strides):
    from boxinstseg_amd import _lib
    arr = (_lib.FcosLevel * len(sizes))()
    for i, ((h, w), st) in enumerate(zip(sizes, strides)):
        arr[i] = _lib.FcosLevel(h, w, st)
    return arr


def _grads_array(gs, n):
    from boxinstseg_amd import _lib
    arr = (_lib.FcosGrads * n)()
    for lv in range(n):
        arr[lv] = _lib.FcosGrads(G.ptr(gs['cls'][lv]), G.ptr(gs['bbox'][lv]), G.ptr(gs['ctr'][lv]))
    return arr


@pytest.mark.parametrize('name', E.LOSS_CASES)
def test_loss_and_rescale_guarded_over_many_tiles(dev, name):
    """One direct call of bxi_fcos_loss_f32 and one of bxi_fcos_grad_rescale_f32 at the configs' sizes with every output inside guard bands
    (lead = 1, pre-filled with the unwritten pattern) and a workspace of exactly the queried size: bands intact, every gradient element,
    the three losses and the whole workspace written, inputs unchanged, results bit-equal to the plain call."""
    from boxinstseg_amd import _lib
    case, s, lc = E.config_case(), E.config_settings(name), E.loss_case(name)
    B, C, n, lead = case['B'], case['C'], len(E.SIZES_A), 1
    lib = _lib.load()
    tg = lib_targets(dev, case, s)
    maps = {k: [torch.from_numpy(a).to(dev) for a in lc['maps'][k]] for k in MAPS}
    nbytes = lib.bxi_fcos_workspace_bytes(_levels(E.SIZES_A, E.STRIDES_A), n, B, C)
    assert nbytes == 16 * 722
    kind = _lib.FCOS_BBOX_KINDS[s['bbox_loss_kind']]

    def call(ins, outs, labels, bt, ct, norm, losses, ws):
        lv = (_lib.DetLevel * n)()
        for i, ((h, w), st) in enumerate(zip(E.SIZES_A, E.STRIDES_A)):
            lv[i] = _lib.DetLevel(G.ptr(ins['cls'][i]), G.ptr(ins['bbox'][i]), G.ptr(ins['ctr'][i]), None, h, w, st)
        G.ok(lib.bxi_fcos_loss_f32(lv, n, B, C, G.ptr(labels), G.ptr(bt), G.ptr(ct), G.ptr(norm), s['gamma'], s['alpha'], s['loss_weight_cls'],
                                   s['loss_weight_bbox'], s['loss_weight_centerness'], kind, s['eps'], _grads_array(outs, n), G.ptr(losses),
                                   G.ptr(ws), nbytes, G.stream(dev)))

    plain_g = {k: [torch.empty_like(t) for t in maps[k]] for k in MAPS}
    plain_l = torch.empty(3, device=dev)
    call(maps, plain_g, tg.labels, tg.bbox_targets, tg.ctr_targets, tg.stats, plain_l, torch.empty(nbytes // 4, dtype=torch.int32, device=dev))
    gin = {k: [G.embed(t, (lead + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
    gout = {k: [G.out(tuple(t.shape), torch.float32, dev, lead, BAND) for t in maps[k]] for k in MAPS}
    glab, gbt, gct, gnorm = G.embed(tg.labels, 1, BAND), G.embed(tg.bbox_targets, lead, BAND), G.embed(tg.ctr_targets, lead, BAND), G.embed(tg.stats, lead, BAND)
    glosses, gw = G.out(3, torch.float32, dev, lead, BAND), G.out(nbytes // 4, torch.int32, dev, lead, BAND)
    call(gin, gout, glab, gbt, gct, gnorm, glosses, gw)
    ins = [t for k in MAPS for t in gin[k]] + [glab, gbt, gct, gnorm]
    outs = [t for k in MAPS for t in gout[k]]
    G.check_bands(*ins, *outs, glosses, gw)
    G.check_written(*outs, glosses, gw)
    G.check_unchanged(*ins)
    assert G.same(glosses.t, plain_l) and bool(torch.isfinite(glosses.t).all()) and float(glosses.t.min()) > 0
    for k in MAPS:
        assert all(G.same(got.t, want) for got, want in zip(gout[k], plain_g[k])), k
    # the backward rescale of those unit gradients, out of place
    up = torch.tensor(E.UPSTREAM, device=dev)
    gup = G.embed(up, lead, BAND)
    gres = {k: [G.out(tuple(t.shape), torch.float32, dev, lead, BAND) for t in maps[k]] for k in MAPS}
    for k in MAPS:
        for t in gout[k]:
            t.is_input, t.before = True, t.interior().clone()
    G.ok(lib.bxi_fcos_grad_rescale_f32(_levels(E.SIZES_A, E.STRIDES_A), n, B, C, _grads_array(gout, n), gup.ptr(), _grads_array(gres, n), G.stream(dev)))
    res = [t for k in MAPS for t in gres[k]]
    G.check_bands(gup, *outs, *res)
    G.check_written(*res)
    G.check_unchanged(gup, *outs)
    for i, k in enumerate(MAPS):
        for got, src in zip(gres[k], plain_g[k]):
            assert G.same(got.t, src * up[i]), k
