"""GPU: the SOLOv2-style training targets at the configs' grids, over the 256-wide chunk edges of the assignment, at every cell edge in
both precisions, through every trip of the mask pass, and the category loss over several tiles.  The cases come from
tests/solo_edges.py; tests/test_host_solo_targets_edges.py shows on the CPU that each reaches the path it is named for.

Every target is an integer: EQUAL to tests/solo_ref.py, no tolerance.  ``loss_cate`` and its gradient: within 4x the difference between
``R.cate_loss`` in float32 and in float64 on the same inputs, measured in the test, against the float64 values.

Which branches of ``floor_div_int`` the planted moments reach (counted by the host test from the restatement): the sign fix (negative
numerators: an edge left of or above the canvas), the ``div == 0`` branch (numerators below 1/S) and ALSO the ``div - floor > 0.5``
correction -- (a - mod) / b falls short of the integer in about 2.5 % of the divisions here, in both precisions, and the correction
is what brings it back.  Not reachable with the positive divisors 1/S and finite inputs: the ``b < 0`` half of the sign fix, the NaN
guard and the 2^30 clamp; nothing is contorted to reach them."""
import functools

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import solo_edges as E
from tests import solo_ref as R
from tests.test_gpu_solo_targets import _check_against

pytestmark = pytest.mark.gpu


# ---- A: the public wrappers at the configs' grids; 3 + 255 / 256 / 257 / 300 instances -----------------------------------------
@pytest.fixture(scope='module')
def big_dev(dev):
    boxes, labels, masks, _ = E.big_batch()
    return [b.to(dev) for b in boxes], [t.to(dev) for t in labels], [torch.from_numpy(m).to(dev) for m in masks]


@functools.lru_cache(maxsize=None)
def _big_rescaled(f):
    _, _, masks, _ = E.big_batch()
    return [R.rescale(m, f) for m in masks]


def _run_big(big_dev, mode, n, grids64):
    import boxinstseg_amd as B
    boxes, labels, masks = big_dev
    boxes, labels, masks = [boxes[0], boxes[1][:n]], [labels[0], labels[1][:n]], [masks[0], masks[1][:n]]
    kw = E.assign_kw(grids64)
    if mode == 'discobox':
        return B.solov2_targets(boxes, labels, masks, E.FEAT, strides=E.STRIDES64 if grids64 else E.STRIDES, **kw)
    return B.box_solov2_targets(boxes, labels, masks, E.PLANES64 if grids64 else E.PLANES, strides=E.STRIDES64 if grids64 else E.STRIDES, **kw)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('n,grids64', [(255, False), (256, False), (257, False), (300, False), (300, True)])
def test_assignment_at_the_configs_grids(dev, big_dev, mode, n, grids64):
    """Grids [40,36,24,16,12] (and [64,1]) on a 256 x 320 canvas: up to seven 256-cell chunks (sixteen at S = 64) per level and two
    256-instance chunks per image, image 1's local indices three below its global ones."""
    tg = _run_big(big_dev, mode, n, grids64)
    _check_against(tg, E.big_want(mode, n, grids64))
    strides = E.STRIDES64 if grids64 else E.STRIDES
    assert sorted(tg.masks) == ([4] if mode == 'discobox' else sorted({s // 2 for s in strides}))
    for f, m in tg.masks.items():
        per = _big_rescaled(f)
        assert m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), np.concatenate([per[0], per[1][:n]])), f


# ---- B: bxi_solo_assign_f32 on planted moments ------------------------------------------------------------------------------------
def _assign(dev, mode, c):
    """One direct call, one image, eight levels, every output inside guard bands and pre-filled with the 'nobody wrote this' pattern."""
    from boxinstseg_amd import _lib
    grids, n = c['num_grids'], len(c['mom'])
    L, N, P = len(grids), sum(s * s for s in grids), _lib.SOLO_PAIRS_PER_INSTANCE * len(grids) * n
    boxes, labels, mom = c['boxes'].to(dev).contiguous(), c['labels'].to(dev), torch.from_numpy(c['mom']).to(dev).contiguous()
    outs = [G.out(N, torch.int64, dev), G.out(N, torch.uint8, dev, 3), G.out(N, torch.int32, dev, 1), G.out(N, torch.int32, dev, 2),
            G.out(P, torch.int32, dev, 3), G.out(P, torch.int32, dev, 1), G.out(2 * L, torch.int32, dev, 1), G.out(1, torch.int32, dev, 2),
            G.out(1, torch.int32, dev, 3)]
    rc = _lib.load().bxi_solo_assign_f32(
        _lib.SOLO_MODES[mode], 1, L, _lib.int_array(grids), _lib.float_array([v for r in c['scale_ranges'] for v in r]), c['sigma'],
        c['num_classes'], c['canvas'][0], c['canvas'][1], boxes.data_ptr(), labels.data_ptr(), mom.data_ptr(), _lib.int_array([0, n]),
        *(o.ptr() for o in outs), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(*outs)
    G.check_written(*outs)
    return [o.t.cpu().numpy() for o in outs]


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', sorted(E.planted_cases()))
def test_assign_on_planted_moments(dev, name, mode):
    """Centres on and one sixteenth of a pixel beside every k/S for S = 1..64 (under a small and under an all-covering box), window
    edges on and beside k * size / S, below 0 and above the canvas, areas on and one fp32 step off the range ends, moments no fp32
    holds: each instance's window in instance order, the per-cell outputs, the compacted owners and the counts."""
    from boxinstseg_amd import _lib
    c = E.planted_cases()[name]
    want = E.planted_want(name, mode)
    cate, ind, owner, sel, pc, pi, counts, num_ins, status = _assign(dev, mode, c)
    n, cap = len(c['mom']), _lib.SOLO_PAIRS_PER_INSTANCE * len(c['mom'])
    at = 0
    for l, S in enumerate(c['num_grids']):
        cells = S * S
        wp, ws = want['pair_cell'][l], want['sel_inst'][l]
        assert counts[2 * l:2 * l + 2].tolist() == [len(wp), len(ws)], (l, S)
        assert np.array_equal(pc[cap * l:cap * l + len(wp)], wp) and bool((pc[cap * l + len(wp):cap * (l + 1)] == -1).all()), (l, S)
        assert np.array_equal(pi[cap * l:cap * l + len(wp)], want['pair_inst'][l]) and bool((pi[cap * l + len(wp):cap * (l + 1)] == -1).all()), (l, S)
        assert np.array_equal(cate[at:at + cells], want['cate_labels'][l]), (l, S)
        assert np.array_equal(owner[at:at + cells], want['cell_owner'][l]), (l, S)
        assert np.array_equal(ind[at:at + cells], (want['cell_owner'][l] >= 0).astype(np.uint8)), (l, S)
        assert np.array_equal(sel[at:at + len(ws)], ws) and bool((sel[at + len(ws):at + cells] == -1).all()), (l, S)
        at += cells
    assert num_ins.tolist() == [want['num_ins']] and status.tolist() == [0] and n > 0


# ---- C: bxi_solo_mask_pass_u8 -----------------------------------------------------------------------------------------------------
def _mask_pass(dev, images, factors, planes):
    """One direct call on device masks (``images``: uint8 [G,H,W] tensors or Guarded views); outputs pre-filled with 0xFF bytes."""
    from boxinstseg_amd import _lib
    ia, pa = _lib.int_array, _lib.ptr_array
    shapes = [tuple((m.t if isinstance(m, G.Guarded) else m).shape) for m in images]
    offsets = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(int).tolist()
    outs = [torch.full((offsets[-1], h, w), 0xFF, dtype=torch.uint8, device=dev) for h, w in planes]
    mom = torch.full((offsets[-1], 3), -1, dtype=torch.int64, device=dev)
    rc = _lib.load().bxi_solo_mask_pass_u8(pa([G.ptr(m) for m in images]), ia(offsets), ia([s[1] for s in shapes]), ia([s[2] for s in shapes]),
                                           len(images), ia(factors), ia([p[0] for p in planes]), ia([p[1] for p in planes]), len(factors),
                                           pa([o.data_ptr() for o in outs]), mom.data_ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    return mom, outs


def _check_mask_case(dev, case, lead=None):
    if lead is None:
        images = [torch.from_numpy(m).to(dev) for m in case['images']]
    else:
        images = [G.embed(torch.from_numpy(m).to(dev), (lead + 7 * i) % 16 or lead) for i, m in enumerate(case['images'])]
    mom, outs = _mask_pass(dev, images, case['factors'], case['planes'])
    want_mom, want_planes = E.mask_want(case)
    assert np.array_equal(mom.cpu().numpy(), want_mom)
    for f, o, w in zip(case['factors'], outs, want_planes):
        assert np.array_equal(o.cpu().numpy(), w), f
    if lead is not None:
        G.check_bands(*images)
        G.check_unchanged(*images)


def test_mask_pass_second_trip_of_the_vector_loop(dev):
    """32 x 272, factors [4, 8]: 272 vectors per 16-row band for 256 threads.  Instance 0 has ones only where the second trip reads."""
    _check_mask_case(dev, E.mask_cases()['second_trip'])


@pytest.mark.parametrize('lead', [None, 1, 15])
@pytest.mark.parametrize('W', [4, 8, 12])
@pytest.mark.parametrize('H', [16, 32])
def test_mask_pass_narrow_masks(dev, H, W, lead):
    """A 16-byte vector spans four, two or one and a third rows; at byte offsets 1 and 15 the head and the tail span several rows too."""
    _check_mask_case(dev, E.mask_cases()[f'narrow_{H}x{W}'], lead)


def test_mask_pass_half_band_and_empty_bands(dev):
    """H = 24 and 48 under bands of 16 rows: a last band that is half full, and for the shorter image a band with no source row."""
    _check_mask_case(dev, E.mask_cases()['half_band'])


@pytest.mark.parametrize('key', ['factors_2', 'factors_2_4_8_16', 'factors_32_64'])
def test_mask_pass_factor_sets(dev, key):
    """Factor 2 samples at offset 0; four factors at once; 32 and 64 make a band of 64 rows.  Planes larger than H/f x W/f: the border is zero."""
    _check_mask_case(dev, E.mask_cases()[key])


@pytest.mark.parametrize('H,W,f', E.LARGE_MASKS)
def test_mask_pass_moments_above_2_to_32(dev, H, W, f):
    """One full mask and one empty one: the closed-form moments, an all-one and an all-zero plane.  2048 x 2304: m10 and m01 above 2^32
    in the total; 64 x 196608 under a band of 64 rows: above 2^32 in one workgroup's partial and in one thread's."""
    masks = torch.zeros(2, H, W, dtype=torch.uint8, device=dev)
    masks[0] = 1
    mom, (out,) = _mask_pass(dev, [masks], [f], [(H // f, W // f)])
    assert mom.cpu().tolist() == E.large_mask_moments(H, W)
    assert bool((out[0] == 1).all()) and bool((out[1] == 0).all())


# ---- E: the category loss over several tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('gamma,alpha', E.CATE_SETTINGS)
def test_cate_loss_over_several_tiles(dev, gamma, alpha):
    """B = 2, C = 3, grids [40,36,1,2,3]: full tiles and a partial one on two levels, hw = 1 (the (c, b) carry wraps on every element),
    hw = 4 (one thread per plane), hw = 9; logits of +-30, +-90, +-200 on positive and negative elements; gamma = 2 and the general kernel."""
    import boxinstseg_amd as B
    c = E.cate_case()
    labels = torch.from_numpy(c['labels']).to(dev)
    num_ins = torch.tensor([c['num_ins']], dtype=torch.int32, device=dev)
    lw, up = E.CATE_LOSS_WEIGHT, E.CATE_UPSTREAM
    l64, g64 = R.cate_loss(c['preds'], c['labels'], c['num_ins'], gamma, alpha, lw)
    l32, g32 = R.cate_loss(c['preds'], c['labels'], c['num_ins'], gamma, alpha, lw, dtype=torch.float32)
    gmax = max(float(g.abs().max()) for g in g64)
    tol_loss = 4 * abs(float(l32) - float(l64)) / abs(float(l64))
    tol_grad = 4 * max(float((a.double() - b).abs().max()) for a, b in zip(g32, g64)) / gmax
    runs = []
    for _ in range(2):
        preds = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in c['preds']]
        loss = B.solo_cate_loss(preds, labels, num_ins, gamma, alpha, lw)
        (loss * up).backward()
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in preds]))
    (loss, grads), (loss2, grads2) = runs
    assert G.same(loss, loss2) and all(G.same(a, b) for a, b in zip(grads, grads2))                # two runs: bit-identical
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
    err = abs(float(loss) - float(l64)) / abs(float(l64))
    errs = [float((g.double() - w * up).abs().max()) / (gmax * up) for g, w in zip(grads, g64)]
    print(f'gamma {gamma}, alpha {alpha}: loss {float(loss):.9g} vs {float(l64):.9g}, relative {err:.3e} (allowed {tol_loss:.3e}); '
          f'gradient errors per level {", ".join(f"{e:.3e}" for e in errs)} (allowed {tol_grad:.3e})')
    assert tol_loss > 0 and tol_grad > 0
    assert err <= tol_loss
    assert max(errs) <= tol_grad
