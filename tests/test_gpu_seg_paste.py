"""GPU: the final masks of the SOLOv2-style heads (csrc/seg_paste.hip, boxinstseg_amd.seg_paste / solo_get_seg / solo_format_results and
_seg_tail on top of them).

Truth is tests/seg_paste_ref.py: the reference's composition in float64 (p64) and the same on the fp32 sampling grid (grid64).  Tie rule:
a mask byte may differ from ``grid64 > thr`` only where |grid64 - thr| <= 1e-6, and from ``p64 > thr`` only inside that band widened, pixel
by pixel, by |grid64 - p64|.  Every parity test also asserts that at least 99 % of its pixels lie outside the band.  The probabilities are
matrix_nms_ref.disc_probs (seed 1): discs of 0.75..0.99 on 0.01..0.4, so almost no resized value comes near the threshold."""
import os

import numpy as np
import pytest
import torch

from tests import matrix_nms_ref as R
from tests import seg_paste_ref as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'matrix_nms.npz')
THR = 0.5

# (h, w), crop, out; up = 4 (h, w)
SHAPES = {
    'up_byte_tail': ((7, 9), (27, 33), (40, 51)),              # stage 2 up-samples; one row group with a byte tail
    'down_odd_width': ((25, 38), (97, 150), (61, 93)),         # down-sampling, out_w not a multiple of 16
    'identity_aligned': ((24, 40), (96, 160), (96, 160)),      # crop = up = out: stage 2 is the identity, rows 16-byte aligned
    'two_bands': ((13, 21), (52, 84), (131, 200)),             # more than one band
    'two_chunks': ((3, 70), (12, 277), (9, 1100)),             # a second column chunk
    'small_band': ((240, 300), (960, 1200), (30, 100)),        # a 16-row band's source rows do not fit the LDS budget
}


def meta(crop, out):
    return dict(img_shape=(crop[0], crop[1], 3), ori_shape=(out[0], out[1], 3))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, probs, keep, hw, crop, out, thr=THR):
    """-> (uint8 masks numpy, stats numpy) of one seg_paste call, with the surface's promises checked."""
    from boxinstseg_amd import seg_paste
    masks, stats = seg_paste(_t(probs, dev), _t(np.asarray(keep, np.int64), dev), hw, meta(crop, out), thr)
    torch.cuda.synchronize()
    n = len(keep)
    assert masks.is_cuda and masks.dtype == torch.bool and tuple(masks.shape) == (n, out[0], out[1])
    assert stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (n, 5)
    return masks.view(torch.uint8).cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_kernel_vs_fp64(dev, name):
    hw, crop, out = SHAPES[name]
    rng = np.random.default_rng(1)
    n_all = 3 if name == 'small_band' else 6
    probs = R.disc_probs(rng, n_all, *hw)
    keep = rng.permutation(n_all)[:max(n_all - 1, 1)]
    up = (4 * hw[0], 4 * hw[1])
    got, stats = run(dev, probs, keep, hw, crop, out)
    S.check_tie(got, probs, keep, up, crop, out, THR, name)
    assert np.array_equal(stats, S.stats_of(got))
    assert got.any() and not got.all()


def test_permutation_repeats_and_bad_indices(dev):
    hw, crop, out = SHAPES['down_odd_width']
    rng = np.random.default_rng(1)
    probs = R.disc_probs(rng, 5, *hw)
    keep = np.array([3, -1, 0, 3, 5, 4, 1, 3, -7, 2 ** 40, 2])
    got, stats = run(dev, probs, keep, hw, crop, out)
    S.check_tie(got, probs, keep, (4 * hw[0], 4 * hw[1]), crop, out, THR, 'permutation')
    bad = (keep < 0) | (keep >= 5)
    assert not got[bad].any() and np.array_equal(stats[bad], np.tile(np.array([0, -1, -1, -1, -1], np.int32), (int(bad.sum()), 1)))
    assert np.array_equal(got[0], got[3]) and np.array_equal(got[0], got[7]) and got[~bad].reshape(int((~bad).sum()), -1).any(1).all()
    assert np.array_equal(stats, S.stats_of(got))


def test_no_kept_masks(dev):
    hw, crop, out = SHAPES['up_byte_tail']
    probs = R.disc_probs(np.random.default_rng(1), 2, *hw)
    got, stats = run(dev, probs, np.zeros(0, np.int64), hw, crop, out)
    assert got.shape == (0, out[0], out[1]) and stats.shape == (0, 5)


def test_stats_are_numpys_count_and_bounds(dev):
    """Exactly, mask by mask -- including a mask with every probability below the threshold, one with a single pixel's blob in a corner,
    a full one, and masks that span two bands and two chunks."""
    for name in ('two_bands', 'two_chunks'):
        hw, crop, out = SHAPES[name]
        rng = np.random.default_rng(2)
        probs = R.disc_probs(rng, 5, *hw)
        probs[1] = rng.uniform(0.01, 0.4, hw).astype(np.float32)          # below the threshold everywhere
        probs[2] = 0.01
        probs[2, -1, -1] = 0.99                                            # the bottom-right corner only
        probs[3] = 0.9                                                      # full
        got, stats = run(dev, probs, np.arange(5), hw, crop, out)
        want = S.stats_of(got)
        assert np.array_equal(stats, want), name
        assert stats[1].tolist() == [0, -1, -1, -1, -1]
        assert stats[2, 0] > 0 and stats[2, 3] == out[1] - 1 and stats[2, 4] == out[0] - 1 and stats[2, 1] > 0 and stats[2, 2] > 0
        assert stats[3].tolist() == [out[0] * out[1], 0, 0, out[1] - 1, out[0] - 1]
        S.check_tie(got, probs, np.arange(5), (4 * hw[0], 4 * hw[1]), crop, out, THR, name, cap=None)


def test_dense_ties(dev):
    """Probabilities within 2.5e-5 of the threshold everywhere: the rule holds outside the band (no cap here: this input is all ties by
    construction; the band is still narrower than the spread)."""
    hw, crop, out = SHAPES['down_odd_width']
    rng = np.random.default_rng(11)
    probs = (0.5 + rng.uniform(-2.5e-5, 2.5e-5, (4,) + hw)).astype(np.float32)
    keep = np.arange(4)
    up = (4 * hw[0], 4 * hw[1])
    got, stats = run(dev, probs, keep, hw, crop, out)
    pg = S.check_tie(got, probs, keep, up, crop, out, THR, 'dense ties', cap=None)
    assert (np.abs(pg - THR) > S.TIE).mean() > 0.75
    assert np.array_equal(stats, S.stats_of(got))


def test_saturated_maps_are_exact(dev):
    """0 / 1 probabilities: the resized values are sums of a few tap-weight products, and at this shape none of them comes within 1e-5
    of the threshold (asserted on grid64), where the kernel's regrouped fp32 products (~1e-7) cannot flip a byte: every byte is the truth."""
    hw, crop, out = SHAPES['two_bands']
    rng = np.random.default_rng(12)
    probs = (rng.random((4,) + hw) < 0.5).astype(np.float32)
    probs[2], probs[3] = 0.0, 1.0
    keep = np.array([0, 1, 2, 3])
    up = (4 * hw[0], 4 * hw[1])
    thr = THR
    got, stats = run(dev, probs, keep, hw, crop, out, thr)
    pg = S.grid64(probs, keep, up, crop, out)
    assert np.abs(pg - float(np.float32(thr))).min() > 1e-5
    assert np.array_equal(got, (pg > float(np.float32(thr))).astype(np.uint8))
    assert not got[2].any() and got[3].all()
    assert np.array_equal(stats, S.stats_of(got))


def test_nan_plane_gives_zeros(dev):
    hw, crop, out = SHAPES['up_byte_tail']
    probs = R.disc_probs(np.random.default_rng(1), 3, *hw)
    probs[1] = np.nan
    got, stats = run(dev, probs, np.array([0, 1, 2]), hw, crop, out)
    assert not got[1].any() and stats[1].tolist() == [0, -1, -1, -1, -1]
    assert got[0].any() and got[2].any()
    S.check_tie(got[[0, 2]], probs, np.array([0, 2]), (4 * hw[0], 4 * hw[1]), crop, out, THR, 'next to a NaN plane')


def test_two_calls_are_bit_identical(dev):
    hw, crop, out = SHAPES['two_chunks']
    probs = R.disc_probs(np.random.default_rng(1), 6, *hw)
    keep = np.array([5, 0, 0, 3, 9])
    a, b = run(dev, probs, keep, hw, crop, out), run(dev, probs.copy(), keep, hw, crop, out)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _golden():
    from tests.test_host_matrix_nms import golden_seg
    g = np.load(GOLDEN)
    cfg, idx, cate_scores, level = golden_seg(g)
    ref = R.seg_nms_ref(g['seg_probs'][idx[:, 0]], idx[:, 1], cate_scores, level, cfg['mask_thr'], cfg['filter_thr'], cfg['nms_pre'],
                        cfg['max_per_img'], cfg['kernel'], cfg['sigma'])
    crop, out = tuple(int(v) for v in g['seg_img_shape'][:2]), tuple(int(v) for v in g['seg_ori_shape'][:2])
    return g, cfg, idx[:, 0][ref['keep_inds']], crop, out


def test_reference_fixture(dev):
    """seg_probs of the fixture the reference's get_seg_single made, with the reference's keep list, against its seg_out_masks."""
    g, cfg, keep, crop, out = _golden()
    assert g['seg_out_labels'].shape[0] == len(keep)
    got, stats = run(dev, g['seg_probs'], keep, (11, 17), crop, out, cfg['mask_thr'])
    want = np.unpackbits(g['seg_out_masks'], axis=1)[:, :out[0] * out[1]].reshape(-1, *out)
    pg = S.check_tie(got, g['seg_probs'], keep, (44, 68), crop, out, cfg['mask_thr'], 'fixture')
    S.check_tie(want, g['seg_probs'], keep, (44, 68), crop, out, cfg['mask_thr'], 'the fixture itself')
    outside = np.abs(pg - float(np.float32(cfg['mask_thr']))) > S.TIE
    assert np.array_equal(got[outside], want[outside])
    assert np.array_equal(stats, S.stats_of(got))


def test_format_results_against_the_restated_loop(dev):
    """solo_format_results on device results against the restated format_results on the same masks on the CPU: equal arrays, with a class
    that gets no mask, a kept mask that is empty, and result order inside a class."""
    import types
    from boxinstseg_amd import seg_paste, solo_format_results
    from boxinstseg_amd.seg_paste import paste_results
    hw, crop, out = SHAPES['down_odd_width']
    rng = np.random.default_rng(4)
    probs = R.disc_probs(rng, 6, *hw)
    probs[4] = 0.2                                                           # kept, but empty after the threshold
    keep = np.array([2, 4, 0, 5, 1])
    labels = torch.tensor([3, 0, 3, 1, 0], device=dev)
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5], device=dev)
    tp, tk = _t(probs, dev), _t(keep, dev)
    res = paste_results(types.SimpleNamespace(scores=scores, labels=labels, masks=None), tp, tk, hw, meta(crop, out), THR)
    want = S.format_results(labels.cpu(), scores.cpu(), res.masks.cpu(), 5)

    def same(got):
        (gb, (gm, gs)), (wb, (wm, ws)) = got, want
        assert len(gb) == len(gm) == len(gs) == 5
        for c in range(5):
            assert gb[c].dtype == wb[c].dtype == np.float64 and gb[c].shape == wb[c].shape and np.array_equal(gb[c], wb[c]), c
            assert len(gm[c]) == len(wm[c]) == len(gs[c]) == len(ws[c])
            for a, b in zip(gm[c], wm[c]):
                assert a.dtype == torch.bool and not a.is_cuda and torch.equal(a, b)
            for a, b in zip(gs[c], ws[c]):
                assert a.dtype == b.dtype and a.dim() == 0 and not a.is_cuda and torch.equal(a, b)
    got = solo_format_results(res, 5)
    same(got)
    assert [len(m) for m in got[1][0]] == [1, 1, 0, 2, 0] and got[0][2].shape == (0, 5) and got[0][4].shape == (0, 5)
    # without the shared buffer (results assembled by a caller) the same values
    masks, stats = seg_paste(tp, tk, hw, meta(crop, out), THR)
    same(solo_format_results(types.SimpleNamespace(scores=scores, labels=labels, masks=masks, mask_stats=stats), 5))
    with pytest.raises(RuntimeError, match='mask_stats'):
        solo_format_results(types.SimpleNamespace(scores=scores, labels=labels, masks=masks), 5)
    empty = solo_format_results(types.SimpleNamespace(scores=scores[:0], labels=labels[:0], masks=masks[:0], mask_stats=stats[:0]), 2)
    assert [b.shape for b in empty[0]] == [(0, 5)] * 2 and empty[1] == ([[], []], [[], []])


def test_format_results_is_one_copy_and_one_sync(dev, monkeypatch):
    import types
    from boxinstseg_amd import solo_format_results
    from boxinstseg_amd.seg_paste import paste_results
    hw, crop, out = SHAPES['up_byte_tail']
    probs = R.disc_probs(np.random.default_rng(1), 4, *hw)
    res = paste_results(types.SimpleNamespace(scores=torch.rand(4, device=dev), labels=torch.tensor([0, 1, 1, 0], device=dev), masks=None),
                        _t(probs, dev), torch.arange(4, device=dev), hw, meta(crop, out), THR)
    torch.cuda.synchronize()
    calls = dict(sync=0, d2h=0)
    real_sync, real_copy = torch.cuda.Stream.synchronize, torch.Tensor.copy_

    def sync(self):
        calls['sync'] += 1
        return real_sync(self)

    def copy_(self, src, *a, **k):
        if not self.is_cuda and src.is_cuda:
            calls['d2h'] += 1
            assert self.is_pinned()
        return real_copy(self, src, *a, **k)
    def refuse(name):
        real = getattr(torch.Tensor, name)

        def fn(self, *a, **k):
            assert not self.is_cuda, f'Tensor.{name} on a device tensor: a second copy or synchronisation'
            return real(self, *a, **k)
        return fn
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', sync)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: pytest.fail('torch.cuda.synchronize'))
    monkeypatch.setattr(torch.Tensor, 'copy_', copy_)
    for name in ('cpu', 'item', 'tolist', 'numpy', 'nonzero'):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    boxes, (masks, _) = solo_format_results(res, 2)
    monkeypatch.undo()
    assert calls == dict(sync=1, d2h=1)
    big = [m for c in masks for m in c]
    assert len(big) == 4 and len({m.untyped_storage().data_ptr() for m in big}) == 1        # views of the one host buffer


def _head_inputs(dev, B=2):
    """Two levels (grids 4 and 3), 3 classes, featmap 11 x 17, C = 8 kernels: inputs of get_seg for both heads."""
    rng = np.random.default_rng(7)
    grids, strides, ncls, C, hw = [4, 3], [8, 16], 3, 8, (11, 17)
    cate = [_t(rng.uniform(0, 1, (B, g, g, ncls)).astype(np.float32) * (rng.random((B, g, g, ncls)) < 0.4), dev) for g in grids]
    seg_levels = [_t(np.stack([R.disc_probs(rng, g * g, *hw) for _ in range(B)]), dev) for g in grids]
    feat = _t(rng.standard_normal((B, C, *hw)).astype(np.float32), dev)
    kernels = [_t(rng.standard_normal((B, C, g, g)).astype(np.float32), dev) for g in grids]
    metas = [meta((41, 66), (50, 80)), meta((44, 60), (33, 45))][:B]
    cfg = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    return grids, strides, ncls, C, hw, cate, seg_levels, feat, kernels, metas, cfg


@pytest.mark.parametrize('head', ['box_solov2', 'discobox'])
def test_solo_get_seg_is_the_loop_of_the_single_image_function(dev, head):
    import boxinstseg_amd as B
    grids, strides, ncls, C, hw, cate, seg_levels, feat, kernels, metas, cfg = _head_inputs(dev)
    if head == 'box_solov2':
        got = B.solo_get_seg(cate, None, seg_levels, metas, cfg, grids, strides, ncls)
    else:
        got = B.solo_get_seg(cate, kernels, feat, metas, cfg, grids, strides, ncls, C)
    assert len(got) == 2
    for i, res in enumerate(got):
        c = torch.cat([x[i].reshape(-1, ncls) for x in cate])
        if head == 'box_solov2':
            want = B.box_solov2_get_seg_single(c, torch.cat([s[i] for s in seg_levels]), hw, metas[i], cfg, grids, strides)
        else:
            k = torch.cat([x[i].permute(1, 2, 0).reshape(-1, C) for x in kernels])
            want = B.discobox_get_seg_single(c, feat[i:i + 1], k, hw, metas[i], cfg, grids, strides)
        assert res.masks.shape[0] > 0 and tuple(res.masks.shape[1:]) == tuple(metas[i]['ori_shape'][:2]) == tuple(res.ori_shape[:2])
        assert res.masks.dtype == torch.bool and res.mask_stats.dtype == torch.int32
        for key in ('scores', 'labels', 'masks', 'mask_stats'):
            assert torch.equal(getattr(res, key), getattr(want, key)), (i, key)
        assert np.array_equal(res.mask_stats.cpu().numpy(), S.stats_of(res.masks.cpu().numpy()))
        fb, (fm, fs) = B.solo_format_results(res, ncls)
        wb, (wm, ws) = S.format_results(res.labels.cpu(), res.scores.cpu(), res.masks.cpu(), ncls)
        assert all(np.array_equal(a, b) for a, b in zip(fb, wb)) and [len(m) for m in fm] == [len(m) for m in wm]


def test_seg_tail_memory_at_the_configs_size(dev):
    """100 kept of 300 candidates, 200 x 304 -> canvas 800 x 1216, img_shape 800 x 1199, ori 427 x 640: the peak device memory _seg_tail
    allocates above its inputs stays below 2 x the output bytes + 8 MB (the output is 27.3 MB; the torch composition allocated a 389 MB fp32
    canvas).  A sample of the masks obeys the tie rule."""
    from boxinstseg_amd import matrix_nms as M
    rng = np.random.default_rng(1)
    n, hw, crop, out = 300, (200, 304), (800, 1199), (427, 640)
    small = R.disc_probs(rng, n, 25, 38)
    probs = torch.from_numpy(small).to(dev).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()      # blocky discs, [300,200,304]
    labels = torch.from_numpy(rng.integers(0, 80, n)).to(dev)
    cate = torch.from_numpy(R.shuffled_scores(rng, n)).to(dev)
    strides = torch.full((n,), 8.0, device=dev)
    cfg = dict(mask_thr=0.5, filter_thr=-1, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    M._seg_tail(probs[:8], labels[:8], cate[:8], strides[:8], hw, meta(crop, out), cfg)                        # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    res = M._seg_tail(probs, labels, cate, strides, hw, meta(crop, out), cfg)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(dev) - base
    out_bytes = 100 * out[0] * out[1]
    assert tuple(res.masks.shape) == (100, *out) and res.masks.dtype == torch.bool
    assert growth < 2 * out_bytes + (8 << 20), growth / 1e6
    got = res.masks.view(torch.uint8)
    assert np.array_equal(res.mask_stats.cpu().numpy(), S.stats_of(got.cpu().numpy()))
    assert torch.equal(res.host_block[:800].view(torch.int64), res.labels)
    # three of the masks against the float64 composition (their source rows found again through the scores' order is not needed: the
    # labels and scores follow keep_inds, so the kernel's own entry point is called on known rows instead)
    keep = np.array([0, 150, 299])
    sub, _ = run(dev, probs.cpu().numpy(), keep, hw, crop, out)
    S.check_tie(sub, probs.cpu().numpy(), keep, (800, 1216), crop, out, THR, 'configs size')


def test_errors(dev):
    from boxinstseg_amd import seg_paste
    p = torch.rand(3, 7, 9, device=dev)
    k = torch.tensor([0, 1], device=dev)
    with pytest.raises(RuntimeError, match='CUDA'):
        seg_paste(p.cpu(), k.cpu(), (7, 9), meta((27, 33), (40, 51)), 0.5)
    with pytest.raises(RuntimeError, match='CUDA'):
        seg_paste(p, k.cpu(), (7, 9), meta((27, 33), (40, 51)), 0.5)
    with pytest.raises(RuntimeError, match='BAD_SHAPE'):
        seg_paste(p, k, (7, 9), meta((29, 33), (40, 51)), 0.5)                 # crop larger than the canvas
    with pytest.raises(RuntimeError, match='BAD_ARGUMENT'):
        seg_paste(p, k, (7, 9), meta((27, 33), (40, 51)), float('nan'))
    with pytest.raises(RuntimeError, match='fp32'):
        seg_paste(p.half(), k, (7, 9), meta((27, 33), (40, 51)), 0.5)
    with pytest.raises(RuntimeError, match='int64'):
        seg_paste(p, k.int(), (7, 9), meta((27, 33), (40, 51)), 0.5)
    with pytest.raises(RuntimeError, match='featmap_size'):
        seg_paste(p, k, (7, 10), meta((27, 33), (40, 51)), 0.5)
