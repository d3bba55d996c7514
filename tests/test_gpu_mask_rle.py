"""GPU: the test-time masks as COCO run-length encodings (csrc/mask_rle.hip, boxinstseg_amd.mask_rle) against the restatement of
tests/rle_ref.py: ``counts``, ``chars`` and both offset arrays BYTE FOR BYTE -- the work is all integer, there is no tolerance.  Every
case runs without and with ``stats`` (the statistics of the masks, as seg_paste leaves them: the kernels then read the boxes only).

The sizes cross h in {1, 63, 64, 65, 129} with w in {1, 63, 64, 65, 130}: one word row and three, a column tile and three, each one short
of, at and one past the 64 that both are cut by.  The patterns are the places where a run can go wrong: nothing set, everything set, the
first and the last pixel, a run across a column border, a transition exactly at row 64, the checkerboard (the most runs there can be),
stripes of period 1, 2 and 64 both ways, blobs with holes, and counts at the 1 / 2 / 3 / 4 character thresholds with negative deltas."""
import types

import numpy as np
import pytest
import torch

from tests import rle_ref as R

pytestmark = pytest.mark.gpu

HS, WS = (1, 63, 64, 65, 129), (1, 63, 64, 65, 130)
PAT = 0xA5                                                                   # what the output buffers hold before a call


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _blobs(rng, n, h, w, holes=True):
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, max(2, min(h, w) / 2))
            d = (yy - cy) ** 2 + (xx - cx) ** 2
            out[i] |= (d <= r * r).astype(np.uint8)
            if holes and rng.random() < 0.5:
                out[i] &= ~(d <= (r / 3) ** 2)
    return out


def _raw(dev, masks, stats=None, cap_runs=None, cap_chars=None):
    """One bxi_mask_rle_u8 call on pattern-filled outputs with exactly the capacities given (default: the need) -> numpy (status,
    run_offsets, counts buffer, char_offsets, chars buffer); the buffers come back whole, sentinel bytes included."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    n, h, w = masks.shape
    want = R.packed(masks)
    cap_runs = len(want[1]) if cap_runs is None else cap_runs
    cap_chars = len(want[3]) if cap_chars is None else cap_chars
    m = _t(masks, dev)
    st = None if stats is None else _t(stats, dev)
    ro = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    co = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    status = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    counts = torch.full((4 * (cap_runs + 8),), PAT, dtype=torch.uint8, device=dev)
    chars = torch.full((cap_chars + 32,), PAT, dtype=torch.uint8, device=dev)
    nbytes = lib.bxi_mask_rle_workspace_bytes(n, h, w)
    ws = torch.full((max(nbytes, 16),), PAT, dtype=torch.uint8, device=dev)
    rc = lib.bxi_mask_rle_u8(m.data_ptr() if n else None, n, h, w, None if st is None else st.data_ptr(), cap_runs, cap_chars, ro.data_ptr(),
                             counts.data_ptr(), co.data_ptr(), chars.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
                             torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _lib.STATUS.get(rc, rc)
    torch.cuda.synchronize()
    return (int(status.cpu()[0]), ro.cpu().numpy(), counts.cpu().numpy().view(np.uint32), co.cpu().numpy(), chars.cpu().numpy())


def _exact(dev, masks, label=''):
    """Both legs (without / with stats) of one block of masks against the restatement, byte for byte; nothing behind the totals changes."""
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    w_ro, w_counts, w_co, w_chars = R.packed(masks)
    for stats in (None, R.stats_of(masks)):
        leg = (label, 'stats' if stats is not None else 'plain')
        status, ro, counts, co, chars = _raw(dev, masks, stats)
        assert status == 0, leg
        assert np.array_equal(ro, w_ro) and np.array_equal(co, w_co), (leg, ro.tolist()[:6], w_ro.tolist()[:6], co.tolist()[:6], w_co.tolist()[:6])
        bad = np.flatnonzero(counts[:len(w_counts)] != w_counts)
        assert bad.size == 0, (leg, 'counts', bad[:4].tolist(), counts[bad[:4]].tolist(), w_counts[bad[:4]].tolist())
        bad = np.flatnonzero(chars[:len(w_chars)] != w_chars)
        assert bad.size == 0, (leg, 'chars', bad[:4].tolist(), chars[bad[:4]].tolist(), w_chars[bad[:4]].tolist())
        assert (counts[len(w_counts):] == 0xA5A5A5A5).all() and (chars[len(w_chars):] == PAT).all(), leg


def _size_patterns(h, w, rng):
    z = np.zeros((h, w), np.uint8)
    out = [z.copy(), np.ones((h, w), np.uint8)]
    a = z.copy(); a[0, 0] = 1; out.append(a)                                                   # counts[0] == 0
    a = z.copy(); a[h - 1, w - 1] = 1; out.append(a)                                           # only the last pixel
    a = z.copy(); a[h - 1, 0] = 1; a[0, w - 1] = 1; a[h - 1, (w - 1) // 2] = 1; a[0, (w - 1) // 2 + (w > 1)] = 1; out.append(a)   # a run across a column border
    a = z.copy(); a[min(64, h - 1):, w // 2] = 1; a[:min(64, h), w - 1] = 1; out.append(a)    # transitions exactly at row 64
    a = z.copy(); a[h - 1, :] = 1; a[0, :] = 1; out.append(a)                                  # every column border carries a run
    a = z.copy(); a[h - 1, :max(1, w - 1)] = 1; out.append(a)                                 # the last row alone: its runs end in row 0, above the box
    out += list(_blobs(rng, 2, h, w))
    out.append((rng.random((h, w)) < 0.5).astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize('w', WS)
@pytest.mark.parametrize('h', HS)
def test_every_size_exact(dev, h, w):
    _exact(dev, _size_patterns(h, w, np.random.default_rng(100 * h + w)), f'{h}x{w}')


def test_checkerboard_and_stripes(dev):
    yy, xx = np.mgrid[:65, :65]
    _exact(dev, np.stack([(yy + xx) % 2, (yy + xx + 1) % 2]).astype(np.uint8), 'checkerboard')          # 65 * 65 (+ 1) runs: the maximum
    yy, xx = np.mgrid[:129, :130]
    stripes = []
    for period in (1, 2, 64):
        stripes += [(xx // period) % 2, (xx // period + 1) % 2, (yy // period) % 2, (yy // period + 1) % 2]
    _exact(dev, np.stack(stripes).astype(np.uint8), 'stripes')


def test_blobs_with_holes_and_nonzero_bytes(dev):
    rng = np.random.default_rng(9)
    m = _blobs(rng, 6, 97, 150)
    _exact(dev, m, 'blobs')
    _exact(dev, m * np.array([1, 2, 255, 128, 7, 1], np.uint8)[:, None, None], 'any non-zero byte is a set pixel')


def test_counts_at_the_character_thresholds_and_negative_deltas(dev):
    h, w = 129, 300
    lists = [[15, 16, 511, 512, 16383, 16384], [0, 16384, 16383, 512, 511, 16, 15], [5, 5, 5, 4, 5, 3, 1, 1, 600, 1, 1, 599, 20000, 17, 3],
             [16384, 15, 16383, 16, 512, 1, 511]]
    masks = []
    for cnts in lists:
        rest = h * w - sum(cnts)
        assert rest > 0
        cnts = cnts + [rest]
        masks.append(R.rle_decode_counts(cnts, h, w).astype(np.uint8))
        assert R.rle_counts_fast(masks[-1]) == cnts
        deltas = [cnts[i] - cnts[i - 2] for i in range(3, len(cnts))]
        assert min(deltas) < 0
    assert {len(R.rle_to_string([v])) for v in (15, 16, 511, 512, 16383, 16384)} == {1, 2, 3, 4}
    _exact(dev, np.stack(masks), 'thresholds')


def test_wide_and_tall_masks_take_the_other_paths(dev):
    """A workgroup walks 1024 columns per round and a column 4 words per group: 2500 columns are three rounds, 330 rows are six words.
    Lone pixels at growing distances make the search for the column of a rank leave the neighbouring column (1, 2, 4, ... columns back,
    then the bisection), across the rounds' borders too."""
    rng = np.random.default_rng(12)
    wide = np.zeros((6, 5, 2500), np.uint8)
    wide[0, 2, [0, 1, 3, 7, 15, 40, 100, 700, 1023, 1024, 1025, 2047, 2048, 2499]] = 1
    wide[1, 4, [5, 1500]] = 1                                                 # runs that end in row 0 of the next column, far apart
    wide[2, :, 1020:1030] = 1
    wide[3] = rng.random((5, 2500)) < 0.02
    wide[4, 0, 2499] = 1
    wide[5] = rng.random((5, 2500)) < 0.5
    _exact(dev, wide, 'wide')
    tall = np.concatenate([_blobs(rng, 5, 330, 70), (rng.random((1, 330, 70)) < 0.01).astype(np.uint8)])
    tall[4] = 0
    tall[4, [0, 63, 64, 255, 256, 257, 329], 35] = 1                          # lone pixels in every word of one column
    _exact(dev, tall, 'tall')


def test_n0_n1_and_70_mixed(dev):
    _exact(dev, np.zeros((0, 40, 56), np.uint8), 'n=0')
    rng = np.random.default_rng(3)
    _exact(dev, _blobs(rng, 1, 40, 56), 'n=1')
    m = _blobs(rng, 70, 40, 56)
    m[5] = 0
    m[17] = 0
    m[33] = 0
    m[33, 21, 40] = 1                                                          # a statistics box of one pixel
    m[69] = 0                                                                  # the last mask is empty
    m[44] = 1
    assert R.stats_of(m)[33].tolist() == [1, 40, 21, 40, 21]
    _exact(dev, m, 'n=70')


def test_two_runs_give_the_same_bits(dev):
    m = _blobs(np.random.default_rng(4), 20, 65, 130)
    a, b = _raw(dev, m, R.stats_of(m)), _raw(dev, m, R.stats_of(m))
    assert a[0] == b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize('short', ['runs', 'chars', 'both'])
def test_over_capacity_is_loud_and_stays_inside(dev, short):
    from boxinstseg_amd import _lib
    m = _blobs(np.random.default_rng(6), 9, 65, 66)
    w_ro, w_counts, w_co, w_chars = R.packed(m)
    cap_runs = len(w_counts) - (short in ('runs', 'both'))
    cap_chars = len(w_chars) - (short in ('chars', 'both'))
    for stats in (None, R.stats_of(m)):
        status, ro, counts, co, chars = _raw(dev, m, stats, cap_runs, cap_chars)
        assert status == {'runs': _lib.RLE_STATUS_OVER_RUNS, 'chars': _lib.RLE_STATUS_OVER_CHARS,
                          'both': _lib.RLE_STATUS_OVER_RUNS | _lib.RLE_STATUS_OVER_CHARS}[short]
        assert np.array_equal(ro, w_ro) and np.array_equal(co, w_co)           # complete, with the true totals
        assert np.array_equal(counts[:cap_runs], w_counts[:cap_runs]) and np.array_equal(chars[:cap_chars], w_chars[:cap_chars])
        assert (counts[cap_runs:] == 0xA5A5A5A5).all() and (chars[cap_chars:] == PAT).all()        # the sentinels past the capacity
    status, ro, counts, co, chars = _raw(dev, m, None, 0, 0)
    assert status == 3 and np.array_equal(ro, w_ro) and np.array_equal(co, w_co) and (counts == 0xA5A5A5A5).all() and (chars == PAT).all()


def test_the_wrapper_retries_once_with_the_exact_totals(dev):
    from boxinstseg_amd import rle_decode, rle_encode
    m = _blobs(np.random.default_rng(7), 5, 40, 56)
    want = [R.encode(x, fast=True) for x in m]
    enc = rle_encode(_t(m, dev), cap_runs=3, cap_chars=3)
    assert enc.to_coco() == want and enc.retried
    assert (enc.cap_runs, enc.cap_chars) == (sum(len(R.rle_counts_fast(x)) for x in m), sum(len(r['counts']) for r in want))
    enc = rle_encode(_t(m, dev).bool(), _t(R.stats_of(m), dev))
    assert enc.to_coco() == want and not enc.retried and (enc.cap_runs, enc.cap_chars) == (5 * 114, 10 * 114)
    assert np.array_equal(rle_decode(enc.to_coco()), m != 0)
    torch.cuda.synchronize()
    assert np.array_equal(enc.counts.cpu().numpy().view(np.uint32)[:int(enc.run_offsets[-1])], R.packed(m)[1])
    assert rle_encode(_t(m[:0], dev)).to_coco() == []


def test_unaligned_views_of_one_buffer(dev):
    """CondInst's paste_masks_device hands out per-image views of one buffer: a view at an odd byte offset encodes like a copy of it."""
    from boxinstseg_amd import rle_encode
    m = _blobs(np.random.default_rng(8), 3, 33, 47)
    buf = torch.zeros(5 + m.size + 3, dtype=torch.uint8, device=dev)
    view = buf[5:5 + m.size].view(3, 33, 47)
    view.copy_(_t(m, dev))
    assert view.data_ptr() % 4 == 1 or view.data_ptr() % 2 == 1
    assert rle_encode(view).to_coco() == [R.encode(x) for x in m]


def test_too_many_pixels_are_refused_before_a_launch(dev):
    """By argument only: nothing of that size is allocated, and no pointer is looked at."""
    from boxinstseg_amd import _lib, mask_rle
    lib = _lib.load()
    for h, w in ((1 << 15, 1 << 14), (1 << 29, 1), (23171, 23171)):
        assert h * w >= 1 << 29
        assert lib.bxi_mask_rle_u8(None, 1, h, w, None, 0, 0, None, None, None, None, None, None, 0, None) == _lib.BXI_ERR_UNSUPPORTED
        assert lib.bxi_mask_rle_workspace_bytes(1, h, w) == 0
        with pytest.raises(NotImplementedError):
            mask_rle.check_shape(1, h, w)
    assert lib.bxi_last_hip_error() == 0


def test_capturable_in_a_graph(dev):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(10)
    first, second = _blobs(rng, 4, 65, 66), _blobs(rng, 4, 65, 66)
    w_ro, w_counts, w_co, w_chars = R.packed(second)
    cap_runs, cap_chars = 4 * 65 * 66 + 4, 2 * (4 * 65 * 66 + 4)
    m = _t(first, dev)
    ro, co = torch.zeros(5, dtype=torch.int32, device=dev), torch.zeros(5, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    counts, chars = torch.zeros(cap_runs, dtype=torch.int32, device=dev), torch.zeros(cap_chars, dtype=torch.uint8, device=dev)
    nbytes = lib.bxi_mask_rle_workspace_bytes(4, 65, 66)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(stream):
        rc = lib.bxi_mask_rle_u8(m.data_ptr(), 4, 65, 66, None, cap_runs, cap_chars, ro.data_ptr(), counts.data_ptr(), co.data_ptr(),
                                 chars.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == 0, _lib.STATUS.get(rc, rc)
    stream = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call(stream.cuda_stream)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            call(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    m.copy_(_t(second, dev))
    graph.replay()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0 and np.array_equal(ro.cpu().numpy(), w_ro) and np.array_equal(co.cpu().numpy(), w_co)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32)[:len(w_counts)], w_counts)
    assert np.array_equal(chars.cpu().numpy()[:len(w_chars)], w_chars)


# ---- the results of the test pipelines ---------------------------------------------------------------------------------------------------

def _count_copies(monkeypatch):
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
    return calls


def test_solo_encode_results_are_the_format_results_encoded(dev, monkeypatch):
    """On a results object of seg_paste's: after rle_decode the masks of solo_format_results, with its classes, order, boxes and scores."""
    from boxinstseg_amd import rle_decode, seg_paste, solo_encode_results, solo_format_results
    from boxinstseg_amd.seg_paste import paste_results
    from tests import matrix_nms_ref as M
    hw, crop, out = (10, 14), (38, 53), (40, 56)
    probs = M.disc_probs(np.random.default_rng(4), 9, *hw)
    probs[4] = 0.2                                                            # kept, but empty after the threshold
    keep = np.array([2, 4, 0, 5, 1, 8, 7, 3])
    labels = torch.tensor([3, 0, 3, 1, 0, 1, 3, 0], device=dev)
    scores = torch.linspace(0.9, 0.2, 8, device=dev)
    meta = dict(img_shape=(*crop, 3), ori_shape=(*out, 3))
    tp, tk = _t(probs, dev), _t(keep, dev)
    res = paste_results(types.SimpleNamespace(scores=scores, labels=labels, masks=None), tp, tk, hw, meta, 0.5)
    wb, (wm, ws) = solo_format_results(res, 5)
    assert sum(len(x) for x in wm) == 7 and tuple(res.masks.shape) == (8, 40, 56)

    def same(got):
        gb, (gm, gs) = got
        assert len(gb) == len(gm) == len(gs) == 5
        for c in range(5):
            assert gb[c].dtype == np.float64 and gb[c].shape == wb[c].shape and np.array_equal(gb[c], wb[c]), c
            assert len(gm[c]) == len(wm[c]) == len(gs[c])
            assert all(set(r) == {'size', 'counts'} and r['size'] == [40, 56] and isinstance(r['counts'], bytes) for r in gm[c])
            if gm[c]:
                assert np.array_equal(rle_decode(gm[c]), torch.stack(wm[c]).numpy()), c
                assert [r for r in gm[c]] == [R.encode(x.numpy()) for x in wm[c]]
            for a, b in zip(gs[c], ws[c]):
                assert a.dtype == b.dtype and a.dim() == 0 and not a.is_cuda and torch.equal(a, b)
    torch.cuda.synchronize()
    calls = _count_copies(monkeypatch)
    got = solo_encode_results(res, 5)
    monkeypatch.undo()
    assert calls == dict(sync=1, d2h=1)
    same(got)
    # results assembled by a caller (no shared buffer): the same values; no statistics: an error, as in solo_format_results
    masks, stats = seg_paste(tp, tk, hw, meta, 0.5)
    same(solo_encode_results(types.SimpleNamespace(scores=scores, labels=labels, masks=masks, mask_stats=stats), 5))
    with pytest.raises(RuntimeError, match='mask_stats'):
        solo_encode_results(types.SimpleNamespace(scores=scores, labels=labels, masks=masks), 5)
    empty = solo_encode_results(types.SimpleNamespace(scores=scores[:0], labels=labels[:0], masks=masks[:0], mask_stats=stats[:0]), 2)
    assert [b.shape for b in empty[0]] == [(0, 5)] * 2 and empty[1] == ([[], []], [[], []])


def test_box2mask_encode_results_are_the_format_results_encoded(dev, monkeypatch):
    """On a results object of box2mask_instances': all `count` detections in the order of box2mask_format_results, empty masks included."""
    import boxinstseg_amd as B
    from tests import inst_post_ref as I
    c = I.CASES['zero_plane']
    cls, pred = I.case_inputs('zero_plane')
    meta = dict(batch_input_shape=tuple(c['up']), img_shape=(*c['crop'], 3), ori_shape=(40, 56, 3))
    r = B.box2mask_instances(_t(cls[None], dev), _t(pred[None], dev), [meta], dict(max_per_image=8), c['things'], c['stuff'], rescale=True)[0]
    wb, wm = B.box2mask_format_results(r, c['things'])
    assert tuple(r.masks.shape) == (8, 40, 56) and sum(len(x) for x in wm) == int(r.count) == 8
    assert any(not m.any() for per in wm for m in per)                        # an empty mask is among them
    torch.cuda.synchronize()
    calls = _count_copies(monkeypatch)
    gb, gm = B.box2mask_encode_results(r, c['things'])
    monkeypatch.undo()
    assert calls == dict(sync=1, d2h=1)
    assert len(gb) == len(gm) == c['things']
    for k in range(c['things']):
        assert gb[k].dtype == np.float32 and gb[k].shape == wb[k].shape and np.array_equal(gb[k], wb[k]), k
        assert len(gm[k]) == len(wm[k])
        if gm[k]:
            assert np.array_equal(B.rle_decode(gm[k]), np.stack(wm[k])), k
            assert gm[k] == [R.encode(x) for x in wm[k]]
    with pytest.raises(RuntimeError, match='host_block'):
        B.box2mask_encode_results(types.SimpleNamespace(masks=r.masks, mask_stats=r.mask_stats), 3)
