"""GPU: the entry points of include/boxinst/boxinst_hip_det.h on misaligned views inside poisoned bands (tests/guarded.py).

Inputs are views at the element's natural alignment only (fp32 at 4, 8 and 12 bytes past a 16-byte boundary, int64 at 8) surrounded by
NaN / -1; outputs are pre-filled with the 'nobody wrote this' pattern and the workspaces are exactly as large as the size queries
say.  Afterwards the bands are intact, every output element the entry point promises is written, the inputs are unchanged, and the
results are bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import box_nms_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.DET_SIGNATURES)
GUARDED = {
    'bxi_det_location_score_f32': 'test_location_score_guarded',
    'bxi_det_candidates_f32': 'test_candidates_guarded',
    'bxi_box_nms_f32': 'test_box_nms_guarded',
    'bxi_det_gather_f32': 'test_gather_guarded',
}
BAND = 4096          # more than the largest plane of the case (12 x 20) times the channels one over-run could cross


def _case(dev):
    g = np.load(R.__file__.replace('box_nms_ref.py', 'golden/det_nms.npz'))
    return {k: [torch.from_numpy(g[f'in_{k}{lv}']).to(dev) for lv in range(len(R.DET_SIZES))] for k in ('cls', 'bbox', 'ctr', 'params')}


def _guarded_levels(inp, lead):
    """Every map of every level as a misaligned view; returns (the ctypes array, the Guarded objects)."""
    from boxinstseg_amd import _lib
    gs, arr = [], (_lib.DetLevel * len(R.DET_SIZES))()
    for lv, ((h, w), s) in enumerate(zip(R.DET_SIZES, R.DET_STRIDES)):
        four = [G.embed(inp[k][lv], (lead + j) % 4, BAND) for j, k in enumerate(('cls', 'bbox', 'ctr', 'params'))]
        gs += four
        arr[lv] = _lib.DetLevel(four[0].ptr(), four[1].ptr(), four[2].ptr(), four[3].ptr(), h, w, s)
    return arr, gs


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_location_score_guarded(dev, lead):
    """bxi_det_location_score_f32: a NaN of the band that was read would win a maximum and reach the output."""
    from boxinstseg_amd import _lib, box_nms
    inp = _case(dev)
    plain = box_nms.location_scores(box_nms._Levels(inp['cls'], inp['bbox'], inp['ctr'], inp['params'], R.DET_STRIDES))
    arr, gs = _guarded_levels(inp, lead)
    out = G.out(tuple(plain.shape), torch.float32, dev, lead)
    rc = _lib.load().bxi_det_location_score_f32(arr, len(R.DET_SIZES), R.DET_B, R.DET_C, out.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(out, *gs)
    G.check_written(out)
    G.check_unchanged(*gs)
    assert G.same(out.t, plain) and bool(torch.isfinite(out.t).all())


@pytest.mark.parametrize('lead', [1, 3])
@pytest.mark.parametrize('with_sel', [True, False])
def test_candidates_guarded(dev, lead, with_sel):
    """bxi_det_candidates_f32: the workspace exactly as large as the query says, every tile count written; the candidate rows up to
    count written, the rows behind them untouched."""
    from boxinstseg_amd import _lib, box_nms
    inp = _case(dev)
    lv = box_nms._Levels(inp['cls'], inp['bbox'], inp['ctr'], inp['params'], R.DET_STRIDES)
    sel = None
    if with_sel:
        sel = torch.from_numpy(R.select({k: [t.cpu().numpy() for t in v] for k, v in inp.items()}, 40)).to(dev)
    dims = R.det_img_dims()
    cap = 48
    plain = box_nms.det_candidates(lv, sel, dims, True, 0.05, cap)
    counts = plain[4].cpu().tolist()
    assert counts[R.DET_EMPTY_IMAGE] == 0 and 0 < max(counts) <= cap
    arr, gs = _guarded_levels(inp, lead)
    M = lv.M_all if sel is None else sel.shape[1]
    gsel = G.embed(sel, 1, BAND) if with_sel else None
    nbytes = _lib.load().bxi_det_candidates_workspace_bytes(R.DET_B, M)
    assert nbytes == 4 * R.DET_B * ((M + 63) // 64)
    gb, gsc = G.out((R.DET_B, cap, 4), torch.float32, dev, lead), G.out((R.DET_B, cap), torch.float32, dev, 4 - lead)
    gl, gp = G.out((R.DET_B, cap), torch.int64, dev, 1), G.out((R.DET_B, cap), torch.int32, dev, lead)
    gc, gw = G.out(R.DET_B, torch.int32, dev, 3), G.out(nbytes // 4, torch.int32, dev, lead)
    rc = _lib.load().bxi_det_candidates_f32(arr, len(R.DET_SIZES), R.DET_B, R.DET_C, gsel.ptr() if with_sel else None, M,
                                            _lib.float_array([v for row in dims for v in row]), 1, 0.05, cap, gb.ptr(), gsc.ptr(), gl.ptr(),
                                            gp.ptr(), gc.ptr(), gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gb, gsc, gl, gp, gc, gw, *gs, *([gsel] if with_sel else []))
    G.check_written(gc, gw)
    G.check_unchanged(*gs, *([gsel] if with_sel else []))
    assert gc.t.cpu().tolist() == counts
    pattern32 = G.pattern_bits(torch.int32)
    for b, n in enumerate(counts):
        assert G.same(gb.t[b, :n], plain[0][b, :n]) and G.same(gsc.t[b, :n], plain[1][b, :n])
        assert torch.equal(gl.t[b, :n], plain[2][b, :n]) and torch.equal(gp.t[b, :n], plain[3][b, :n])
        assert bool(torch.isfinite(gb.t[b, :n]).all()) and bool(torch.isfinite(gsc.t[b, :n]).all())
        assert bool((gp.t[b, n:] == pattern32).all()) and bool((gsc.t[b, n:].view(torch.int32) == G.PATTERN_F32).all())   # rows behind count: untouched


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('own_sort', [True, False])
def test_box_nms_guarded(dev, lead, own_sort):
    """bxi_box_nms_f32: boxes, scores, labels, counts (and the caller's order) at misaligned addresses inside NaN / -1; keep, n_keep and
    status written in full; a kept list that spills past the LDS tile into a workspace of exactly the queried size."""
    from boxinstseg_amd import _lib, box_nms
    P, cap = 3, box_nms.KEEP_TILE + 70
    boxes = np.zeros((P, cap, 4), np.float32)
    scores = np.zeros((P, cap), np.float32)
    labels = np.zeros((P, cap), np.int64)
    counts = [cap, 0, 300]
    b0, s0, l0 = R.clustered_boxes_with_margin(5, 300, 3, 0.5)
    boxes[2, :300], scores[2, :300], labels[2, :300] = b0, s0, l0
    i = np.arange(cap)                                            # disjoint boxes: everything is kept, the kept list outgrows the tile
    boxes[0] = np.stack([(i % 64) * 10, (i // 64) * 10, (i % 64) * 10 + 8, (i // 64) * 10 + 8], 1)
    scores[0] = np.random.default_rng(lead).permutation(np.linspace(0.1, 0.9, cap)).astype(np.float32)
    tb, ts, tl = (torch.from_numpy(a).to(dev) for a in (boxes, scores, labels))
    tc = torch.tensor(counts, dtype=torch.int32, device=dev)
    order = None if own_sort else box_nms._stable_order(ts)
    plain = box_nms.box_nms(tb, ts, tl, tc, 0.5, 0, -1, order)
    assert plain[1].cpu().tolist()[:2] == [cap, 0] and plain[2].cpu().tolist() == [0, 0, 0]
    want2 = R.greedy_nms(b0, s0, l0, 0.5)
    assert plain[0][2, :len(want2)].cpu().tolist() == want2 and int(plain[1][2]) == len(want2)
    gb, gs, gl, gc = G.embed(tb, lead, BAND), G.embed(ts, 4 - lead, BAND), G.embed(tl, 1, BAND), G.embed(tc, lead, BAND)
    go = None if own_sort else G.embed(order, lead, BAND)
    nbytes = _lib.load().bxi_box_nms_workspace_bytes(P, cap, cap)
    assert nbytes == 4 * (P * cap + P * 70 * 6)
    gk, gn, gst = G.out((P, cap), torch.int32, dev, lead), G.out(P, torch.int32, dev, 1), G.out(P, torch.int32, dev, 3)
    gw = G.out(nbytes // 4, torch.int32, dev, lead, BAND)
    rc = _lib.load().bxi_box_nms_f32(gb.ptr(), gs.ptr(), gl.ptr(), gc.ptr(), None if own_sort else go.ptr(), P, cap, 0.5, 0, -1, gk.ptr(),
                                     gn.ptr(), gst.ptr(), gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    ins = [gb, gs, gl, gc] + ([] if own_sort else [go])
    G.check_bands(gk, gn, gst, gw, *ins)
    G.check_written(gk, gn, gst)
    G.check_unchanged(*ins)
    for got, want in zip((gk.t, gn.t, gst.t), plain):
        assert torch.equal(got, want)


@pytest.mark.parametrize('own_sort', [True, False])
def test_box_nms_guarded_max_num_above_cap(dev, own_sort):
    """max_num > cap: max_keep is max_num, so `keep` has rows of max_num words although a segment holds at most cap boxes.  Every row is
    written at that stride (-1 behind n_keep), and the workspace query takes the same value."""
    from boxinstseg_amd import _lib, box_nms
    P, cap, max_num, lead = 3, 48, 100, 3
    counts = [cap, 0, 30]
    boxes, scores, labels = np.zeros((P, cap, 4), np.float32), np.zeros((P, cap), np.float32), np.zeros((P, cap), np.int64)
    want = []
    for p, n in enumerate(counts):
        if n:
            boxes[p, :n], scores[p, :n], labels[p, :n] = R.clustered_boxes_with_margin(11 + p, n, 2, 0.5)
        want.append(R.greedy_nms(boxes[p, :n], scores[p, :n], labels[p, :n], 0.5))
    assert 0 < len(want[0]) < cap and 0 < len(want[2]) < 30
    tb, ts, tl = (torch.from_numpy(a).to(dev) for a in (boxes, scores, labels))
    tc = torch.tensor(counts, dtype=torch.int32, device=dev)
    order = None if own_sort else box_nms._stable_order(ts)
    gb, gs, gl, gc = G.embed(tb, lead, BAND), G.embed(ts, 4 - lead, BAND), G.embed(tl, 1, BAND), G.embed(tc, lead, BAND)
    go = None if own_sort else G.embed(order, lead, BAND)
    nbytes = _lib.load().bxi_box_nms_workspace_bytes(P, cap, max_num)
    assert nbytes == 4 * P * cap
    gk, gn, gst = G.out((P, max_num), torch.int32, dev, lead), G.out(P, torch.int32, dev, 1), G.out(P, torch.int32, dev, 3)
    gw = G.out(nbytes // 4, torch.int32, dev, lead, BAND)
    rc = _lib.load().bxi_box_nms_f32(gb.ptr(), gs.ptr(), gl.ptr(), gc.ptr(), None if own_sort else go.ptr(), P, cap, 0.5, 0, max_num, gk.ptr(),
                                     gn.ptr(), gst.ptr(), gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    ins = [gb, gs, gl, gc] + ([] if own_sort else [go])
    G.check_bands(gk, gn, gst, gw, *ins)
    G.check_written(gk, gn, gst)
    G.check_unchanged(*ins)
    assert gn.t.cpu().tolist() == [len(w) for w in want] and gst.t.cpu().tolist() == [0, 0, 0]
    for p, w in enumerate(want):
        assert gk.t[p].cpu().tolist() == w + [-1] * (max_num - len(w)), p
    # the wrapper follows the same rule, and the gather takes the same stride
    keep, n_keep, _ = box_nms.box_nms(tb, ts, tl, tc, 0.5, 0, max_num, order)
    assert tuple(keep.shape) == (P, max_num) and torch.equal(keep, gk.t) and torch.equal(n_keep, gn.t)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_gather_guarded(dev, lead):
    """bxi_det_gather_f32: every row of every output written (zeros from n_keep on), nothing outside."""
    from boxinstseg_amd import _lib, box_nms
    inp = _case(dev)
    lv = box_nms._Levels(inp['cls'], inp['bbox'], inp['ctr'], inp['params'], R.DET_STRIDES)
    sel = torch.from_numpy(R.select({k: [t.cpu().numpy() for t in v] for k, v in inp.items()}, 40)).to(dev)
    cap, max_keep = 48, 20
    cand = box_nms.det_candidates(lv, sel, R.det_img_dims(), False, 0.05, cap, fill_scores=0.0)
    cand = (cand[0].nan_to_num(0.0), cand[1], cand[2].clamp(0, R.DET_C - 1), cand[3].clamp(0, sel.shape[1] - 1), cand[4])
    keep, n_keep, status = box_nms.box_nms(cand[0], cand[1], cand[2], cand[4], 0.5, 0, max_keep)
    assert status.cpu().tolist() == [0, 0, 0]
    plain = box_nms.det_gather(lv, sel, cand, keep, n_keep)
    arr, gs = _guarded_levels(inp, lead)
    gsel, gk, gn = G.embed(sel, 1, BAND), G.embed(keep, lead, BAND), G.embed(n_keep, lead, BAND)
    gc = [G.embed(cand[0], lead, BAND), G.embed(cand[1], 4 - lead, BAND), G.embed(cand[2], 1, BAND), G.embed(cand[3], lead, BAND)]
    outs = [G.out((R.DET_B, max_keep, 5), torch.float32, dev, lead), G.out((R.DET_B, max_keep), torch.int64, dev, 1),
            G.out((R.DET_B, max_keep, R.DET_P), torch.float32, dev, 4 - lead), G.out((R.DET_B, max_keep, 2), torch.float32, dev, lead),
            G.out((R.DET_B, max_keep), torch.int64, dev, 1)]
    rc = _lib.load().bxi_det_gather_f32(arr, len(R.DET_SIZES), R.DET_B, R.DET_C, R.DET_P, gsel.ptr(), sel.shape[1], gc[0].ptr(), gc[1].ptr(),
                                        gc[2].ptr(), gc[3].ptr(), cap, gk.ptr(), gn.ptr(), max_keep, outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                        outs[3].ptr(), outs[4].ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(*outs, *gs, gsel, gk, gn, *gc)
    G.check_written(*outs)
    G.check_unchanged(*gs, gsel, gk, gn, *gc)
    for got, want in zip(outs, plain):
        assert torch.equal(got.t.view(torch.int32) if got.t.dtype == torch.float32 else got.t, want.view(torch.int32) if want.dtype == torch.float32 else want)
        assert not got.t.dtype.is_floating_point or bool(torch.isfinite(got.t).all())
    for b, n in enumerate(n_keep.cpu().tolist()):
        assert 0 <= n <= max_keep and all(bool((o.t[b, n:] == 0).all()) for o in outs)
