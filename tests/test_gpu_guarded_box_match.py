"""GPU: the entry points of include/boxinst/boxinst_hip_assign.h on misaligned views inside poisoned bands (tests/guarded.py).

Inputs are views at the element's natural alignment only (fp32 at 4, 8 and 12 bytes past a 16-byte boundary, mask bytes at odd
addresses, int64 at 8) surrounded by NaN / 0xFF / -1; outputs and the workspace are pre-filled with the 'nobody wrote this' pattern and
the workspace is exactly as large as bxi_box_match_workspace_bytes says.  Afterwards the bands are intact, every output element and every
workspace element is written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.ASSIGN_SIGNATURES)
GUARDED = {
    'bxi_match_project_pred_f32': 'test_project_pred_guarded',
    'bxi_match_project_gt_u8': 'test_project_gt_u8_guarded',
    'bxi_match_project_gt_f32': 'test_project_gt_f32_guarded',
    'bxi_match_cost_f32': 'test_match_cost_guarded',
    'bxi_linear_sum_assignment_f32': 'test_linear_sum_assignment_guarded',
}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _proj_outs(n, H, W, dev, lead):
    from boxinstseg_amd import _lib
    nbytes = _lib.load().bxi_box_match_workspace_bytes(n, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    return (G.out((n, H), torch.float32, dev, lead), G.out((n, W), torch.float32, dev, 4 - lead), G.out((n, 2), torch.float32, dev, 1),
            G.out(nbytes // 4, torch.float32, dev, lead), nbytes)


# one tile; down-sampling; two column tiles and two row bands; the path without resampling
@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('shape', [(7, 9, 20, 30), (12, 10, 6, 5), (9, 300, 130, 1100), (20, 30, 20, 30)])
def test_project_pred_guarded(dev, shape, lead):
    """bxi_match_project_pred_f32: a NaN of the band that was read would reach a maximum, and through it the comparison below."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.box_match import project_pred
    h, w, H, W = shape
    n = 3
    logits = _t(np.random.default_rng(lead).normal(0, 2, (n, h, w)).astype(np.float32), dev)
    for act in (1, 0):
        plain = project_pred(logits, (H, W), bool(act))
        gl = G.embed(logits, lead, G.plane_band(h, w))
        gr, gc, gs, gw, nbytes = _proj_outs(n, H, W, dev, lead)
        rc = _lib.load().bxi_match_project_pred_f32(gl.ptr(), n, h, w, H, W, act, gr.ptr(), gc.ptr(), gs.ptr(), gw.ptr(), nbytes, G.stream(dev))
        assert rc == 0, _lib.STATUS.get(rc, rc)
        G.check_bands(gl, gr, gc, gs, gw)
        G.check_written(gr, gc, gs, gw)
        G.check_unchanged(gl)
        assert G.same(gr.t, plain[0]) and G.same(gc.t, plain[1]) and G.same(gs.t, plain[2])
        assert bool(torch.isfinite(gr.t).all()) and bool(torch.isfinite(gc.t).all()) and bool(torch.isfinite(gs.t).all())


@pytest.mark.parametrize('lead', [1, 6, 15])
@pytest.mark.parametrize('HW', [(20, 30), (130, 1100), (5, 4)])
def test_project_gt_u8_guarded(dev, HW, lead):
    """bxi_match_project_gt_u8: mask bytes at odd addresses; the band around them is 0xFF, larger than any mask byte here, so a read
    outside shows in a maximum."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.box_match import project_gt
    H, W = HW
    g = 3
    masks = _t((np.random.default_rng(lead).uniform(size=(g, H, W)) < 0.02).astype(np.uint8) * 3, dev)
    plain = project_gt(masks)
    gm = G.embed(masks, lead, G.plane_band(H, W))
    gr, gc, gs, gw, nbytes = _proj_outs(g, H, W, dev, 1)
    rc = _lib.load().bxi_match_project_gt_u8(gm.ptr(), g, H, W, gr.ptr(), gc.ptr(), gs.ptr(), gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gm, gr, gc, gs, gw)
    G.check_written(gr, gc, gs, gw)
    G.check_unchanged(gm)
    assert G.same(gr.t, plain[0]) and G.same(gc.t, plain[1]) and G.same(gs.t, plain[2])
    assert torch.equal(gr.t, masks.amax(2).float()) and torch.equal(gc.t, masks.amax(1).float()) and float(gr.t.max()) <= 3.0


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('HW', [(20, 30), (130, 1100)])
def test_project_gt_f32_guarded(dev, HW, lead):
    """bxi_match_project_gt_f32: float masks at 4, 8, 12 bytes past a 16-byte boundary inside NaN."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.box_match import project_gt
    H, W = HW
    g = 3
    masks = _t((np.random.default_rng(lead).uniform(size=(g, H, W)) < 0.02).astype(np.float32) * 0.75, dev)
    plain = project_gt(masks)
    gm = G.embed(masks, lead, G.plane_band(H, W))
    gr, gc, gs, gw, nbytes = _proj_outs(g, H, W, dev, lead)
    rc = _lib.load().bxi_match_project_gt_f32(gm.ptr(), g, H, W, gr.ptr(), gc.ptr(), gs.ptr(), gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gm, gr, gc, gs, gw)
    G.check_written(gr, gc, gs, gw)
    G.check_unchanged(gm)
    assert G.same(gr.t, plain[0]) and G.same(gc.t, plain[1]) and G.same(gs.t, plain[2])
    assert torch.equal(gr.t, masks.amax(2)) and torch.equal(gc.t, masks.amax(1))


def _problems(dev, Q, counts, H, W, C, seed):
    rng = np.random.default_rng(seed)
    P, total = len(counts), sum(counts)
    f = lambda *s: _t(rng.uniform(0, 1, s).astype(np.float32), dev)              # noqa: E731
    return dict(cls=_t(rng.normal(0, 1, (P * Q, C)).astype(np.float32), dev), labels=_t(rng.integers(0, C, total), dev),
                pred=(f(P * Q, H), f(P * Q, W), f(P * Q, 2) * H), gt=(f(total, H), f(total, W), f(total, 2) * H))


@pytest.mark.parametrize('Q,counts', [(12, (0, 4, 7)), (3, (5,)), (70, (1, 0))])
def test_match_cost_guarded(dev, Q, counts):
    """bxi_match_cost_f32: every input at a misaligned address; the cost blocks and the status words written in full."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.box_match import match_cost
    H, W, C = 20, 30, 5
    d = _problems(dev, Q, counts, H, W, C, Q)
    P, total = len(counts), sum(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).tolist()
    plain_cost, plain_status = match_cost(d['cls'], d['labels'], d['pred'], d['gt'], Q, counts, 2.0, 5.0, 1.0)
    gcls, glab = G.embed(d['cls'], 1), G.embed(d['labels'], 1)
    gp = [G.embed(t, k + 1) for k, t in enumerate(d['pred'])]
    gg = [G.embed(t, 3 - k) for k, t in enumerate(d['gt'])]
    gcost, gst = G.out(total * Q, torch.float32, dev, 3), G.out(P, torch.int32, dev, 1)
    rc = _lib.load().bxi_match_cost_f32(gcls.ptr(), C, glab.ptr(), gp[0].ptr(), gp[1].ptr(), gp[2].ptr(), gg[0].ptr(), gg[1].ptr(), gg[2].ptr(),
                                        P, Q, _lib.int_array(offsets), H, W, 2.0, 5.0, 1.0, gcost.ptr(), gst.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gcls, glab, gcost, gst, *gp, *gg)
    G.check_written(gcost, gst)
    G.check_unchanged(gcls, glab, *gp, *gg)
    assert G.same(gcost.t, plain_cost) and torch.equal(gst.t, plain_status) and gst.t.cpu().tolist() == [0] * P
    assert bool(torch.isfinite(gcost.t).all())


@pytest.mark.parametrize('Q,counts', [(12, (0, 4, 7)), (3, (5,)), (70, (1, 0)), (65, (65, 64))])
def test_linear_sum_assignment_guarded(dev, Q, counts):
    """bxi_linear_sum_assignment_f32: the cost at a misaligned address inside NaN (a read outside would make the problem non-finite);
    every query's two words, every compacted slot and every status word written."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.box_match import linear_sum_assignment
    rng = np.random.default_rng(Q)
    P, total = len(counts), sum(counts)
    npos = sum(min(Q, c) for c in counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).tolist()
    cost, labels = _t(rng.uniform(0, 10, total * Q).astype(np.float32), dev), _t(rng.integers(0, 9, total), dev)
    plain = linear_sum_assignment(cost, labels, Q, counts)
    gcost, glab = G.embed(cost, 3), G.embed(labels, 1)
    ggi, gl = G.out((P, Q), torch.int64, dev, 1), G.out((P, Q), torch.int64, dev, 1)
    gpos, gpg, gst = G.out(npos, torch.int64, dev, 1), G.out(npos, torch.int64, dev, 1), G.out(P, torch.int32, dev, 3)
    rc = _lib.load().bxi_linear_sum_assignment_f32(gcost.ptr(), glab.ptr(), P, Q, _lib.int_array(offsets), ggi.ptr(), gl.ptr(), gpos.ptr(),
                                                   gpg.ptr(), gst.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gcost, glab, ggi, gl, gpos, gpg, gst)
    G.check_written(ggi, gl, gpos, gpg, gst)
    G.check_unchanged(gcost, glab)
    for got, want in zip((ggi.t, gl.t, gpos.t, gpg.t, gst.t), plain):
        assert torch.equal(got, want)
    assert gst.t.cpu().tolist() == [0] * P and int((ggi.t > 0).sum()) == npos
