"""GPU: the entry points of include/boxinst/boxinst_hip_post.h on misaligned views inside poisoned bands (tests/guarded.py).

Inputs are views at the element's natural alignment only (fp32 at 4, 8 and 12 bytes past a 16-byte boundary, mask bytes at odd
addresses) surrounded by NaN / -1; outputs and the workspace are pre-filled with the 'nobody wrote this' pattern.  Afterwards the
bands are intact, every output element and every workspace element is written, the inputs are unchanged, and the results are
bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import matrix_nms_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.POST_SIGNATURES)
GUARDED = {
    'bxi_mask_pack_f32': 'test_mask_pack_f32_guarded',
    'bxi_mask_pack_u8': 'test_mask_pack_u8_guarded',
    'bxi_matrix_nms_f32': 'test_matrix_nms_guarded',
}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _words(h, w):
    return (h * w + 63) // 64


def _bits_set(bits):
    """Set bits per candidate: whatever the private layout, they are as many as the mask has pixels."""
    wd = bits.cpu().numpy().view(np.uint64)
    return [int(sum(bin(int(x)).count('1') for x in row)) for row in wd]


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('hw', [(25, 38), (24, 40), (7, 9)])
def test_mask_pack_f32_guarded(dev, hw, lead):
    """bxi_mask_pack_f32: probabilities at 4, 8, 12 bytes past a 16-byte boundary; h*w = 950 moves every candidate's base by 8 bytes more,
    960 keeps it, 63 is less than one word.  (A NaN of the band compares false, so a stray LOAD cannot show here -- the uint8 test's 0xFF
    band is the one that sees loads; this one sees stores, unwritten words and results that depend on the alignment.)"""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.matrix_nms import pack_probs
    lib = _lib.load()
    h, w = hw
    n = 5
    probs = _t(R.disc_probs(np.random.default_rng(lead), n, h, w), dev)
    plain = pack_probs(probs, 0.5)
    gp = G.embed(probs, lead, G.plane_band(h, w))
    gb, ga, gs = G.out((n, _words(h, w)), torch.int64, dev, 1), G.out(n, torch.int32, dev, lead), G.out(n, torch.float32, dev, 4 - lead)
    rc = lib.bxi_mask_pack_f32(gp.ptr(), n, h, w, 0.5, gb.ptr(), ga.ptr(), gs.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gp, gb, ga, gs)
    G.check_written(gb, ga, gs)
    G.check_unchanged(gp)
    assert torch.equal(gb.t, plain[0]) and torch.equal(ga.t, plain[1]) and torch.equal(gs.t.view(torch.int32), plain[2].view(torch.int32))
    assert ga.t.cpu().tolist() == (probs > 0.5).sum((1, 2)).cpu().tolist() == _bits_set(gb.t)


@pytest.mark.parametrize('lead', [1, 6, 15])
@pytest.mark.parametrize('hw', [(25, 38), (7, 9)])
def test_mask_pack_u8_guarded(dev, hw, lead):
    """bxi_mask_pack_u8: mask bytes at odd addresses; the band around them is 0xFF, i.e. set pixels, so a read outside shows in area."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.matrix_nms import pack_masks
    lib = _lib.load()
    h, w = hw
    n = 5
    masks = _t(R.disc_masks(np.random.default_rng(lead), n, h, w).astype(np.uint8) * 7, dev)
    plain = pack_masks(masks)
    gm = G.embed(masks, lead, G.plane_band(h, w))
    gb, ga = G.out((n, _words(h, w)), torch.int64, dev, 1), G.out(n, torch.int32, dev, 3)
    rc = lib.bxi_mask_pack_u8(gm.ptr(), n, h, w, gb.ptr(), ga.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gm, gb, ga)
    G.check_written(gb, ga)
    G.check_unchanged(gm)
    assert torch.equal(gb.t, plain[0]) and torch.equal(ga.t, plain[1])
    assert ga.t.cpu().tolist() == (masks != 0).sum((1, 2)).cpu().tolist() == _bits_set(gb.t)


@pytest.mark.parametrize('kernel', [0, 1])
@pytest.mark.parametrize('n,n_all,hw', [(70, 90, (25, 38)), (33, 33, (7, 9))])
def test_matrix_nms_guarded(dev, n, n_all, hw, kernel):
    """bxi_matrix_nms_f32: three tile rows with a partial last tile (70) and one candidate past a tile edge (33); rows fetched through
    `order` out of more candidates than enter.  The workspace is exactly bxi_matrix_nms_workspace_bytes(n) and is written in full."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd.matrix_nms import matrix_nms_decay, pack_masks
    lib = _lib.load()
    h, w = hw
    rng = np.random.default_rng(n + kernel)
    masks, labels, scores = R.disc_masks(rng, n_all, h, w), rng.integers(0, 3, n_all), R.shuffled_scores(rng, n_all)
    bits, area = pack_masks(_t(masks, dev))
    s, order = torch.sort(_t(scores, dev), descending=True, stable=True)
    s, order = s[:n].contiguous(), order[:n].contiguous()
    name = 'linear' if kernel else 'gaussian'
    plain = matrix_nms_decay(bits, area, _t(labels, dev), order, s, hw, name, 2.0)
    gbits, garea = G.embed(bits, 1), G.embed(area, 1)
    glab, gord, gsc = G.embed(_t(labels, dev), 1), G.embed(order, 1), G.embed(s, 3)
    ws_bytes = lib.bxi_matrix_nms_workspace_bytes(n)
    assert ws_bytes % 4 == 0
    gd, gi, gw = G.out(n, torch.float32, dev, 1), G.out((n, n), torch.float32, dev, 3), G.out(ws_bytes // 4, torch.float32, dev, 1)
    rc = lib.bxi_matrix_nms_f32(gbits.ptr(), garea.ptr(), glab.ptr(), gord.ptr(), gsc.ptr(), n_all, n, h, w, kernel, 2.0, gd.ptr(), gi.ptr(),
                                gw.ptr(), ws_bytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gbits, garea, glab, gord, gsc, gd, gi, gw)
    G.check_written(gd, gi, gw)
    G.check_unchanged(gbits, garea, glab, gord, gsc)
    for got, want in ((gd.t, plain[0]), (gi.t, plain[1]), (gw.t[:n], plain[2])):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    ref = R.matrix_nms_ref(masks, labels, scores, nms_pre=n, kernel=name)
    assert np.array_equal(gi.t.cpu().numpy().view(np.uint32), ref['decay_iou'].view(np.uint32))
    err = np.abs(gd.t.cpu().numpy() - ref['decayed']) / ref['decayed']
    assert np.nanmax(err) <= 2e-6 and np.array_equal(np.isnan(err), np.isnan(ref['decayed']) | (ref['decayed'] == 0))
