"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_dconv.h on misaligned views inside poisoned bands
(tests/guarded.py).

The feature, the kernel maps, the saved masks and the upstream gradient start 4, 8 or 12 bytes past a 16-byte boundary inside NaN bands (a
NaN that was read reaches a result: it would differ from the plain call), the cells sit between -1 words (outside every map); the masks,
the image indices, ``grad_feat`` and the gradient maps are pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which
is exactly as large as the size query says.  Afterwards the bands are intact, every element of every output and of the workspace is written,
the inputs are unchanged, the status word is still 0, and the results are bit-identical to the same call on plain tensors.  Both layouts;
E = 5 (the odd tail of E) and E = 33 (a second, nearly empty block of channels), 13 x 21 pixels (five tiles, the last one short)."""
import pytest
import torch

from tests import guarded as G
from tests import solo_conv_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.DCONV_SIGNATURES)
GUARDED = {
    'bxi_solo_dconv_forward_f32': 'test_forward_guarded',
    'bxi_solo_dconv_backward_f32': 'test_backward_guarded',
}
H, W = 13, 21
GRIDS, COUNTS = [3, 2], [[3, 0, 2], [1, 0, 34]]               # an image without rows; 36 rows in image 2: a second chunk of 32


def _call(lib, dev, which, layout, E, feat, maps, cells, counts, act, out, img, status, ws, nbytes, gout=None, gfeat=None, gmaps=None):
    from boxinstseg_amd import _lib
    B = 1 if layout else 3
    grids = [maps[0].t.shape[0] if isinstance(maps[0], G.Guarded) else maps[0].shape[0]] if layout else GRIDS
    head = (G.ptr(feat), B, E, H, W, _lib.ptr_array([G.ptr(m) for m in maps]), _lib.int_array(grids), len(maps), layout, G.ptr(cells),
            _lib.int_array(counts), sum(counts), act)
    if which == 'forward':
        rc = lib.bxi_solo_dconv_forward_f32(*head, G.ptr(out), G.ptr(img), G.ptr(status), G.ptr(ws), nbytes, G.stream(dev))
    else:
        rc = lib.bxi_solo_dconv_backward_f32(*head, G.ptr(out), G.ptr(gout), G.ptr(gfeat),
                                             None if gmaps is None else _lib.ptr_array([G.ptr(m) for m in gmaps]), G.ptr(status), G.ptr(ws), nbytes,
                                             G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


def _inputs(dev, layout, E):
    if layout:
        rng = torch.Generator().manual_seed(5)
        feat = torch.randn(1, E, H, W, generator=rng).to(dev)
        maps = [torch.randn(12, E, generator=rng).to(dev)]
        cells = torch.tensor([5, 0, 5, 11, 3] * 7, device=dev)
        counts = [35]
    else:
        case = R.make_case(3, 3, E, H, W, GRIDS, COUNTS, dups=[(1, 2, 31)])
        feat, maps, order, _ = R.to_torch(case, torch.float32, dev)
        cells = torch.cat([o for row in order for o in row])
        counts = [c for row in COUNTS for c in row]
    g = torch.randn(sum(counts), H, W, generator=torch.Generator().manual_seed(6)).to(dev)
    return feat, maps, cells, counts, g


@pytest.mark.parametrize('E', [5, 33])
@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('lead', [1, 2, 3])
def test_forward_guarded(dev, lead, layout, E):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    feat, maps, cells, counts, _ = _inputs(dev, layout, E)
    n = sum(counts)
    want, want_img = torch.empty((n, H, W), device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    fbytes = lib.bxi_solo_dconv_forward_workspace_bytes(n, 1 if layout else 3, E)
    assert fbytes == 4 * 32 * ((E + 7) // 8 * 8) * (n // 32 + (1 if layout else 3))
    _call(lib, dev, 'forward', layout, E, feat, maps, cells, counts, 1, want, want_img, status, torch.empty(fbytes, dtype=torch.uint8, device=dev), fbytes)
    band = G.plane_band(H, W)
    gf, gm, gc = G.embed(feat, lead, band), [G.embed(m, 4 - lead, band) for m in maps], G.embed(cells, 1)
    gs = G.embed(status, lead)
    go, gi = G.out((n, H, W), torch.float32, dev, 4 - lead, band), G.out(n, torch.int64, dev, 1)
    assert gf.ptr() % 16 == 4 * lead and go.ptr() % 16 == 4 * (4 - lead) % 16 and gc.ptr() % 16 == 8
    ws = G.out(fbytes // 4, torch.float32, dev, 0)                            # 16-byte aligned, exactly the size asked for
    _call(lib, dev, 'forward', layout, E, gf, gm, gc, counts, 1, go, gi, gs, ws, fbytes)
    G.check_bands(gf, gc, go, gi, gs, ws, *gm)
    G.check_written(go, gi, ws)
    G.check_unchanged(gf, gc, gs, *gm)
    assert torch.equal(go.t, want) and torch.equal(gi.t, want_img) and bool(torch.isfinite(want).all()) and int(status) == 0
    assert want_img.tolist() == ([0] * 35 if layout else [0, 0, 0, 2, 2, 0] + [2] * 34)


@pytest.mark.parametrize('E', [5, 33])
@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('lead', [1, 2, 3])
def test_backward_guarded(dev, lead, layout, E):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    feat, maps, cells, counts, g = _inputs(dev, layout, E)
    n = sum(counts)
    out, img = torch.empty((n, H, W), device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    fbytes = lib.bxi_solo_dconv_forward_workspace_bytes(n, 1 if layout else 3, E)
    _call(lib, dev, 'forward', layout, E, feat, maps, cells, counts, 1, out, img, status, torch.empty(fbytes, dtype=torch.uint8, device=dev), fbytes)
    nbytes = lib.bxi_solo_dconv_backward_workspace_bytes(n, 1 if layout else 3, E, H, W)
    assert nbytes == fbytes + 4 * n * E * (5 + 1)
    want_f, want_m = torch.empty_like(feat), [torch.empty_like(m) for m in maps]
    _call(lib, dev, 'backward', layout, E, feat, maps, cells, counts, 1, out, img, status, torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes,
          g, want_f, want_m)
    band = G.plane_band(H, W)
    gf, gm, gc = G.embed(feat, lead, band), [G.embed(m, 4 - lead, band) for m in maps], G.embed(cells, 1)
    go, gg, gs = G.embed(out, 4 - lead, band), G.embed(g, lead, band), G.embed(status, lead)
    rf, rm = G.out(feat.shape, torch.float32, dev, lead, band), [G.out(m.shape, torch.float32, dev, 4 - lead, band) for m in maps]
    ws = G.out(nbytes // 4, torch.float32, dev, 0)                            # 16-byte aligned, exactly the size asked for
    assert ws.ptr() % 16 == 0 and gg.ptr() % 16 == 4 * lead and rf.ptr() % 16 == 4 * lead
    _call(lib, dev, 'backward', layout, E, gf, gm, gc, counts, 1, go, None, gs, ws, nbytes, gg, rf, rm)
    G.check_bands(gf, gc, go, gg, gs, rf, ws, *gm, *rm)
    G.check_written(rf, ws, *rm)
    G.check_unchanged(gf, gc, go, gg, gs, *gm)
    assert torch.equal(rf.t, want_f) and all(torch.equal(a.t, b) for a, b in zip(rm, want_m)) and int(status) == 0
    assert bool(torch.isfinite(want_f).all()) and all(bool(torch.isfinite(m).all()) for m in want_m)
    if not layout:
        assert not bool(want_f[1].any()) and not bool(want_m[0][1].any()) and bool(want_f[0].any())       # the image without rows: zeros
    # either gradient alone: the same bits, and the other output is not asked for
    rf2, ws1 = G.out(feat.shape, torch.float32, dev, lead, band), G.out(nbytes // 4, torch.float32, dev, 0)
    _call(lib, dev, 'backward', layout, E, gf, gm, gc, counts, 1, go, None, gs, ws1, nbytes, gg, rf2, None)
    rm2, ws2 = [G.out(m.shape, torch.float32, dev, 4 - lead, band) for m in maps], G.out(nbytes // 4, torch.float32, dev, 0)
    _call(lib, dev, 'backward', layout, E, gf, gm, gc, counts, 1, go, None, gs, ws2, nbytes, gg, None, rm2)
    G.check_bands(rf2, ws1, ws2, *rm2)
    assert torch.equal(rf2.t, want_f) and all(torch.equal(a.t, b) for a, b in zip(rm2, want_m))
