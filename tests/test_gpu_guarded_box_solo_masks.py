"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_dconvl.h on misaligned views inside poisoned bands
(tests/guarded.py).

The feature, the kernel maps and the upstream gradient start 4 bytes past a 16-byte boundary inside NaN bands (a NaN that was read
reaches a result: it would differ from the plain call), the cells sit between -1 words (outside every map); the rows, ``grad_feat`` and
the gradient maps are pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which is exactly as large as the size
query says.  Afterwards the bands are intact, every element of every output is written, the inputs are unchanged, the status word is still
0, and the results are bit-identical to the same call on plain tensors -- and to a second guarded run.  Image 1 of 3 has no rows (its
part of the resized feature is neither written nor read); E = 5 (padded to 8) and E = 33; a 13 x 21 feature with levels of its own size,
of (7, 11) (a non-integer ratio, twice) and of (14, 22) (a slight up-size: clamped taps at both edges)."""
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_dconvl.py checks the table against _lib.DCONVL_SIGNATURES)
GUARDED = {
    'bxi_solo_dconvl_forward_f32': 'test_forward_guarded',
    'bxi_solo_dconvl_backward_f32': 'test_backward_guarded',
}
B, H, W = 3, 13, 21
GRIDS, SIZES = [3, 6, 2, 2], [(13, 21), (7, 11), (7, 11), (14, 22)]
COUNTS = [[3, 0, 2], [1, 0, 34], [0, 0, 2], [2, 0, 1]]                        # an image without rows; 36 rows of image 2 in one group


def _call(lib, dev, which, E, feat, maps, cells, out, status, ws, nbytes, gout=None, gfeat=None, gmaps=None):
    from boxinstseg_amd import _lib
    counts = [c for row in COUNTS for c in row]
    head = (G.ptr(feat), B, E, H, W, _lib.ptr_array([G.ptr(m) for m in maps]), _lib.int_array(GRIDS), _lib.int_array([v for s in SIZES for v in s]),
            len(GRIDS), G.ptr(cells), _lib.int_array(counts), sum(counts))
    if which == 'forward':
        rc = lib.bxi_solo_dconvl_forward_f32(*head, G.ptr(out), G.ptr(status), G.ptr(ws), nbytes, G.stream(dev))
    else:
        rc = lib.bxi_solo_dconvl_backward_f32(*head, G.ptr(gout), G.ptr(gfeat), None if gmaps is None else _lib.ptr_array([G.ptr(m) for m in gmaps]),
                                              G.ptr(status), G.ptr(ws), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


def _sizes(lib, E):
    from boxinstseg_amd import _lib
    args = (B, E, H, W, _lib.int_array([v for s in SIZES for v in s]), _lib.int_array([c for row in COUNTS for c in row]), len(GRIDS))
    return lib.bxi_solo_dconvl_forward_workspace_bytes(*args), lib.bxi_solo_dconvl_backward_workspace_bytes(*args)


def _inputs(dev, E):
    rng = torch.Generator().manual_seed(7)
    feat = (0.5 * torch.randn(B, E, H, W, generator=rng)).to(dev)
    maps = [(torch.randn(B, E, S, S, generator=rng) / E ** 0.5).to(dev) for S in GRIDS]
    cells = torch.cat([torch.randperm(S * S, generator=rng)[:n].sort().values for S, row in zip(GRIDS, COUNTS) for n in row]).to(dev)
    total = sum(sum(row) * oh * ow for row, (oh, ow) in zip(COUNTS, SIZES))
    g = torch.randn(total, generator=rng).to(dev)
    return feat, maps, cells, total, g


@pytest.mark.parametrize('E', [5, 33])
def test_forward_guarded(dev, E):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    feat, maps, cells, total, _ = _inputs(dev, E)
    fbytes, _ = _sizes(lib, E)
    # the largest resampled group's feature (3 x E x 14 x 22, a multiple of 4 floats), then the product's own workspace
    assert fbytes == 4 * ((B * E * 14 * 22 + 3) // 4 * 4) + lib.bxi_solo_dconv_forward_workspace_bytes(37, B, E)
    want, status = torch.empty(total, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    _call(lib, dev, 'forward', E, feat, maps, cells, want, status, torch.empty(fbytes, dtype=torch.uint8, device=dev), fbytes)
    band = G.plane_band(H, W)
    runs = []
    for _ in range(2):
        gf, gm, gc, gs = G.embed(feat, 1, band), [G.embed(m, 1, band) for m in maps], G.embed(cells, 1), G.embed(status, 1)
        go = G.out(total, torch.float32, dev, 1, band)
        assert gf.ptr() % 16 == 4 and all(m.ptr() % 16 == 4 for m in gm) and go.ptr() % 16 == 4 and gc.ptr() % 16 == 8
        ws = G.out(fbytes // 4, torch.int32, dev, 0)                          # 16-byte aligned, exactly the size asked for
        _call(lib, dev, 'forward', E, gf, gm, gc, go, gs, ws, fbytes)
        G.check_bands(gf, gc, go, gs, ws, *gm)
        G.check_written(go)
        G.check_unchanged(gf, gc, gs, *gm)
        assert G.same(go.t, want) and bool(torch.isfinite(want).all()) and int(status) == 0
        runs.append(go.t.clone())
    assert G.same(runs[0], runs[1])


@pytest.mark.parametrize('E', [5, 33])
def test_backward_guarded(dev, E):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    feat, maps, cells, total, g = _inputs(dev, E)
    _, nbytes = _sizes(lib, E)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    want_f, want_m = torch.empty_like(feat), [torch.empty_like(m) for m in maps]
    _call(lib, dev, 'backward', E, feat, maps, cells, None, status, torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes, g, want_f, want_m)
    band = G.plane_band(H, W)
    gf, gm, gc = G.embed(feat, 1, band), [G.embed(m, 1, band) for m in maps], G.embed(cells, 1)
    gg, gs = G.embed(g, 1, band), G.embed(status, 1)
    assert gf.ptr() % 16 == 4 and gg.ptr() % 16 == 4
    for _ in range(2):
        rf, rm = G.out(feat.shape, torch.float32, dev, 1, band), [G.out(m.shape, torch.float32, dev, 1, band) for m in maps]
        ws = G.out(nbytes // 4, torch.int32, dev, 0)
        assert ws.ptr() % 16 == 0 and rf.ptr() % 16 == 4
        _call(lib, dev, 'backward', E, gf, gm, gc, None, gs, ws, nbytes, gg, rf, rm)
        G.check_bands(gf, gc, gg, gs, rf, ws, *gm, *rm)
        G.check_written(rf, *rm)
        G.check_unchanged(gf, gc, gg, gs, *gm)
        assert G.same(rf.t, want_f) and all(G.same(a.t, b) for a, b in zip(rm, want_m)) and int(status) == 0
    assert bool(torch.isfinite(want_f).all()) and all(bool(torch.isfinite(m).all()) for m in want_m)
    assert not bool(want_f[1].any()) and not any(bool(m[1].any()) for m in want_m) and bool(want_f[0].any())     # the image without rows: zeros
    # either gradient alone: the same bits, and the other output is not asked for
    rf2, ws1 = G.out(feat.shape, torch.float32, dev, 1, band), G.out(nbytes // 4, torch.int32, dev, 0)
    _call(lib, dev, 'backward', E, gf, gm, gc, None, gs, ws1, nbytes, gg, rf2, None)
    rm2, ws2 = [G.out(m.shape, torch.float32, dev, 1, band) for m in maps], G.out(nbytes // 4, torch.int32, dev, 0)
    _call(lib, dev, 'backward', E, gf, gm, gc, None, gs, ws2, nbytes, gg, None, rm2)
    G.check_bands(rf2, ws1, ws2, *rm2)
    assert G.same(rf2.t, want_f) and all(G.same(a.t, b) for a, b in zip(rm2, want_m))
