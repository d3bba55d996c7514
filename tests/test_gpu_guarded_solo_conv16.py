"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_dconv16.h on misaligned views inside poisoned bands
(tests/guarded.py).

The half-precision feature, kernel maps, saved masks and upstream gradient start 2 bytes past a 16-byte boundary inside NaN bands (a NaN
that was read reaches a result: it would differ from the plain call), the cells sit between -1 words (outside every map); the masks, the
image indices, ``grad_feat`` and the gradient maps are pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which is
exactly as large as the size query says.  Afterwards the bands are intact, every element of every output and every word of the workspace
is written, the inputs are unchanged, the status word is still 0, and the results are bit-identical to the same call on plain tensors --
and to a second guarded run.  Both layouts (MAPS with masks in the half type, ROWS with fp32 masks), both types; E = 5 (padded to 16) and
E = 33 (a second, nearly empty block of channels, three k steps), 13 x 21 pixels (five tiles, the last one short, odd rows: the element
loads at the head and tail of every feature row)."""
import pytest
import torch

from tests import guarded as G
from tests import solo_conv_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_dconv16.py checks the table against _lib.DCONV16_SIGNATURES)
GUARDED = {
    'bxi_solo_dconv16_forward': 'test_forward_guarded',
    'bxi_solo_dconv16_backward': 'test_backward_guarded',
}
H, W = 13, 21
GRIDS, COUNTS = [3, 2], [[3, 0, 2], [1, 0, 34]]               # an image without rows; 36 rows in image 2: a second chunk of 32
DTYPES = [torch.float16, torch.bfloat16]


def _call(lib, dev, which, layout, E, dtype, odt, feat, maps, cells, counts, out, img, status, ws, nbytes, gout=None, gfeat=None, gmaps=None):
    from boxinstseg_amd import _lib
    B = 1 if layout else 3
    t = lambda x: x.t if isinstance(x, G.Guarded) else x                                                   # noqa: E731
    grids = [t(maps[0]).shape[0]] if layout else GRIDS
    code = _lib.DCONV16_F16 if dtype == torch.float16 else _lib.DCONV16_BF16
    ocode = _lib.DCONV16_OUT_F32 if odt == torch.float32 else code
    head = (G.ptr(feat), code, B, E, H, W, _lib.ptr_array([G.ptr(m) for m in maps]), _lib.int_array(grids), len(maps), layout, G.ptr(cells),
            _lib.int_array(counts), sum(counts), 1)
    if which == 'forward':
        rc = lib.bxi_solo_dconv16_forward(*head, G.ptr(out), ocode, G.ptr(img), G.ptr(status), G.ptr(ws), nbytes, G.stream(dev))
    else:
        rc = lib.bxi_solo_dconv16_backward(*head, G.ptr(out), G.ptr(gout), ocode, G.ptr(gfeat),
                                           None if gmaps is None else _lib.ptr_array([G.ptr(m) for m in gmaps]), G.ptr(status), G.ptr(ws), nbytes,
                                           G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


def _inputs(dev, layout, E, dtype, odt):
    if layout:
        rng = torch.Generator().manual_seed(5)
        feat = torch.randn(1, E, H, W, generator=rng).to(dev, dtype)
        maps = [torch.randn(12, E, generator=rng).to(dev, dtype)]
        cells = torch.tensor([5, 0, 5, 11, 3] * 7, device=dev)
        counts = [35]
    else:
        case = R.make_case(3, 3, E, H, W, GRIDS, COUNTS, dups=[(1, 2, 31)])
        feat, maps, order, _ = R.to_torch(case, dtype, dev)
        cells = torch.cat([o for row in order for o in row])
        counts = [c for row in COUNTS for c in row]
    g = torch.randn(sum(counts), H, W, generator=torch.Generator().manual_seed(6)).to(dev, odt)
    return feat, maps, cells, counts, g


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('E', [5, 33])
@pytest.mark.parametrize('layout', [0, 1])
def test_forward_guarded(dev, layout, E, dtype):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    odt = torch.float32 if layout else dtype
    feat, maps, cells, counts, _ = _inputs(dev, layout, E, dtype, odt)
    n, B = sum(counts), 1 if layout else 3
    want, want_img = torch.empty((n, H, W), dtype=odt, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    fbytes = lib.bxi_solo_dconv16_forward_workspace_bytes(n, B, E)
    assert fbytes == 2 * 32 * ((E + 15) // 16 * 16) * (n // 32 + B)
    _call(lib, dev, 'forward', layout, E, dtype, odt, feat, maps, cells, counts, want, want_img, status,
          torch.empty(fbytes, dtype=torch.uint8, device=dev), fbytes)
    band = G.plane_band(H, W)
    runs = []
    for _ in range(2):
        gf, gm, gc, gs = G.embed(feat, 1, band), [G.embed(m, 1, band) for m in maps], G.embed(cells, 1), G.embed(status, 1)
        go, gi = G.out((n, H, W), odt, dev, 1, band), G.out(n, torch.int64, dev, 1)
        assert gf.ptr() % 16 == 2 and all(m.ptr() % 16 == 2 for m in gm) and go.ptr() % 16 == (4 if layout else 2) and gc.ptr() % 16 == 8
        ws = G.out(fbytes // 4, torch.int32, dev, 0)                          # 16-byte aligned, exactly the size asked for
        _call(lib, dev, 'forward', layout, E, dtype, odt, gf, gm, gc, counts, go, gi, gs, ws, fbytes)
        G.check_bands(gf, gc, go, gi, gs, ws, *gm)
        G.check_written(go, gi, ws)
        G.check_unchanged(gf, gc, gs, *gm)
        assert G.same(go.t, want) and torch.equal(gi.t, want_img) and bool(torch.isfinite(want.float()).all()) and int(status) == 0
        runs.append((go.t.clone(), ws.t.clone()))
    assert G.same(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert want_img.tolist() == ([0] * 35 if layout else [0, 0, 0, 2, 2, 0] + [2] * 34)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('E', [5, 33])
@pytest.mark.parametrize('layout', [0, 1])
def test_backward_guarded(dev, layout, E, dtype):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    odt = torch.float32 if layout else dtype
    feat, maps, cells, counts, g = _inputs(dev, layout, E, dtype, odt)
    n, B = sum(counts), 1 if layout else 3
    out, img = torch.empty((n, H, W), dtype=odt, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    fbytes = lib.bxi_solo_dconv16_forward_workspace_bytes(n, B, E)
    _call(lib, dev, 'forward', layout, E, dtype, odt, feat, maps, cells, counts, out, img, status, torch.empty(fbytes, dtype=torch.uint8, device=dev),
          fbytes)
    nbytes = lib.bxi_solo_dconv16_backward_workspace_bytes(n, B, E, H, W)
    assert nbytes == fbytes + 4 * n * E * (5 + 1)
    want_f, want_m = torch.empty_like(feat), [torch.empty_like(m) for m in maps]
    _call(lib, dev, 'backward', layout, E, dtype, odt, feat, maps, cells, counts, out, img, status,
          torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes, g, want_f, want_m)
    band = G.plane_band(H, W)
    gf, gm, gc = G.embed(feat, 1, band), [G.embed(m, 1, band) for m in maps], G.embed(cells, 1)
    go, gg, gs = G.embed(out, 1, band), G.embed(g, 1, band), G.embed(status, 1)
    assert gf.ptr() % 16 == 2 and go.ptr() % 16 == (4 if layout else 2) and gg.ptr() % 16 == (4 if layout else 2)
    runs = []
    for _ in range(2):
        rf, rm = G.out(feat.shape, dtype, dev, 1, band), [G.out(m.shape, dtype, dev, 1, band) for m in maps]
        ws = G.out(nbytes // 4, torch.int32, dev, 0)                          # 16-byte aligned, exactly the size asked for
        assert ws.ptr() % 16 == 0 and rf.ptr() % 16 == 2
        _call(lib, dev, 'backward', layout, E, dtype, odt, gf, gm, gc, counts, go, None, gs, ws, nbytes, gg, rf, rm)
        G.check_bands(gf, gc, go, gg, gs, rf, ws, *gm, *rm)
        G.check_written(rf, ws, *rm)
        G.check_unchanged(gf, gc, go, gg, gs, *gm)
        assert G.same(rf.t, want_f) and all(G.same(a.t, b) for a, b in zip(rm, want_m)) and int(status) == 0
        runs.append(ws.t.clone())
    assert torch.equal(runs[0], runs[1])
    assert bool(torch.isfinite(want_f.float()).all()) and all(bool(torch.isfinite(m.float()).all()) for m in want_m)
    if not layout:
        assert not bool(want_f[1].any()) and not bool(want_m[0][1].any()) and bool(want_f[0].any())       # the image without rows: zeros
    # either gradient alone: the same bits, and the other output is not asked for
    rf2, ws1 = G.out(feat.shape, dtype, dev, 1, band), G.out(nbytes // 4, torch.int32, dev, 0)
    _call(lib, dev, 'backward', layout, E, dtype, odt, gf, gm, gc, counts, go, None, gs, ws1, nbytes, gg, rf2, None)
    rm2, ws2 = [G.out(m.shape, dtype, dev, 1, band) for m in maps], G.out(nbytes // 4, torch.int32, dev, 0)
    _call(lib, dev, 'backward', layout, E, dtype, odt, gf, gm, gc, counts, go, None, gs, ws2, nbytes, gg, None, rm2)
    G.check_bands(rf2, ws1, ws2, *rm2)
    assert G.same(rf2.t, want_f) and all(G.same(a.t, b) for a, b in zip(rm2, want_m))
