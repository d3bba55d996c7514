"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_bls.h on misaligned views inside poisoned bands (tests/guarded.py).

Every float input starts 4, 8 or 12 bytes off a 16-byte boundary (or on one) between bands of NaN, every index array between bands of
-1, the target bytes between bands of 0xFF; outputs and ``state`` are exactly as large as the call needs and pre-filled with the 'nobody
wrote this' pattern.  Afterwards the bands are intact, every element of every output is written (the inert row included: zeros), the
inputs are unchanged, and the results are bit-identical to the same call on plain tensors.  ``state`` mixes doubles, 64-bit keys, ints
and bytes behind 8-byte roundings, so it is checked for its bands and for giving the same results, not element by element.

Two size groups -- (9, 11) with three rows in two levels, (5, 6) with two rows in one --, rows out of level order, one row inert."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_bls.py checks the table against _lib.BLS_SIGNATURES)
GUARDED = {
    'bxi_bls_front_f32': 'test_front_guarded',
    'bxi_bls_backward_f32': 'test_backward_guarded',
    'bxi_bls_high_forward_f32': 'test_high_guarded',
    'bxi_bls_high_backward_f32': 'test_high_guarded',
}
SIZES, ROWS, GTS, B = [(9, 11), (5, 6)], [3, 2], [3, 2], 2
LEVEL_GROUP, LEVEL_ROWS = [0, 1, 0], [2, 2, 1]
LR = 1 << 20
ROW_SRC = np.array([0 * LR + 0, 2 * LR + 0, 0 * LR + 1, 1 * LR + 1, 1 * LR + 0], np.int32)
TGT_OF = np.array([2, -1, 0, 1, 0], np.int32)              # row 1 is inert
IMG_OF = np.array([1, 0, 0, 1, 0], np.int32)
M, W_PROJ, W_IMG, W_HIGH = 5, 3.0, 0.05, 5.0
PIX = [0, 3 * 99, 3 * 99 + 2 * 30]
ROW_PIX = [(0, 99), (99, 198), (198, 297), (297, 327), (327, 357)]       # [lo, hi) of every row in a ragged per-pixel buffer
ROW_GROUP = [0, 0, 0, 1, 1]


def _groups(imgs, masks):
    from boxinstseg_amd import _lib
    return (_lib.BlsGroup * 2)(*[_lib.BlsGroup(G.ptr(imgs[g]) if imgs is not None else None, G.ptr(masks[g]), SIZES[g][0], SIZES[g][1], ROWS[g], GTS[g])
                                 for g in range(2)])


def _call(lib, dev, entry, imgs, masks, *a):
    from boxinstseg_amd import _lib
    groups = _groups(imgs, masks)
    ptr = lambda x: G.ptr(x) if isinstance(x, (G.Guarded, torch.Tensor)) or x is None else x
    if entry in ('front', 'backward'):
        levels, rest = a[0], [ptr(x) for x in a[1:]]
        table = (groups, 2, _lib.ptr_array([ptr(t) for t in levels]), _lib.int_array(LEVEL_ROWS), _lib.int_array(LEVEL_GROUP), 3)
        if entry == 'front':
            rc = lib.bxi_bls_front_f32(*table, *rest, G.stream(dev))
        else:
            rc = lib.bxi_bls_backward_f32(*table, *rest, G.stream(dev))
    elif entry == 'high_forward':
        rc = lib.bxi_bls_high_forward_f32(groups, 2, *[ptr(x) for x in a], G.stream(dev))
    else:
        rc = lib.bxi_bls_high_backward_f32(groups, 2, *[ptr(x) for x in a], G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _inputs(rng, dev):
    imgs = [_rand(rng, B, 3, h, w).to(dev) for h, w in SIZES]
    masks = [torch.from_numpy((rng.random((g, h, w)) > 0.5).astype(np.uint8)).to(dev) for g, (h, w) in zip(GTS, SIZES)]
    levels = [(2.0 * _rand(rng, n, *SIZES[g])).to(dev) for n, g in zip(LEVEL_ROWS, LEVEL_GROUP)]
    idx = [torch.from_numpy(a).to(dev) for a in (ROW_SRC, TGT_OF, IMG_OF)]
    return imgs, masks, levels, idx


def _front_outputs(dev, guarded, lead=0):
    mk = (lambda n, k: G.out(n, torch.float32, dev, (lead + k) % 4)) if guarded else (lambda n, k: torch.empty(n, device=dev))
    return [mk(PIX[-1], 0)] + [mk(M, k) for k in range(1, 5)]


def _state(lib, dev, guarded, query, lead=0):
    from boxinstseg_amd import _lib
    n = getattr(lib, query)(_groups(None, [None, None]), 2)
    assert n > 0 and n % 8 == 0
    return (G.out(n // 8, torch.float64, dev, lead % 2) if guarded else torch.empty(n // 8, dtype=torch.float64, device=dev)), n


def _plane(levels, m):
    return levels[int(ROW_SRC[m]) // LR][int(ROW_SRC[m]) % LR]


def _reference(imgs, masks, levels, rows, y=None):
    """The per-row statements of tests/bls_loss_ref.py in fp64 on the CPU for the live rows -> per row (proj, img term, high term)."""
    from tests.b2m_loss_ref import box_projection_loss, levelset_loss
    out = {}
    for m in rows:
        g = ROW_GROUP[m]
        x = _plane(levels, m).double().cpu()[None, None]
        T = masks[g][int(TGT_OF[m])].double().cpu()[None, None]
        p = torch.sigmoid(x)
        phi = torch.cat((p, 1 - p), 1) * T
        pn = T.sum((1, 2, 3)).clamp(min=1)
        proj = box_projection_loss(p, T, W_PROJ)
        img = levelset_loss(phi, imgs[g][int(IMG_OF[m])].double().cpu()[None] * T, pn, 1.0) * W_IMG
        high = None
        if y is not None:
            lo, hi = ROW_PIX[m]
            yy = torch.stack([y[0][lo:hi], y[1][lo:hi]]).double().cpu().view(1, 2, *SIZES[g])
            high = levelset_loss(phi, yy * T, pn, 1.0) * W_HIGH
        out[m] = (proj, img, high, pn)
    return out


@pytest.mark.parametrize('lead', range(4))
def test_front_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(lead)
    imgs, masks, levels, idx = _inputs(rng, dev)
    outs = _front_outputs(dev, False)
    state, nbytes = _state(lib, dev, False, 'bxi_bls_state_bytes')
    _call(lib, dev, 'front', imgs, masks, levels, *idx, M, B, W_PROJ, W_IMG, *outs, state, nbytes)
    gi = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(imgs)]
    gm = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(masks)]
    gl = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(levels)]
    gx = [G.embed(t, (lead + k) % 4) for k, t in enumerate(idx)]
    gouts = _front_outputs(dev, True, lead)
    gstate, _ = _state(lib, dev, True, 'bxi_bls_state_bytes', lead)
    _call(lib, dev, 'front', gi, gm, gl, *gx, M, B, W_PROJ, W_IMG, *gouts, gstate, nbytes)
    G.check_bands(*gi, *gm, *gl, *gx, *gouts, gstate)
    G.check_written(*gouts)
    G.check_unchanged(*gi, *gm, *gl, *gx)
    for a, b in zip(gouts, outs):
        assert G.same(a.t, b)
    p, lp, li, pn, live = outs
    assert live.tolist() == [1, 0, 1, 1, 1] and float(lp[1]) == 0 and float(li[1]) == 0 and float(pn[1]) == 1 and not bool(p[99:198].any())
    want = _reference(imgs, masks, levels, [0, 2, 3, 4])
    for m, (proj, img, _, n) in want.items():
        lo, hi = ROW_PIX[m]
        assert float((p[lo:hi].view(SIZES[ROW_GROUP[m]]) - torch.sigmoid(_plane(levels, m))).abs().max()) < 1e-6
        assert float(pn[m]) == float(n)
        assert abs(float(lp[m]) - float(proj)) <= 1e-5 * abs(float(proj)) and abs(float(li[m]) - float(img)) <= 1e-5 * abs(float(img))


@pytest.mark.parametrize('lead', range(4))
def test_backward_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(10 + lead)
    imgs, masks, levels, idx = _inputs(rng, dev)
    p, lp, li, pn, live = _front_outputs(dev, False)
    state, nbytes = _state(lib, dev, False, 'bxi_bls_state_bytes')
    _call(lib, dev, 'front', imgs, masks, levels, *idx, M, B, W_PROJ, W_IMG, p, lp, li, pn, live, state, nbytes)
    g_p, g_lp, g_li = _rand(rng, PIX[-1]).to(dev) * 0.1, torch.from_numpy(rng.random(M).astype(np.float32)).to(dev), torch.from_numpy(rng.random(M).astype(np.float32)).to(dev)
    grads = [torch.empty_like(t) for t in levels]
    _call(lib, dev, 'backward', imgs, masks, grads, *idx, M, B, W_PROJ, W_IMG, p, g_p, g_lp, g_li, state, nbytes)
    gi = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(imgs)]
    gm = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(masks)]
    gx = [G.embed(t, (lead + k) % 4) for k, t in enumerate(idx)]
    ge = [G.embed(p, lead), G.embed(g_p, (lead + 1) % 4), G.embed(g_lp, (lead + 2) % 4), G.embed(g_li, (lead + 3) % 4), G.embed(state, lead % 2)]
    gg = [G.out(tuple(t.shape), torch.float32, dev, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(levels)]
    _call(lib, dev, 'backward', gi, gm, gg, *gx, M, B, W_PROJ, W_IMG, *ge[:4], ge[4], nbytes)
    G.check_bands(*gi, *gm, *gx, *ge, *gg)
    G.check_written(*gg)
    G.check_unchanged(*gi, *gm, *gx, *ge)
    for a, b in zip(gg, grads):
        assert G.same(a.t, b)
    assert not bool(_plane(grads, 1).any())                                  # the inert row's plane
    # against autograd through the per-row statements in fp64
    for m in (0, 2, 3, 4):
        g, (lo, hi) = ROW_GROUP[m], ROW_PIX[m]
        x = _plane(levels, m).double().cpu().clone().requires_grad_(True)
        from tests.b2m_loss_ref import box_projection_loss, levelset_loss
        T = masks[g][int(TGT_OF[m])].double().cpu()[None, None]
        pp = torch.sigmoid(x)[None, None]
        phi = torch.cat((pp, 1 - pp), 1) * T
        total = (float(g_lp[m]) * box_projection_loss(pp, T, W_PROJ) + float(g_li[m]) * W_IMG * levelset_loss(
            phi, imgs[g][int(IMG_OF[m])].double().cpu()[None] * T, T.sum((1, 2, 3)).clamp(min=1), 1.0)).sum() + (pp[0, 0] * g_p[lo:hi].double().cpu().view(SIZES[g])).sum()
        total.backward()
        got = _plane(grads, m).double().cpu()
        assert float((got - x.grad).abs().max()) <= 1e-5 * float(x.grad.abs().max()), m


@pytest.mark.parametrize('lead', range(4))
def test_high_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(20 + lead)
    imgs, masks, levels, idx = _inputs(rng, dev)
    p, lp, li, pn, live = _front_outputs(dev, False)
    state, nbytes = _state(lib, dev, False, 'bxi_bls_state_bytes')
    _call(lib, dev, 'front', imgs, masks, levels, *idx, M, B, W_PROJ, W_IMG, p, lp, li, pn, live, state, nbytes)
    y = [_rand(rng, PIX[-1]).to(dev), _rand(rng, PIX[-1]).to(dev)]
    g_loss = torch.from_numpy(rng.random(M).astype(np.float32)).to(dev)
    tgt = idx[1]

    def both(p_, y0, y1, tgt_, live_, pn_, gl_, loss_, hs_, hbytes, gp_, gy0, gy1, masks_):
        _call(lib, dev, 'high_forward', None, masks_, p_, y0, y1, tgt_, live_, pn_, M, W_HIGH, loss_, hs_, hbytes)
        _call(lib, dev, 'high_backward', None, masks_, p_, y0, y1, tgt_, live_, pn_, M, W_HIGH, hs_, hbytes, gl_, gp_, gy0, gy1)

    hstate, hbytes = _state(lib, dev, False, 'bxi_bls_high_state_bytes')
    loss, gp, gy0, gy1 = torch.empty(M, device=dev), torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
    both(p, y[0], y[1], tgt, live, pn, g_loss, loss, hstate, hbytes, gp, gy0, gy1, masks)
    gm = [G.embed(t, (lead + k) % 4, G.plane_band(*t.shape[-2:])) for k, t in enumerate(masks)]
    e = [G.embed(p, lead), G.embed(y[0], (lead + 1) % 4), G.embed(y[1], (lead + 2) % 4), G.embed(tgt, lead), G.embed(live, (lead + 3) % 4),
         G.embed(pn, (lead + 1) % 4), G.embed(g_loss, (lead + 2) % 4)]
    gloss = G.out(M, torch.float32, dev, (lead + 1) % 4)
    ghs, _ = _state(lib, dev, True, 'bxi_bls_high_state_bytes', lead)
    go = [G.out(PIX[-1], torch.float32, dev, (lead + k) % 4) for k in range(3)]
    both(*e, gloss, ghs, hbytes, *go, gm)
    G.check_bands(*gm, *e, gloss, ghs, *go)
    G.check_written(gloss, ghs, *go)
    G.check_unchanged(*gm, *e)
    assert G.same(gloss.t, loss) and G.same(go[0].t, gp) and G.same(go[1].t, gy0) and G.same(go[2].t, gy1)
    assert float(loss[1]) == 0.0 and not bool(gp[99:198].any()) and not bool(gy0[99:198].any()) and not bool(gy1[99:198].any())
    from tests.b2m_loss_ref import levelset_loss
    for m in (0, 2, 3, 4):
        g, (lo, hi) = ROW_GROUP[m], ROW_PIX[m]
        T = masks[g][int(TGT_OF[m])].double().cpu()[None, None]
        pp = p[lo:hi].double().cpu().view(1, 1, *SIZES[g]).clone().requires_grad_(True)
        yy = torch.stack([y[0][lo:hi], y[1][lo:hi]]).double().cpu().view(1, 2, *SIZES[g]).clone().requires_grad_(True)
        want = levelset_loss(torch.cat((pp, 1 - pp), 1) * T, yy * T, T.sum((1, 2, 3)).clamp(min=1), 1.0) * W_HIGH
        (want * float(g_loss[m])).sum().backward()
        assert abs(float(loss[m]) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
        assert float((gp[lo:hi].double().cpu() - pp.grad.reshape(-1)).abs().max()) <= 1e-5 * float(pp.grad.abs().max())
        for k, gy in enumerate((gy0, gy1)):
            assert float((gy[lo:hi].double().cpu() - yy.grad[0, k].reshape(-1)).abs().max()) <= 1e-5 * float(yy.grad.abs().max())


def test_status_codes(dev):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(40)
    imgs, masks, levels, idx = _inputs(rng, dev)
    outs = _front_outputs(dev, False)
    state, nbytes = _state(lib, dev, False, 'bxi_bls_state_bytes')
    st = G.stream(dev)

    def front(groups, n_groups, level_rows=LEVEL_ROWS, level_group=LEVEL_GROUP, L=3, lv=levels, m=M, row_src=idx[0], state_=state, nb=nbytes):
        return lib.bxi_bls_front_f32(groups, n_groups, (ctypes.c_void_p * len(lv))(*[G.ptr(t) for t in lv]), _lib.int_array(level_rows), _lib.int_array(level_group), L,
                                     G.ptr(row_src), G.ptr(idx[1]), G.ptr(idx[2]), m, B, W_PROJ, W_IMG, *[G.ptr(o) for o in outs], G.ptr(state_), nb, st)

    good = _groups(imgs, masks)
    assert front(good, 2) == 0
    name = lambda rc: _lib.STATUS.get(rc, rc)
    five = (_lib.BlsGroup * 5)(*[good[0]] * 5)
    assert name(front(five, 5)) == 'BXI_ERR_UNSUPPORTED'                                     # too many groups
    assert name(front(good, 0)) == 'BXI_ERR_BAD_SHAPE'
    assert name(front(good, 2, L=9)) == 'BXI_ERR_UNSUPPORTED'                                # too many levels
    assert name(front(good, 2, level_rows=[2, 2, 2])) == 'BXI_ERR_BAD_SHAPE'                 # the planes of a group's levels are not its rows
    assert name(front(good, 2, m=M - 1)) == 'BXI_ERR_BAD_SHAPE'
    assert name(front(good, 2, level_group=[0, 2, 0])) == 'BXI_ERR_BAD_SHAPE'
    bad = _groups(imgs, masks)
    bad[1].h = 0
    assert name(front(bad, 2)) == 'BXI_ERR_BAD_SHAPE' and lib.bxi_bls_state_bytes(bad, 2) == 0
    bad = _groups(imgs, masks)
    bad[0].w = _lib.BLS_MAX_W + 1
    assert name(front(bad, 2)) == 'BXI_ERR_UNSUPPORTED' and lib.bxi_bls_high_state_bytes(bad, 2) == 0
    bad = _groups(imgs, masks)
    bad[0].img = None
    assert name(front(bad, 2)) == 'BXI_ERR_NULL_POINTER'
    assert name(front(None, 2)) == 'BXI_ERR_NULL_POINTER'
    assert name(front(good, 2, row_src=None)) == 'BXI_ERR_NULL_POINTER'
    assert name(front(good, 2, lv=[levels[0], None, levels[2]])) == 'BXI_ERR_NULL_POINTER'
    assert name(front(good, 2, state_=None)) == 'BXI_ERR_WORKSPACE' and name(front(good, 2, nb=nbytes - 8)) == 'BXI_ERR_WORKSPACE'
    assert name(lib.bxi_bls_high_forward_f32(good, 2, None, None, None, None, None, None, M, W_HIGH, None, None, 0, st)) == 'BXI_ERR_NULL_POINTER'
    assert name(lib.bxi_bls_high_backward_f32(good, 2, G.ptr(outs[0]), G.ptr(outs[0]), G.ptr(outs[0]), G.ptr(idx[1]), G.ptr(outs[4]), G.ptr(outs[3]), M, W_HIGH,
                                              None, 0, G.ptr(outs[1]), G.ptr(outs[0]), G.ptr(outs[0]), G.ptr(outs[0]), st)) == 'BXI_ERR_WORKSPACE'
    assert name(lib.bxi_bls_backward_f32(good, 2, _lib.ptr_array([G.ptr(t) for t in levels]), _lib.int_array(LEVEL_ROWS), _lib.int_array(LEVEL_GROUP), 3,
                                         G.ptr(idx[0]), G.ptr(idx[1]), G.ptr(idx[2]), M, B, W_PROJ, W_IMG, G.ptr(outs[0]), None, G.ptr(outs[1]),
                                         G.ptr(outs[2]), G.ptr(state), nbytes, st)) == 'BXI_ERR_NULL_POINTER'
    empty = _groups(imgs, masks)
    empty[0].rows = empty[1].rows = 0                                                        # M == 0 is a no-op
    assert front(empty, 2, level_rows=[0, 0, 0], m=0) == 0
