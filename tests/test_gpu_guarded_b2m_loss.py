"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_b2m.h on misaligned views inside poisoned bands (tests/guarded.py).

Every float input starts 4, 8 or 12 bytes off a 16-byte boundary (or on one) between bands of NaN, every index array between bands of
-1; outputs, ``state`` and the workspace are exactly as large as the call needs and pre-filled with the 'nobody wrote this' pattern.
Afterwards the bands are intact, every element of every output is written (inert rows and unmatched planes included: zeros), the inputs
are unchanged, and the results are bit-identical to the same call on plain tensors.  One row is inert (index -1) in every call."""
import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_b2m.py checks the table against _lib.B2M_SIGNATURES)
GUARDED = {
    'bxi_b2m_scores_f32': 'test_scores_guarded',
    'bxi_b2m_scores_backward_f32': 'test_scores_backward_guarded',
    'bxi_b2m_levelset_forward_f32': 'test_levelset_guarded',
    'bxi_b2m_levelset_backward_f32': 'test_levelset_guarded',
    'bxi_b2m_lcm_refine_f32': 'test_lcm_refine_guarded',
}
L, PLANES, M, GN, B = 2, 6, 5, 3, 2
ROW_PLANE = np.array([7, 0, -1, 11, 4], np.int32)        # l * PLANES + plane; row 2 is inert
TGT_OF = np.array([2, 0, -1, 1, 0], np.int32)
IMG_OF = np.array([1, 0, -1, 1, 0], np.int32)


def _call(lib, dev, entry, *a):
    from boxinstseg_amd import _lib
    a = [G.ptr(x) if isinstance(x, (G.Guarded, torch.Tensor)) or x is None else x for x in a]
    if entry == 'scores':
        ptrs = _lib.ptr_array(a[0])
        rc = lib.bxi_b2m_scores_f32(ptrs, *a[1:], G.stream(dev))
    elif entry == 'scores_backward':
        rc = lib.bxi_b2m_scores_backward_f32(*a, G.stream(dev))
    elif entry == 'levelset_forward':
        rc = lib.bxi_b2m_levelset_forward_f32(*a, G.stream(dev))
    elif entry == 'levelset_backward':
        rc = lib.bxi_b2m_levelset_backward_f32(*a, G.stream(dev))
    else:
        rc = lib.bxi_b2m_lcm_refine_f32(*a, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize('h,w,sh,sw', [(9, 11, 7, 6), (5, 6, 12, 9)], ids=['down', 'up'])
@pytest.mark.parametrize('lead', range(4))
def test_scores_guarded(dev, lead, h, w, sh, sw):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(lead)
    layers = [_rand(rng, PLANES, h, w).to(dev) for _ in range(L)]
    rp = torch.from_numpy(ROW_PLANE).to(dev)
    p, ps = torch.empty((M, h, w), device=dev), torch.empty((M, sh, sw), device=dev)
    _call(lib, dev, 'scores', [t.data_ptr() for t in layers], L, PLANES, h, w, rp, M, sh, sw, p, ps)
    gl = [G.embed(t, (lead + i) % 4, G.plane_band(h, w)) for i, t in enumerate(layers)]
    grp = G.embed(rp, lead % 4)
    gp, gps = G.out((M, h, w), torch.float32, dev, (lead + 1) % 4, G.plane_band(h, w)), G.out((M, sh, sw), torch.float32, dev, (lead + 2) % 4)
    _call(lib, dev, 'scores', [g.ptr() for g in gl], L, PLANES, h, w, grp, M, sh, sw, gp, gps)
    G.check_bands(*gl, grp, gp, gps)
    G.check_written(gp, gps)
    G.check_unchanged(*gl, grp)
    assert G.same(gp.t, p) and G.same(gps.t, ps)
    assert not bool(p[2].any()) and not bool(ps[2].any())                                   # the inert row
    assert G.same(p[0], torch.sigmoid(layers[1][1])) or float((p[0] - torch.sigmoid(layers[1][1])).abs().max()) < 1e-6
    want = torch.nn.functional.interpolate(p[:, None], size=(sh, sw), mode='bilinear', align_corners=False)[:, 0]
    assert float((ps - want).abs().max()) < 1e-5


@pytest.mark.parametrize('h,w,sh,sw', [(9, 11, 7, 6), (5, 6, 12, 9)], ids=['down', 'up'])
@pytest.mark.parametrize('lead', range(4))
def test_scores_backward_guarded(dev, lead, h, w, sh, sw):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(10 + lead)
    g_p, g_ps, p = _rand(rng, M, h, w).to(dev), _rand(rng, M, sh, sw).to(dev), torch.sigmoid(_rand(rng, M, h, w)).to(dev)
    plane_row = torch.from_numpy(np.array([1, -1, 4, -1, 0, 3], np.int32)).to(dev)          # planes 1, 3 unmatched; row 2 has no plane
    out = torch.empty((PLANES, h, w), device=dev)
    _call(lib, dev, 'scores_backward', g_p, g_ps, p, plane_row, PLANES, M, h, w, sh, sw, out)
    band = G.plane_band(h, w)
    ggp, ggs, gpp = G.embed(g_p, lead, band), G.embed(g_ps, (lead + 1) % 4, band), G.embed(p, (lead + 2) % 4, band)
    gpr = G.embed(plane_row, (lead + 3) % 4)
    gout = G.out((PLANES, h, w), torch.float32, dev, (lead + 1) % 4, band)
    _call(lib, dev, 'scores_backward', ggp, ggs, gpp, gpr, PLANES, M, h, w, sh, sw, gout)
    G.check_bands(ggp, ggs, gpp, gpr, gout)
    G.check_written(gout)
    G.check_unchanged(ggp, ggs, gpp, gpr)
    assert G.same(gout.t, out) and not bool(out[1].any()) and not bool(out[3].any())
    # the adjoint of the resize, by autograd on the same resize
    x = p.clone().requires_grad_(True)
    y = torch.nn.functional.interpolate(x[:, None], size=(sh, sw), mode='bilinear', align_corners=False)[:, 0]
    ((y * g_ps).sum() + (x * g_p).sum()).backward()
    for plane, row in ((0, 1), (2, 4), (4, 0), (5, 3)):
        want = x.grad[row] * p[row] * (1 - p[row])
        assert float((out[plane] - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize('shared,C', [(1, 3), (0, 2)], ids=['image', 'own'])
@pytest.mark.parametrize('lead', range(4))
def test_levelset_guarded(dev, lead, shared, C):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(20 + lead)
    h, w = 9, 11
    p = torch.sigmoid(_rand(rng, M, h, w)).to(dev)
    T = torch.from_numpy((rng.random((GN, h, w)) > 0.5).astype(np.float32) * rng.random((GN, h, w)).astype(np.float32)).to(dev)
    target = _rand(rng, B if shared else M, C, h, w).to(dev)
    tgt, img = torch.from_numpy(TGT_OF).to(dev), torch.from_numpy(IMG_OF).to(dev)
    pn, gl = T.sum((1, 2)).clamp(min=1), torch.from_numpy(rng.random(M).astype(np.float32)).to(dev)
    nstate = lib.bxi_b2m_levelset_state_bytes(M, C) // 8
    assert nstate == M * (2 + 4 * C) * 9

    def both(p_, T_, target_, tgt_, img_, pn_, gl_, loss_, state_, gp_, gt_):
        _call(lib, dev, 'levelset_forward', p_, T_, target_, shared, tgt_, img_, pn_, M, GN, B, C, h, w, 1.5, loss_, state_)
        _call(lib, dev, 'levelset_backward', p_, T_, target_, shared, tgt_, img_, pn_, M, GN, B, C, h, w, 1.5, state_, gl_, gp_, gt_)

    loss, state = torch.empty(M, device=dev), torch.empty(nstate, dtype=torch.float64, device=dev)
    gp, gt = torch.empty_like(p), (None if shared else torch.empty_like(target))
    both(p, T, target, tgt, img, pn, gl, loss, state, gp, gt)
    band = G.plane_band(h, w)
    e = [G.embed(p, lead, band), G.embed(T, (lead + 1) % 4, band), G.embed(target, (lead + 2) % 4, band), G.embed(tgt, lead), G.embed(img, (lead + 1) % 4),
         G.embed(pn, (lead + 3) % 4), G.embed(gl, (lead + 2) % 4)]
    gloss, gstate = G.out(M, torch.float32, dev, (lead + 1) % 4), G.out(nstate, torch.float64, dev, lead % 2)
    ggp = G.out((M, h, w), torch.float32, dev, (lead + 3) % 4, band)
    ggt = None if shared else G.out((M, C, h, w), torch.float32, dev, lead, band)
    both(*e, gloss, gstate, ggp, ggt)
    outs = [gloss, gstate, ggp] + ([] if shared else [ggt])
    G.check_bands(*e, *outs)
    G.check_written(*outs)
    G.check_unchanged(*e)
    assert G.same(gloss.t, loss) and G.same(ggp.t, gp) and (shared or G.same(ggt.t, gt))
    assert float(loss[2]) == 0.0 and not bool(gp[2].any()) and (shared or not bool(gt[2].any()))
    # against the existing kernels on the materialised operands
    from boxinstseg_amd import LevelsetLoss
    live = [0, 1, 3, 4]
    pl = p[live].clone().requires_grad_(True)
    Tl = T[torch.from_numpy(TGT_OF[live]).long().to(dev)][:, None]
    tl = (target[torch.from_numpy(IMG_OF[live]).long().to(dev)] if shared else target[live]).clone().requires_grad_(True)
    want = LevelsetLoss(1.5)(torch.cat((pl[:, None], 1 - pl[:, None]), 1) * Tl, tl * Tl, pn[torch.from_numpy(TGT_OF[live]).long().to(dev)])
    (want * gl[live]).sum().backward()
    want = want.detach()
    assert float((loss[live] - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-12)
    assert float((gp[live] - pl.grad).abs().max()) <= 1e-5 * float(pl.grad.abs().max())
    if not shared:
        assert float((gt[live] - tl.grad).abs().max()) <= 1e-5 * float(tl.grad.abs().max())


@pytest.mark.parametrize('transpose', [0, 1])
@pytest.mark.parametrize('h,w', [(12, 12), (9, 11)])
@pytest.mark.parametrize('lead', range(4))
def test_lcm_refine_guarded(dev, lead, h, w, transpose):
    from boxinstseg_amd import _lib
    from boxinstseg_amd.levelset import _refine
    lib = _lib.load()
    rng = np.random.default_rng(30 + lead)
    aff = torch.softmax(_rand(rng, B, 8, h, w), 1).contiguous().to(dev)
    phi = _rand(rng, M, h, w).to(dev)
    img = torch.from_numpy(IMG_OF).to(dev)
    nws = lib.bxi_lcm_workspace_bytes(M, h, w)
    out = torch.empty_like(phi)
    _call(lib, dev, 'lcm_refine', aff, phi, img, B, M, h, w, 2, 10, transpose, out, torch.empty(nws, dtype=torch.uint8, device=dev), nws)
    band = G.plane_band(h, w, 2)
    ga, gphi, gi = G.embed(aff, lead, band), G.embed(phi, (lead + 1) % 4, band), G.embed(img, (lead + 2) % 4)
    gout, ws = G.out((M, h, w), torch.float32, dev, (lead + 3) % 4, band), G.out(nws // 4, torch.int32, dev, 0)
    _call(lib, dev, 'lcm_refine', ga, gphi, gi, B, M, h, w, 2, 10, transpose, gout, ws, nws)
    G.check_bands(ga, gphi, gi, gout, ws)
    G.check_written(gout)
    G.check_unchanged(ga, gphi, gi)
    assert G.same(gout.t, out) and not bool(out[2].any())
    live = [0, 1, 3, 4]
    want = _refine(aff[torch.from_numpy(IMG_OF[live]).long().to(dev)].contiguous(), phi[live].contiguous(), 2, 10, transpose)
    assert G.same(out[live], want)
