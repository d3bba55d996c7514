"""GPU: the kernels of csrc/box2mask_loss.hip through the C ABI at the slice, trip, block, chunk and resize edges of tests/b2m_edges.py,
which tests/test_host_b2m_edges.py shows to be what they claim.  The referees (torch's own fp64 resize and its autograd; the level-set
statements in long double from exact sums), the exact inputs and the derivation of every bound stand in tests/b2m_edges.py.

Every output and ``state`` is a guarded, pattern-filled tensor (tests/guarded.py): afterwards the bands are intact and every element is
written.  Every entry point runs at least twice and the results are bit-identical.  No element is left out of a comparison: where a
bound is 0 the error must be 0.  Each test prints the largest share of its bound that it reached.  What each group is the first to reach
at the C ABI:

    scores forward    b2m_scores_kernel<true> (float4), both paths on the same shape, 1024 and 1025 work items per row, an axis of one
                      element, x8 up-scaling with every output clamped to tap 0, sixteen layer tensors, row_plane beyond the table
    scores backward   more than one block per plane, windows of 1 to 20 candidates per axis, elements that no small-grid pixel reads,
                      unmatched planes first / in the middle / last, a plane_row beyond M
    level set         1 to 8 non-empty slices, a slice of exactly 512 and of 516 (u = 1 live in four lanes), one full trip and a second
                      trip of four pixels, backward blocks of 255 .. 1025 pixels, C = 1 and 4, 64 and 65 rows in the finish kernel,
                      an inert row by tgt_of and by img_of, as -1 and as an index beyond the range
"""
import numpy as np
import pytest
import torch

from tests import b2m_edges as E
from tests import guarded as G

pytestmark = pytest.mark.gpu


def _lib():
    from boxinstseg_amd import _lib as L
    return L


def _scores(dev, layers, planes, rp, M, h, w, sh, sw, lead_p=0, lead_layer=None):
    """One guarded call of bxi_b2m_scores_f32: (p, p_small).  ``lead_p``: p starts that many floats off a 16-byte boundary;
    ``lead_layer`` (layer, lead): that layer tensor does."""
    L = _lib()
    band = G.plane_band(h, w)
    ptrs, keep = [], []
    for i, t in enumerate(layers):
        if lead_layer is not None and lead_layer[0] == i:
            g = G.embed(t, lead_layer[1], band)
            keep.append(g)
            ptrs.append(g.ptr())
        else:
            assert t.data_ptr() % 16 == 0
            ptrs.append(t.data_ptr())
    p, ps = G.out((M, h, w), torch.float32, dev, lead_p, band), G.out((M, sh, sw), torch.float32, dev, 0, G.plane_band(sh, sw))
    G.ok(L.load().bxi_b2m_scores_f32(L.ptr_array(ptrs), len(layers), planes, h, w, rp.data_ptr(), M, sh, sw, p.ptr(), ps.ptr(), G.stream(dev)))
    G.check_bands(p, ps, *keep)
    G.check_written(p, ps)
    G.check_unchanged(*keep)
    return p.t, ps.t


def _compare_scores(name, c, p, ps, dyadic):
    want_p = c['p'].float()
    assert G.same(p.cpu(), want_p), f'{name}: p is not exactly 0 / 0.5 / 1'
    if dyadic:
        err = float((ps.cpu().double() - c['p_small']).abs().max())
        print(f'{name}: p_small exact, largest error {err:.3e}')
        assert G.same(ps.cpu(), c['p_small'].float()) and err == 0.0
    else:
        err = float((ps.cpu().double() - c['p_small']).abs().max())
        print(f'{name}: p_small error {err:.3e}, bound {E.FWD_BOUND:.3e}, share {err / E.FWD_BOUND:.3f}')
        assert err <= E.FWD_BOUND
    assert not bool(ps[2].any())                                            # the inert row: exact zeros


@pytest.mark.parametrize('name', list(E.SCORES))
def test_scores_forward_exact(dev, name):
    (h, w, sh, sw), claim = E.SCORES[name]
    c = E.scores_exact(name)
    layers, rp = [t.to(dev) for t in c['layers']], c['row_plane'].to(dev)
    first = _scores(dev, layers, E.S_PLANES, rp, E.S_M, h, w, sh, sw)
    again = _scores(dev, layers, E.S_PLANES, rp, E.S_M, h, w, sh, sw)
    assert G.same(first[0], again[0]) and G.same(first[1], again[1])
    _compare_scores(name + (' (float4)' if claim['vec'] else ' (scalar)'), c, *first, claim['dyadic'])
    if claim['vec']:                                                        # the same shape on the scalar path: p off the 16-byte boundary
        other = _scores(dev, layers, E.S_PLANES, rp, E.S_M, h, w, sh, sw, lead_p=1)
        _compare_scores(name + ' (scalar, forced)', c, *other, claim['dyadic'])
        assert G.same(other[0], first[0]) and G.same(other[1], first[1])


def test_scores_layer_table(dev):
    h, w, sh, sw = E.TABLE_SHAPE
    c = E.scores_table()
    layers, rp = [t.to(dev) for t in c['layers']], c['row_plane'].to(dev)
    M = len(E.TABLE_ROW_PLANE)
    first = _scores(dev, layers, E.TABLE_PLANES, rp, M, h, w, sh, sw)
    again = _scores(dev, layers, E.TABLE_PLANES, rp, M, h, w, sh, sw, lead_p=2)
    assert G.same(first[0], again[0]) and G.same(first[1], again[1])
    assert G.same(first[0].cpu(), c['p'].float()) and G.same(first[1].cpu(), c['p_small'].float())
    for m, lp in enumerate(E.TABLE_LAYER_PLANE):
        assert lp is not None or (not bool(first[0][m].any()) and not bool(first[1][m].any()))
    L = _lib()
    ptrs = L.ptr_array([t.data_ptr() for t in layers] + [layers[0].data_ptr()])
    out = torch.empty((M, h, w), device=dev), torch.empty((M, sh, sw), device=dev)
    rc = L.load().bxi_b2m_scores_f32(ptrs, E.MAX_LAYERS + 1, E.TABLE_PLANES, h, w, rp.data_ptr(), M, sh, sw, out[0].data_ptr(), out[1].data_ptr(),
                                     G.stream(dev))
    assert L.STATUS.get(rc, rc) == 'BXI_ERR_UNSUPPORTED'
    # a small grid of more than MAX_UP times an axis of one element: refused, nothing launched
    rc = L.load().bxi_b2m_scores_f32(ptrs, 2, E.TABLE_PLANES, 1, 36, rp.data_ptr(), M, 24, 24, out[0].data_ptr(), out[1].data_ptr(), G.stream(dev))
    assert L.STATUS.get(rc, rc) == 'BXI_ERR_UNSUPPORTED'


@pytest.mark.parametrize('name', E.SCORES_RANDOM)
def test_scores_forward_random(dev, name):
    """Random logits: p against the fp64 sigmoid, p_small against torch's fp64 resize of the kernel's own p, and the float4 path against
    the scalar path, forced by a layer tensor or p off the 16-byte boundary, bit for bit."""
    (h, w, sh, sw), claim = E.SCORES[name]
    layers = [t.to(dev) for t in E.scores_random(name)]
    rp = torch.tensor(E.S_ROW_PLANE, dtype=torch.int32, device=dev)
    p, ps = _scores(dev, layers, E.S_PLANES, rp, E.S_M, h, w, sh, sw)
    want = torch.zeros((E.S_M, h, w), dtype=torch.float64)
    for m, r in enumerate(E.S_ROW_PLANE):
        if r >= 0:
            want[m] = torch.sigmoid(E.scores_random(name)[r // E.S_PLANES][r % E.S_PLANES].double())
    err_p = float((p.cpu().double() - want).abs().max())
    err_s = float((ps.cpu().double() - E.resize64(p.cpu(), (sh, sw))).abs().max())
    print(f'{name}: p error {err_p:.3e} (bound {E.SIGMOID_TOL:.1e}); p_small error {err_s:.3e}, bound {E.FWD_BOUND:.3e}, share {err_s / E.FWD_BOUND:.3f}')
    assert err_p <= E.SIGMOID_TOL and err_s <= E.FWD_BOUND
    assert not bool(p[2].any()) and not bool(ps[2].any())
    runs = [dict(lead_layer=(0, 1)), dict(lead_layer=(1, 2)), dict(lead_p=3)] if claim['vec'] else [dict()]
    for kw in runs:
        q, qs = _scores(dev, layers, E.S_PLANES, rp, E.S_M, h, w, sh, sw, **kw)
        assert G.same(q, p) and G.same(qs, ps), f'{name}: {kw} differs from the first call'


@pytest.mark.parametrize('name', list(E.SCORES))
def test_scores_backward(dev, name):
    (h, w, sh, sw), claim = E.SCORES[name]
    c = E.scores_bwd(name)
    L = _lib()
    g_p, g_ps, p = c['g_p'].to(dev), c['g_ps'].to(dev), c['p'].to(dev)
    outs = []
    for rows in (E.B_PLANE_ROW, E.B_PLANE_ROW_BEYOND, E.B_PLANE_ROW):
        pr = torch.tensor(rows, dtype=torch.int32, device=dev)
        out = G.out((E.B_PLANES, h, w), torch.float32, dev, len(outs), G.plane_band(h, w))
        G.ok(L.load().bxi_b2m_scores_backward_f32(g_p.data_ptr(), g_ps.data_ptr(), p.data_ptr(), pr.data_ptr(), E.B_PLANES, E.S_M, h, w, sh, sw,
                                                  out.ptr(), G.stream(dev)))
        G.check_bands(out)
        G.check_written(out)
        outs.append(out.t)
    assert G.same(outs[1], outs[0]) and G.same(outs[2], outs[0])
    got = outs[0].cpu()
    for plane, row in enumerate(E.B_PLANE_ROW):
        assert row >= 0 or G.same(got[plane], torch.zeros(h, w))           # unmatched planes: +0 everywhere
    err = (got.double() - c['want']).abs().numpy()
    share = E.share(err, c['bound'].numpy())
    print(f'{name}: backward error {float(err.max()):.3e}, bound at most {float(c["bound"].max()):.3e}, share {share:.3f}'
          + (' (exact)' if claim['dyadic'] else ''))
    assert share <= 1.0


def _levelset(dev, c, tgt, img):
    """One guarded forward + backward of the level-set pair: (loss, g_p, g_target or None)."""
    L = _lib()
    lib = L.load()
    h, w, shared, C, M = c['h'], c['w'], c['shared'], c['C'], c['M']
    p, T, target, pn, gl = (c[k].to(dev) for k in ('p', 'T', 'target', 'pixel_num', 'g_loss'))
    t_of = torch.from_numpy(tgt).to(dev)
    i_of = None if img is None else torch.from_numpy(img).to(dev)
    nstate = lib.bxi_b2m_levelset_state_bytes(M, C) // 8
    assert nstate == M * (2 + 4 * C) * (1 + E.SLICES)
    band = G.plane_band(h, w)
    loss, state = G.out(M, torch.float32, dev, 1), G.out(nstate, torch.float64, dev, 1)
    gp = G.out((M, h, w), torch.float32, dev, 3, band)
    gt = None if shared else G.out((M, C, h, w), torch.float32, dev, 1, band)
    G.ok(lib.bxi_b2m_levelset_forward_f32(p.data_ptr(), T.data_ptr(), target.data_ptr(), shared, t_of.data_ptr(), G.ptr(i_of), pn.data_ptr(), M,
                                          E.LS_G, E.LS_B, C, h, w, c['weight'], loss.ptr(), state.ptr(), G.stream(dev)))
    G.ok(lib.bxi_b2m_levelset_backward_f32(p.data_ptr(), T.data_ptr(), target.data_ptr(), shared, t_of.data_ptr(), G.ptr(i_of), pn.data_ptr(), M,
                                           E.LS_G, E.LS_B, C, h, w, c['weight'], state.ptr(), gl.data_ptr(), gp.ptr(), G.ptr(gt), G.stream(dev)))
    outs = [loss, state, gp] + ([] if shared else [gt])
    G.check_bands(*outs)
    G.check_written(*outs)
    return loss.t, gp.t, None if shared else gt.t


@pytest.mark.parametrize('case', E.LS_CASES, ids=E.ls_id)
def test_levelset(dev, case):
    h, w, shared, C, M = case
    c, r = E.ls_case(*case), E.ls_ref(*case)
    runs = [_levelset(dev, c, tgt, img) for tgt, img in E.inert_variants(c)]
    for other in runs[1:]:
        assert G.same(other[0], runs[0][0]) and G.same(other[1], runs[0][1]) and (shared or G.same(other[2], runs[0][2]))
    loss, gp, gt = (None if t is None else t.cpu() for t in runs[0])
    k = c['inert']
    zero = torch.zeros(h, w)
    assert G.same(loss[k], torch.zeros(())) and G.same(gp[k], zero) and (shared or all(G.same(gt[k, ch], zero) for ch in range(C)))
    want, bound = E.ls_loss_bound(r)
    err = np.abs(loss.numpy().astype(np.longdouble) - want.astype(np.longdouble))
    line = f'{E.ls_id(case)}: loss share {E.share(err, bound):.3f} of {float(bound.max()):.3e}'
    s_loss = E.share(err, bound)
    s_gp = E.share(np.abs(gp.numpy().astype(np.longdouble) - r['g_p']), E.grad_bound(r, 'g_p'))
    line += f'; g_p share {s_gp:.3f}'
    s_gt = 0.0
    if not shared:
        s_gt = E.share(np.abs(gt.numpy().astype(np.longdouble) - r['g_target']), E.grad_bound(r, 'g_target'))
        line += f'; g_target share {s_gt:.3f}'
    print(line)
    assert s_loss <= 1.0 and s_gp <= 1.0 and s_gt <= 1.0
