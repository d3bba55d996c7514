"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_dbx.h on misaligned views inside poisoned bands (tests/guarded.py).

Every float input starts 4, 8 or 12 bytes off a 16-byte boundary (or on one) between bands of NaN, the uint8 targets at any byte, the index
arrays between bands of -1; outputs and the workspace are exactly as large as the call needs and pre-filled with the 'nobody wrote this'
pattern.  Afterwards the bands are intact, every element of every output and every word of the workspace is written, the inputs are
unchanged, and the results are bit-identical to the same calls on plain tensors.  One row is dead, one level has a null iiu pointer."""
import numpy as np
import pytest
import torch

from tests import dbx_loss_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_dbx.py checks the table against _lib.DBX_SIGNATURES)
GUARDED = {
    'bxi_dbx_prepare_f32': 'test_forward_chain_guarded',
    'bxi_dbx_steps_f32': 'test_forward_chain_guarded',
    'bxi_dbx_dice_forward_f32': 'test_forward_chain_guarded',
    'bxi_dbx_dice_backward_f32': 'test_forward_chain_guarded',
    'bxi_dbx_unpack_u8': 'test_forward_chain_guarded',
    'bxi_dbx_means_f32': 'test_means_guarded',
    'bxi_dbx_means_backward_f32': 'test_means_guarded',
}


def _call(lib, dev, entry, *a):
    from boxinstseg_amd import _lib
    a = [G.ptr(x) if isinstance(x, (G.Guarded, torch.Tensor)) or x is None else x for x in a]
    if entry == 'prepare':
        rc = lib.bxi_dbx_prepare_f32(*a, G.stream(dev))
    elif entry == 'steps':
        rc = lib.bxi_dbx_steps_f32(*a, G.stream(dev))
    elif entry == 'dice_forward':
        rc = lib.bxi_dbx_dice_forward_f32(*a, G.stream(dev))
    elif entry == 'dice_backward':
        rc = lib.bxi_dbx_dice_backward_f32(*a, G.stream(dev))
    elif entry == 'unpack':
        rc = lib.bxi_dbx_unpack_u8(*a, G.stream(dev))
    elif entry == 'means':
        rc = lib.bxi_dbx_means_f32(*a, G.stream(dev))
    else:
        rc = lib.bxi_dbx_means_backward_f32(*a, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


@pytest.mark.parametrize('name,legs', [('level_gap', 2), ('dead', 2), ('w129', 1)])
@pytest.mark.parametrize('lead', range(4))
def test_forward_chain_guarded(dev, lead, name, legs):
    import boxinstseg_amd as B
    from boxinstseg_amd import _lib
    lib = _lib.load()
    d = R.case(name)
    Rr, H, W = d['R'], d['H'], d['W']
    s, t = torch.tensor(d['s'], device=dev), torch.tensor(d['t'], device=dev)
    target, img = torch.tensor(d['target'], device=dev), torch.tensor(d['img'], device=dev)
    kernel = B.meanfield_kernel(torch.tensor(d['feats'], device=dev), d['ks'], 2.0, 0.5, 30.0)
    iiu = [None if x is None else torch.tensor(x, device=dev) for x in d['inter']]
    g_rows = torch.from_numpy(np.random.default_rng(lead).uniform(0.5, 2.0, (legs, Rr)).astype(np.float32)).to(dev)
    nws = lib.bxi_dbx_workspace_bytes(Rr, H, W, legs)
    assert nws % 8 == 0 and nws > 0

    def chain(s, t, target, img, kernel, iiu, g_rows, live, n_live, ws, nws, loss, sums, g_s, planes):
        from boxinstseg_amd import _lib
        Rr, H, W, it = d['R'], d['H'], d['W'], d['iters']
        ptrs = _lib.ptr_array([0 if x is None else G.ptr(x) for x in iiu])
        firsts = _lib.int_array(np.cumsum([0] + d['level_rows'][:-1]))
        _call(lib, dev, 'prepare', s, t, target, Rr, H, W, legs, live, n_live, ws, nws)
        _call(lib, dev, 'steps', kernel, 2, H, W, d['ks'], img, Rr, it, d['base'], R.GAMMA, legs, ptrs, firsts, len(d['level_rows']), ws, nws)
        _call(lib, dev, 'dice_forward', s, Rr, H, W, legs, it, R.GAMMA, ws, nws, loss, sums)
        _call(lib, dev, 'dice_backward', s, Rr, H, W, legs, it, R.GAMMA, ws, nws, sums, g_rows, g_s)
        for which, out in enumerate(planes):
            _call(lib, dev, 'unpack', ws, nws, which, it, Rr, H, W, legs, out)

    def outs():
        return (torch.empty(Rr, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev), torch.empty(nws // 8, dtype=torch.int64, device=dev),
                torch.empty((legs, Rr), device=dev), torch.empty((legs, Rr, 2), dtype=torch.float64, device=dev), torch.empty((Rr, H, W), device=dev),
                [torch.empty((Rr, H, W), dtype=torch.uint8, device=dev) for _ in range(2 + legs)])
    live, n_live, ws, loss, sums, g_s, planes = outs()
    chain(s, t, target, img, kernel, iiu, g_rows, live, n_live, ws, nws, loss, sums, g_s, planes)
    band = G.plane_band(H, W, 2)
    ins = [G.embed(s, lead, band), G.embed(t, (lead + 1) % 4, band), G.embed(target, (5 * lead + 3) % 16, band), G.embed(img, lead % 2),
           G.embed(kernel, (lead + 2) % 4, band), G.embed(g_rows, (lead + 3) % 4)]
    giiu = [None if x is None else G.embed(x, (lead + i) % 4, band) for i, x in enumerate(iiu)]
    glive, gn = G.out(Rr, torch.int32, dev, (lead + 1) % 4), G.out(1, torch.int32, dev, lead % 4)
    gws = G.out(nws // 8, torch.int64, dev, lead % 2)
    gloss, gsums = G.out((legs, Rr), torch.float32, dev, (lead + 2) % 4), G.out((legs, Rr, 2), torch.float64, dev, lead % 2)
    gg = G.out((Rr, H, W), torch.float32, dev, (lead + 3) % 4, band)
    gplanes = [G.out((Rr, H, W), torch.uint8, dev, (3 * lead + i) % 16, band) for i in range(2 + legs)]
    chain(ins[0], ins[1], ins[2], ins[3], ins[4], giiu, ins[5], glive, gn, gws, nws, gloss, gsums, gg, gplanes)
    every_in = ins + [x for x in giiu if x is not None]
    every_out = [glive, gn, gws, gloss, gsums, gg] + gplanes
    G.check_bands(*every_in, *every_out)
    G.check_written(*every_out)
    G.check_unchanged(*every_in)
    assert torch.equal(glive.t, live) and torch.equal(gn.t, n_live) and G.same(gloss.t, loss) and G.same(gsums.t, sums) and G.same(gg.t, g_s)
    assert torch.equal(gws.t, ws)
    for a, b in zip(gplanes, planes):
        assert torch.equal(a.t, b)
    assert torch.equal(planes[0], (target != 0).to(torch.uint8)) and torch.equal(planes[1], R.enlarged_of(target))
    assert torch.equal(live.bool(), R.live_of(target)) and not bool(g_s[~R.live_of(target)].any())


@pytest.mark.parametrize('Rr', [1, 7, 300])
@pytest.mark.parametrize('lead', range(4))
def test_means_guarded(dev, lead, Rr):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(40 + lead)
    K = 3
    rows = [torch.from_numpy(rng.uniform(0, 2, Rr).astype(np.float32)).to(dev) for _ in range(K)]
    live_np = (rng.random(Rr) < 0.6).astype(np.int32)
    rows[1][torch.from_numpy(live_np == 0).to(dev)] = float('nan')          # a value of a dead row is never used
    live, n_live = torch.from_numpy(live_np).to(dev), torch.tensor([int(live_np.sum())], dtype=torch.int32, device=dev)
    g_means = torch.from_numpy(rng.uniform(0.5, 2, K).astype(np.float32)).to(dev)
    means, g_rows = torch.empty(K, device=dev), torch.empty((K, Rr), device=dev)
    _call(lib, dev, 'means', _lib.ptr_array([r.data_ptr() for r in rows]), K, live, n_live, Rr, means)
    _call(lib, dev, 'means_backward', g_means, K, live, n_live, Rr, g_rows)
    grows = [G.embed(r, (lead + k) % 4) for k, r in enumerate(rows)]
    glive, gn, ggm = G.embed(live, (lead + 1) % 4), G.embed(n_live, (lead + 2) % 4), G.embed(g_means, (lead + 3) % 4)
    gmeans, ggr = G.out(K, torch.float32, dev, (lead + 1) % 4), G.out((K, Rr), torch.float32, dev, lead)
    _call(lib, dev, 'means', _lib.ptr_array([g.ptr() for g in grows]), K, glive, gn, Rr, gmeans)
    _call(lib, dev, 'means_backward', ggm, K, glive, gn, Rr, ggr)
    G.check_bands(*grows, glive, gn, ggm, gmeans, ggr)
    G.check_written(gmeans, ggr)
    G.check_unchanged(*grows, glive, gn, ggm)
    assert G.same(gmeans.t, means) and G.same(ggr.t, g_rows)
    n = max(int(live_np.sum()), 1)
    for k in range(K):
        want = float(torch.where(live.bool(), rows[k].double(), torch.zeros((), dtype=torch.float64, device=dev)).sum() / n)
        assert abs(float(means[k]) - want) <= R.TOL_MEAN * max(abs(want), 1.0)
        assert G.same(g_rows[k], torch.where(live.bool(), (g_means[k].double() / n).float(), torch.zeros((), device=dev)).expand(Rr).contiguous())
