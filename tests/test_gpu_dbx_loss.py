"""GPU: discobox_pseudo_losses / live_means (csrc/discobox_loss.hip) on every case of tests/dbx_loss_ref.py, with one leg and with two.

Exact, no tolerance:
* the target / enlarged-target planes are ``target != 0`` and ``F.max_pool2d(target.float(), 3, 1, 1)``;
* ``live`` / ``n_live`` are ``target.flatten(1).any(1)`` and its count;
* the pseudo-labels of each leg are, bit for bit, what the existing ``meanfield_forward`` returns on the materialised x = (t + s) / 2,
  img_inds and the concatenated iiu (zeros for a level whose pointer is null);
* the leg-0 dice rows are the fp64 value rounded once: the inputs are dyadic, every sum is exact in fp64 (tests/dbx_loss_ref.py);
* two runs are bit-identical.
Within the bounds that tests/dbx_loss_ref.py derives from the number formats (TOL_ROW, TOL_MEAN, TOL_GRAD_REL): the leg-1 rows, the means
and the gradient w.r.t. s against the fp64 restatement and its autograd."""
import numpy as np
import pytest
import torch

from tests import dbx_loss_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu


def _inputs(d, dev, legs):
    import boxinstseg_amd as B
    s, t = torch.tensor(d['s'], device=dev), torch.tensor(d['t'], device=dev)
    target, img = torch.tensor(d['target'], device=dev), torch.tensor(d['img'], device=dev)
    kernel = B.meanfield_kernel(torch.tensor(d['feats'], device=dev), d['ks'], 2.0, 0.5, 30.0)
    iiu = [None if x is None else torch.tensor(x, device=dev) for x in d['inter']] if legs == 2 else None
    return s, t, target, img, kernel, iiu


def _run(d, dev, legs, weights):
    import boxinstseg_amd as B
    s, t, target, img, kernel, iiu = _inputs(d, dev, legs)
    s = s.clone().requires_grad_(True)
    details = {}
    mil, ts, tsc, live, n_live = B.discobox_pseudo_losses(s, t, target, img, kernel, iiu, d['level_rows'] if legs == 2 else None, iters=d['iters'],
                                                          base=d['base'], details=details)
    rows = (mil, ts) + ((tsc,) if legs == 2 else ())
    means = B.live_means(live, n_live, *rows)
    obj = (ts * weights[0]).sum() + ((tsc * weights[1]).sum() if legs == 2 else 0.0)
    (g_s,) = torch.autograd.grad(obj, s, retain_graph=True)
    (g_mean,) = torch.autograd.grad(means[1:].sum(), s)
    return dict(mil=mil.detach(), ts=ts.detach(), tsc=None if tsc is None else tsc.detach(), live=live, n_live=n_live, means=means.detach(), g_s=g_s,
                g_mean=g_mean, details=details)


@pytest.mark.parametrize('legs', [1, 2])
@pytest.mark.parametrize('name', list(R.CASES))
def test_pseudo_losses(dev, name, legs):
    import boxinstseg_amd as B
    d = R.case(name)
    s, t, target, img, kernel, _ = _inputs(d, dev, legs)
    rng = np.random.default_rng(5)
    weights = [torch.from_numpy(rng.uniform(0.5, 2.0, d['R']).astype(np.float32)).to(dev) for _ in range(2)]
    with G.poisoned_empty():
        got = _run(d, dev, legs, weights)
    det = got['details']
    # planes
    assert torch.equal(det['target'], (target != 0).to(torch.uint8))
    enlarged = R.enlarged_of(target)
    assert torch.equal(det['enlarged'], enlarged)
    want_live = R.live_of(target)
    assert torch.equal(got['live'].bool(), want_live) and got['live'].dtype == torch.int32 and int(got['n_live']) == int(want_live.sum())
    # labels: the existing entry point on the materialised operands
    x = (t + s) / 2
    want0, _ = B.meanfield_forward(kernel, x, target, d['iters'], d['base'], img, None)
    assert torch.equal(det['pseudo'], want0.to(torch.uint8))
    pseudo, pseudo_corr = det['pseudo'], None
    if legs == 2:
        inter = torch.tensor(R.inter_cat(d), device=dev)
        want1, _ = B.meanfield_forward(kernel, x, target, d['iters'], d['base'], img, inter, R.GAMMA)
        assert torch.equal(det['pseudo_corr'], want1.to(torch.uint8))
        pseudo_corr = det['pseudo_corr']
    else:
        assert det['pseudo_corr'] is None and got['tsc'] is None
    assert not bool((pseudo.bool() & ~(target != 0)).any())                # no label outside the target
    # leg 0, exact: a = s e, sums exact in fp64 (dyadic), D = (sum a^2 + sum b^2) + 0.002, 1 - 2 A / D rounded once
    a = (s.double() * enlarged.double()).flatten(1)
    b = pseudo.double().flatten(1)
    want_ts = (1.0 - 2.0 * (a * b).sum(1) / (((a * a).sum(1) + b.sum(1)) + 0.002)).float()
    assert G.same(got['ts'], want_ts), (got['ts'], want_ts)
    # the fp64 restatement and its autograd
    s64 = s.double().requires_grad_(True)
    ts64, tsc64 = R.terms(s64, target, pseudo, pseudo_corr)
    assert float((got['ts'].double() - ts64.detach()).abs().max()) <= R.TOL_ROW
    obj = (ts64 * weights[0].double()).sum()
    rows64 = [ts64]
    if legs == 2:
        err = float((got['tsc'].double() - tsc64.detach()).abs().max())
        print(f'{name}: leg-1 rows differ by at most {err:.3e} (bound {R.TOL_ROW:.3e})')
        assert err <= R.TOL_ROW
        obj = obj + (tsc64 * weights[1].double()).sum()
        rows64.append(tsc64)
    (g64,) = torch.autograd.grad(obj, s64, retain_graph=True)
    scale = g64.abs().flatten(1).max(1).values.clamp(min=1e-30)[:, None, None]
    err = float(((got['g_s'].double() - g64).abs() / scale).max())
    print(f'{name}: gradient differs by at most {err:.3e} of the row maximum (bound {R.TOL_GRAD_REL:.3e})')
    assert err <= R.TOL_GRAD_REL
    assert not bool(got['g_s'][~want_live].any()) and not bool(got['g_s'][enlarged == 0].any())
    # means over the live rows (mil through the existing kernel: its own rows are the reference here)
    n = max(int(want_live.sum()), 1)
    lv = want_live.double()
    want_means = [float((got['mil'].double() * lv).sum() / n)] + [float((r.detach() * lv).sum() / n) for r in rows64]
    for k, w in enumerate(want_means):
        assert abs(float(got['means'][k]) - w) <= R.TOL_MEAN * max(abs(w), 1.0), (k, float(got['means'][k]), w)
    (gm64,) = torch.autograd.grad(sum((r * lv).sum() / n for r in rows64), s64)
    scale = gm64.abs().flatten(1).max(1).values.clamp(min=1e-30)[:, None, None]
    assert float(((got['g_mean'].double() - gm64).abs() / scale).max()) <= R.TOL_GRAD_REL
    # determinism
    with G.poisoned_empty():
        again = _run(d, dev, legs, weights)
    for key in ('mil', 'ts', 'means', 'g_s', 'g_mean') + (('tsc',) if legs == 2 else ()):
        assert G.same(got[key], again[key]), key
    for key in ('target', 'enlarged', 'pseudo'):
        assert torch.equal(det[key], again['details'][key]), key


@pytest.mark.parametrize('name', R.FIXTURE_CASES)
def test_against_the_reference_fixture(dev, name):
    """tests/golden/discobox_loss.npz: the reference's own statements (:1271-1306, :1335-1339, :1127-1137) in fp64.  Labels of both legs and
    ``live`` are equal; mil / ts / leg-1 rows, both means and the gradient of loss_ts w.r.t. s are within 4 x the reference's own
    fp32-against-fp64 difference (tol_*) of the fp64 values.  The mean of the mil rows is held to tol_mil_rows: a mean of rows is no more
    accurate than the rows, and the fp32 reference's own mean happens to land closer than its rows."""
    import boxinstseg_amd as B
    f = R.fixture(name)
    s = torch.tensor(f['s'], device=dev).requires_grad_(True)
    t, target, img = torch.tensor(f['t'], device=dev), torch.tensor(f['target'], device=dev), torch.tensor(f['img'], device=dev)
    kernel = B.meanfield_kernel(torch.tensor(f['feats'], device=dev), int(f['ks']), f['mf']['alpha0'], f['mf']['theta0'], f['mf']['theta1'])
    rows = [int(v) for v in f['level_rows']]
    first = np.cumsum([0] + rows)
    iiu = [torch.tensor(f['inter'][first[l]:first[l + 1]], device=dev) if rows[l] else None for l in range(len(rows))]
    det = {}
    mil, ts, tsc, live, n_live = B.discobox_pseudo_losses(s, t, target, img, kernel, iiu, rows, iters=int(f['iters']), base=f['mf']['base'],
                                                          gamma=f['gamma'], details=det)
    means = B.live_means(live, n_live, mil, ts, tsc)
    (g,) = torch.autograd.grad(means[1] + means[2], s)
    assert np.array_equal(live.cpu().numpy() != 0, f['live'] != 0) and int(n_live) == int((f['live'] != 0).sum())
    assert np.array_equal(det['pseudo'].cpu().numpy(), f['pseudo']) and np.array_equal(det['pseudo_corr'].cpu().numpy(), f['pseudo_corr'])
    lv = f['live'] != 0
    R.within(mil.detach().cpu().numpy()[lv], f['mil_rows'][lv], f['tol_mil_rows'], f'{name} mil rows')
    R.within(ts.detach().cpu().numpy()[lv], f['ts_rows'][lv], f['tol_ts_rows'], f'{name} ts rows')
    R.within(tsc.detach().cpu().numpy()[lv], f['ts_corr_rows'][lv], f['tol_ts_corr_rows'], f'{name} leg-1 rows')
    R.within(float(means[0]), f['mean_ins'], f['tol_mil_rows'], f'{name} mean of the mil rows')
    R.within(float(means[1]), f['mean_ts'], f['tol_mean_ts'], f'{name} mean_ts')
    R.within(float(means[2]), f['mean_ts_corr'], f['tol_mean_ts_corr'], f'{name} mean_ts_corr')
    R.within(g.cpu().numpy(), f['grad'], f['tol_grad'], f'{name} gradient')


def test_legs_differ_where_the_census_says(dev):
    """The competing inter_img_mask moves labels: leg 1 is not a copy of leg 0 (tests/test_host_dbx_loss.py counts the same on the host)."""
    d = R.case('w70')
    got = _run(d, dev, 2, [torch.ones(d['R'], device=dev)] * 2)
    assert not torch.equal(got['details']['pseudo'], got['details']['pseudo_corr'])
    assert bool(got['details']['pseudo'].any())


def test_unsupported_is_said_before_any_launch(dev):
    import boxinstseg_amd as B
    d = R.case('w13')
    s, t, target, img, kernel, iiu = _inputs(d, dev, 2)
    with pytest.raises(NotImplementedError):
        B.discobox_pseudo_losses(s.half(), t, target, img, kernel, iters=1, base=0.1)
    with pytest.raises(NotImplementedError):
        B.discobox_pseudo_losses(s, t, target, img, kernel[:, :4], iters=1, base=0.1)
    from boxinstseg_amd import _lib
    lib = _lib.load()
    assert lib.bxi_dbx_workspace_bytes(65536, 4, 4, 1) == 0 and lib.bxi_dbx_workspace_bytes(4, 4, 4, 3) == 0
    ws = torch.empty(lib.bxi_dbx_workspace_bytes(4, 9, 13, 2), dtype=torch.uint8, device=dev)
    rc = lib.bxi_dbx_steps_f32(kernel.data_ptr(), 2, 9, 13, 7, img.data_ptr(), 4, 1, 0.1, 0.01, 1, None, None, 0, ws.data_ptr(), ws.numel(), G.stream(dev))
    assert rc == _lib.BXI_ERR_UNSUPPORTED


def test_captured_in_a_graph(dev):
    """prepare + steps + dice + means allocate nothing, synchronise nothing and read no device value on the host: a hipGraph replays them."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    d = R.case('w70')
    s, t, target, img, kernel, iiu = _inputs(d, dev, 2)
    Rr, H, W, it = d['R'], d['H'], d['W'], d['iters']
    import boxinstseg_amd as B
    det = {}
    _, ts, tsc, live, n_live = B.discobox_pseudo_losses(s, t, target, img, kernel, iiu, d['level_rows'], iters=it, base=d['base'], details=det)
    nws = lib.bxi_dbx_workspace_bytes(Rr, H, W, 2)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    glive, gn = torch.empty(Rr, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    loss, sums = torch.empty((2, Rr), device=dev), torch.empty((2, Rr, 2), dtype=torch.float64, device=dev)
    ptrs, firsts = _lib.ptr_array([x.data_ptr() for x in iiu]), _lib.int_array([0, d['level_rows'][0]])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = G.stream(dev)
        rcs = [lib.bxi_dbx_prepare_f32(s.data_ptr(), t.data_ptr(), target.data_ptr(), Rr, H, W, 2, glive.data_ptr(), gn.data_ptr(), ws.data_ptr(), nws, st),
               lib.bxi_dbx_steps_f32(kernel.data_ptr(), 2, H, W, d['ks'], img.data_ptr(), Rr, it, d['base'], R.GAMMA, 2, ptrs, firsts, 2, ws.data_ptr(), nws, st),
               lib.bxi_dbx_dice_forward_f32(s.data_ptr(), Rr, H, W, 2, it, R.GAMMA, ws.data_ptr(), nws, loss.data_ptr(), sums.data_ptr(), st)]
    assert rcs == [0, 0, 0], rcs
    loss.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert G.same(loss[0], ts.detach()) and G.same(loss[1], tsc.detach()) and torch.equal(glive, live) and int(gn) == int(n_live)
