"""The level-set and LocalConsistencyModule kernels at every dispatch boundary, bit for bit (run on a real MI355X: -m gpu).

On the cases of tests/levelset_exact.py fp32 is exact in any summation order (tests/test_host_levelset_exact.py establishes that
without a device), so every kernel owes the fp64 oracle's result cast to fp32: the comparisons are np.array_equal, there is no
tolerance.  Refinement: every regime of bxi_lcm_refine_f32 on its boundary shape and on maps of one row, one column and d >= h, in
both directions, at 0 .. 3 iterations.  Level set: the scalar and the vector partial sums with a second trip, a ragged last slice,
slices without pixels and 1 .. 3 channel groups, scores planted on every slice and trip boundary, and the backward with and
without a target gradient.  Only the module route with a real affinity and the far-from-zero targets carry tolerances, those of
tests/test_gpu_levelset.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import levelset_oracle as lo
from tests import levelset_exact as X

pytestmark = pytest.mark.gpu
TOL = 1e-4            # tests/test_gpu_levelset.py: losses and gradients relative to their largest magnitude


def _close(got, want, tol=TOL):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max() <= tol * max(np.abs(want).max(), 1e-12)


class _Hook:
    """The launch labels between __enter__ and __exit__, one per launch (the hook brackets a launch: phase 0 before, 1 after)."""

    def __init__(self):
        from boxinstseg_amd import _lib
        self.names, self._lib = [], _lib
        self._cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: self.names.append(name.decode()) if phase == 0 else None)

    def __enter__(self):
        self._lib.load().bxi_dev_set_launch_hook(C.cast(self._cb, C.c_void_p), None)
        return self

    def __exit__(self, *exc):
        self._lib.load().bxi_dev_set_launch_hook(None, None)
        return False


def _first_difference(got, want):
    """'' when the arrays are equal element by element; otherwise the first differing index with both values and the count."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return ''
    bad = np.argwhere(got != want)
    idx = tuple(int(v) for v in bad[0])
    return f'[{idx}] = {got[idx]!r}, expected {want[idx]!r}; {len(bad)} of {got.size} elements differ'


# ------------------------------------------------------------------------------------------------------------------------------
# refinement, exact
# ------------------------------------------------------------------------------------------------------------------------------
def _run_refine(dev, h, w, d, iters, transpose):
    from boxinstseg_amd.levelset import _refine
    aff, phi, g = X.lcm_exact_case(X.LCM_N, h, w, X.lcm_seed(h, w, d))
    x = g if transpose else phi
    xd = torch.tensor(x, device=dev)
    with _Hook() as hk:
        out = _refine(torch.tensor(aff, device=dev), xd, d, iters, transpose)
    torch.cuda.synchronize()
    regime = X.lcm_regime(h, w, d, transpose)
    if regime == 'step':
        assert hk.names == ['lcm_step'] * iters, hk.names          # iters = 0: a copy, no launch
    else:
        assert hk.names == ['lcm_adjoint' if transpose else 'lcm_refine'], (regime, hk.names)
    assert np.array_equal(xd.cpu().numpy(), x)                     # the input plane is not the ping-pong partner
    want = X.lcm_expected(X.LCM_N, h, w, X.lcm_seed(h, w, d), iters, d, transpose)[1]
    return out.cpu().numpy(), want, x, regime


@pytest.mark.parametrize('transpose', [0, 1], ids=['forward', 'adjoint'])
@pytest.mark.parametrize('h,w,d', X.REFINE_SHAPES, ids=['%dx%d-d%d' % s for s in X.REFINE_SHAPES])
def test_refine_exact(built, dev, h, w, d, transpose):
    got, want, _, regime = _run_refine(dev, h, w, d, 3, transpose)
    diff = _first_difference(got, want)
    assert np.array_equal(got, want), f'{h}x{w} d={d} transpose={transpose} ({regime}): out{diff}'


ITER_RUNS = [(h, w, d, it) for h, w, d, its in X.ITER_CASES for it in its]


@pytest.mark.parametrize('transpose', [0, 1], ids=['forward', 'adjoint'])
@pytest.mark.parametrize('h,w,d,iters', ITER_RUNS, ids=['%dx%d-d%d-it%d' % r for r in ITER_RUNS])
def test_refine_iteration_counts(built, dev, h, w, d, iters, transpose):
    """0, 1, an even and an odd number of iterations: the per-iteration path ends in `out` at either parity and copies at 0; the
    one-launch kernels return their first plane untouched at 0."""
    got, want, x, regime = _run_refine(dev, h, w, d, iters, transpose)
    if iters == 0:
        assert np.array_equal(got.view(np.int32), x.view(np.int32)), (regime, _first_difference(got, x))
    diff = _first_difference(got, want)
    assert np.array_equal(got, want), f'{h}x{w} d={d} iters={iters} transpose={transpose} ({regime}): out{diff}'


def test_refine_autograd_route_exact(built, dev):
    """_LcmRefine.apply reaches the same kernels: forward and backward of the compile-time shape and of the mixed regime, bit for bit."""
    from boxinstseg_amd.levelset import _LcmRefine
    for h, w, d in [(96, 96, 2), (128, 128, 2)]:
        aff, phi, g = X.lcm_exact_case(X.LCM_N, h, w, X.lcm_seed(h, w, d))
        pd = torch.tensor(phi[:, None], device=dev).requires_grad_(True)
        with _Hook() as hk:
            out = _LcmRefine.apply(torch.tensor(aff, device=dev), pd, d, 3)
            out.backward(torch.tensor(g[:, None], device=dev))
        torch.cuda.synchronize()
        assert hk.names == ['lcm_refine'] + (['lcm_step'] * 3 if X.lcm_regime(h, w, d, 1) == 'step' else ['lcm_adjoint']), hk.names
        assert out.shape == pd.shape == pd.grad.shape
        assert np.array_equal(out.detach().cpu().numpy()[:, 0], X.lcm_expected(X.LCM_N, h, w, X.lcm_seed(h, w, d), 3, d, 0)[1])
        assert np.array_equal(pd.grad.cpu().numpy()[:, 0], X.lcm_expected(X.LCM_N, h, w, X.lcm_seed(h, w, d), 3, d, 1)[1])


def test_refine_without_instances(built, dev):
    from boxinstseg_amd.levelset import _refine
    for transpose in (0, 1):
        with _Hook() as hk:
            out = _refine(torch.zeros((0, 8, 128, 129), device=dev), torch.zeros((0, 128, 129), device=dev), 2, 3, transpose)
        assert out.shape == (0, 128, 129) and out.dtype == torch.float32 and hk.names == []


# ------------------------------------------------------------------------------------------------------------------------------
# affinity of a constant image
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc', [1, 3])
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('h,w', [(1, 1), (5, 1), (1, 5), (4, 5)])
def test_affinity_of_a_constant_image(built, dev, h, w, d, Cc):
    """Every neighbour equals the centre: every exponent is 0 and the softmax over 8 equal values is exactly 1/8."""
    from boxinstseg_amd import LocalConsistencyModule
    value = np.array([0.7, -1.3, 2.0, 0.1, 0.0, 5.5], np.float32).reshape(2, 3)[:, :Cc]       # one constant per instance and channel
    img = np.broadcast_to(value[:, :, None, None], (2, Cc, h, w)).copy()
    aff = LocalConsistencyModule(num_iter=1, dilations=[d]).affinity(torch.from_numpy(img).to(dev)).cpu().numpy()
    assert aff.shape == (2, 8, h, w) and np.array_equal(aff, np.full((2, 8, h, w), 0.125, np.float32))


# ------------------------------------------------------------------------------------------------------------------------------
# the module route with a real affinity, at the boundary shapes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,d', [r[:3] for r in X.REGIME_TABLE], ids=['%dx%d-d%d' % r[:3] for r in X.REGIME_TABLE])
def test_module_at_the_boundaries(built, dev, h, w, d):
    """LocalConsistencyModule forward and backward on seeded images (those of test_lcm_vs_oracle), at that test's tolerances."""
    from boxinstseg_amd import LocalConsistencyModule
    N, iters = X.LCM_N, 3
    rng = np.random.default_rng(h * 31 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([np.stack([np.sin(xx / 5.0 + i), np.cos(yy / 4.0), 0.1 * rng.standard_normal((h, w))]) for i in range(N)])
    img = (img + 0.05 * rng.standard_normal(img.shape)).astype(np.float32)
    phi = rng.uniform(0, 1, (N, 1, h, w)).astype(np.float32)
    gout = rng.standard_normal((N, 1, h, w)).astype(np.float32)
    lcm = LocalConsistencyModule(num_iter=iters, dilations=[d])
    aw = lo.lcm_affinity(img, d)
    pd = torch.from_numpy(phi).to(dev).requires_grad_(True)
    with _Hook() as hk:
        aff = lcm.affinity(torch.from_numpy(img).to(dev))
        ref = lcm(torch.from_numpy(img).to(dev), pd)
        ref.backward(torch.from_numpy(gout).to(dev))
    torch.cuda.synchronize()
    label = {0: 'lcm_refine', 1: 'lcm_adjoint'}
    want_names = ['lcm_affinity', 'lcm_affinity']
    for t in (0, 1):
        want_names += ['lcm_step'] * iters if X.lcm_regime(h, w, d, t) == 'step' else [label[t]]
    assert hk.names == want_names, hk.names
    err = np.abs(aff.cpu().numpy() - aw).max()
    print(f'{h}x{w} d={d}: affinity error {err:.3g}')
    assert err < 2e-5
    assert _close(ref.detach().cpu().numpy()[:, 0], lo.lcm_refine(aw, phi[:, 0], iters, d), 5e-5)
    assert _close(pd.grad.cpu().numpy()[:, 0], lo.lcm_refine_backward(aw, gout[:, 0], iters, d), 5e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# level set, exact
# ------------------------------------------------------------------------------------------------------------------------------
def _device_leaf(array, dev, offset):
    """The array on the device as a leaf; with `offset`, a contiguous view one float into a buffer of one element more."""
    t = torch.tensor(array, device=dev)                            # (a copy: the cases are read-only arrays)
    if offset:
        base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
        base[1:] = t.reshape(-1)
        t = base[1:].view(t.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t.detach().requires_grad_(True)


LS_RUNS = [s[:4] + (False,) for s in X.LS_SHAPES] + [X.LS_OFFSET_VIEW + (True,)]


@pytest.mark.parametrize('N,Cc,H,W,offset', LS_RUNS, ids=['N%d-C%d-%dx%d%s' % (r[:4] + ('-offset' if r[4] else '',)) for r in LS_RUNS])
def test_levelset_exact(built, dev, N, Cc, H, W, offset):
    """LevelsetLoss forward and backward twice: with a target that requires a gradient, and with one that does not (the image-level
    term: the backward kernels get a null pointer and must leave d mask_score what it was)."""
    from boxinstseg_amd import LevelsetLoss
    ms, T, total, ugm, ugT = X.levelset_case_and_unit(N, Cc, H, W, X.ls_seed(N, Cc, H, W))
    weight, j = 4.0, -3
    pn = np.array([2.0 ** (3 + n) for n in range(N)], np.float32)
    g_loss = np.full(N, Cc * 2.0 ** j, np.float32)
    want_loss, want_gm, want_gT = X.levelset_expected((total, ugm, ugT), Cc, weight, pn, j)
    vec = (H * W) % 4 == 0 and not offset
    groups = -(-Cc // X.LS_MAXC)
    grads = []
    for target_grad in (True, False):
        md, Td = _device_leaf(ms, dev, offset), _device_leaf(T, dev, offset)
        Td.requires_grad_(target_grad)
        assert vec == (md.data_ptr() % 16 == 0 and Td.data_ptr() % 16 == 0 and (H * W) % 4 == 0)
        with _Hook() as hk:
            loss = LevelsetLoss(loss_weight=weight)(md, Td, torch.from_numpy(pn).to(dev))
            loss.backward(torch.from_numpy(g_loss).to(dev))
        torch.cuda.synchronize()
        assert hk.names == ['levelset_partial'] * groups + ['levelset_finish', 'levelset_bwd'], hk.names
        got = loss.detach().cpu().numpy()
        assert np.array_equal(got, want_loss), f'loss{_first_difference(got, want_loss)} (totals {total})'
        gm = md.grad.cpu().numpy()
        assert np.array_equal(gm, want_gm), 'd mask_score' + _first_difference(gm, want_gm)
        if target_grad:
            gT = Td.grad.cpu().numpy()
            assert np.array_equal(gT, want_gT), 'd target' + _first_difference(gT, want_gT)
        else:
            assert Td.grad is None
        assert np.array_equal(md.detach().cpu().numpy(), ms) and np.array_equal(Td.detach().cpu().numpy(), T)
        grads.append(gm)
    assert np.array_equal(grads[0].view(np.int32), grads[1].view(np.int32))          # unchanged by the null target gradient


# ------------------------------------------------------------------------------------------------------------------------------
# level set, targets far from zero
# ------------------------------------------------------------------------------------------------------------------------------
def test_levelset_targets_far_from_zero(built, dev):
    """T = 200 + U(-0.5, 0.5): the energy is 1e-6 of Q = sum f T^2.  The one-pass form Q - 2 a A + a^2 S keeps the file's 1e-4 against
    the two-pass fp64 oracle only while A and Q are accumulated in double (in fp32 it loses about 4e-3)."""
    from boxinstseg_amd import LevelsetLoss
    N, Cc, H, W = 2, 3, 129, 131
    rng = np.random.default_rng(129 * 131)
    ms = rng.uniform(0, 1, (N, 2, H, W)).astype(np.float32)
    T = (200.0 + rng.uniform(-0.5, 0.5, (N, Cc, H, W))).astype(np.float32)
    pn = np.array([5000.0, 12000.0], np.float32)
    md = torch.from_numpy(ms).to(dev).requires_grad_(True)
    Td = torch.from_numpy(T).to(dev).requires_grad_(True)
    loss = LevelsetLoss(loss_weight=5.0)(md, Td, torch.from_numpy(pn).to(dev))
    loss.sum().backward()
    lw, gm, gT = lo.levelset_loss(ms, T, pn, 5.0)
    rel = lambda got, want: np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max()
    print('relative errors: loss %.3g, d mask_score %.3g, d target %.3g' % (rel(loss.detach().cpu().numpy(), lw), rel(md.grad.cpu().numpy(), gm),
                                                                            rel(Td.grad.cpu().numpy(), gT)))
    assert _close(loss.detach().cpu().numpy(), lw) and _close(md.grad.cpu().numpy(), gm) and _close(Td.grad.cpu().numpy(), gT)
