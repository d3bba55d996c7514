"""CPU: every case of tests/b2m_edges.py is what it claims to be.  No kernel runs here: each figure comes from the dispatch arithmetic of
csrc/box2mask_loss.hip restated in tests/b2m_edges.py, from torch's own fp64 resize or from integer arithmetic on the case's inputs, and
is printed before it is asserted.  The conditions under which tests/test_gpu_b2m_edges.py may compare exactly (dyadic inputs, region sums
away from the clamps, the cancellation cap of the loss) are asserted for every case, and every bound is printed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import b2m_edges as E


def test_kernel_constants_are_the_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'boxinstseg_amd', 'csrc', 'box2mask_loss.hip')) as fh:
        code = fh.read()
    assert int(re.search(r'constexpr int kB2mSlices = (\d+)', code).group(1)) == E.SLICES
    assert int(re.search(r'constexpr int kB2mLsThreads = (\d+)', code).group(1)) == E.LS_THREADS
    assert 'p0 += 4 * kB2mLsThreads' in code and 'blockIdx.x * 1024 + threadIdx.x' in code and '(total + 1023) / 1024' in code
    assert '(h * w + 1023) / 1024' in code and 'blockIdx.x * 64 + threadIdx.x' in code and '(h * w) % 4 == 0 && bxi::aligned(p, 16)' in code
    with open(os.path.join(root, 'include', 'boxinst', 'boxinst_hip_b2m.h')) as fh:
        head = fh.read()
    for name, value in (('BXI_B2M_MAX_LAYERS', E.MAX_LAYERS), ('BXI_B2M_MAX_UP', E.MAX_UP), ('BXI_B2M_MAX_C', E.MAX_C)):
        assert int(re.search(rf'#define {name} (\d+)', head).group(1)) == value


@pytest.mark.parametrize('name', list(E.SCORES))
def test_scores_census(name):
    (h, w, sh, sw), claim = E.SCORES[name]
    assert sh <= E.MAX_UP * h and sw <= E.MAX_UP * w
    got = dict(E.scores_census(h, w, sh, sw), dyadic=E.is_dyadic(h, w, sh, sw))
    window = []
    for n_in, n_out in ((h, sh), (w, sw)):
        R = E.axis_matrix(n_in, n_out).numpy()
        widest = 0
        for fused in (False, True):
            lo, hi = E.candidates(n_in, n_out, fused)
            for i in range(n_in):
                taps = np.nonzero(R[:, i])[0]
                assert taps.size == 0 or (lo[i] <= taps.min() and taps.max() <= hi[i]), f'axis {n_in} -> {n_out}: a tap of element {i} is no candidate'
            widest = max(widest, int((hi - lo + 1).max()))
        window.append(widest)
    got['window'] = tuple(window)
    print(f'{name} {h}x{w} -> {sh}x{sw}: {got}')
    assert got == claim


def test_scores_shapes_reach_the_edges():
    S = E.SCORES
    total = lambda n, vec: (S[n][0][0] * S[n][0][1] // (4 if vec else 1)) + S[n][0][2] * S[n][0][3]  # noqa: E731
    assert total('chunk1024', False) == 1024 and total('chunk1025', False) == 1025 and total('chunk1024_vec', True) == 1024
    assert S['chunk1024'][0][0] * S['chunk1024'][0][1] % 4 == 0          # the scalar path there is forced by a misaligned p
    assert len(E.TABLE_ROW_PLANE) == len(E.TABLE_LAYER_PLANE) and max(E.TABLE_ROW_PLANE) >= E.MAX_LAYERS * E.TABLE_PLANES
    for rp, lp in zip(E.TABLE_ROW_PLANE, E.TABLE_LAYER_PLANE):
        assert (lp is None) == (rp < 0 or rp >= E.MAX_LAYERS * E.TABLE_PLANES) and (lp is None or rp == lp[0] * E.TABLE_PLANES + lp[1])
    assert {lp[0] for lp in E.TABLE_LAYER_PLANE if lp} == {0, E.MAX_LAYERS - 1}
    assert E.B_PLANE_ROW[0] < 0 and E.B_PLANE_ROW[-1] < 0 and E.B_PLANE_ROW[3] < 0 and E.B_PLANE_ROW_BEYOND[3] >= E.S_M
    assert sorted(r for r in E.B_PLANE_ROW if r >= 0) == [0, 1, 3]       # row 2 has no plane


@pytest.mark.parametrize('name', list(E.SCORES))
def test_scores_inputs_are_exact(name):
    (h, w, sh, sw), claim = E.SCORES[name]
    c = E.scores_exact(name)
    for t in c['layers']:
        assert set(np.unique(t.numpy()).tolist()) <= {0.0, 200.0, -200.0}
    assert set(np.unique(c['p'].numpy()).tolist()) <= {0.0, 0.5, 1.0} and not bool(c['p'][2].any()) and not bool(c['p_small'][2].any())
    ps = c['p_small']
    if claim['dyadic']:
        assert bool((ps * 1024 == torch.floor(ps * 1024)).all())           # ten bits: fp32 holds every partial result
        for R in (E.axis_matrix(h, sh), E.axis_matrix(w, sw)):
            assert bool((R * 16 == torch.floor(R * 16)).all())
    b = E.scores_bwd(name)
    for key, step in (('p', 8), ('g_p', 4), ('g_ps', 4)):
        assert bool((b[key] * step == torch.floor(b[key] * step)).all())
    assert float(b['p'].min()) >= 0 and float(b['p'].max()) <= 1 and float(b['g_p'].abs().max()) <= 2 and float(b['g_ps'].abs().max()) <= 2
    if claim['dyadic']:
        assert not bool(b['bound'].any())
        assert bool((b['want'] * 2 ** 16 == torch.floor(b['want'] * 2 ** 16)).all()) and float(b['want'].abs().max()) < 2 ** 8
        assert torch.equal(b['want'].float().double(), b['want'])          # fp32 holds the gradient
    else:
        live = [pl for pl, r in enumerate(E.B_PLANE_ROW) if r >= 0]
        assert float(b['bound'][live].max()) > 0 and float(b['bound'].min()) >= 0
    print(f'{name}: forward bound {0.0 if claim["dyadic"] else E.FWD_BOUND:.3e}; backward bound at most {float(b["bound"].max()):.3e} '
          f'(largest gradient {float(b["want"].abs().max()):.3e}, most taps {int(b["K"].max())})')


def test_the_adjoint_referee_is_an_adjoint():
    """autograd of the fp64 resize against the dense transposed resize matrix, (7, 5) -> (12, 9) and back."""
    for (h, w), (sh, sw) in (((7, 5), (12, 9)), ((12, 9), (7, 5))):
        rng = np.random.default_rng(9)
        x = torch.from_numpy(rng.standard_normal((1, h, w))).requires_grad_(True)
        g = torch.from_numpy(rng.standard_normal((1, sh, sw)))
        y = E.resize64(x, (sh, sw))
        (y * g).sum().backward()
        Ry, Rx = E.axis_matrix(h, sh), E.axis_matrix(w, sw)
        dense = torch.kron(Ry, Rx)                                         # [sh sw, h w]
        assert float((dense @ x.detach().reshape(-1) - y.detach().reshape(-1)).abs().max()) <= 1e-14
        err = float((dense.t() @ g.reshape(-1) - x.grad.reshape(-1)).abs().max())
        print(f'{h}x{w} -> {sh}x{sw}: autograd against the transposed matrix {err:.3e}')
        assert err <= 1e-14


@pytest.mark.parametrize('hw', list(E.LS_SHAPES), ids=lambda s: f'{s[0]}x{s[1]}')
def test_levelset_census(hw):
    got = E.ls_census(hw[0] * hw[1])
    print(f'{hw[0]}x{hw[1]} = {hw[0] * hw[1]}: {got}')
    assert got == E.LS_SHAPES[hw]


@pytest.mark.parametrize('case', E.LS_CASES, ids=E.ls_id)
def test_levelset_conditions(case):
    h, w, shared, C, M = case
    c, r = E.ls_case(*case), E.ls_ref(*case)
    assert 1 <= C <= E.MAX_C and c['tgt'][c['inert']] == -1 and 0 < c['inert'] < M - 1
    for key, step, lo, hi in (('p', 64, 0, 1), ('T', 8, 0, 1), ('target', 16, -2, 2)):
        t = c[key].double()
        assert bool((t * step == torch.floor(t * step)).all()) and float(t.min()) >= lo and float(t.max()) <= hi, key
    if h >= 4 and w >= 4:
        T = c['T']                                                         # zeros outside the box, which touches the last / the first / no edge
        assert not bool(T[0, 0].any()) and not bool(T[0, :, 0].any()) and bool(T[0, -1, -1]) and not bool(T[1, -1].any()) and not bool(T[1, :, -1].any())
        assert bool(T[1, 0, 0]) and not bool(T[2, 0].any()) and not bool(T[2, -1].any()) and not bool(T[2, :, 0].any()) and not bool(T[2, :, -1].any())
    # f, g, t in fp32 are the exact products
    tg = int(c['tgt'][0])
    assert np.array_equal((c['p'][0] * c['T'][tg]).double().numpy() * 512, (c['P'][0] * c['T8'][tg]).astype(np.float64))
    assert np.array_equal(((1 - c['p'][0]) * c['T'][tg]).double().numpy() * 512, ((64 - c['P'][0]) * c['T8'][tg]).astype(np.float64))
    assert r['top'] < 2 ** 53                                              # every sum is an integer that fp64 holds
    live = [m for m in range(M) if c['tgt'][m] >= 0]
    if M == 4:
        assert list(c['tgt']) == [2, 0, -1, 1] and list(c['img']) == [1, 0, -1, 0]
    floor = 1.0 if h * w > 1 else 0.5
    assert float(r['sums'][live].min()) >= floor
    want, bound = E.ls_loss_bound(r)
    if h * w > 1:
        cap = float((r['loss_mag'][live] / np.abs(r['loss'][live])).max())
        assert bool((r['total'][live] != 0).all()) and cap <= E.LS_CAP
    else:
        cap = float('inf')
        assert not bool(r['total'].any()) and not bool(r['g_p'].any()) and not bool(r['g_target'].any())
    assert bool((bound[live] > 0).all()) and float(r['loss'][c['inert']]) == 0.0
    bp = E.grad_bound(r, 'g_p')
    assert float(bp.min()) >= 0 and float(bp[live].max()) > 0 and not bool(bp[c['inert']].any())
    line = f'{E.ls_id(case)} (seed {c["seed"]}): region sums >= {float(r["sums"][live].min()):.3f}, mag / |loss| <= {cap:.3e}, loss bound ' \
           f'{float(bound[live].max()):.3e}, g_p bound <= {float(bp.max()):.3e}'
    if not shared:
        bt = E.grad_bound(r, 'g_target')
        assert float(bt.min()) >= 0 and float(bt[live].max()) > 0
        line += f', g_target bound <= {float(bt.max()):.3e}'
    print(line)
    for tgt, img in E.inert_variants(c):
        k = c['inert']
        assert tgt[k] < 0 or tgt[k] >= E.LS_G or (shared and (img[k] < 0 or img[k] >= E.LS_B))
        assert np.array_equal(np.delete(tgt, k), np.delete(c['tgt'], k))
