"""Host: the premises of tests/test_gpu_levelset_edges.py, checked without a device for every case that file runs exactly.

(1) every refinement case is order-free in fp32, in both directions, and the fp64 oracle result survives the round trip through
fp32; (2) every level-set case has power-of-two score sums and an fp64 total equal to the rational one; (3) lcm_regime restates the
dispatch of bxi_lcm_refine_f32: its constants are read out of csrc/levelset.hip, and the regime of every boundary shape is pinned,
so a change of the dispatch rules fails here instead of silently moving a GPU case off its boundary."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import levelset_exact as X

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'boxinstseg_amd', 'csrc', 'levelset.hip')


# ------------------------------------------------------------------------------------------------------------------------------
# refinement
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,d,iters', X.refine_runs(), ids=lambda v: str(v))
def test_refine_cases_are_order_free_and_round_trip(h, w, d, iters):
    aff, phi, g = X.lcm_exact_case(X.LCM_N, h, w, X.lcm_seed(h, w, d))
    assert np.array_equal(aff.sum(axis=1), np.ones_like(phi)) and np.array_equal(np.mod(aff * 8, 1), np.zeros_like(aff))
    assert np.abs(phi).max() <= 3 and np.abs(g).max() <= 3 and np.array_equal(phi, np.round(phi)) and np.array_equal(g, np.round(g))
    assert h * w == 1 or not np.array_equal(phi[0], phi[1])                  # different data per instance
    for transpose, x in ((0, phi), (1, g)):
        ratio = X.lcm_order_free_ratio(aff, x, iters, d, transpose)
        print(f'{h}x{w} d={d} iters={iters} transpose={transpose}: premise ratio {ratio:.3g}')
        assert X.lcm_order_free(aff, x, iters, d, transpose) and ratio < 1.0
        want64, want32 = X.lcm_expected(X.LCM_N, h, w, X.lcm_seed(h, w, d), iters, d, transpose)
        assert want32.dtype == np.float32 and np.array_equal(want32.astype(np.float64), want64)
        if iters == 0:
            assert np.array_equal(want32, x)
        elif h * w > 1:                                                  # one iteration fewer (the other ping-pong plane) is another result
            assert not np.array_equal(want32, X.lcm_expected(X.LCM_N, h, w, X.lcm_seed(h, w, d), iters - 1, d, transpose)[1])


def test_premise_margin_of_the_named_cases():
    """At iters = 3 the products max * 2^9 stay below 2^13 -- eleven bits under the limit -- for these shapes."""
    for h, w, d in [(96, 96, 2), (5, 1, 3), (2, 512, 1), (128, 129, 2), (3, 3, 5)]:
        aff, phi, g = X.lcm_exact_case(X.LCM_N, h, w, X.lcm_seed(h, w, d))
        for transpose, x in ((0, phi), (1, g)):
            assert X.lcm_order_free_ratio(aff, x, 3, d, transpose) < 2.0 ** 13 / 2.0 ** 24


def test_order_free_rejects_a_case_that_is_not():
    aff, phi, _ = X.lcm_exact_case(1, 3, 3, 1)
    assert not X.lcm_order_free(aff, phi * 2.0 ** 21, 1, 1, 0) and X.lcm_order_free(aff, phi * 2.0 ** 19, 1, 1, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# level set
# ------------------------------------------------------------------------------------------------------------------------------
def _rational_total(ms, T, n):
    """sum over sides and channels of sum_p (T - a)^2 f with a = A / S, as a Fraction.  Over the pixels with a score only: with
    S = 2^k, f in {1/2, 1} and integer T the numerators 2 S T - 2 A are integers below 2^20 and their squares times 2 f sum to below
    2^60 -- plain integer arithmetic --, and sum (T - a)^2 f = that sum / (8 S^2)."""
    total = Fraction(0)
    for side in range(2):
        f = ms[n, side].reshape(-1).astype(np.float64)
        live = np.nonzero(f)[0]
        f2 = np.round(2 * f[live]).astype(np.int64)                      # 1 or 2
        S2 = int(f2.sum())                                               # 2 S
        for c in range(T.shape[1]):
            t = np.round(T[n, c].reshape(-1)[live]).astype(np.int64)
            A2 = int((f2 * t).sum())                                     # 2 A
            num = S2 * t - A2                                            # (T - a) * 2 S
            total += Fraction(int((num * num * f2).sum()), 2 * S2 * S2)
    return total


@pytest.mark.parametrize('N,C,H,W', [s[:4] for s in X.LS_SHAPES], ids=lambda v: str(v))
def test_levelset_cases_are_exact(N, C, H, W):
    ms, T, total, gm, gT = X.levelset_case_and_unit(N, C, H, W, X.ls_seed(N, C, H, W))
    assert set(np.unique(ms)) <= {0.0, 0.5, 1.0} and np.abs(T).max() <= 4 and np.array_equal(T, np.round(T))
    S = ms.astype(np.float64).sum(axis=(2, 3))
    assert np.all(np.frexp(S)[0] == 0.5), S                              # every instance and side: a power of two
    assert np.all(((ms == 0.5).sum(axis=(2, 3)) % 2) == 0)
    if H * W == 1:
        assert np.all(S == 1.0)
    P = X.planted_pixels(H, W)
    flat_ms, flat_T = ms.reshape(N, 2, -1), T.reshape(N, C, -1)
    assert np.all(flat_ms[:, :, P] == 1.0) and np.all(np.abs(flat_T[:, :, P]) == 4.0)
    assert N == 1 or H * W <= 4 or not np.array_equal(ms[0], ms[1])
    for n in range(N):
        want = _rational_total(ms, T, n)
        assert Fraction(float(total[n])) == want, (n, float(total[n]), float(want))
    # R = A - a S is exactly 0, so the unit gradients are (T - a)^2 summed over the channels and 2 (T - a) f summed over the sides:
    # every one a dyadic number of few bits, and the fp32 expectation is one rounding of it
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gT)) and np.all(gm >= 0)
    C_ = np.float64(C)
    assert C_ * (np.float64(1.0) / C_) == 1.0


@pytest.mark.parametrize('N,C,H,W', [s[:4] for s in X.LS_SHAPES if s[2] * s[3] > 1], ids=lambda v: str(v))
def test_a_boundary_pixel_dropped_or_doubled_changes_the_bits(N, C, H, W):
    """What the planted scores are for: a pixel at a slice or trip boundary counted 0 or 2 times moves the fp32 loss of the case,
    so the exact comparison on the device cannot pass by accident."""
    ms, T, total, gm, gT = X.levelset_case_and_unit(N, C, H, W, X.ls_seed(N, C, H, W))
    pn = [2.0 ** (3 + n) for n in range(N)]
    want = X.levelset_expected((total, gm, gT), C, 4.0, pn, -3)[0]
    P, chunk = X.planted_pixels(H, W), X.ls_chunk(H * W)
    picks = [p for p in (0, chunk - 1, chunk, chunk + 511, chunk + 512, chunk + 2047, chunk + 2048, H * W - 1) if p in P]
    assert len(picks) >= 3
    for p in picks:
        for factor in (0.0, 2.0):
            bad = ms.copy().reshape(N, 2, -1)
            bad[:, :, p] *= factor
            bad = bad.reshape(ms.shape)
            got = X.levelset_expected(X.levelset_unit(bad, T), C, 4.0, pn, -3)[0]
            assert np.all(got != want), (p, factor, got, want)


def test_small_case_pixel_by_pixel():
    """The rational total once more with one Fraction per pixel, on the maps small enough for it, and the expected loss of one."""
    for N, C, H, W in [(1, 9, 3, 2), (1, 17, 7, 9), (2, 8, 1, 1), (2, 7, 4, 9)]:
        ms, T, total, _, _ = X.levelset_case_and_unit(N, C, H, W, X.ls_seed(N, C, H, W))
        for n in range(N):
            want = Fraction(0)
            for side in range(2):
                f = [Fraction(float(v)) for v in ms[n, side].reshape(-1)]
                S = sum(f)
                for c in range(C):
                    t = [Fraction(float(v)) for v in T[n, c].reshape(-1)]
                    a = sum(x * y for x, y in zip(f, t)) / S
                    want += sum((y - a) ** 2 * x for x, y in zip(f, t))
            assert Fraction(float(total[n])) == want
    assert np.all(X.levelset_case_and_unit(2, 8, 1, 1, X.ls_seed(2, 8, 1, 1))[2] == 0.0)      # one pixel: T = a
    ms, T, total, gm, gT = X.levelset_case_and_unit(1, 9, 3, 2, X.ls_seed(1, 9, 3, 2))
    loss, em, eT = X.levelset_expected((total, gm, gT), 9, 4.0, [8.0], -2)
    assert loss.dtype == np.float32 and loss[0] == np.float32(4.0 * total[0] / 72.0)
    assert np.array_equal(em, (gm / 8.0).astype(np.float32)) and np.array_equal(eT, (gT / 8.0).astype(np.float32))


def test_planted_pixels():
    assert X.ls_chunk(129 * 131) == 2116 and X.ls_chunk(100 * 164) == 2052 and X.ls_chunk(36) == 8 and X.ls_chunk(6) == 4 and X.ls_chunk(1) == 4
    assert X.planted_pixels(1, 1) == [0] and X.planted_pixels(3, 2) == [0, 3, 4, 5]
    assert X.planted_pixels(4, 9) == [0, 7, 8, 15, 16, 23, 24, 31, 32, 35]
    P = X.planted_pixels(100, 164)
    assert {0, 2047, 2048, 2051, 2052, 2052 + 511, 2052 + 512, 6 * 2052 + 2048, 7 * 2052, 16399} <= set(P) and max(P) == 16399
    P = X.planted_pixels(129, 131)
    assert {7 * 2116, 7 * 2116 + 2047, 7 * 2116 + 2048, 16898} <= set(P) and max(P) == 16898


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch
# ------------------------------------------------------------------------------------------------------------------------------
def test_regime_constants_match_the_source():
    src = open(SRC).read()
    assert int(re.search(r'constexpr\s+int\s+kLcmPadSPT\s*=\s*(\d+)\s*;', src).group(1)) == X.PAD_SPT
    assert int(re.search(r'constexpr\s+int\s+kLcmPadThreads\s*=\s*(\d+)\s*;', src).group(1)) == X.PAD_THREADS
    host = src[src.index('int bxi_lcm_refine_f32('):]
    limits = re.findall(r'(lds\w*)\s*<=\s*(\d+)\s*\*\s*(\d+)', host)
    assert sorted(name for name, _, _ in limits) == ['lds', 'lds_adj', 'lds_adj2', 'lds_fwd'], limits
    assert all(int(a) * int(b) == X.LDS_LIMIT for _, a, b in limits), limits
    m = re.search(r'ref_shape\s*=\s*h\s*==\s*(\d+)\s*&&\s*w\s*==\s*(\d+)\s*&&\s*dilation\s*==\s*(\d+)\s*;', host)
    assert tuple(int(v) for v in m.groups()) == X.REF_SHAPE
    assert len(re.findall(r'_pad_kernel<%d, %d, %d>' % X.REF_SHAPE, host)) == 4 and X.REF_SHAPE in [r[:3] for r in X.REGIME_TABLE]
    # the level-set constants planted_pixels() restates
    assert int(re.search(r'constexpr\s+int\s+kLsSlices\s*=\s*(\d+)\s*;', src).group(1)) == X.LS_SLICES
    assert int(re.search(r'constexpr\s+int\s+kLsThreads\s*=\s*(\d+)\s*;', src).group(1)) == X.LS_THREADS
    assert int(re.search(r'constexpr\s+int\s+kLsMaxC\s*=\s*(\d+)\s*;', src).group(1)) == X.LS_MAXC


@pytest.mark.parametrize('h,w,d,fwd,adj,what', X.REGIME_TABLE, ids=['%dx%d-d%d' % r[:3] for r in X.REGIME_TABLE])
def test_regime_table(h, w, d, fwd, adj, what):
    assert (X.lcm_regime(h, w, d, 0), X.lcm_regime(h, w, d, 1)) == (fwd, adj), what


def test_regime_boundaries_are_where_the_table_says():
    hp_wp = lambda h, w, d: (h + 2 * d) * (w + 2 * d)
    assert hp_wp(76, 124, 2) == X.PAD_SPT * X.PAD_THREADS and hp_wp(73, 129, 2) == X.PAD_SPT * X.PAD_THREADS + 1
    assert 96 * 96 == (X.PAD_SPT - 1) * X.PAD_THREADS
    assert 2 * 512 == X.PAD_THREADS and 2 * 511 + 2 * (3 - 2) == X.PAD_THREADS
    adj2 = lambda h, w, d: 4 * ((h + 4 * d) * (w + 4 * d) + hp_wp(h, w, d))
    assert adj2(40, 40, 28) <= X.LDS_LIMIT < adj2(40, 40, 29)
    assert 4 * 2 * 120 * 128 > 64 * 1024 and 4 * (120 * 128 + hp_wp(120, 128, 2)) > 64 * 1024
    assert 4 * 2 * 128 * 128 == X.LDS_LIMIT and 4 * (128 * 128 + hp_wp(128, 128, 2)) > X.LDS_LIMIT
    # the constants are parameters: one position per thread fewer moves 76 x 124 off the padded kernels
    assert X.lcm_regime(76, 124, 2, 0, spt=9) == 'lds' and X.lcm_regime(2, 512, 1, 1, threads=512) == 'lds'
    for h, w, d in X.DEGENERATE:
        assert X.lcm_regime(h, w, d, 0) == 'pad' and X.lcm_regime(h, w, d, 1) == 'pad'
