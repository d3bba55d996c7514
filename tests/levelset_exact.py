"""Exactly representable cases for the level-set loss and the LocalConsistencyModule refinement (a plain module, no tests in it; in
the manner of tests/dyn_exact.py).

Refinement.  One iteration is phi <- sum_k aff_k * phi(neighbour_k) (forward) or its transpose.  With every coefficient a multiple
of 1/8 and an integer start, every term of iteration `it` is a multiple of 2^(-3 it); while the operator applied to |x| stays below
2^(24 - 3 it), every partial sum of every summation order (taps in any order, padded gathers, fold-backs, FMAs) is a multiple of
that quantum below quantum * 2^24: exactly representable in fp32.  A kernel then owes the fp64 result bit for bit.

Level set.  Scores in {0, 1/2, 1} whose sum per instance and side is a power of two, integer targets: S, A = sum f T and
Q = sum f T^2 are exact in fp64 in any order, the region mean a = A / S is dyadic, the clamp of S is inactive and R = A - a S is
exactly 0.  Every quantity of the forward and of the backward is exact in fp64 -- in the reference's two-pass form and in the
kernel's one-pass form Q - 2 a A + a^2 S alike --, so loss and gradients are the fp64 values rounded once to fp32.

  lcm_exact_case(N, h, w, seed)                   aff [N,8,h,w], phi [N,h,w], g [N,h,w]
  lcm_order_free(aff, x, iters, d, transpose)     the premise (lcm_order_free_ratio < 1 after every iteration)
  lcm_expected(N, h, w, seed, iters, d, transpose)  the oracle in fp64, cast to fp32; computed once per case
  lcm_regime(h, w, d, transpose)                  'pad' | 'lds' | 'step': the host rules of bxi_lcm_refine_f32
  levelset_exact_case(N, C, H, W, seed)           mask_score [N,2,H,W], target [N,C,H,W]
  planted_pixels(H, W)                            slice and trip boundaries of levelset_partial_kernel
  levelset_expected(ms, T, weight, pixel_num, j)  loss, d mask_score, d target as the kernel owes them, in fp32
"""
from __future__ import annotations

import numpy as np

from oracle import levelset_oracle as lo

# ------------------------------------------------------------------------------------------------------------------------------
# the host rules of bxi_lcm_refine_f32 (csrc/levelset.hip); tests/test_host_levelset_exact.py compares them with the source
# ------------------------------------------------------------------------------------------------------------------------------
PAD_SPT = 10                  # kLcmPadSPT: padded positions per thread
PAD_THREADS = 1024            # kLcmPadThreads
LDS_LIMIT = 128 * 1024        # bytes of LDS a one-launch kernel may ask for
REF_SHAPE = (96, 96, 2)       # the compile-time instantiations <96, 96, 2>


def lcm_regime(h, w, d, transpose, spt=PAD_SPT, threads=PAD_THREADS, lds_limit=LDS_LIMIT) -> str:
    """Which kernel bxi_lcm_refine_f32 launches: 'pad' (padded planes in LDS), 'lds' (two planes in LDS, clamped taps) or 'step'
    (one launch per iteration, planes in global memory)."""
    hp, wp = h + 2 * d, w + 2 * d
    if not transpose:
        if hp * wp <= spt * threads and 4 * 2 * hp * wp <= lds_limit:
            return 'pad'
        if 4 * 2 * h * w <= lds_limit:
            return 'lds'
    else:
        lds_adj2 = 4 * ((h + 4 * d) * (w + 4 * d) + hp * wp)
        if hp * wp <= spt * threads and h * w <= (spt - 1) * threads and 2 * w + 2 * max(h - 2, 0) <= threads and lds_adj2 <= lds_limit:
            return 'pad'
        if 4 * (h * w + hp * wp) <= lds_limit:
            return 'lds'
    return 'step'


# (h, w, d, forward, adjoint, what it pins)
REGIME_TABLE = [
    (76, 124, 2, 'pad', 'lds', 'padded plane = 10240 exactly; h*w > 9216'),
    (73, 129, 2, 'lds', 'lds', 'padded plane = 10241'),
    (96, 96, 1, 'pad', 'pad', 'h*w = 9216 exactly, run-time shape'),
    (97, 96, 1, 'pad', 'lds', 'h*w just over'),
    (2, 512, 1, 'pad', 'pad', 'perimeter = 1024, no interior pixel'),
    (2, 513, 1, 'pad', 'lds', 'perimeter 1026'),
    (3, 511, 1, 'pad', 'pad', 'perimeter = 1024 with an interior row'),
    (3, 512, 1, 'pad', 'lds', ''),
    (40, 40, 28, 'pad', 'pad', 'd >> h, last one under the lds_adj2 limit'),
    (40, 40, 29, 'pad', 'lds', 'first one over it'),
    (120, 128, 2, 'lds', 'lds', 'more than 64 KiB of LDS on both sides'),
    (128, 128, 2, 'lds', 'step', 'mixed regime; h*w = 16384 exactly'),
    (128, 129, 2, 'step', 'step', 'smallest per-iteration map'),
    (96, 96, 2, 'pad', 'pad', 'the compile-time instantiations'),
]
# maps on which the perimeter walk and the fold-back degenerate: one row, one column, d >= h
DEGENERATE = [(1, 1, 1), (1, 1, 3), (1, 2, 1), (2, 1, 2), (5, 1, 1), (5, 1, 3), (1, 5, 2), (2, 7, 3), (3, 3, 5), (3, 2, 1)]
REFINE_SHAPES = [r[:3] for r in REGIME_TABLE] + DEGENERATE
# (h, w, d, the iteration counts run there besides 3)
ITER_CASES = [(128, 129, 2, (0, 1, 2, 3)), (76, 124, 2, (0, 1)), (2, 512, 1, (0, 1)), (96, 96, 2, (0, 1))]
LCM_N = 2


def lcm_seed(h, w, d) -> int:
    return 1000 * h + 10 * w + d


def refine_runs():
    """Every distinct (h, w, d, iters) the GPU file runs exactly, in both directions."""
    runs = [(h, w, d, 3) for h, w, d in REFINE_SHAPES]
    for h, w, d, its in ITER_CASES:
        runs += [(h, w, d, it) for it in its if (h, w, d, it) not in runs]
    return runs


_CACHE: dict = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def lcm_exact_case(N, h, w, seed):
    """aff [N,8,h,w]: per pixel a histogram of 8 draws from 0..7, divided by 8 (multiples of 1/8 that sum to 1); phi and g [N,h,w]:
    integers in [-3, 3], different per instance.  float32, drawn once per (N, h, w, seed), read-only."""
    key = ('lcm', N, h, w, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        draws = rng.integers(0, 8, size=(N, 8, h, w))
        aff = np.stack([(draws == k).sum(axis=1) for k in range(8)], axis=1) / 8.0
        phi = rng.integers(-3, 4, size=(N, h, w))
        g = rng.integers(-3, 4, size=(N, h, w))
        _CACHE[key] = _frozen(aff.astype(np.float32), phi.astype(np.float32), g.astype(np.float32))
    return _CACHE[key]


def _apply(aff, x, d, transpose):
    return (lo.lcm_refine_backward if transpose else lo.lcm_refine)(aff, x, 1, d)


def lcm_order_free_ratio(aff, x, iters, d, transpose) -> float:
    """The largest max(operator^it |x|) * 2^(3 it) / 2^24 over it = 1 .. iters (0 for iters = 0): the operator on |x| bounds the sum of
    the absolute values of the terms of every element, and 2^(-3 it) is the quantum of iteration it."""
    a, worst = np.abs(np.asarray(x, np.float64)), 0.0
    for it in range(1, iters + 1):
        a = _apply(aff, a, d, transpose)
        worst = max(worst, float(a.max()) * 2.0 ** (3 * it) / 2.0 ** 24)
    return worst


def lcm_order_free(aff, x, iters, d, transpose) -> bool:
    return lcm_order_free_ratio(aff, x, iters, d, transpose) < 1.0


def lcm_expected(N, h, w, seed, iters, d, transpose):
    """(fp64 oracle result one iteration at a time, the same cast to fp32) for lcm_exact_case(N, h, w, seed): phi through the
    operator, or g through its transpose.  Computed once."""
    key = ('lcm_want', N, h, w, seed, iters, d, bool(transpose))
    if key not in _CACHE:
        aff, phi, g = lcm_exact_case(N, h, w, seed)
        x = (g if transpose else phi).astype(np.float64)
        for _ in range(iters):
            x = _apply(aff, x, d, transpose)
        _CACHE[key] = _frozen(x, x.astype(np.float32))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------
# level set
# ------------------------------------------------------------------------------------------------------------------------------
LS_SLICES = 8                 # kLsSlices: workgroups per instance
LS_THREADS = 512              # kLsThreads; the scalar kernel takes 4 pixels per thread and trip at p0 + u * 512, both kernels 2048 per trip
LS_MAXC = 8                   # kLsMaxC: channels per launch of the partial sums
# (N, C, H, W, path covered)
LS_SHAPES = [
    (2, 3, 129, 131, 'scalar path, second trip, ragged last slice'),
    (2, 3, 100, 164, 'vector path, second trip'),
    (1, 5, 199, 303, 'scalar path at workload scale, odd H*W'),
    (1, 9, 3, 2, 'slices without pixels, channel groups 8 + 1'),
    (1, 17, 7, 9, 'groups 8 + 8 + 1'),
    (2, 8, 1, 1, 'one-pixel map, full channel group'),
    (2, 7, 4, 9, '36 pixels: short last slice on the vector path'),
]
LS_OFFSET_VIEW = (2, 3, 100, 164)      # also run on views offset by one float: the vector-sized plane takes the scalar kernel


def ls_seed(N, C, H, W) -> int:
    return 7000 + 100 * H + W + C


def ls_chunk(HW: int) -> int:
    return ((HW + LS_SLICES - 1) // LS_SLICES + 3) & ~3


def planted_pixels(H, W):
    """The pixels at which levelset_partial_kernel changes hands: the last pixel of the map, the first and last pixel of every slice,
    and inside a slice every pixel at lo + 512 m (the scalar kernel's lanes u = 1..3; m = 4: the second trip of both kernels) with
    the one before it."""
    HW, out = H * W, {H * W - 1}
    chunk = ls_chunk(HW)
    for sl in range(LS_SLICES):
        lo_, hi = sl * chunk, min(sl * chunk + chunk, HW)
        if lo_ >= hi:
            continue
        out |= {lo_, hi - 1}
        for p in range(lo_ + LS_THREADS, hi, LS_THREADS):
            out |= {p - 1, p}
    return sorted(out)


def levelset_exact_case(N, C, H, W, seed, plant=True):
    """mask_score [N,2,H,W] in {0, 1/2, 1}: per instance and side n1 ones and an even number n2 of halves at random places with
    n1 + n2 / 2 = 2^k (k the same for all; S = 1 for a one-pixel map); target [N,C,H,W]: integers in [-4, 4].  With `plant` the pixels
    of planted_pixels() hold score 1 on both sides and target +-4 (they are among the n1 ones: the sums stay powers of two); everything
    else is random.  float32, drawn once, read-only."""
    key = ('ls', N, C, H, W, seed, plant)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    HW = H * W
    P = np.array(planted_pixels(H, W) if plant else [], np.int64)
    k = max(int(np.floor(np.log2(HW))) - 1, int(np.ceil(np.log2(max(len(P), 1)))), 0)
    S = 2 ** k
    assert len(P) <= S <= HW, (H, W, len(P), S)
    free = np.setdiff1d(np.arange(HW), P)
    ms = np.zeros((N, 2, HW))
    T = rng.integers(-4, 5, size=(N, C, HW)).astype(np.float64)
    T[:, :, P] = rng.choice(np.array([-4.0, 4.0]), size=(N, C, len(P)))
    n2_max = min(2 * (S - len(P)), 2 * (HW - S))                   # n1 >= planted, n1 + n2 <= H W
    for n in range(N):
        for side in range(2):
            n2 = 2 * int(rng.integers(n2_max // 4, n2_max // 2 + 1))
            n1 = S - n2 // 2
            order = rng.permutation(free)
            ms[n, side, P] = 1.0
            ms[n, side, order[:n1 - len(P)]] = 1.0
            ms[n, side, order[n1 - len(P):n1 - len(P) + n2]] = 0.5
    _CACHE[key] = _frozen(ms.reshape(N, 2, H, W).astype(np.float32), T.reshape(N, C, H, W).astype(np.float32))
    return _CACHE[key]


def levelset_unit(ms, T):
    """(total [N], d total / d mask_score, d total / d target) in fp64: the oracle with pixel_num = 1 / C and loss_weight = 1, whose
    weight 1 / (C * (1 / C)) is exactly 1 (asserted)."""
    C = T.shape[1]
    pn = np.float64(1.0) / np.float64(C)
    assert np.float64(C) * pn == 1.0, C
    return lo.levelset_loss(ms, T, np.full(ms.shape[0], pn), 1.0)


def levelset_case_and_unit(N, C, H, W, seed):
    """levelset_exact_case(N, C, H, W, seed) and levelset_unit() of it, computed once and read-only."""
    key = ('ls_unit', N, C, H, W, seed)
    if key not in _CACHE:
        ms, T = levelset_exact_case(N, C, H, W, seed)
        _CACHE[key] = (ms, T) + _frozen(*levelset_unit(ms, T))
    return _CACHE[key]


def levelset_expected(unit, C, weight, pixel_num, j):
    """What LevelsetLoss(loss_weight=weight)(ms, T, pixel_num) and its backward under the upstream gradient C * 2^j owe, in fp32;
    `unit` = levelset_unit(ms, T).  `weight` and every pixel_num are powers of two.  The kernel states the loss as
    (float)(weight * total / (C * pixel_num)) -- one fp64 division, one cast -- and the gradients as (float)(w * unit gradient) with
    w = g * weight / (C * pixel_num) = 2^j * weight / pixel_num, a power of two."""
    total, gm, gT = unit
    pn = np.asarray(pixel_num, np.float64)
    for v in [weight] + list(pn):
        assert np.frexp(v)[0] == 0.5, v                            # a power of two
    loss = (np.float64(weight) * total / (np.float64(C) * pn)).astype(np.float32)
    w = (2.0 ** j) * np.float64(weight) / pn
    return loss, (w[:, None, None, None] * gm).astype(np.float32), (w[:, None, None, None] * gT).astype(np.float32)
