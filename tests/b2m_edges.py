"""Case builders and referees for the edge tests of csrc/box2mask_loss.hip (tests/test_host_b2m_edges.py checks on the CPU that every
case is what it claims to be; tests/test_gpu_b2m_edges.py runs the kernels on them through the C ABI).  numpy / torch on the CPU only;
everything is deterministic from the seeds below, built once per process (functools.lru_cache) and must not be modified.

REFEREES
  scores     p_small: torch.nn.functional.interpolate(mode='bilinear', align_corners=False) on the CPU in fp64 (``resize64``), torch's
             own upsample, not a restatement of b2m_axis.  The adjoint: autograd of that same resize (``scores_bwd``).  The number of
             taps K of an element and sum |wy wx g_ps| come from the per-axis matrices of that resize (``axis_matrix``: torch's upsample
             of the identity); tests/test_host_b2m_edges.py shows that the autograd is the transposed matrix.
  level set  head.py:305-312,325-327 (include/boxinst/boxinst_hip_b2m.h) in np.longdouble from exact integer sums (``ls_ref``), with
             ``mag``, the sum of the magnitudes of the terms, alongside each value.

EXACT INPUTS AND DERIVED BOUNDS (u = 2^-24, the unit roundoff of fp32; no figure below comes from a run of a kernel)
  scores forward   logits in {0, +200, -200}: expf(-200) = 0 and expf(200) = inf in fp32, so p is exactly {0.5, 1, 0}.  Where every
                   weight of both axes is a multiple of 2^-4 (identity, x2 / x4 / x8 up, x2 / x4 down, an axis of one input or one
                   output element: ``dyadic``), every product and sum has at most 10 significant bits: exact in fp32, fused or not,
                   and p_small is compared bit for bit.  Otherwise the bound is FWD_BOUND = 8 u = 2^-21 absolute.  Count: all
                   intermediates lie in [0, 1], where one rounding is at most u / 2; per axis l1 = fl(frac) and l0 = fl(1 - frac)
                   (2 + 2), per row of taps two products and one sum (3 + 3, weighted by ly0 + ly1 <= 1 + u: 3), the two outer products
                   and the last sum (3): 10 roundings of u / 2 = 5 u, inside the 8 u that the issue states and that holds here.
                   A wrong tap or a wrong clamp shows as an error of order 0.5.  The random-logit set reuses the bound: the four taps are
                   the same sigmoid of the same logits as p, so p_small lies within 8 u of resize64(p) of the kernel's own p.
  scores backward  p in multiples of 2^-3, g_p and g_p_small in multiples of 2^-2 in [-2, 2].  On dyadic ratios a weight has at most
                   4 fractional bits and at most 16 x 16 small-grid pixels read one element, so acc is a multiple of 2^-10 below 2^9,
                   (g_p + acc) has at most 20 bits, p (1 - p) = k (8 - k) / 64 at most 4: exact, compared as numbers, every element.
                   Otherwise, per element, |got - ref| <= (K + 4) u (|g_p| + sum |wy wx g_ps|) p (1 - p): each of the K taps enters
                   through one sum whose terms carry a bounded number of roundings (two weights, two products, its additions), and
                   g_p + acc, * p, * (1 - p) add three; the issue states the factor K + 4 and it holds here.
  level set        p in multiples of 2^-6 in [0, 1], T in multiples of 2^-3 in [0, 1] (zero outside a box), target in multiples of
                   2^-4 in [-2, 2]: f = p T, g = (1 - p) T (10 bits) and t = x T (9 bits) are exact in fp32, f t (19) and f t t (28) in
                   fp64, and a sum of 2^17 of them stays below 2^46: exact in any order, fused or not.  The loss is one fp64 expression
                   of these sums (a = A / S, Q - 2 a A + a a S per side and channel, * weight / (C pixel_num): under 64 operations of
                   2^-53 on terms of total magnitude mag), rounded once to fp32.  With mag / |total| <= 2^20 (LS_CAP) the fp64 noise is
                   below 64 * 2^-53 * 2^20 = 2^-27 relative, far less than the distance of a tie, so |got - fl32(ref)| <= 1 ulp.
                   g_p / g_target, per element: the same kind of expression, (float) of at most 64 fp64 operations on terms of
                   magnitude mag: |got - ref| <= u |ref| + 2^-45 mag (64 * 2^-53 = 2^-47, four times over).  The saved remainder
                   R = A - a S is rounding noise of at most 2^-52 |A|; its terms 2 R (t - a) / S and 2 R f / S are at most
                   2^-51 |a| (|t| + |a|) and 2^-51 |a| f with S >= 1: inside 2^-45 mag.
  Both region sums of every live row are >= 1 (away from the 1e-5 clamps, which belong to the existing 'zero_target' case), except at
  1 x 1, where p T + (1 - p) T <= 1 makes that impossible: there both are exactly 0.5, a = t exactly, the energy is identically zero
  (LS_CAP cannot hold) and loss and gradients must be exactly zero, which the bounds above demand as well (ref = 0: the loss within
  2^-45 mag).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FWD_BOUND = 8 * U                     # 2^-21
LS_CAP = 2.0 ** 20
LS_NOISE = 2.0 ** -45
SIGMOID_TOL = 1e-6                    # the project's figure (tests/test_gpu_guarded_b2m_loss.py)

# the dispatch constants of csrc/box2mask_loss.hip (tests/test_host_b2m_edges.py reads them from the source)
SLICES, LS_THREADS, LS_UNROLL, BLOCK, MAX_LAYERS, MAX_C, MAX_UP, FINISH_ROWS = 8, 512, 4, 1024, 16, 4, 8, 64


# ---- the scores: shapes and what each claims -------------------------------------------------------------------------------------------------
# name -> (h, w, sh, sw), then the claims: vec (the host's choice at 16-byte aligned pointers), chunks on that path, chunks on the scalar
# path, dyadic, blocks of the backward, widest adjoint window (candidates per element) of the y and of the x axis
SCORES = {
    'one':            ((1, 1, 1, 1),       dict(vec=False, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(1, 1))),
    'one_up8':        ((1, 1, 8, 8),       dict(vec=False, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(8, 8))),      # every output clamped to tap 0
    'row':            ((1, 5, 8, 3),       dict(vec=False, chunks=1, chunks_scalar=1, dyadic=False, bwd_blocks=1, window=(8, 3))),
    'col56':          ((7, 5, 56, 1),      dict(vec=False, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(20, 1))),
    'up8_3':          ((3, 3, 24, 24),     dict(vec=False, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(20, 20))),
    'up8_12':         ((12, 12, 96, 96),   dict(vec=True, chunks=10, chunks_scalar=10, dyadic=True, bwd_blocks=1, window=(20, 20))),   # x8 onto the real small grid
    'ident16':        ((16, 16, 16, 16),   dict(vec=True, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(5, 5))),
    'down2':          ((24, 32, 12, 16),   dict(vec=True, chunks=1, chunks_scalar=1, dyadic=True, bwd_blocks=1, window=(5, 5))),
    'up4':            ((24, 32, 96, 128),  dict(vec=True, chunks=13, chunks_scalar=13, dyadic=True, bwd_blocks=1, window=(12, 12))),
    'odd':            ((17, 23, 12, 12),   dict(vec=False, chunks=1, chunks_scalar=1, dyadic=False, bwd_blocks=1, window=(6, 6))),
    'mid':            ((40, 56, 96, 96),   dict(vec=True, chunks=10, chunks_scalar=12, dyadic=False, bwd_blocks=3, window=(9, 8))),
    'real_down':      ((200, 304, 96, 96), dict(vec=True, chunks=24, chunks_scalar=69, dyadic=False, bwd_blocks=60, window=(5, 5))),
    'real':           ((256, 256, 96, 96), dict(vec=True, chunks=25, chunks_scalar=73, dyadic=False, bwd_blocks=64, window=(5, 5))),
    'to_one':         ((200, 304, 1, 1),   dict(vec=True, chunks=15, chunks_scalar=60, dyadic=True, bwd_blocks=60, window=(1, 1))),   # all but four pixels receive g_p alone
    'chunk1024':      ((16, 28, 24, 24),   dict(vec=True, chunks=1, chunks_scalar=1, dyadic=False, bwd_blocks=1, window=(7, 6))),     # scalar path: 448 + 576 = 1024 exactly
    # scalar path: 449 + 576 = 1025.  449 is prime, and a 24 x 24 small grid is beyond BXI_B2M_MAX_UP of an axis of one element (UNSUPPORTED,
    # which the GPU test pins): the same 576 small-grid pixels as 8 x 72
    'chunk1025':      ((1, 449, 8, 72),    dict(vec=False, chunks=2, chunks_scalar=2, dyadic=False, bwd_blocks=1, window=(8, 5))),
    'chunk1024_vec':  ((32, 56, 24, 24),   dict(vec=True, chunks=1, chunks_scalar=3, dyadic=False, bwd_blocks=2, window=(6, 5))),     # float4 path: 448 + 576 = 1024 exactly
}
SCORES_RANDOM = ('ident16', 'down2', 'chunk1024', 'chunk1024_vec', 'odd', 'real_down', 'real')       # the random-logit set
S_L, S_PLANES, S_M = 2, 5, 4
S_ROW_PLANE = (7, 1, -1, 4)                     # layer 1 plane 2, layer 0 plane 1, inert, layer 0 plane 4: not monotone
B_PLANES = 6
B_PLANE_ROW = (-1, 3, 0, -1, 1, -1)             # unmatched planes first, in the middle and last; no plane names row 2
B_PLANE_ROW_BEYOND = (-1, 3, 0, S_M, 1, -1)     # the same with an index >= M in the middle
# the layer table: BXI_B2M_MAX_LAYERS tensors of 3 planes, rows from layers 0 and 15, row_plane = -1 and >= L * planes
TABLE_SHAPE, TABLE_PLANES = (6, 6, 12, 12), 3
TABLE_ROW_PLANE = (15 * 3 + 2, 0 * 3 + 1, -1, 16 * 3, 15 * 3 + 0, 0 * 3 + 0)
TABLE_LAYER_PLANE = ((15, 2), (0, 1), None, None, (15, 0), (0, 0))


def scores_census(h, w, sh, sw):
    hw = h * w
    vec = hw % 4 == 0
    return dict(vec=vec, chunks=((hw // 4 if vec else hw) + sh * sw + BLOCK - 1) // BLOCK, chunks_scalar=(hw + sh * sw + BLOCK - 1) // BLOCK,
                bwd_blocks=(hw + BLOCK - 1) // BLOCK)


def resize64(x, size):
    """[N, h, w] -> [N, sh, sw]: torch's own bilinear upsample in fp64 on the CPU."""
    return F.interpolate(x.double()[:, None], size=tuple(size), mode='bilinear', align_corners=False)[:, 0]


@functools.lru_cache(maxsize=None)
def axis_matrix(n_in, n_out):
    """[n_out, n_in] fp64: torch's upsample of the identity along one axis (the other axis has one element)."""
    eye = torch.eye(n_in, dtype=torch.float64)
    return F.interpolate(eye[None, :, :, None], size=(n_out, 1), mode='bilinear', align_corners=False)[0, :, :, 0].t().contiguous()


def is_dyadic(h, w, sh, sw):
    return all(bool((R * 16 == torch.floor(R * 16)).all()) for R in (axis_matrix(h, sh), axis_matrix(w, sw)))


def candidates(n_in, n_out, fused):
    """b2m_candidates in float32 for every element of an axis: (lo, hi) arrays.  ``fused``: the multiply-subtract contracted."""
    i = np.arange(n_in, dtype=np.float32)
    inv = np.float32(1.0 / (float(n_in) / float(n_out)))
    if fused:
        a = ((i - np.float32(0.5)).astype(np.float64) * np.float64(inv) - 0.5).astype(np.float32)
        b = ((i + np.float32(1.5)).astype(np.float64) * np.float64(inv) - 0.5).astype(np.float32)
    else:
        a = (i - np.float32(0.5)) * inv - np.float32(0.5)
        b = (i + np.float32(1.5)) * inv - np.float32(0.5)
    lo, hi = np.floor(a).astype(np.int64) - 1, np.ceil(b).astype(np.int64) + 1
    lo[0] = 0
    return np.clip(lo, 0, None), np.clip(hi, None, n_out - 1)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=None)
def scores_exact(name):
    """dict(layers [L][planes,h,w], row_plane, p [M,h,w] exact, p_small [M,sh,sw] fp64 referee) with logits in {0, 200, -200}."""
    h, w, sh, sw = SCORES[name][0]
    rng = _rng(1, *SCORES[name][0])
    layers = [torch.from_numpy(rng.choice(np.array([0.0, 200.0, -200.0], np.float32), (S_PLANES, h, w))) for _ in range(S_L)]
    return _scores_ref(layers, S_PLANES, S_ROW_PLANE, (sh, sw), [divmod(r, S_PLANES) if r >= 0 else None for r in S_ROW_PLANE])


def _scores_ref(layers, planes, row_plane, size, where):
    h, w = layers[0].shape[1:]
    p = torch.zeros((len(row_plane), h, w), dtype=torch.float64)
    for m, lp in enumerate(where):
        if lp is not None:
            x = layers[lp[0]][lp[1]].double()
            p[m] = torch.where(x == 0, torch.full_like(x, 0.5), (x > 0).double())
    ps = resize64(p, size)
    return dict(layers=layers, planes=planes, row_plane=torch.tensor(row_plane, dtype=torch.int32), p=p, p_small=ps)


@functools.lru_cache(maxsize=None)
def scores_table():
    h, w, sh, sw = TABLE_SHAPE
    rng = _rng(2)
    layers = [torch.from_numpy(rng.choice(np.array([0.0, 200.0, -200.0], np.float32), (TABLE_PLANES, h, w))) for _ in range(MAX_LAYERS)]
    return _scores_ref(layers, TABLE_PLANES, TABLE_ROW_PLANE, (sh, sw), TABLE_LAYER_PLANE)


@functools.lru_cache(maxsize=None)
def scores_random(name):
    """Random logits (standard normal x 3) of the case's shape."""
    h, w, _, _ = SCORES[name][0]
    rng = _rng(3, *SCORES[name][0])
    return [torch.from_numpy((3 * rng.standard_normal((S_PLANES, h, w))).astype(np.float32)) for _ in range(S_L)]


@functools.lru_cache(maxsize=None)
def scores_bwd(name):
    """dict(g_p, g_ps, p (fp32 inputs), want [planes,h,w] fp64, bound [planes,h,w] fp64 (zeros where the case is dyadic), K)."""
    h, w, sh, sw = SCORES[name][0]
    rng = _rng(4, *SCORES[name][0])
    p = torch.from_numpy(rng.integers(0, 9, (S_M, h, w)).astype(np.float32) / 8)
    g_p = torch.from_numpy(rng.integers(-8, 9, (S_M, h, w)).astype(np.float32) / 4)
    g_ps = torch.from_numpy(rng.integers(-8, 9, (S_M, sh, sw)).astype(np.float32) / 4)
    x = p.double().requires_grad_(True)
    (resize64(x, (sh, sw)) * g_ps.double()).sum().backward()
    adj = x.grad
    Ry, Rx = axis_matrix(h, sh), axis_matrix(w, sw)
    mag = g_p.double().abs() + Ry.abs().t() @ g_ps.double().abs() @ Rx.abs()
    K = (Ry != 0).sum(0).double()[:, None] * (Rx != 0).sum(0).double()[None, :]
    pq = p.double() * (1 - p.double())
    want_rows = (g_p.double() + adj) * pq
    bound_rows = torch.zeros_like(want_rows) if is_dyadic(h, w, sh, sw) else (K + 4) * U * mag * pq
    want, bound = torch.zeros((B_PLANES, h, w), dtype=torch.float64), torch.zeros((B_PLANES, h, w), dtype=torch.float64)
    for plane, row in enumerate(B_PLANE_ROW):
        if row >= 0:
            want[plane], bound[plane] = want_rows[row], bound_rows[row]
    return dict(g_p=g_p, g_ps=g_ps, p=p, want=want, bound=bound, K=K, adjoint=adj)


# ---- the level-set pair --------------------------------------------------------------------------------------------------------------------
LS_G, LS_B, LS_WEIGHT = 3, 2, 1.5
LS_PIXEL_NUM = (3.0, 1.0, 6.0)
# (h, w) -> the claims: slice length, non-empty slices, length of the last non-empty slice, trips of a full slice, the highest live u of
# its last trip and how many lanes have it, blocks of the backward and the pixels of the last one
LS_SHAPES = {
    (1, 1):     dict(slice=4, nonempty=1, last_slice=1, trips=1, u_live=0, lanes=1, blocks=1, tail=1),
    (1, 7):     dict(slice=4, nonempty=2, last_slice=3, trips=1, u_live=0, lanes=4, blocks=1, tail=7),
    (4, 8):     dict(slice=4, nonempty=8, last_slice=4, trips=1, u_live=0, lanes=4, blocks=1, tail=32),                # every slice is exactly 4
    (3, 11):    dict(slice=8, nonempty=5, last_slice=1, trips=1, u_live=0, lanes=8, blocks=1, tail=33),                # five slices, the last with one pixel
    (64, 64):   dict(slice=512, nonempty=8, last_slice=512, trips=1, u_live=0, lanes=512, blocks=4, tail=1024),        # u = 0 exactly full
    (54, 76):   dict(slice=516, nonempty=8, last_slice=492, trips=1, u_live=1, lanes=4, blocks=5, tail=8),             # u = 1 live in four lanes
    (128, 128): dict(slice=2048, nonempty=8, last_slice=2048, trips=1, u_live=3, lanes=512, blocks=16, tail=1024),     # one full trip
    (113, 145): dict(slice=2052, nonempty=8, last_slice=2021, trips=2, u_live=0, lanes=4, blocks=17, tail=1),          # a second trip of four pixels
    (96, 96):   dict(slice=1152, nonempty=8, last_slice=1152, trips=1, u_live=2, lanes=128, blocks=9, tail=1024),
    (200, 304): dict(slice=7600, nonempty=8, last_slice=7600, trips=4, u_live=2, lanes=432, blocks=60, tail=384),
    (256, 256): dict(slice=8192, nonempty=8, last_slice=8192, trips=4, u_live=3, lanes=512, blocks=64, tail=1024),
    (15, 17):   dict(slice=32, nonempty=8, last_slice=31, trips=1, u_live=0, lanes=32, blocks=1, tail=255),
    (16, 16):   dict(slice=32, nonempty=8, last_slice=32, trips=1, u_live=0, lanes=32, blocks=1, tail=256),
    (1, 257):   dict(slice=36, nonempty=8, last_slice=5, trips=1, u_live=0, lanes=36, blocks=1, tail=257),
    (11, 93):   dict(slice=128, nonempty=8, last_slice=127, trips=1, u_live=0, lanes=128, blocks=1, tail=1023),
    (32, 32):   dict(slice=128, nonempty=8, last_slice=128, trips=1, u_live=0, lanes=128, blocks=1, tail=1024),
    (25, 41):   dict(slice=132, nonempty=8, last_slice=101, trips=1, u_live=0, lanes=132, blocks=2, tail=1),
}
# (h, w, shared, C, M): both sharings everywhere; C = 1 and MAX_C at the two slice / trip edges; the finish kernel's 64 rows and one more
LS_CASES = tuple((h, w, sh_, c, 4) for (h, w) in LS_SHAPES for sh_, c in ((1, 3), (0, 2))) \
    + tuple((h, w, sh_, c, 4) for (h, w) in ((3, 11), (54, 76)) for sh_ in (1, 0) for c in (1, MAX_C)) \
    + tuple((4, 8, sh_, c, m) for m in (FINISH_ROWS, FINISH_ROWS + 1) for sh_, c in ((1, 3), (0, 2)))


def ls_id(c):
    return f'{c[0]}x{c[1]}-{"image" if c[2] else "own"}-C{c[3]}-M{c[4]}'


def ls_census(HW):
    chunk = ((HW + SLICES - 1) // SLICES + 3) & ~3
    lens = [max(0, min(HW, (s + 1) * chunk) - s * chunk) for s in range(SLICES)]
    nonempty = sum(n > 0 for n in lens)
    trip = LS_THREADS * LS_UNROLL
    trips = (lens[0] + trip - 1) // trip
    last = lens[0] - (trips - 1) * trip
    u_live = (last + LS_THREADS - 1) // LS_THREADS - 1
    blocks = (HW + BLOCK - 1) // BLOCK
    return dict(slice=chunk, nonempty=nonempty, last_slice=lens[nonempty - 1], trips=trips, u_live=u_live, lanes=last - u_live * LS_THREADS,
                blocks=blocks, tail=HW - (blocks - 1) * BLOCK)


def ls_box(g, n, border):
    """One axis of the box of ground truth g: 0 touches the last row and column (zeros before it), 1 the first (zeros behind it), 2 lies
    in the middle.  With one style alone the first or the last pixel of every slice of a row-aligned shape would be a zero of T, and a
    pixel dropped there would cost nothing; the three live rows of a case of four use one style each."""
    return ((border, n), (0, n - border), (border, n - border))[g]


def _ls_ints(h, w, shared, C, M, seed):
    """Integer images: P = 64 p, T8 = 8 T, X = 16 target; indices with the inert row M // 2 as -1."""
    rng = _rng(5, h, w, shared, C, M, seed)
    if h * w == 1:
        P, T8 = np.full((M, 1, 1), 32, np.int64), np.full((LS_G, 1, 1), 8, np.int64)
    else:
        P = rng.integers(0, 65, (M, h, w)).astype(np.int64)
        T8 = np.zeros((LS_G, h, w), np.int64)
        by, bx = (max(1, h // 8) if h >= 4 else 0), (max(1, w // 8) if w >= 4 else 0)
        for g in range(LS_G):                         # the box of ground truth g: see ls_box
            (y0, y1), (x0, x1) = ls_box(g, h, by), ls_box(g, w, bx)
            T8[g, y0:y1, x0:x1] = rng.integers(1, 9, (y1 - y0, x1 - x0))
    X = rng.integers(-32, 33, (LS_B if shared else M, C, h, w)).astype(np.int64)
    if M == 4:
        tgt, img = np.array([2, 0, -1, 1], np.int32), np.array([1, 0, -1, 0], np.int32)        # not monotone
    else:
        tgt, img = rng.integers(0, LS_G, M).astype(np.int32), rng.integers(0, LS_B, M).astype(np.int32)
        tgt[M // 2] = img[M // 2] = -1
    g_loss = rng.integers(1, 9, M).astype(np.float32) / 4 * rng.choice(np.array([-1.0, 1.0], np.float32), M)
    return P, T8, X, tgt, img, g_loss


def _ls_sums(P, T8, tgt):
    live = [m for m in range(len(tgt)) if tgt[m] >= 0]
    return np.array([[(P[m] * T8[tgt[m]]).sum(), ((64 - P[m]) * T8[tgt[m]]).sum()] for m in live], np.int64) / 512.0


@functools.lru_cache(maxsize=None)
def ls_case(h, w, shared, C, M):
    """The first seed whose live rows all have both region sums >= 1 (0.5 at 1 x 1).  float32 tensors and the integer images."""
    for seed in range(64):
        P, T8, X, tgt, img, g_loss = _ls_ints(h, w, shared, C, M, seed)
        if float(_ls_sums(P, T8, tgt).min()) >= (1.0 if h * w > 1 else 0.5):
            break
    else:
        raise AssertionError('no seed gives region sums >= 1')
    return dict(h=h, w=w, shared=shared, C=C, M=M, inert=M // 2, seed=seed, P=P, T8=T8, X=X, tgt=tgt, img=img,
                p=torch.from_numpy((P / 64.0).astype(np.float32)), T=torch.from_numpy((T8 / 8.0).astype(np.float32)),
                target=torch.from_numpy((X / 16.0).astype(np.float32)), pixel_num=torch.tensor(LS_PIXEL_NUM, dtype=torch.float32),
                g_loss=torch.from_numpy(g_loss), weight=LS_WEIGHT)


def inert_variants(c):
    """(tgt_of, img_of) pairs of one case: the inert row as -1 and as an index beyond the range, in tgt_of and (shared) in img_of, one at
    a time, the other index of that row valid.  ``img_of`` None: the entry point gets NULL (shared == 0 only)."""
    k = c['inert']
    out = []
    for t_val, i_val in ((-1, 0), (LS_G, 1)) + (((1, -1), (0, LS_B)) if c['shared'] else ()):
        tgt, img = c['tgt'].copy(), c['img'].copy()
        tgt[k], img[k] = t_val, i_val
        out.append((tgt, img))
    if not c['shared']:
        out[0] = (out[0][0], None)
        out[1] = (out[1][0], np.full_like(c['img'], -1))           # ignored when shared == 0
    return out


@functools.lru_cache(maxsize=None)
def ls_ref(h, w, shared, C, M):
    """np.longdouble: loss [M], loss_mag, total (the energy before the scale), g_p [M,h,w], g_p_mag, g_target [M,C,h,w], g_target_mag
    (own targets only), sums [M,2]; the largest integer any sum reached."""
    c = ls_case(h, w, shared, C, M)
    ld = np.longdouble
    loss, loss_mag, total_of = np.zeros(M, ld), np.zeros(M, ld), np.zeros(M, ld)
    gp, gp_mag = np.zeros((M, h, w), ld), np.zeros((M, h, w), ld)
    gt, gt_mag = np.zeros((M, C, h, w), ld), np.zeros((M, C, h, w), ld)
    sums, top = np.zeros((M, 2), ld), 0
    for m in range(M):
        tg, im = int(c['tgt'][m]), int(c['img'][m]) if shared else m
        if tg < 0:
            continue
        T8 = c['T8'][tg]
        f = (c['P'][m] * T8, (64 - c['P'][m]) * T8)                  # x 2^9
        t = c['X'][im] * T8[None]                                    # x 2^7, [C,h,w]
        scale = ld(c['weight']) / (ld(C) * ld(LS_PIXEL_NUM[tg]))
        wgt = ld(float(c['g_loss'][m])) * scale
        Tf, tf = T8.astype(ld) / 8, t.astype(ld) / 128
        total = mag = ld(0)
        a = np.zeros((2, C), ld)
        for side in range(2):
            Si = int(f[side].sum())
            S = ld(Si) / 512
            sums[m, side] = S
            Sc = S if S > ld(1e-5) else ld(1e-5)
            for ch in range(C):
                Ai, Qi = int((f[side] * t[ch]).sum()), int((f[side] * t[ch] * t[ch]).sum())
                top = max(top, abs(Si), abs(Ai), abs(Qi))
                A, Q = ld(Ai) / 2 ** 16, ld(Qi) / 2 ** 23
                a[side, ch] = A / Sc
                total += Q - 2 * a[side, ch] * A + a[side, ch] * a[side, ch] * S
                mag += abs(Q) + 2 * abs(a[side, ch] * A) + a[side, ch] * a[side, ch] * S
        loss[m], loss_mag[m], total_of[m] = scale * total, abs(scale) * mag, total
        fl = (f[0].astype(ld) / 512, f[1].astype(ld) / 512)
        for ch in range(C):
            d0, d1 = tf[ch] - a[0, ch], tf[ch] - a[1, ch]
            gp[m] += d0 * d0 - d1 * d1
            gp_mag[m] += 2 * tf[ch] * tf[ch] + 2 * np.abs(tf[ch]) * (abs(a[0, ch]) + abs(a[1, ch])) + a[0, ch] ** 2 + a[1, ch] ** 2
            gt[m, ch] = wgt * Tf * 2 * (fl[0] * d0 + fl[1] * d1)
            gt_mag[m, ch] = abs(wgt) * Tf * 2 * (fl[0] * (np.abs(tf[ch]) + abs(a[0, ch])) + fl[1] * (np.abs(tf[ch]) + abs(a[1, ch])))
        gp[m] *= wgt * Tf
        gp_mag[m] *= abs(wgt) * Tf
    return dict(loss=loss, loss_mag=loss_mag, total=total_of, g_p=gp, g_p_mag=gp_mag, g_target=gt, g_target_mag=gt_mag, sums=sums, top=top)


def ls_loss_bound(ref):
    """Per row: (fl32(ref), bound).  One ulp of fl32(ref) where the energy is not zero; 2^-45 mag (ref = 0: an absolute bound) where it is."""
    want = ref['loss'].astype(np.float32)
    bound = np.where(ref['total'] != 0, np.spacing(np.abs(want)).astype(np.longdouble), LS_NOISE * ref['loss_mag'])
    return want, bound


def grad_bound(ref, key):
    return U * np.abs(ref[key]) + LS_NOISE * ref[key + '_mag']


def share(err, bound):
    """max err / bound over the elements with a positive bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, np.longdouble), np.asarray(bound, np.longdouble)
    zero = bound == 0
    assert not bool((err[zero] != 0).any()), f'{int((err[zero] != 0).sum())} elements with a zero bound are not exact'
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
