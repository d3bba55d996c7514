"""Case builders for the edge tests of the masked attention (tests/test_host_masked_attn_edges.py checks on the CPU, with the reference
alone, that every case reaches the trip it is built for; tests/test_gpu_masked_attn_edges.py runs the kernels on them).

The referee is tests/masked_attn_ref.py; nothing here launches a kernel.  The numbers of csrc/masked_attn.hip that the cases are built
around are restated here (a span is ``_lib.ATTN_SPAN`` keys; the forward cuts the queries into groups of 128, a wave's 32 each, and the keys
of a span into chunks of KC(D) and tiles of 32; the backward walks the queries in blocks of 32; combine and dq walk the spans in batches of
eight), and :func:`trips` does the arithmetic from them.

Everything is built once per process (functools.lru_cache) and must not be modified by a test."""
import functools

import torch

from tests import masked_attn_ref as R

Q_GROUP, Q_BLOCK, TILE, SPAN_BATCH = 128, 32, 32, 8
BITS_TRIP = 256                                                       # positions per trip of attn_bits_kernel (one per thread)


def span():
    from boxinstseg_amd import _lib
    return _lib.ATTN_SPAN


def kc(D):
    """Keys per LDS chunk of the forward."""
    return 64 if D == 64 else 128


def _ceil(a, b):
    return -(-a // b)


def trips(Q, S, D):
    """What the kernels' loops do at (Q, S, D), from the constants above alone."""
    sp = span()
    nspans = _ceil(S, sp)
    last_span = S - (nspans - 1) * sp
    last_chunk = last_span - (_ceil(last_span, kc(D)) - 1) * kc(D)
    groups = _ceil(Q, Q_GROUP)
    last_group = Q - (groups - 1) * Q_GROUP
    return dict(nspans=nspans, batches=_ceil(nspans, SPAN_BATCH), last_batch=nspans - (_ceil(nspans, SPAN_BATCH) - 1) * SPAN_BATCH,
                last_span_keys=last_span, last_chunk_keys=last_chunk, last_tile_keys=S - (_ceil(S, TILE) - 1) * TILE,
                q_groups=groups, last_group_queries=last_group, last_group_waves=_ceil(last_group, Q_BLOCK),
                q_blocks=_ceil(Q, Q_BLOCK), last_block_queries=Q - (_ceil(Q, Q_BLOCK) - 1) * Q_BLOCK)


# ---- 1: tolerance cases ------------------------------------------------------------------------------------------------------------
def tol_shapes():
    """name -> dict(Q, S, D, B, M, and optionally keep_spans / mask_2d)."""
    sp = span()
    c = {
        'spans9': dict(Q=33, S=8 * sp + 1, D=32),
        'spans9_dead': dict(Q=33, S=8 * sp + 1, D=32, keep_spans=(8,)),
        'spans17': dict(Q=33, S=16 * sp + 1, D=16),
        'spans17_dead': dict(Q=33, S=16 * sp + 1, D=16, keep_spans=(8, 16)),
        'spans9_full_D64': dict(Q=8, S=9 * sp, D=64),
        'one_group_one_span': dict(Q=128, S=sp, D=32),
        'second_group_of_one_query': dict(Q=129, S=sp + 1, D=16),
        'three_groups': dict(Q=257, S=40, D=16),
        'kc64_chunk_of_one_key': dict(Q=32, S=65, D=64),
        'kc64_one_chunk': dict(Q=64, S=64, D=64),
        'kc128_chunk_of_one_key': dict(Q=31, S=129, D=32),
        'one_query_one_key': dict(Q=1, S=1, D=16),
        'heads8': dict(Q=100, S=300, D=32, B=1, M=8),
        'images3_mask3d': dict(Q=40, S=300, D=32, B=3, M=1),
        'images3_mask2d': dict(Q=40, S=300, D=32, B=3, M=1, mask_2d=True),
    }
    for v in c.values():
        v.setdefault('B', 2), v.setdefault('M', 2)
    return c


TOL_NAMES = tuple(tol_shapes())


@functools.lru_cache(maxsize=None)
def tol_case(name):
    """(case, fp32 reference, fp64 reference, M) of one shape of :func:`tol_shapes`.  ``keep_spans``: row 0 of every (b, m) keeps keys only
    in those spans (at least the first key of each), so that everything real in that row comes from a later batch of eight spans."""
    s = tol_shapes()[name]
    Q, S, D, B, M = (s[n] for n in 'QSDBM')
    t = R.make_case(2000 + TOL_NAMES.index(name), Q, S, D, B, M)
    if s.get('keep_spans'):
        sp = span()
        dead = torch.ones(S, dtype=torch.bool)
        for i in s['keep_spans']:
            dead[i * sp:(i + 1) * sp] = False
        t['mask'][:, 0, dead] = True
        for i in s['keep_spans']:
            t['mask'][:, 0, i * sp] = False
    if s.get('mask_2d'):
        t['mask'] = t['mask'][0].clone()                              # torch's 2-D attn_mask [Q,S], shared by every image and head
    return t, R.core_with_grads(t, M, torch.float32), R.core_with_grads(t, M, torch.float64), M


# ---- 2: a key that dominates -------------------------------------------------------------------------------------------------------
HOT = 40.0
DOMINANT = (('three_spans', 16), ('three_spans', 32), ('three_spans', 64), ('nine_spans', 32))
# expf(x) is exactly 0 in fp32 for x < -104 (2^-150 = e^-103.97 is half the smallest denormal); a gap above this leaves room for the
# rounding of the scores themselves
EXP_IS_ZERO = 150.0


def dominant_shape(shape, D):
    sp = span()
    if shape == 'three_spans':
        Q, S = 40, 2 * sp + 70
        hot = [0, 31, 32, kc(D) - 1, kc(D), sp - 1, sp, sp + 44, S - 1]
    else:
        Q, S = 33, 8 * sp + 1
        hot = [0, 31, 32, sp - 1, 7 * sp, 7 * sp + 44, 8 * sp - 1, 8 * sp]         # spans 0, 7 and 8 (whose only key is S - 1)
    return Q, S, sorted(set(hot))


@functools.lru_cache(maxsize=None)
def dominant_case(shape, D, B=2, M=2, solo=4):
    """make_case with channel 0 of every head planted: q = 40 everywhere, k = 40 at the hot keys and 0 elsewhere.  Every hot key is masked
    for every row, then each (b, m, query) gets ONE seeded hot key back: its score is 1600 / sqrt(D) + O(1), every other unmasked score is
    O(1).  Per (b, m), ``solo`` hot keys are given to exactly one query each.  Returns the case with ``hot`` (sorted key list), ``pick``
    (int64 [B*M,Q], the key of each row) and ``solo`` (list of (bm, key, query))."""
    Q, S, hot = dominant_shape(shape, D)
    t = R.make_case(3000 + D + S, Q, S, D, B, M)
    t['q'].view(Q, B, M, D)[..., 0] = HOT
    kv = t['k'].view(S, B, M, D)
    kv[..., 0] = 0.0
    kv[hot, :, :, 0] = HOT
    hot_t = torch.tensor(hot)
    t['mask'][:, :, hot_t] = True
    g = torch.Generator().manual_seed(17 + D + S)
    pick = torch.empty(B * M, Q, dtype=torch.int64)
    solos = []
    for bm in range(B * M):
        keys, rows = torch.randperm(len(hot), generator=g), torch.randperm(Q, generator=g)
        shared = keys[solo:]
        p = shared[torch.randint(len(shared), (Q,), generator=g)]
        p[rows[:solo]] = keys[:solo]
        pick[bm] = hot_t[p]
        t['mask'][bm, torch.arange(Q), pick[bm]] = False
        solos += [(bm, int(hot_t[keys[i]]), int(rows[i])) for i in range(solo)]
    return dict(t, hot=hot, pick=pick, solo=solos, B=B, M=M, D=D)


def dominant_scores(c):
    """fp64 scores [B*M,Q,S] of a dominant case, masked keys at -inf."""
    Q, S, B, M, D = c['q'].shape[0], c['k'].shape[0], c['B'], c['M'], c['D']
    s = torch.einsum('qbmd,sbmd->bmqs', c['q'].double().view(Q, B, M, D), c['k'].double().view(S, B, M, D)).reshape(B * M, Q, S) / D ** 0.5
    return s.masked_fill(c['mask'], float('-inf'))


def dominant_want(c):
    """out [Q,B,E]: the v row of each row's hot key; and the bool [S,B,E] of the elements of dv whose key is hot."""
    Q, S, B, M, D = c['q'].shape[0], c['k'].shape[0], c['B'], c['M'], c['D']
    v = c['v'].view(S, B * M, D)
    out = torch.stack([v[c['pick'][bm], bm] for bm in range(B * M)], 1)             # [Q, B*M, D]
    is_hot = torch.zeros(S, dtype=torch.bool)
    is_hot[torch.tensor(c['hot'])] = True
    return out.reshape(Q, B, M * D), is_hot


# ---- 3: the same data laid out two ways --------------------------------------------------------------------------------------------
PAD_DIMS = (16, 32, 64)
CROWD_ROWS = (0, 31, 32, 127, 128, 255, 256)
COMPANY_HEADS = ((0, 0), (0, 5), (1, 7))                              # (b, m): the first, an inner and the last head of B = 2, M = 8


@functools.lru_cache(maxsize=None)
def padding_case(D):
    """(base case at S0 = span + 44, {S: the case with keys appended up to S}) for S = 2 span (the same span count) and 2 span + 5 (one more
    span, wholly masked).  The appended keys are masked for every row; their k and v are 1e3 * randn."""
    sp = span()
    Q, S0 = 40, sp + 44
    t = R.make_case(4000 + D, Q, S0, D)
    g = torch.Generator().manual_seed(41 + D)
    padded = {}
    for S in (2 * sp, 2 * sp + 5):
        extra = S - S0
        p = dict(t)
        p['k'] = torch.cat([t['k'], 1e3 * torch.randn(extra, *t['k'].shape[1:], generator=g)])
        p['v'] = torch.cat([t['v'], 1e3 * torch.randn(extra, *t['v'].shape[1:], generator=g)])
        p['mask'] = torch.cat([t['mask'], torch.ones(*t['mask'].shape[:2], extra, dtype=torch.bool)], -1)
        padded[S] = p
    return t, padded


@functools.lru_cache(maxsize=None)
def company_case():
    """B = 2, M = 8, Q = 40, S = span + 44, D = 32 with a mask per head [B*M,Q,S]; the mask per image is ``image_mask`` [B,Q,S]."""
    t = R.make_case(4100, 40, span() + 44, 32, 2, 8)
    return dict(t, image_mask=t['mask'][::8].clone(), B=2, M=8, D=32)


def head_alone(c, b, m, per_head):
    """The (b, m) head of a company case as a B = 1, M = 1 case on contiguous copies."""
    M, D = c['M'], c['D']
    cols = slice(m * D, (m + 1) * D)
    t = {n: c[n][:, b:b + 1, cols].contiguous() for n in ('q', 'k', 'v', 'g')}
    t['mask'] = (c['mask'][b * M + m] if per_head else c['image_mask'][b])[None].contiguous()
    return t


@functools.lru_cache(maxsize=None)
def crowd_case():
    """Q = 257 (three query groups, the last one holds one query), S = span + 44, D = 32."""
    return R.make_case(4200, 257, span() + 44, 32)


def query_alone(t, r):
    """Query r of a case as a Q = 1 case."""
    return dict(q=t['q'][r:r + 1].contiguous(), k=t['k'], v=t['v'], g=t['g'][r:r + 1].contiguous(), mask=t['mask'][:, r:r + 1].contiguous())


def only_row(g, r):
    out = torch.zeros_like(g)
    out[r] = g[r]
    return out


# ---- 4: mask bits ------------------------------------------------------------------------------------------------------------------
BITS_PLANTED_SIZES = ((17, 19), (9, 29))
BITS_SEEDED_SIZES = ((17, 19), (9, 29), (1, 33), (25, 42), (50, 84))  # the last two: 1/32 and 1/16 of an 800 x 1333 image
PACK_SHAPES = ((2, 3, 323, 2), (1, 2, 8 * 32 + 1, 1))                 # (rows, Q, S, num_heads)


def bits_trips(S):
    """(trips of 256 positions, positions of the last trip, bits of the last word) of attn_bits_kernel at S positions."""
    words = _ceil(S, 32)
    n = _ceil(words * 32, BITS_TRIP)
    return n, S - (n - 1) * BITS_TRIP, S - (words - 1) * 32


def decided_bits(pred, size):
    """The rule of test_mask_bits_against_the_reference_statements: a bit is compared where the fp64 resized logit is further from 0 than
    4 x the fp32-against-fp64 difference of the resize plus 2^-22.  Returns (decided bool [B,Q,S], margin)."""
    v32, v64 = R.resized(pred, size), R.resized(pred.double(), size)
    margin = 4 * float((v32.double() - v64).abs().max()) + 2.0 ** -22
    return v64.abs() > margin, margin


@functools.lru_cache(maxsize=None)
def bits_case(kind, size):
    """(logits [2,5,64,64], expected bool [2,5,S] by the reference's statements with one head, decided, margin); kind 'planted' / 'seeded'."""
    pred = R.planted_mask_pred() if kind == 'planted' else torch.from_numpy(R.golden()['mask_pred'])
    S = size[0] * size[1]
    want = R.unpack_bits(R.pack_bits(R.box2mask_mask(pred, size, 1)), S).view(*R.MASK_SHAPE, S)
    decided, margin = decided_bits(pred, size)
    return pred, want, decided, margin


@functools.lru_cache(maxsize=None)
def pack_case(shape):
    rows, Q, S, M = shape
    mask = torch.rand(rows, Q, S, generator=torch.Generator().manual_seed(6 + S)) < 0.5
    mask[0, 1, :] = True                                              # an all-set row: pack_attn_mask does not repair
    return mask, M
