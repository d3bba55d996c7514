"""CPU: the cases of tests/attn_edges.py do what they claim (no kernel is launched here; the reference alone).

* every tolerance case reaches the trip it is named for, by arithmetic from _lib.ATTN_SPAN and the kernels' 128 / 32 / KC / 8: a change of
  BXI_ATTN_SPAN fails here instead of quietly un-testing the edges;
* the dominant-key cases: the gap between a row's hot key and every other unmasked key is what makes fp32 expf exactly 0, torch's own fp32
  attention already returns exactly the hot key's v row, and the picks put hot keys before and after cooler ones, in and across spans;
* the re-layout cases hold the same data;
* the mask-bit sizes reach more than one trip with a partial last word, the planted rows are what they were planted for at those sizes, and
  the seeded logits leave the decided-bits rule room under its cap."""
import pytest
import torch

from tests import attn_edges as E
from tests import masked_attn_ref as R

SP = E.span()

# name -> the entries of E.trips that the case is there for
REACHES = {
    'spans9': dict(nspans=9, batches=2, last_batch=1, last_span_keys=1, last_tile_keys=1, q_groups=1, last_block_queries=1),
    'spans9_dead': dict(nspans=9, batches=2, last_batch=1, last_span_keys=1),
    'spans17': dict(nspans=17, batches=3, last_batch=1, last_span_keys=1, last_tile_keys=1),
    'spans17_dead': dict(nspans=17, batches=3, last_batch=1, last_span_keys=1),
    'spans9_full_D64': dict(nspans=9, batches=2, last_batch=1, last_span_keys=SP, last_chunk_keys=64, last_tile_keys=32),
    'one_group_one_span': dict(nspans=1, q_groups=1, last_group_queries=128, last_group_waves=4, last_block_queries=32, last_span_keys=SP,
                               last_chunk_keys=128, last_tile_keys=32),
    'second_group_of_one_query': dict(nspans=2, last_span_keys=1, q_groups=2, last_group_queries=1, last_group_waves=1, q_blocks=5,
                                      last_block_queries=1),
    'three_groups': dict(nspans=1, q_groups=3, last_group_queries=1, last_group_waves=1, last_chunk_keys=40, last_tile_keys=8),
    'kc64_chunk_of_one_key': dict(nspans=1, last_chunk_keys=1, last_tile_keys=1, q_blocks=1, last_block_queries=32),
    'kc64_one_chunk': dict(nspans=1, last_span_keys=64, last_chunk_keys=64, last_tile_keys=32, q_blocks=2, last_block_queries=32),
    'kc128_chunk_of_one_key': dict(nspans=1, last_chunk_keys=1, last_tile_keys=1, q_blocks=1, last_block_queries=31),
    'one_query_one_key': dict(nspans=1, last_span_keys=1, q_groups=1, last_group_queries=1, q_blocks=1, last_block_queries=1),
    'heads8': dict(nspans=2, last_span_keys=300 - SP),
    'images3_mask3d': dict(nspans=2),
    'images3_mask2d': dict(nspans=2),
}


def test_the_kernel_constants_the_cases_are_built_around():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'boxinstseg_amd/csrc/masked_attn.hip')) as fh:
        code = fh.read()
    assert 'KC = D == 64 ? 64 : 128' in code and re.search(r'qblock = \(\(int\)blockIdx\.z \* 4 \+ wave\) \* 32', code)
    assert 'i0 += 8' in code and 'q0 += 32' in code and 'base += 256' in code
    assert (E.kc(16), E.kc(32), E.kc(64)) == (128, 128, 64) and (E.Q_GROUP, E.Q_BLOCK, E.TILE, E.SPAN_BATCH, E.BITS_TRIP) == (128, 32, 32, 8, 256)
    assert SP % 128 == 0 and SP >= 256                                # the chunk and tile edges below lie inside the first span


@pytest.mark.parametrize('name', E.TOL_NAMES)
def test_tolerance_case_reaches_its_trip(name):
    assert sorted(REACHES) == sorted(E.TOL_NAMES)
    s = E.tol_shapes()[name]
    got = E.trips(s['Q'], s['S'], s['D'])
    for key, want in REACHES[name].items():
        assert got[key] == want, (name, key, got)
    t, ref32, ref64, M = E.tol_case(name)
    Q, S, D, B = s['Q'], s['S'], s['D'], s['B']
    assert M == s['M'] and t['q'].shape == (Q, B, M * D) and t['k'].shape == (S, B, M * D)
    assert t['mask'].shape == ((Q, S) if s.get('mask_2d') else (B * M, Q, S))
    assert not bool(t['mask'].all(-1).any())                          # no row without a key: nothing is NaN
    assert all(bool(torch.isfinite(ref64[n]).all()) for n in ref64)
    if s.get('keep_spans'):                                           # row 0: keys only in the named spans, and in each of them
        kept = (~t['mask'][:, 0]).nonzero()[:, 1] // SP
        assert sorted(set(kept.tolist())) == list(s['keep_spans']) and min(s['keep_spans']) >= E.SPAN_BATCH
        assert got['nspans'] - 1 in s['keep_spans']
    if name == 'heads8':
        assert (B, M) == (1, 8)
    if name.startswith('images3'):
        assert (B, M) == (3, 1)


def test_one_query_one_key_has_bound_zero():
    """The reference's own fp32 run is exact here, so 4 x its error is 0: out == v, dv == g, dq == 0 and dk == 0 bit for bit."""
    t, ref32, ref64, M = E.tol_case('one_query_one_key')
    assert not bool(t['mask'].any())
    for n in ref32:
        assert torch.equal(ref32[n].double(), ref64[n]) and R.bound(ref32[n], ref64[n]) == 0.0, n
    assert torch.equal(ref32['out'], t['v']) and torch.equal(ref32['dv'], t['g'])
    assert float(ref32['dq'].abs().max()) == 0.0 and float(ref32['dk'].abs().max()) == 0.0


@pytest.mark.parametrize('shape,D', E.DOMINANT, ids=lambda v: str(v))
def test_dominant_key_case(shape, D):
    c = E.dominant_case(shape, D)
    Q, S, hot = E.dominant_shape(shape, D)
    B, M = c['B'], c['M']
    assert c['hot'] == hot and len(hot) == len(set(hot)) and hot[0] == 0 and hot[-1] == S - 1
    edges = {0, 31, 32, SP - 1, S - 1}
    edges |= {E.kc(D) - 1, E.kc(D), SP, SP + 44} if shape == 'three_spans' else {7 * SP, 7 * SP + 44, 8 * SP - 1, 8 * SP}
    assert edges == set(hot)
    if shape == 'nine_spans':
        assert E.trips(Q, S, D)['nspans'] == 9 and {h // SP for h in hot} == {0, 7, 8}
    else:
        assert E.trips(Q, S, D)['nspans'] == 3 and {h // SP for h in hot} == {0, 1, 2}
    is_hot = torch.zeros(S, dtype=torch.bool)
    is_hot[torch.tensor(hot)] = True
    keep = ~c['mask']
    assert bool((keep[:, :, is_hot].sum(-1) == 1).all())              # one hot key per row ...
    assert bool(keep[torch.arange(B * M)[:, None], torch.arange(Q)[None], c['pick']].all())    # ... and it is the pick
    # the gap
    s = E.dominant_scores(c)
    top = s.gather(-1, c['pick'][..., None])[..., 0]
    rest = s.scatter(-1, c['pick'][..., None], float('-inf')).max(-1).values
    gap = float((top - rest).min())
    print(f'{shape} D={D}: hot score >= {float(top.min()):.1f}, every other <= {float(rest.max()):.2f}, gap >= {gap:.1f}')
    assert gap > E.EXP_IS_ZERO and bool(torch.isfinite(rest).all())   # every row has cooler unmasked keys
    if D <= 32:
        assert gap > 200
    assert float(torch.exp(torch.tensor(-E.EXP_IS_ZERO, dtype=torch.float32))) == 0.0
    # hot keys before and after cooler unmasked keys: inside the first tile's span and across spans
    cool = keep & ~is_hot
    pos = torch.arange(S)
    first_cool = torch.where(cool, pos, S).min(-1).values
    last_cool = torch.where(cool, pos, -1).max(-1).values
    assert bool((c['pick'] < first_cool).any()) and bool((c['pick'] > last_cool).any())
    assert bool((c['pick'] // SP < last_cool // SP).any()) and bool((c['pick'] // SP > first_cool // SP).any())
    assert bool(((c['pick'] > first_cool) & (c['pick'] < last_cool)).any())
    # hot keys seen by exactly one query
    assert len(c['solo']) == 4 * B * M
    for bm, key, row in c['solo']:
        assert int(c['pick'][bm, row]) == key and int((c['pick'][bm] == key).sum()) == 1
    assert len({key for _, key, _ in c['solo']}) >= 4
    # torch's own fp32 attention is already exact
    out = R.mha_torch(c['q'], c['k'], c['v'], c['mask'], M, R.identity_params(M * D, torch.float32))
    want, hot_rows = E.dominant_want(c)
    assert torch.equal(out, want) and torch.equal(hot_rows, is_hot)


@pytest.mark.parametrize('D', E.PAD_DIMS)
def test_padding_case(D):
    t, padded = E.padding_case(D)
    S0 = t['k'].shape[0]
    assert S0 == SP + 44 and sorted(padded) == [2 * SP, 2 * SP + 5]
    assert E.trips(40, S0, D)['nspans'] == E.trips(40, 2 * SP, D)['nspans'] == 2 and E.trips(40, 2 * SP + 5, D)['nspans'] == 3
    assert S0 % 32 != 0                                               # the tail predicate cuts inside a tile
    ref = R.core_with_grads(t, 2, torch.float64)
    for S, p in padded.items():
        assert p['k'].shape[0] == p['v'].shape[0] == p['mask'].shape[-1] == S
        assert torch.equal(p['k'][:S0], t['k']) and torch.equal(p['v'][:S0], t['v']) and torch.equal(p['mask'][..., :S0], t['mask'])
        assert bool(p['mask'][..., S0:].all()) and torch.equal(p['q'], t['q']) and torch.equal(p['g'], t['g'])
        tail = torch.cat([p['k'][S0:], p['v'][S0:]]).abs()
        assert bool(torch.isfinite(tail).all()) and 100 < float(tail.max()) < 1e4
        got = R.core_with_grads(p, 2, torch.float64)                  # the reference agrees that masked padding changes nothing
        assert float((got['out'] - ref['out']).abs().max()) < 1e-12 and float((got['dk'][:S0] - ref['dk']).abs().max()) < 1e-12
        assert float(got['dk'][S0:].abs().max()) == 0.0 and float(got['dv'][S0:].abs().max()) == 0.0


def test_company_and_crowd_cases():
    c = E.company_case()
    assert c['q'].shape == (40, 2, 256) and c['mask'].shape == (16, 40, SP + 44) and c['image_mask'].shape == (2, 40, SP + 44)
    assert E.COMPANY_HEADS[0] == (0, 0) and E.COMPANY_HEADS[-1] == (1, 7) and 0 < E.COMPANY_HEADS[1][1] < 7
    assert not bool(c['image_mask'].all(-1).any())
    full = R.core_with_grads(c, 8, torch.float64)
    for b, m in E.COMPANY_HEADS:
        t = E.head_alone(c, b, m, True)
        assert all(t[n].is_contiguous() for n in t) and t['q'].shape == (40, 1, 32) and t['mask'].shape == (1, 40, SP + 44)
        alone = R.core_with_grads(t, 1, torch.float64)
        for n in alone:
            assert float((alone[n][:, 0] - full[n][:, b, m * 32:(m + 1) * 32]).abs().max()) < 1e-12, n
        assert torch.equal(E.head_alone(c, b, m, False)['mask'][0], c['mask'][b * 8])
    t = E.crowd_case()
    assert t['q'].shape == (257, 2, 64) and E.trips(257, SP + 44, 32)['last_group_queries'] == 1
    assert E.CROWD_ROWS == (0, 31, 32, 127, 128, 255, 256)
    one = E.query_alone(t, 128)
    assert one['q'].shape == (1, 2, 64) and one['mask'].shape == (4, 1, SP + 44) and torch.equal(one['mask'][:, 0], t['mask'][:, 128])
    g = E.only_row(t['g'], 128)
    assert torch.equal(g[128], t['g'][128]) and int((g != 0).any(-1).any(-1).sum()) == 1


# ---- mask bits -------------------------------------------------------------------------------------------------------------------------
def test_bits_sizes_reach_a_second_trip_and_a_partial_word():
    assert E.bits_trips(17 * 19) == (2, 323 - 256, 3)                 # two trips, a partial last word
    assert E.bits_trips(9 * 29) == (2, 5, 5)                          # a second trip of 5 positions
    assert E.bits_trips(33) == (1, 33, 1) and E.bits_trips(25 * 42)[0] == 5 and E.bits_trips(50 * 84)[0] == 17
    assert all(E.bits_trips(h * w)[2] != 32 for h, w in E.BITS_SEEDED_SIZES)
    for rows, Q, S, M in E.PACK_SHAPES:
        assert E.bits_trips(S)[0] == 2 and E.bits_trips(S)[2] != 32 and rows % M == 0
        mask, _ = E.pack_case((rows, Q, S, M))
        assert bool(mask[0, 1].all()) and not bool(mask[0, 0].all())


@pytest.mark.parametrize('size', E.BITS_PLANTED_SIZES, ids=lambda s: '%dx%d' % s)
def test_bits_planted_rows_at_odd_sizes(size):
    pred, want, decided, margin = E.bits_case('planted', size)
    v = R.resized(pred.double(), size)
    assert bool((v[0, 1] < -0.5).all()) and bool(decided[0, 1].all()) and not bool(want[0, 1].any())     # all negative: repaired to all clear
    assert float(v[1, 3].abs().max()) == 0.0 and not bool(want[1, 3].any())                               # all zero: nothing masked
    other = torch.ones(2, 5, dtype=torch.bool)
    other[0, 1] = other[1, 3] = False
    assert bool(want[other].any()) and not bool(want[other].all(-1).any()) and bool(decided[other].any())


@pytest.mark.parametrize('size', E.BITS_SEEDED_SIZES, ids=lambda s: '%dx%d' % s)
def test_bits_seeded_logits_leave_room_under_the_cap(size):
    pred, want, decided, margin = E.bits_case('seeded', size)
    excluded, cap = int((~decided).sum()), 1e-3 * decided.numel()
    print(f'{size}: {excluded} of {decided.numel()} bits within {margin:.3e} of zero; cap {cap:.2f}')
    assert excluded <= cap and excluded <= 1
    v64 = R.resized(pred.double(), size)
    assert torch.equal(want[decided], (v64 < 0)[decided])             # no row of the seeded logits is all negative: no repair here
