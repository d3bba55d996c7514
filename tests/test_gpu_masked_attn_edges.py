"""GPU: csrc/masked_attn.hip at the span counts and block edges the workload hits, on the cases of tests/attn_edges.py (checked on the
CPU by tests/test_host_masked_attn_edges.py).

1. tolerance cases with the yardstick of tests/test_gpu_masked_attn.py (4 x the fp32 error of torch.nn.MultiheadAttention against its own
   fp64 run): 9 and 17 spans (a second and a third batch of eight in combine and dq), Q on and one past the forward's and the backward's
   block edges, chunks of one key, the configs' head count, three images under a 3-D and under one shared 2-D mask;
2. no tolerance: a key whose score leads by more than 150 wins bit for bit, whether it comes before or after the cooler keys;
3. no tolerance, no reference: the same data laid out two ways (masked padding against a shorter S, a head alone against the head in
   company, a query alone against the query in a crowd) gives the same bits;
4. the mask bits beyond one trip of 256 positions with a partial last word;
5. the module's batch_first and identity arguments."""
import pytest
import torch

from tests import attn_edges as E
from tests import masked_attn_ref as R
from tests.test_gpu_masked_attn import _close

pytestmark = pytest.mark.gpu

NAMES = ('out', 'dq', 'dk', 'dv')


def _run(t, dev, M, per_image=False, g=None):
    """out and the gradients of one call; ``per_image``: t['mask'] is [B,Q,S], one row per image for all its heads."""
    import boxinstseg_amd as B
    q, k, v = (t[n].to(dev).requires_grad_(True) for n in ('q', 'k', 'v'))
    m = None
    if t.get('mask') is not None:
        m = B.pack_attn_mask(t['mask'].to(dev), 1 if per_image else M)
        if per_image:
            m = B.PackedAttnMask(m.bits, m.S, False)
    out = B.masked_attention(q, k, v, m, M)
    out.backward((t['g'] if g is None else g).to(dev))
    return {'out': out.detach().cpu(), 'dq': q.grad.cpu(), 'dk': k.grad.cpu(), 'dv': v.grad.cpu()}


def _same(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and bool(torch.isfinite(a).all()), what
    assert torch.equal(a, b), f'{what}: {int((a != b).sum())} of {a.numel()} elements differ, by at most {float((a - b).abs().max()):.3e}'


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.TOL_NAMES)
def test_against_torch_mha_at_the_edges(dev, name):
    t, ref32, ref64, M = E.tol_case(name)
    got = _run(t, dev, M)
    for n in NAMES:
        assert got[n].shape == ref64[n].shape
        _close(got[n], ref32[n], ref64[n], f'{name} {n}')
    if name == 'one_query_one_key':                                   # the bound is 0: said once more in the kernel's own terms
        assert torch.equal(got['out'], t['v']) and torch.equal(got['dv'], t['g'])
        assert float(got['dq'].abs().max()) == 0.0 and float(got['dk'].abs().max()) == 0.0


def test_shared_2d_mask_is_one_row_for_three_images(dev):
    import boxinstseg_amd as B
    t = E.tol_case('images3_mask2d')[0]
    m = B.pack_attn_mask(t['mask'].to(dev), 1)
    assert not m.per_head and tuple(m.bits.shape) == (1, 40, (300 + 31) // 32)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,D', E.DOMINANT, ids=lambda v: str(v))
def test_dominant_key_wins_bit_for_bit(dev, shape, D):
    c = E.dominant_case(shape, D)
    got = _run(c, dev, c['M'])
    want, is_hot = E.dominant_want(c)
    _same(got['out'], want, 'out is the v row of the hot key')
    assert float(got['dq'].abs().max()) == 0.0 and float(got['dk'].abs().max()) == 0.0      # dP and delta run the same chain
    assert float(got['dv'][~is_hot].abs().max()) == 0.0
    S, Bn, M = c['k'].shape[0], c['B'], c['M']
    dv, g = got['dv'].view(S, Bn * M, D), c['g'].view(-1, Bn * M, D)
    for bm, key, row in c['solo']:
        _same(dv[key, bm], g[row, bm], f'dv of key {key}, seen by query {row} of head {bm} alone')


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', E.PAD_DIMS)
def test_masked_padding_equals_a_shorter_S(dev, D):
    t, padded = E.padding_case(D)
    S0 = t['k'].shape[0]
    base = _run(t, dev, 2)
    for S, p in padded.items():
        got = _run(p, dev, 2)
        for n in ('out', 'dq'):
            _same(got[n], base[n], f'S = {S}: {n}')
        for n in ('dk', 'dv'):
            _same(got[n][:S0].contiguous(), base[n], f'S = {S}: {n} of the real keys')
            assert float(got[n][S0:].abs().max()) == 0.0, f'S = {S}: {n} of the padding'


@pytest.mark.parametrize('per_head', [True, False], ids=['mask_per_head', 'mask_per_image'])
def test_a_head_alone_equals_the_head_in_company(dev, per_head):
    c = E.company_case()
    M, D = c['M'], c['D']
    full = _run(c if per_head else dict(c, mask=c['image_mask']), dev, M, per_image=not per_head)
    for b, m in E.COMPANY_HEADS:
        alone = _run(E.head_alone(c, b, m, per_head), dev, 1)
        for n in NAMES:
            _same(alone[n][:, 0], full[n][:, b, m * D:(m + 1) * D].contiguous(), f'head ({b}, {m}) {n}')


def test_a_query_alone_equals_the_query_in_a_crowd(dev):
    t = E.crowd_case()
    crowd = _run(t, dev, 2)
    for r in E.CROWD_ROWS:
        one = E.query_alone(t, r)
        alone = _run(one, dev, 2)
        _same(alone['out'][0], crowd['out'][r], f'out of query {r}')
        _same(alone['dq'][0], crowd['dq'][r], f'dq of query {r}')
        onto_keys = _run(t, dev, 2, g=E.only_row(t['g'], r))          # every other row adds 0 * p and p * (0 - 0)
        for n in ('dk', 'dv'):
            _same(alone[n], onto_keys[n], f'{n} from query {r} alone')


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def _bits(dev, kind, size):
    import boxinstseg_amd as B
    pred, want, decided, margin = E.bits_case(kind, size)
    S = size[0] * size[1]
    m = B.attn_mask_bits(pred.to(dev), size)
    assert isinstance(m, B.PackedAttnMask) and (m.S, m.per_head) == (S, False) and tuple(m.bits.shape) == (2, 5, (S + 31) // 32)
    got = R.unpack_bits(m.bits.cpu(), m.bits.shape[-1] * 32)
    assert not bool(got[..., S:].any())                               # tail bits clear
    got = got[..., :S]
    excluded = int((~decided).sum())
    print(f'{kind} {size}: excluded / total = {excluded} / {decided.numel()} (within {margin:.3e} of zero); {int((got != want).sum())} bits differ in all')
    assert torch.equal(got[decided], want[decided])
    return got, excluded, decided.numel()


@pytest.mark.parametrize('size', E.BITS_PLANTED_SIZES, ids=lambda s: '%dx%d' % s)
def test_mask_bits_planted_rows_beyond_one_trip(dev, size):
    got, _, _ = _bits(dev, 'planted', size)
    assert not bool(got[0, 1].any())                                  # negative everywhere: all set, so repaired to all clear
    assert not bool(got[1, 3].any())                                  # all zero: 0 is not masked
    assert bool(got.any())


@pytest.mark.parametrize('size', E.BITS_SEEDED_SIZES, ids=lambda s: '%dx%d' % s)
def test_mask_bits_seeded_logits_beyond_one_trip(dev, size):
    _, excluded, total = _bits(dev, 'seeded', size)
    assert excluded <= 1e-3 * total


@pytest.mark.parametrize('shape', E.PACK_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_pack_attn_mask_beyond_one_trip(dev, shape):
    import boxinstseg_amd as B
    mask, M = E.pack_case(shape)
    m = B.pack_attn_mask(mask.to(dev), M)
    assert m.per_head and m.S == shape[2]
    assert torch.equal(m.bits.cpu(), R.pack_bits(mask))
    assert bool(R.unpack_bits(m.bits.cpu()[0, 1], shape[2]).all())    # the all-set row stays all set: no repair here


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['batch_first', 'identity'])
def test_module_arguments_against_the_restated_wrapper(dev, how):
    import boxinstseg_amd as B
    M, Em, Q, size, bf = 2, 64, 5, (8, 8), how == 'batch_first'
    S = size[0] * size[1]
    gen = torch.Generator().manual_seed(22)
    pred = torch.from_numpy(R.golden()['mask_pred'])
    ref_mask = R.box2mask_mask(pred, size, M)
    shape = lambda L: (2, L, Em) if bf else (L, 2, Em)                # noqa: E731
    ins = {n: torch.randn(*shape(L), generator=gen) for n, L in (('query', Q), ('key', S), ('query_pos', Q), ('key_pos', S), ('g', Q), ('identity', Q))}
    params = {f'attn.{k}': v for k, v in R.random_params(Em, 8).items()}
    kw = lambda x: dict(identity=x['identity'] if how == 'identity' else None, query_pos=x['query_pos'], key_pos=x['key_pos'])  # noqa: E731

    def run_ref(dtype):
        ref = R.RefMultiheadAttention(Em, M, dropout_layer=None, batch_first=bf).to(dtype)
        ref.load_state_dict({k: v.to(dtype) for k, v in params.items()})
        x = {n: v.to(dtype).clone().requires_grad_(n == 'identity') for n, v in ins.items()}      # a copy: ins stays without grad
        out = ref(x['query'], x['key'], x['key'], attn_mask=ref_mask, **kw(x))
        (out * x['g']).sum().backward()
        res = {'out': out.detach(), **{k: p.grad for k, p in ref.named_parameters()}}
        if how == 'identity':
            res['d_identity'] = x['identity'].grad
        return res

    ref32, ref64 = run_ref(torch.float32), run_ref(torch.float64)
    mine = B.MultiheadAttention(Em, M, dropout_layer=None, batch_first=bf)
    mine.load_state_dict({k: v.float() for k, v in params.items()})
    mine = mine.to(dev)
    x = {n: v.to(dev).requires_grad_(n == 'identity') for n, v in ins.items()}
    out = mine(x['query'], x['key'], x['key'], attn_mask=B.box2mask_attn_mask(pred.to(dev), size), **kw(x))
    assert out.shape == ins['query'].shape
    (out * x['g']).sum().backward()
    got = {'out': out.detach().cpu(), **{k: p.grad.cpu() for k, p in mine.named_parameters()}}
    if how == 'identity':
        got['d_identity'] = x['identity'].grad.cpu()
        assert torch.equal(got['d_identity'], ins['g'])               # identity is added, nothing else touches it
    assert sorted(got) == sorted(ref64)
    for name in got:
        _close(got[name], ref32[name], ref64[name], f'{how} {name}')
