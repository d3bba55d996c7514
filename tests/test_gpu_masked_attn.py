"""GPU: the masked attention of csrc/masked_attn.hip against torch's own nn.MultiheadAttention on the CPU (tests/masked_attn_ref.py).

The yardstick: out, dq, dk and dv stay within 4 x the fp32 error of statement (i) against its own fp64 run on the same inputs (computed
here, once per case).  On top of it cases without any tolerance (a row with one unmasked key, q = 0 with 2^n unmasked keys), planted rows
(two wholly masked spans, scores of magnitude 200, no mask, a 2-D mask, an all-masked row), the mask bits against the reference's statements, run-to-run
identity, the module end to end and the memory bound of forward + backward."""
import functools

import pytest
import torch

from tests import masked_attn_ref as R

pytestmark = pytest.mark.gpu

B_, M_ = 2, 2
# (Q, S, D): the smallest shapes that reach each path (one span / several, a tail tile, one query / several query blocks, every head dimension)
SHAPES = [(100, 35, 32), (33, 1000, 32), (1, 64, 32), (100, 32 * 33, 16), (37, 257, 64),
          (150, 70, 32)]                                              # more than 128 queries: a second group of query blocks in the forward


def _span():
    from boxinstseg_amd import _lib
    return _lib.ATTN_SPAN


def _three_spans():
    return (40, 2 * _span() + 70, 32)                                 # at least three spans whatever the span length is


@functools.lru_cache(maxsize=None)
def _case(Q, S, D, kind='masked'):
    t = R.make_case(1000 + Q + S + D, Q, S, D, B_, M_, mask=kind != 'none', spread=8.0 if kind == 'hot' else 1.0)
    if kind == 'dead_spans':                                          # row 0 of every (b, m): nothing in the first two spans
        t['mask'][:, 0, :2 * _span()] = True
        t['mask'][:, 0, 2 * _span() + 3] = False
    ref32, ref64 = R.core_with_grads(t, M_, torch.float32), R.core_with_grads(t, M_, torch.float64)
    return t, ref32, ref64


def _run(t, dev):
    import boxinstseg_amd as B
    q, k, v = (t[n].to(dev).requires_grad_(True) for n in ('q', 'k', 'v'))
    m = None
    if t.get('mask') is not None:
        m = B.pack_attn_mask(t['mask'].to(dev), M_)
    out = B.masked_attention(q, k, v, m, M_)
    out.backward(t['g'].to(dev))
    return {'out': out.detach().cpu(), 'dq': q.grad.cpu(), 'dk': k.grad.cpu(), 'dv': v.grad.cpu()}


def _close(got, ref32, ref64, what):
    err, bound = float((got.double() - ref64).abs().max()), R.bound(ref32, ref64) * float(ref64.abs().max())
    print(f'{what}: max error {err:.3e}, bound {bound:.3e} (4 x the fp32 error of torch.nn.MultiheadAttention)')
    assert bool(torch.isfinite(got).all()) and err <= bound, what


def _check(t, ref32, ref64, dev, what):
    got = _run(t, dev)
    for name in ('out', 'dq', 'dk', 'dv'):
        assert got[name].shape == ref64[name].shape
        _close(got[name], ref32[name], ref64[name], f'{what} {name}')
    return got


@pytest.mark.parametrize('shape', SHAPES + ['three_spans'], ids=lambda s: s if isinstance(s, str) else 'Q%d_S%d_D%d' % s)
def test_against_torch_mha(dev, shape):
    Q, S, D = _three_spans() if shape == 'three_spans' else shape
    if shape == 'three_spans':
        assert (S + _span() - 1) // _span() >= 3
    t, ref32, ref64 = _case(Q, S, D)
    _check(t, ref32, ref64, dev, f'Q={Q} S={S} D={D}')


@pytest.mark.parametrize('kind', ['dead_spans', 'hot', 'none'])
def test_planted(dev, kind):
    Q, S, D = _three_spans()
    t, ref32, ref64 = _case(Q, S, D, kind)
    if kind == 'hot':                                                 # exp(200) overflows fp32: only the max subtraction keeps this finite
        scores = torch.einsum('qbmd,sbmd->bmqs', t['q'].view(Q, B_, M_, D), t['k'].view(S, B_, M_, D)) / D ** 0.5
        assert float(scores.masked_fill(t['mask'].view(B_, M_, Q, S), 0).abs().max()) > 200
    if kind == 'none':
        assert 'mask' not in t
    _check(t, ref32, ref64, dev, kind)


def test_one_mask_for_every_image_and_head(dev):
    """torch's 2-D attn_mask [Q,S]: packed once, read by every (image, head)."""
    import boxinstseg_amd as B
    Q, S, D = _three_spans()
    t = dict(_case(Q, S, D)[0])
    t['mask'] = t['mask'][0].clone()
    ref32, ref64 = R.core_with_grads(t, M_, torch.float32), R.core_with_grads(t, M_, torch.float64)
    q, k, v = (t[n].to(dev).requires_grad_(True) for n in ('q', 'k', 'v'))
    m = B.pack_attn_mask(t['mask'].to(dev), M_)
    assert not m.per_head and tuple(m.bits.shape) == (1, Q, (S + 31) // 32)
    out = B.masked_attention(q, k, v, m, M_)
    out.backward(t['g'].to(dev))
    for name, got in (('out', out.detach()), ('dq', q.grad), ('dk', k.grad), ('dv', v.grad)):
        _close(got.cpu(), ref32[name], ref64[name], f'2-D mask {name}')


def test_all_masked_row_is_nan_in_that_row_only(dev):
    import boxinstseg_amd as B
    Q, S, D = _three_spans()
    t = dict(_case(Q, S, D)[0])
    t['mask'] = t['mask'].clone()
    t['mask'][1 * M_ + 0, 5] = True                                   # image 1, head 0, query 5
    out = B.masked_attention(t['q'].to(dev), t['k'].to(dev), t['v'].to(dev), B.pack_attn_mask(t['mask'].to(dev), M_), M_).cpu()
    nan = torch.isnan(out)
    want = torch.zeros_like(nan)
    want[5, 1, 0:D] = True
    assert torch.equal(nan, want)
    ref = R.mha_torch(t['q'], t['k'], t['v'], t['mask'], M_, R.identity_params(M_ * D, torch.float32))
    want[5, 1, :] = True                                              # torch gives NaN there too; its out-projection (NaN * 0) spreads it over
    assert torch.equal(torch.isnan(ref), want)                        # the row's other head, which the core alone leaves finite


def test_one_unmasked_key_is_exact(dev):
    """Rows 3, 11 and 35 of every (b, m) see only key 5 (first span), row 7 only key S - 2 (last span), and nobody else sees those keys:
    out is that v row, dq is 0, and dv of key 5 is dout of rows 3, 11, 35 added in that order -- all bit for bit."""
    Q, S, D = _three_spans()
    t = dict(_case(Q, S, D)[0])
    mask = t['mask'].clone()
    first, last, rows = 5, S - 2, (3, 11, 35)
    mask[:, :, first] = True
    mask[:, :, last] = True
    for r in rows + (7,):
        mask[:, r, :] = True
    for r in rows:
        mask[:, r, first] = False
    mask[:, 7, last] = False
    t['mask'] = mask
    got = _run(t, dev)
    E = M_ * D
    for r, key in [(r, first) for r in rows] + [(7, last)]:
        assert torch.equal(got['out'][r].view(torch.int32), t['v'][key].view(torch.int32)), (r, key)
        assert float(got['dq'][r].abs().max()) == 0.0 and got['dq'][r].shape == (B_, E)
    want = (t['g'][3] + t['g'][11]) + t['g'][35]
    assert torch.equal(got['dv'][first].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got['dv'][last].view(torch.int32), t['g'][7].view(torch.int32))
    assert float(got['dk'][first].abs().max()) == 0.0                # softmax over one key: no gradient reaches the scores


def test_zero_query_is_the_exact_mean(dev):
    """q = 0: every unmasked key weighs the same.  With 64 unmasked keys spread over all spans and v in quarters the mean is exact."""
    import boxinstseg_amd as B
    Q, S, D = _three_spans()
    g = torch.Generator().manual_seed(9)
    t = dict(_case(Q, S, D)[0])
    v = torch.randint(-8, 9, (S, B_, M_ * D), generator=g).float() / 4
    mask = torch.ones(B_ * M_, Q, S, dtype=torch.bool)
    for r in range(B_ * M_):
        for qi in range(Q):
            mask[r, qi, torch.randperm(S, generator=g)[:64]] = False
    assert bool((~mask[:, :, :_span()]).any()) and bool((~mask[:, :, 2 * _span():]).any())
    out = B.masked_attention(torch.zeros(Q, B_, M_ * D, device=dev), t['k'].to(dev), v.to(dev), B.pack_attn_mask(mask.to(dev), M_), M_).cpu()
    keep = (~mask).view(B_, M_, Q, S).double()
    want = torch.einsum('bmqs,sbmd->qbmd', keep, v.double().view(S, B_, M_, D)).reshape(Q, B_, M_ * D) / 64
    assert torch.equal(want.float().double(), want) and torch.equal(out.view(torch.int32), want.float().view(torch.int32))


def test_run_to_run_identical(dev):
    Q, S, D = _three_spans()
    t = _case(Q, S, D)[0]
    a, b = _run(t, dev), _run(t, dev)
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


# ---- mask bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.MASK_CASES))
def test_mask_bits_against_the_reference_statements(dev, name):
    import boxinstseg_amd as B
    g = R.golden()
    H, W, h, w = R.MASK_CASES[name]
    pred = torch.from_numpy(g['mask_pred'])
    m = B.box2mask_attn_mask(pred.to(dev), (h, w))
    S = h * w
    assert isinstance(m, B.PackedAttnMask) and (m.S, m.per_head) == (S, False) and tuple(m.bits.shape) == (2, 5, (S + 31) // 32)
    got = R.unpack_bits(m.bits.cpu(), m.bits.shape[-1] * 32)
    assert not bool(got[..., S:].any())                               # tail bits clear
    got = got[..., :S]
    want = R.unpack_bits(torch.from_numpy(g[f'bits_{name}']), S).view(2, R.MASK_HEADS, 5, S)[:, 0]      # the heads' copies are equal
    v32, v64 = R.resized(pred, (h, w)), R.resized(pred.double(), (h, w))
    margin = 4 * float((v32.double() - v64).abs().max()) + 2.0 ** -22
    decided = v64.abs() > margin
    excluded = int((~decided).sum())
    print(f'{name}: {excluded} of {decided.numel()} bits within {margin:.3e} of zero; {int((got != want).sum())} bits differ in all')
    assert excluded <= 1e-3 * decided.numel()
    assert torch.equal(got[decided], want[decided])


def test_mask_bits_planted_exact(dev):
    """Integer logits at factor 8 (weights 1/2 * 1/2): no exclusion at all.  Values exactly 0 are not masked, whole rows negative are repaired."""
    import boxinstseg_amd as B
    g = R.golden()
    pred = torch.from_numpy(g['planted']).float()
    m = B.attn_mask_bits(pred.to(dev), (8, 8))
    want = torch.from_numpy(g['planted_bits_f8']).view(2, R.MASK_HEADS, 5, 2)[:, 0]
    assert torch.equal(m.bits.cpu(), want)
    got = R.unpack_bits(m.bits.cpu(), 64)
    assert not bool(got[0, 1].any()) and not bool(got[0, 2, 0]) and not bool(got[0, 2, 8]) and not bool(got[1, 3].any()) and bool(got.any())


def test_pack_attn_mask_is_the_bits_of_the_mask(dev):
    import boxinstseg_amd as B
    g = torch.Generator().manual_seed(4)
    for shape in ((B_ * M_, 7, 35), (3, 300), (B_ * M_, 2, 64)):
        mask = torch.rand(*shape, generator=g) < 0.5
        mask[..., 0, :] = True                                        # an all-set row stays all set
        m = B.pack_attn_mask(mask.to(dev), M_)
        want = R.pack_bits(mask)
        assert m.per_head == (len(shape) == 3) and m.S == shape[-1]
        assert torch.equal(m.bits.cpu(), want if len(shape) == 3 else want[None])


# ---- the module ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['packed', 'repeated_bool', 'self_attention'])
def test_module_against_the_restated_wrapper(dev, how):
    import boxinstseg_amd as B
    M, E, Q, size = 2, 64, 5, (8, 8)
    S = size[0] * size[1]
    gen = torch.Generator().manual_seed(21)
    pred = torch.from_numpy(R.golden()['mask_pred'])
    ref_mask = R.box2mask_mask(pred, size, M)
    ins = {n: torch.randn(*s, generator=gen) for n, s in (('query', (Q, 2, E)), ('key', (S, 2, E)), ('query_pos', (Q, 2, E)), ('key_pos', (S, 2, E)),
                                                           ('g', (Q, 2, E)))}
    params = {f'attn.{k}': v for k, v in R.random_params(E, 8).items()}

    def run_ref(dtype):
        ref = R.RefMultiheadAttention(E, M, dropout_layer=None).to(dtype)
        ref.load_state_dict({k: v.to(dtype) for k, v in params.items()})
        x = {n: v.to(dtype) for n, v in ins.items()}
        if how == 'self_attention':
            out = ref(x['query'], query_pos=x['query_pos'], attn_mask=None)
        else:
            out = ref(x['query'], x['key'], x['key'], query_pos=x['query_pos'], key_pos=x['key_pos'], attn_mask=ref_mask)
        (out * x['g']).sum().backward()
        return {'out': out.detach(), **{k: p.grad for k, p in ref.named_parameters()}}

    ref32, ref64 = run_ref(torch.float32), run_ref(torch.float64)
    mine = B.MultiheadAttention(E, M, dropout_layer=None)
    mine.load_state_dict({k: v.float() for k, v in params.items()})
    mine = mine.to(dev)
    x = {n: v.to(dev) for n, v in ins.items()}
    if how == 'self_attention':
        out = mine(x['query'], query_pos=x['query_pos'], attn_mask=None)
    else:
        mask = B.box2mask_attn_mask(pred.to(dev), size) if how == 'packed' else ref_mask.to(dev)
        out = mine(x['query'], x['key'], x['key'], query_pos=x['query_pos'], key_pos=x['key_pos'], attn_mask=mask)
    (out * x['g']).sum().backward()
    got = {'out': out.detach().cpu(), **{k: p.grad.cpu() for k, p in mine.named_parameters()}}
    assert sorted(got) == sorted(ref64)
    for name in got:
        _close(got[name], ref32[name], ref64[name], f'{how} {name}')


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def test_memory_stays_below_one_score_matrix(dev):
    import boxinstseg_amd as B
    Bm, M, Q, S, D = 1, 8, 100, 4096, 32
    gen = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(n, Bm, M * D, generator=gen).to(dev).requires_grad_(True) for n in (Q, S, S))
    g = torch.randn(Q, Bm, M * D, generator=gen).to(dev)
    mask = B.pack_attn_mask((torch.rand(Bm * M, Q, S, generator=gen) < 0.5).to(dev), M)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = B.masked_attention(q, k, v, mask, M)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print(f'peak above the inputs {peak} bytes; one score matrix {Bm * M * Q * S * 4} bytes')
    assert bool(torch.isfinite(q.grad).all()) and peak < Bm * M * Q * S * 4
