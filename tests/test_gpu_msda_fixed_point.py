"""GPU: the four promises include/boxinst/boxinst_hip_msda.h makes about the fixed-point grad_value of csrc/msda.hip, each held sharply.

* exact cases: on inputs that are small dyadic rationals (tests/msda_ref.py:dyadic_case) every intermediate of the restatement is exact in
  fp32 (tests/test_host_msda.py checks that for the restatement alone), and with Mx a power of two so is the fixed-point path: out and every
  gradient equal the fp64 results BIT FOR BIT.  No tolerance.
* quantisation: with Mx = 7, and with one batch item 2^-32 below the other, |grad_value - fp64| <= n 2^-41 Mx + 2^-23 |fp64| element by
  element, n the number of corners that land on the cell (msda_ref.cell_hits).
* order independence: a permutation of the queries changes no bit of grad_value; scaling grad_out or the weights by 2^+-40 scales every
  gradient exactly.
* Mx == 0 (an all-zero grad_out, all-zero plain weights): zeros, +0 bits in grad_value, nothing non-finite.
* non-finite input: NaN / infinity in grad_out or the plain weights turn every element of grad_value into NaN; a NaN logit of the fused form
  takes its (b, q, m) out of grad_value and nothing else.
* no host synchronisation, forward and backward, both forms, with the level tensors on the device."""
import pytest
import torch

from tests import guarded as G
from tests import msda_ref as R

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(name, gmax, scale_b1):
    """The fp64 results of one dyadic case, computed once."""
    key = (name, gmax, scale_b1)
    if key not in _WANT:
        t, spec = R.dyadic(*key)
        _WANT[key] = R.run_case({k: v.double() for k, v in t.items()}, spec)
    return _WANT[key]


def _levels(spec, dev):
    shapes = [tuple(s) for s in spec['shapes']]
    return torch.tensor(shapes, device=dev), torch.tensor(R.level_starts(shapes), device=dev)


def _run(t, spec, dev):
    """The inputs through the public functions, level tensors on the device: out and every gradient, as CPU tensors."""
    import boxinstseg_amd as B
    ss, ls = _levels(spec, dev)
    value = t['value'].to(dev).requires_grad_(True)
    if spec['fused']:
        leaves = {'grad_offsets': t['off'].to(dev).requires_grad_(True), 'grad_logits': t['logits'].to(dev).requires_grad_(True)}
        out = B.multi_scale_deformable_attn_fused(value, ss, ls, t['ref'].to(dev), leaves['grad_offsets'], leaves['grad_logits'])
    else:
        leaves = {'grad_loc': t['loc'].to(dev).requires_grad_(True), 'grad_attn': t['w'].to(dev).requires_grad_(True)}
        out = B.multi_scale_deformable_attn(value, ss, ls, leaves['grad_loc'], leaves['grad_attn'])
    grads = torch.autograd.grad(out, [value] + list(leaves.values()), t['grad_out'].to(dev))
    res = {'out': out.detach().cpu()}
    res.update({n: g.cpu() for n, g in zip(['grad_value'] + list(leaves), grads)})
    return res


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('name,gmax,scale_b1', R.DYADIC_EXACT)
def test_exact_cases_bit_for_bit(dev, name, gmax, scale_b1):
    """Every intermediate of the kernel is exact on these inputs, as the restatement's is (csrc/msda.hip, the worst of the four cases):
    h, w are multiples of 1/16 below 2^4, so lh, lw, hh, hw have at most 4 fraction bits and a corner weight 8; value is a 4-bit integer:
    the bilinear value is a multiple of 2^-8 below 2^4 (12 bits), times a weight that is a multiple of 1/16, summed over L * P = 16 samples,
    20 bits.  The gradients: g * val and g * gw are multiples of 2^-8 below 2^8, their total over D <= 64 lanes below 2^14 (22 bits), times
    the weight and W <= 8 a shift or a 5-bit factor of a value that then has fewer bits.  The softmax of four 0s and -infs is 1/4 and 0.
    Fixed point: Mx = 8, the scale 2^37, a contribution a multiple of 2^-16: an integer before it is rounded; the sum times 2^-37 is the
    fp64 result, which fp32 holds.  Nothing exceeds 24 significant bits, so there is no tolerance here: any difference is a defect.  The comparison is torch.equal, of
    values: where a location gradient is zero the kernel may give -0 for the restatement's +0 (the count of differing bit patterns is
    printed)."""
    t, spec = R.dyadic(name, gmax, scale_b1)
    got, want = _run(t, spec, dev), _want(name, gmax, scale_b1)
    assert sorted(got) == sorted(want) == sorted(['out', 'grad_value'] + (['grad_offsets', 'grad_logits'] if spec['fused'] else ['grad_loc', 'grad_attn']))
    for k in want:
        w32 = want[k].float()
        assert got[k].dtype == torch.float32 and got[k].shape == w32.shape
        diff = int((_bits(got[k]) != _bits(w32)).sum())
        print(f'{name} {k}: {diff} of {w32.numel()} elements differ, max |difference| {float((got[k].double() - want[k]).abs().max()):.3e}')
        assert torch.equal(got[k], w32), (name, k)


@pytest.mark.parametrize('name,gmax,scale_b1', R.DYADIC_BOUND)
def test_quantisation_bound(dev, name, gmax, scale_b1):
    """The header's bound, element by element: n contributions of at most 2^-41 Mx each, then ONE fp32 rounding of the result (2^-24,
    taken with a factor two).  Everything but the fixed-point path is exact on these inputs, so out and the per-query gradients still
    equal fp64 bit for bit; with a batch item 2^-32 below Mx the bound on that item is far below what a tolerance relative to the
    largest element of the tensor would ask."""
    t, spec = R.dyadic(name, gmax, scale_b1)
    got, want = _run(t, spec, dev), _want(name, gmax, scale_b1)
    for k in want:
        if k != 'grad_value':
            assert torch.equal(got[k], want[k].float()), (name, k)
    mx = R.fixed_point_mx(t, spec)
    assert mx == gmax
    n = R.cell_hits([tuple(s) for s in spec['shapes']], R.plain_locations(t, spec), spec['B'], t['value'].shape[1], spec['M'])
    bound = n[..., None].double() * (2.0 ** -41 * mx) + 2.0 ** -23 * want['grad_value'].abs()
    err = (got['grad_value'].double() - want['grad_value']).abs()
    assert bool(torch.isfinite(got['grad_value']).all())
    assert bool((err[bound == 0] == 0).all())                  # a cell nothing lands on is an exact zero
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    tail = f', batch 1 alone {float(ratio[1].max()):.4f} (max |grad_value| there {float(want["grad_value"][1].abs().max()):.3e})' if spec['B'] > 1 else ''
    print(f'{name} gmax {gmax} scale_b1 {scale_b1}: largest error / bound {float(ratio.max()):.4f}{tail}; max n {int(n.max())}, '
          f'inexact elements {int((err > 0).sum())} of {err.numel()}')
    assert bool((err <= bound).all()), name
    if spec['B'] > 1:
        assert bool((err[1] <= bound[1]).all()) and float(want['grad_value'][1].abs().max()) > 0, name


def _plain_call(t, spec, dev, loc=None, w=None, grad_out=None):
    d = dict(t)
    for k, v in (('loc', loc), ('w', w), ('grad_out', grad_out)):
        if v is not None:
            d[k] = v
    return _run(d, spec, dev)


@pytest.mark.parametrize('name', ['hot_cell', 'plain'])
def test_query_order_changes_no_bit(dev, name):
    """Integer sums do not depend on the order of the adds: the queries permuted, grad_value keeps every bit (hot_cell: 1200 samples of
    magnitudes over nine decades on ONE cell), and the per-query results move with their queries."""
    t, spec = R.case_tensors(name)
    assert not spec['fused']
    perm = torch.randperm(spec['Q'], generator=torch.Generator().manual_seed(17))
    assert not torch.equal(perm, torch.arange(spec['Q']))
    a = _plain_call(t, spec, dev)
    b = _plain_call(t, spec, dev, loc=t['loc'][:, perm], w=t['w'][:, perm], grad_out=t['grad_out'][:, perm])
    assert _same(a['grad_value'], b['grad_value'])
    for k in ('out', 'grad_loc', 'grad_attn'):
        assert _same(a[k][:, perm], b[k]), k


@pytest.mark.parametrize('k', [-40, 40])
def test_power_of_two_scaling_is_exact(dev, k):
    """Mx scales with its inputs, so the fixed-point integers are the same and the results scale exactly (no value of `plain` comes near
    the ends of the fp32 range at 2^+-40)."""
    t, spec = R.case_tensors('plain')
    base = _plain_call(t, spec, dev)
    for x in base.values():
        nz = x[x != 0].abs()
        assert float(nz.max()) < 2.0 ** 80 and float(nz.min()) > 2.0 ** -80
    kk = torch.tensor(k)
    up = lambda x: torch.ldexp(x, kk)  # noqa: E731
    scaled = _plain_call(t, spec, dev, grad_out=up(t['grad_out']))
    assert _same(scaled['out'], base['out'])
    for q in ('grad_value', 'grad_loc', 'grad_attn'):
        assert _same(scaled[q], up(base[q])), q
    scaled = _plain_call(t, spec, dev, w=up(t['w']))
    for q in ('out', 'grad_value', 'grad_loc'):
        assert _same(scaled[q], up(base[q])), q
    assert _same(scaled['grad_attn'], base['grad_attn'])


def _all_plus_zero(x):
    return bool((_bits(x) == 0).all())


@pytest.mark.parametrize('name', ['plain', 'heads_d16_l8_p1'])
def test_zero_grad_out(dev, name):
    """Mx == 0 with Q > 0: scale = 0 and unit = 0, and still every element of grad_value is written over the poison, as +0."""
    t, spec = R.case_tensors(name)
    assert spec['Q'] > 0
    t = dict(t, grad_out=torch.zeros_like(t['grad_out']))
    with G.poisoned_empty():
        got = _run(t, spec, dev)
    assert _all_plus_zero(got['grad_value'])
    for k, x in got.items():
        assert bool(torch.isfinite(x).all()), k
        if k != 'out':
            assert float(x.abs().max()) == 0.0, k
    assert float(got['out'].abs().max()) > 0


def test_zero_plain_weights(dev):
    """Mx == 0 through the weights: grad_value and grad_loc are zero, grad_attn (which does not depend on the weights) is untouched."""
    t, spec = R.case_tensors('plain')
    t = dict(t, w=torch.zeros_like(t['w']))
    assert float(t['grad_out'].abs().max()) > 0
    with G.poisoned_empty():
        got = _run(t, spec, dev)
    want = R.run_case({k: v.double() for k, v in t.items()}, spec)
    assert _all_plus_zero(got['grad_value']) and float(want['grad_value'].abs().max()) == 0.0
    assert float(got['grad_loc'].abs().max()) == 0.0 and float(got['out'].abs().max()) == 0.0
    err, bound = float((got['grad_attn'].double() - want['grad_attn']).abs().max()), R.tol('grad_attn') * float(want['grad_attn'].abs().max())
    print(f'zero weights grad_attn: max error {err:.3e}, bound {bound:.3e}')
    assert bool(torch.isfinite(got['grad_attn']).all()) and 0 < bound and err <= bound


@pytest.mark.parametrize('where,bad', [('grad_out', float('nan')), ('w', float('nan')), ('w', float('inf')), ('w', float('-inf'))])
def test_nonfinite_plain_input_is_visible(dev, where, bad):
    """Mx is not finite: every element of grad_value is NaN, cells that nothing reaches included."""
    t, spec = R.case_tensors('plain')
    x = t[where].clone()
    x.view(-1)[x.numel() // 2 + 3] = bad                     # one element, in the second batch item
    got = _run(dict(t, **{where: x}), spec, dev)
    assert bool(torch.isnan(got['grad_value']).all())


def test_nan_logit_takes_its_item_out_of_grad_value(dev):
    """A NaN logit makes every weight of its (b, q, m) NaN: the item contributes nothing to grad_value, exactly as if its grad_out row were
    zero (it does not hold max|grad_out|, which is planted in batch 0: Mx is the same in both runs), and nothing else changes."""
    t, spec = R.dyadic('fused_d16', gmax=7)
    b, q, m, D = 1, 2, 1, spec['D']
    row = t['grad_out'][b, q, m * D:(m + 1) * D]
    assert float(row.abs().max()) > 0 and float(t['grad_out'][0].abs().max()) == 7 == R.fixed_point_mx(t, spec)
    logits = t['logits'].clone()
    logits[b, q, m, 5] = float('nan')
    grad_out = t['grad_out'].clone()
    grad_out[b, q, m * D:(m + 1) * D] = 0
    with_nan, zeroed, base = _run(dict(t, logits=logits), spec, dev), _run(dict(t, grad_out=grad_out), spec, dev), _run(t, spec, dev)
    assert bool(torch.isfinite(with_nan['grad_value']).all())
    assert _same(with_nan['grad_value'], zeroed['grad_value'])
    assert not _same(base['grad_value'], zeroed['grad_value'])                # the item did reach grad_value
    item = torch.zeros(spec['B'], spec['Q'], spec['M'], dtype=torch.bool)
    item[b, q, m] = True
    assert bool(torch.isnan(with_nan['out'].view(spec['B'], spec['Q'], spec['M'], D)[item]).all())          # the NaN is visible in the forward
    for k, shape in (('out', (D,)), ('grad_offsets', (-1,)), ('grad_logits', (-1,))):
        a, c = (x[k].reshape(spec['B'], spec['Q'], spec['M'], *shape)[~item] for x in (with_nan, base))
        assert _same(a, c), k                                                   # every other item: untouched


def test_no_host_synchronisation(dev):
    """Forward and backward of both forms with the level tensors on the device: nothing is read back."""
    import boxinstseg_amd as B
    calls = []
    for name in ('plain', 'heads_d16_l8_p1'):
        t, spec = R.case_tensors(name)
        d = {k: v.to(dev) for k, v in t.items()}
        d['ss'], d['ls'] = _levels(spec, dev)
        calls.append((spec['fused'], d))

    def both():
        res = []
        for fused, d in calls:
            value = d['value'].detach().requires_grad_(True)
            if fused:
                leaves = [value] + [d[k].detach().requires_grad_(True) for k in ('ref', 'off', 'logits')]
                out = B.multi_scale_deformable_attn_fused(value, d['ss'], d['ls'], *leaves[1:])
            else:
                leaves = [value] + [d[k].detach().requires_grad_(True) for k in ('loc', 'w')]
                out = B.multi_scale_deformable_attn(value, d['ss'], d['ls'], *leaves[1:])
            res.append((out.detach(),) + torch.autograd.grad(out, leaves, d['grad_out']))
        return res

    warm = both()                                           # a first call: the library is loaded, the allocator is warm
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')                 # a host synchronisation inside raises
    try:
        again = both()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(warm, again):
        assert len(a) == len(b) >= 4
        for x, y in zip(a, b):
            assert _same(x.cpu(), y.cpu())
