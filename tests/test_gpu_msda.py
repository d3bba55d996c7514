"""GPU: multi-scale deformable attention (csrc/msda.hip) against the fp64 results of the per-sample restatement (tests/msda_ref.py,
tests/golden/msda*.npz), within the tolerances measured when the fixture was made: 4 x the fp32 error of the restatement itself, relative to
the largest fp64 magnitude of the quantity.  Then the fused form against the plain one, bit-identical backward runs, the module end to end,
the box form of the reference points, the empty query set and the edge of the support set."""
import pytest
import torch

from tests import guarded as G
from tests import msda_ref as R

pytestmark = pytest.mark.gpu

SPEC = R.load_cases()
NAMES = list(SPEC['cases'])
FUSED = [n for n in NAMES if SPEC['cases'][n]['fused']]
_RUNS = {}


def _levels(spec, dev):
    shapes = [tuple(s) for s in spec['shapes']]
    return torch.tensor(shapes, device=dev), torch.tensor(R.level_starts(shapes), device=dev)


def _run(name, dev, cache=True):
    """The case through the public functions: out and every gradient, as CPU tensors."""
    if cache and name in _RUNS:
        return _RUNS[name]
    import boxinstseg_amd as B
    t, spec = R.case_tensors(name)
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
    if cache:
        _RUNS[name] = res
    return res


def _close(got, want, quantity, what, mask=None):
    d = (got.double() - want).abs()
    if mask is not None:
        d = d[mask]
    err, bound = float(d.max()), R.tol(quantity) * float(want.abs().max())
    print(f'{what}: max error {err:.3e}, bound {bound:.3e}')
    assert bool(torch.isfinite(got).all()) and err <= bound, what


@pytest.mark.parametrize('name', NAMES)
def test_against_fp64(dev, name):
    got, want = _run(name, dev), R.expected(name)
    t, spec = R.case_tensors(name)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32
        mask = ~t['boundary'][..., None].expand_as(want[k]) if (k == 'grad_loc' and 'boundary' in t) else None
        _close(got[k], want[k], k, f'{name} {k}', mask)
    if 'zero' in t:                              # far outside, on h = -1 / w = -1, w = W, NaN: nothing counted, exact zeros
        assert float(got['grad_loc'][t['zero']].abs().max()) == 0.0 and float(got['grad_attn'][t['zero']].abs().max()) == 0.0
        value = t['value'].view(4 * 8 + 1, 2, 16)
        alone = torch.zeros_like(t['w'])
        alone[0, 1, :, 0, 0] = 1.0               # the planted pixel centre alone returns pixel (1, 2) exactly
        import boxinstseg_amd as B
        ss, ls = _levels(spec, dev)
        out = B.multi_scale_deformable_attn(t['value'].to(dev), ss, ls, t['loc'].to(dev), alone.to(dev)).cpu()
        assert torch.equal(out[0, 1].view(2, 16), value[1 * 8 + 2]) and float(out[0, [0, 2, 3, 4, 5]].abs().max()) == 0.0


@pytest.mark.parametrize('name', FUSED)
def test_fused_equals_plain_on_torch_locations(dev, name):
    import boxinstseg_amd as B
    t, spec = R.case_tensors(name)
    shapes = [tuple(s) for s in spec['shapes']]
    ss, ls = _levels(spec, dev)
    value = t['value'].to(dev).requires_grad_(True)
    off, logits = t['off'].to(dev).requires_grad_(True), t['logits'].to(dev).requires_grad_(True)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=dev)
    loc = t['ref'].to(dev)[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    w = logits.softmax(-1).view(spec['B'], spec['Q'], spec['M'], len(shapes), spec['P'])
    out = B.multi_scale_deformable_attn(value, ss, ls, loc, w)
    grads = torch.autograd.grad(out, [value, off, logits], t['grad_out'].to(dev))
    fused, want = _run(name, dev), R.expected(name)
    for k, g in zip(('out', 'grad_value', 'grad_offsets', 'grad_logits'), (out.detach(),) + grads):
        _close(g.cpu(), want[k], k, f'{name} plain {k}')
        err = float((g.cpu() - fused[k]).abs().max())
        assert err <= 2 * R.tol(k) * float(want[k].abs().max()), (k, err)           # both are within tol of the same fp64 result


@pytest.mark.parametrize('name', ['plain', 'decoder_small', 'hot_cell'])
def test_backward_twice_is_bit_identical(dev, name):
    a, b = _run(name, dev), _run(name, dev, cache=False)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_reference_point_gradient(dev):
    """The fused form's gradient w.r.t. the reference points is the sum over (m, p) of the offsets' gradients times (W, H): within
    M * P * max(W, H) * tol_grad_offsets * max|grad_offsets| of fp64, one term's bound per term of the sum."""
    import boxinstseg_amd as B
    t, spec = R.case_tensors('heads_d16_l8_p1')
    shapes = [tuple(s) for s in spec['shapes']]
    ss, ls = _levels(spec, dev)
    ref = t['ref'].to(dev).requires_grad_(True)
    out = B.multi_scale_deformable_attn_fused(t['value'].to(dev), ss, ls, ref, t['off'].to(dev), t['logits'].to(dev))
    got, = torch.autograd.grad(out, ref, t['grad_out'].to(dev))
    d = {k: v.double() for k, v in t.items()}
    r64 = d['ref'].clone().requires_grad_(True)
    loc, w = R.fused_to_plain(shapes, r64, d['off'], d['logits'])
    want, = torch.autograd.grad((R.msda_scalar(d['value'], shapes, loc, w) * d['grad_out']).sum(), r64)
    bound = spec['M'] * spec['P'] * max(max(s) for s in shapes) * R.tol('grad_offsets') * float(R.expected('heads_d16_l8_p1')['grad_offsets'].abs().max())
    assert float((got.cpu().double() - want).abs().max()) <= bound


def _module(dev):
    import boxinstseg_amd as B
    g = R.golden()
    mod = B.MultiScaleDeformableAttention(**SPEC['module']['cfg'])
    mod.load_state_dict({k[len('module_param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('module_param_')})
    return mod.to(dev), g


@pytest.mark.parametrize('key', ['ref', 'ref4'])
def test_module_end_to_end(dev, key):
    """ref: reference points [B,Q,L,2], the fused kernel; ref4: boxes [B,Q,L,4], torch locations and the plain kernel.  With a padding
    mask, a query_pos and the keyword arguments BaseTransformerLayer passes."""
    mod, g = _module(dev)
    shapes = [tuple(s) for s in SPEC['module']['shapes']]
    q = torch.from_numpy(g['module_query']).to(dev).requires_grad_(True)
    out = mod(q, key=None, value=None, query_pos=torch.from_numpy(g['module_query_pos']).to(dev), key_padding_mask=torch.from_numpy(g['module_mask']).to(dev),
              reference_points=torch.from_numpy(g[f'module_{key}']).to(dev), spatial_shapes=torch.tensor(shapes, device=dev),
              level_start_index=torch.tensor(R.level_starts(shapes), device=dev), key_pos=None, attn_mask=None, valid_radios=None)
    _close(out.detach().cpu(), torch.from_numpy(g[f'module_want_out_{key}']), 'module_out', f'module {key} out')
    up = torch.sin(torch.arange(out.numel(), dtype=torch.float32, device=dev)).view(out.shape)
    names = [n for n, _ in mod.named_parameters()]
    grads = torch.autograd.grad(out, [q] + [p for _, p in mod.named_parameters()], up)
    for n, gr in zip(['query'] + names, grads):
        _close(gr.cpu(), torch.from_numpy(g[f'module_want_grad_{key}_{n}']), 'module_param_grad', f'module {key} grad {n}')


def test_host_shapes_are_checked_and_accepted(dev):
    import boxinstseg_amd as B
    t, spec = R.case_tensors('plain')
    shapes = [tuple(s) for s in spec['shapes']]
    args = [t[k].to(dev) for k in ('loc', 'w')]
    out = B.multi_scale_deformable_attn(t['value'].to(dev), torch.tensor(shapes), torch.tensor(R.level_starts(shapes)), *args, im2col_step=7)
    assert torch.equal(out.cpu(), _run('plain', dev)['out'])
    with pytest.raises(RuntimeError, match='add up'):
        B.multi_scale_deformable_attn(t['value'].to(dev), torch.tensor([(5, 7), (3, 5)]), torch.tensor([0, 35]), *args)
    with pytest.raises(RuntimeError, match='attention_weights'):
        B.multi_scale_deformable_attn(t['value'].to(dev), torch.tensor(shapes), torch.tensor([0, 35]), args[0], args[1][:, :5])
    # inconsistent shapes given ON THE DEVICE are not read back: the kernel bounds them, a level that does not fit contributes nothing
    ss_bad = torch.tensor([(5, 7), (300, 400)], device=dev)
    out = B.multi_scale_deformable_attn(t['value'].to(dev), ss_bad, torch.tensor([0, 35], device=dev), *args)
    w0 = args[1].clone()
    w0[:, :, :, 1] = 0
    want = B.multi_scale_deformable_attn(t['value'].to(dev), torch.tensor(shapes, device=dev), torch.tensor([0, 35], device=dev), args[0], w0)
    assert torch.equal(out, want)


def test_empty_query_set(dev):
    import boxinstseg_amd as B
    t, spec = R.case_tensors('plain')
    ss, ls = _levels(spec, dev)
    with G.poisoned_empty():
        value = t['value'].to(dev).requires_grad_(True)
        loc = torch.zeros(2, 0, 2, 2, 2, 2, device=dev, requires_grad=True)
        w = torch.zeros(2, 0, 2, 2, 2, device=dev, requires_grad=True)
        out = B.multi_scale_deformable_attn(value, ss, ls, loc, w)
        assert tuple(out.shape) == (2, 0, 64)
        gv, gl, gw = torch.autograd.grad(out, [value, loc, w], torch.zeros_like(out))
        off = torch.zeros(2, 0, 2, 2, 2, 2, device=dev, requires_grad=True)
        out = B.multi_scale_deformable_attn_fused(value, ss, ls, torch.zeros(2, 0, 2, 2, device=dev), off, torch.zeros(2, 0, 2, 4, device=dev))
        gv2, = torch.autograd.grad(out, [value], torch.zeros_like(out))
    for g in (gv, gv2):
        assert g.shape == value.shape and torch.equal(g.view(torch.int32), torch.zeros_like(g).view(torch.int32))       # written over the poison
    assert tuple(gl.shape) == (2, 0, 2, 2, 2, 2) and tuple(gw.shape) == (2, 0, 2, 2, 2)


def test_nonfinite_grad_out_is_visible(dev):
    """Mx is not finite: every element of grad_value is NaN (include/boxinst/boxinst_hip_msda.h), nothing is silently dropped."""
    import boxinstseg_amd as B
    t, spec = R.case_tensors('plain')
    ss, ls = _levels(spec, dev)
    value = t['value'].to(dev).requires_grad_(True)
    out = B.multi_scale_deformable_attn(value, ss, ls, t['loc'].to(dev), t['w'].to(dev))
    g = t['grad_out'].to(dev).clone()
    g[1, 3, 5] = float('inf')
    gv, = torch.autograd.grad(out, value, g)
    assert bool(torch.isnan(gv).all())


def test_outside_the_support_set(dev):
    import boxinstseg_amd as B
    from boxinstseg_amd import _lib
    ss, ls = torch.tensor([[2, 3]], device=dev), torch.tensor([0], device=dev)

    def call(D=8, L=1, P=1, dtype=torch.float32):
        v = torch.zeros(1, 6 * L, 2, D, device=dev, dtype=dtype)
        return B.multi_scale_deformable_attn(v, ss.repeat(L, 1), ls.repeat(L) if L == 1 else torch.arange(L, device=dev) * 6,
                                             torch.full((1, 3, 2, L, P, 2), 0.5, device=dev, dtype=dtype), torch.ones(1, 3, 2, L, P, device=dev, dtype=dtype))

    assert tuple(call().shape) == (1, 3, 16) and tuple(call(D=64, L=8, P=8).shape) == (1, 3, 128)
    for kw in (dict(D=4), dict(D=12), dict(D=128), dict(L=9), dict(P=9)):
        with pytest.raises(NotImplementedError, match='power of two'):
            call(**kw)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match='float32'):
            call(dtype=dtype)
    lib = _lib.load()
    X = 0x1000                                   # the ABI itself answers the same way, before any launch
    assert lib.bxi_msda_forward_f32(X, X, X, X, X, X, 1, 6, 2, 12, 3, 1, 1, 0, X, None) == _lib.BXI_ERR_UNSUPPORTED
