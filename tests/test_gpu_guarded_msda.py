"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_msda.h on misaligned views inside poisoned bands (tests/guarded.py).

fp32 inputs start 4, 8 or 12 bytes past a 16-byte boundary, the int64 level tensors at 8, surrounded by NaN / -1 (a NaN that was read reaches
the output or a gradient; a -1 read as a shape fails the kernel's level check); outputs are pre-filled with the 'nobody wrote this' pattern,
and so is the workspace, which is exactly as large as the size query says.  Afterwards the bands are intact, every output element and the
whole workspace are written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import pytest
import torch

from tests import guarded as G
from tests import msda_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.MSDA_SIGNATURES)
GUARDED = {
    'bxi_msda_forward_f32': 'test_forward_guarded',
    'bxi_msda_backward_f32': 'test_backward_guarded',
}
CASES = ['plain', 'heads_d16_l8_p1', 'heads_d64_l1_p8', 'heads_d8_l1_p1']      # plain, fused, fused, plain: every head dimension


def _inputs(name, dev):
    t, spec = R.case_tensors(name)
    shapes = [tuple(s) for s in spec['shapes']]
    dims = (spec['B'], int(t['value'].shape[1]), spec['M'], spec['D'], spec['Q'], len(shapes), spec['P'])
    a, off, w = (t['ref'], t['off'], t['logits']) if spec['fused'] else (t['loc'], None, t['w'])
    flags = 1 if spec['fused'] else 0
    dev_t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    return (dev_t(t['value']), torch.tensor(shapes, device=dev), torch.tensor(R.level_starts(shapes), device=dev), dev_t(a), dev_t(off), dev_t(w),
            dev_t(t['grad_out'])), dims, flags


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('name', CASES)
def test_forward_guarded(dev, name, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    (value, ss, ls, a, off, w, _), dims, flags = _inputs(name, dev)
    B, S, M, D, Q, L, P = dims

    def call(v, s_, l_, a_, o_, w_, out):
        G.ok(lib.bxi_msda_forward_f32(G.ptr(v), G.ptr(s_), G.ptr(l_), G.ptr(a_), G.ptr(o_), G.ptr(w_), B, S, M, D, Q, L, P, flags, G.ptr(out), G.stream(dev)))

    want = torch.empty((B, Q, M * D), device=dev)
    call(value, ss, ls, a, off, w, want)
    gv, gs, gl = G.embed(value, lead), G.embed(ss, 1), G.embed(ls, 1)
    ga, gw = G.embed(a, 4 - lead), G.embed(w, lead)
    go = G.embed(off, 4 - lead) if off is not None else None
    out = G.out((B, Q, M * D), torch.float32, dev, 4 - lead)
    call(gv, gs, gl, ga, go, gw, out)
    ins = [g for g in (gv, gs, gl, ga, go, gw) if g is not None]
    G.check_bands(*ins, out)
    G.check_written(out)
    G.check_unchanged(*ins)
    assert G.same(out.t, want) and bool(torch.isfinite(out.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('name', CASES)
def test_backward_guarded(dev, name, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    (value, ss, ls, a, off, w, g), dims, flags = _inputs(name, dev)
    B, S, M, D, Q, L, P = dims
    nbytes = lib.bxi_msda_backward_workspace_bytes(B, S, M, D, Q, L, P)
    assert nbytes > 0 and nbytes % 16 == 0

    def call(g_, v, s_, l_, a_, o_, w_, gv, ga, gw, ws):
        G.ok(lib.bxi_msda_backward_f32(G.ptr(g_), G.ptr(v), G.ptr(s_), G.ptr(l_), G.ptr(a_), G.ptr(o_), G.ptr(w_), B, S, M, D, Q, L, P, flags,
                                       G.ptr(gv), G.ptr(ga), G.ptr(gw), G.ptr(ws), nbytes, G.stream(dev)))

    want = [torch.empty((B, S, M, D), device=dev), torch.empty((B, Q, M, L, P, 2), device=dev), torch.empty(tuple(w.shape), device=dev)]
    call(g, value, ss, ls, a, off, w, *want, torch.empty(nbytes, dtype=torch.uint8, device=dev))
    gg, gv, gs, gl = G.embed(g, 4 - lead), G.embed(value, lead), G.embed(ss, 1), G.embed(ls, 1)
    ga, gw = G.embed(a, 4 - lead), G.embed(w, lead)
    go = G.embed(off, lead) if off is not None else None
    outs = [G.out(tuple(x.shape), torch.float32, dev, lead if i else 4 - lead) for i, x in enumerate(want)]
    ws = G.out(nbytes // 4, torch.float32, dev, 0)                           # 16-byte aligned, exactly the size asked for
    call(gg, gv, gs, gl, ga, go, gw, *outs, ws)
    ins = [x for x in (gg, gv, gs, gl, ga, go, gw) if x is not None]
    G.check_bands(*ins, *outs, ws)
    G.check_written(*outs, ws)                                                # the partial maxima and the accumulator fill the workspace
    G.check_unchanged(*ins)
    for got, exp in zip(outs, want):
        assert G.same(got.t, exp) and bool(torch.isfinite(got.t).all())
