"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_attn.h on misaligned views inside poisoned bands (tests/guarded.py).

fp32 inputs start 4, 8 or 12 bytes past a 16-byte boundary, the bit words and the byte mask likewise off their natural 16, surrounded by NaN
/ -1 / 0xFF (a NaN that was read reaches an output or a gradient; a band word of all ones read as mask bits changes the result); outputs are
pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which is exactly as large as the size query says.  Afterwards the
bands are intact, every output element and the whole workspace are written, the inputs are unchanged, and the results are bit-identical to
the same call on plain tensors."""
import pytest
import torch

from tests import guarded as G
from tests import masked_attn_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.ATTN_SIGNATURES)
GUARDED = {
    'bxi_attn_mask_bits_f32': 'test_mask_bits_guarded',
    'bxi_attn_pack_mask_u8': 'test_pack_mask_guarded',
    'bxi_masked_attn_forward_f32': 'test_forward_guarded',
    'bxi_masked_attn_backward_f32': 'test_backward_guarded',
}
B_, M_ = 2, 2
SHAPES = [(37, 300, 32), (33, 70, 16), (5, 257, 64)]                 # (Q, S, D): two spans with a tail, one span, every head dimension


def _inputs(shape, dev, per_head):
    Q, S, D = shape
    t = R.make_case(50 + Q + S + D, Q, S, D, B_, M_)
    mask = t['mask'] if per_head else t['mask'].view(B_, M_, Q, S)[:, 0].contiguous()
    bits = R.pack_bits(mask).to(dev)
    return tuple(t[n].to(dev) for n in ('q', 'k', 'v', 'g')) + (bits,)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_mask_bits_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    pred = torch.from_numpy(R.golden()['mask_pred']).to(dev)
    for h, w in ((5, 7), (32, 32), (96, 80)):
        words = (h * w + 31) // 32
        want = torch.empty((2, 5, words), dtype=torch.int32, device=dev)
        G.ok(lib.bxi_attn_mask_bits_f32(pred.data_ptr(), 2, 5, 64, 64, h, w, want.data_ptr(), G.stream(dev)))
        gp, out = G.embed(pred, lead), G.out((2, 5, words), torch.int32, dev, 4 - lead)
        G.ok(lib.bxi_attn_mask_bits_f32(gp.ptr(), 2, 5, 64, 64, h, w, out.ptr(), G.stream(dev)))
        G.check_bands(gp, out)
        G.check_written(out)
        G.check_unchanged(gp)
        assert torch.equal(out.t, want)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_pack_mask_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(6)
    for rows, S in ((7, 35), (3, 300)):
        mask = (torch.rand(rows, S, generator=gen) < 0.5).to(torch.uint8).to(dev)
        words = (S + 31) // 32
        gm, out = G.embed(mask, lead, poison=0xFF), G.out((rows, words), torch.int32, dev, lead)
        G.ok(lib.bxi_attn_pack_mask_u8(gm.ptr(), rows, S, out.ptr(), G.stream(dev)))
        G.check_bands(gm, out)
        G.check_written(out)
        G.check_unchanged(gm)
        assert torch.equal(out.t.cpu(), R.pack_bits(mask.cpu().bool()))


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('per_head', [0, 1])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'Q%d_S%d_D%d' % s)
def test_forward_guarded(dev, shape, per_head, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    Q, S, D = shape
    q, k, v, _, bits = _inputs(shape, dev, per_head)
    nbytes = lib.bxi_masked_attn_forward_workspace_bytes(B_, M_, Q, S, D)
    assert nbytes > 0 and nbytes % 4 == 0

    def call(q_, k_, v_, b_, out, lse, ws):
        G.ok(lib.bxi_masked_attn_forward_f32(G.ptr(q_), G.ptr(k_), G.ptr(v_), G.ptr(b_), per_head, B_, M_, Q, S, D, D ** -0.5, G.ptr(out), G.ptr(lse),
                                             G.ptr(ws), nbytes, G.stream(dev)))

    want = [torch.empty((Q, B_, M_ * D), device=dev), torch.empty((B_, M_, Q), device=dev)]
    call(q, k, v, bits, *want, torch.empty(nbytes, dtype=torch.uint8, device=dev))
    gq, gk, gv, gb = G.embed(q, lead), G.embed(k, 4 - lead), G.embed(v, lead), G.embed(bits, 4 - lead)
    out, lse = G.out((Q, B_, M_ * D), torch.float32, dev, 4 - lead), G.out((B_, M_, Q), torch.float32, dev, lead)
    ws = G.out(nbytes // 4, torch.float32, dev, 0)                    # 16-byte aligned, exactly the size asked for
    call(gq, gk, gv, gb, out, lse, ws)
    G.check_bands(gq, gk, gv, gb, out, lse, ws)
    G.check_written(out, lse, ws)
    G.check_unchanged(gq, gk, gv, gb)
    assert G.same(out.t, want[0]) and G.same(lse.t, want[1]) and bool(torch.isfinite(out.t).all()) and bool(torch.isfinite(lse.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('per_head', [0, 1])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'Q%d_S%d_D%d' % s)
def test_backward_guarded(dev, shape, per_head, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    Q, S, D = shape
    q, k, v, g, bits = _inputs(shape, dev, per_head)
    scale = D ** -0.5
    out, lse = torch.empty((Q, B_, M_ * D), device=dev), torch.empty((B_, M_, Q), device=dev)
    fbytes = lib.bxi_masked_attn_forward_workspace_bytes(B_, M_, Q, S, D)
    G.ok(lib.bxi_masked_attn_forward_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), bits.data_ptr(), per_head, B_, M_, Q, S, D, scale, out.data_ptr(),
                                         lse.data_ptr(), torch.empty(fbytes, dtype=torch.uint8, device=dev).data_ptr(), fbytes, G.stream(dev)))
    nbytes = lib.bxi_masked_attn_backward_workspace_bytes(B_, M_, Q, S, D)
    assert nbytes > 0 and nbytes % 4 == 0

    def call(g_, q_, k_, v_, b_, o_, l_, dq, dk, dv, ws):
        G.ok(lib.bxi_masked_attn_backward_f32(G.ptr(g_), G.ptr(q_), G.ptr(k_), G.ptr(v_), G.ptr(b_), per_head, G.ptr(o_), G.ptr(l_), B_, M_, Q, S, D, scale,
                                              G.ptr(dq), G.ptr(dk), G.ptr(dv), G.ptr(ws), nbytes, G.stream(dev)))

    want = [torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)]
    call(g, q, k, v, bits, out, lse, *want, torch.empty(nbytes, dtype=torch.uint8, device=dev))
    ins = [G.embed(g, 4 - lead), G.embed(q, lead), G.embed(k, 4 - lead), G.embed(v, lead), G.embed(bits, lead), G.embed(out, 4 - lead), G.embed(lse, lead)]
    outs = [G.out(tuple(x.shape), torch.float32, dev, lead if i else 4 - lead) for i, x in enumerate(want)]
    ws = G.out(nbytes // 4, torch.float32, dev, 0)
    call(*ins, *outs, ws)
    G.check_bands(*ins, *outs, ws)
    G.check_written(*outs, ws)                                        # delta and every span's share of dq fill the workspace
    G.check_unchanged(*ins)
    for got, exp in zip(outs, want):
        assert G.same(got.t, exp) and bool(torch.isfinite(got.t).all())
