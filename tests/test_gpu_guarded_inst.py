"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_inst.h on misaligned views inside poisoned bands (tests/guarded.py).

The logits (class logits of the top-k, mask logits of the paste) start 4, 8 or 12 bytes past a 16-byte boundary inside NaN bands (a NaN
that was read reaches a score or a mask byte's neighbourhood: the results would differ from the plain call), ``query`` sits between -1
words; ``masks`` starts at every byte offset 0..15 with rows of 64 and of 61 bytes; the other outputs are 4, 8 or 12 bytes off, all
pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which is exactly as large as the size query says.  Afterwards the
bands are intact, every element of every output and of the workspace is written, the inputs are unchanged, and the results are
bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import inst_post_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_inst.py checks the table against _lib.INST_SIGNATURES)
GUARDED = {
    'bxi_inst_topk_f32': 'test_inst_topk_guarded',
    'bxi_inst_paste_u8': 'test_inst_paste_guarded',
}
HW, CROP = (13, 21), (50, 81)
QUERY = [4, 0, -1, 2, 2, 5]                                  # a repeat and two indices outside [0, 5)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_inst_topk_guarded(dev, lead, B=2, Q=12, things=3, stuff=2, k=14):
    """(the shape arguments have defaults, so they are no fixtures: test_inst_topk_guarded_largest_launch passes its own)"""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    C = things + stuff
    cls = torch.from_numpy(np.random.default_rng(3).normal(0, 2, (B, Q, C + 1)).astype(np.float32)).to(dev)
    want = [torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev),
            torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)]
    G.ok(lib.bxi_inst_topk_f32(G.ptr(cls), B, Q, C, things, k, *[G.ptr(t) for t in want], G.stream(dev)))
    gc = G.embed(cls, lead)
    gs, gl = G.out((B, k), torch.float32, dev, 4 - lead), G.out((B, k), torch.int64, dev, 1)
    gq, gn = G.out((B, k), torch.int64, dev, 1), G.out((B,), torch.int32, dev, lead)
    assert gc.ptr() % 16 == 4 * lead and gl.ptr() % 16 == 8
    G.ok(lib.bxi_inst_topk_f32(G.ptr(gc), B, Q, C, things, k, G.ptr(gs), G.ptr(gl), G.ptr(gq), G.ptr(gn), G.stream(dev)))
    G.check_bands(gc, gs, gl, gq, gn)
    G.check_written(gs, gl, gq, gn)
    G.check_unchanged(gc)
    for g, w in zip((gs, gl, gq, gn), want):
        assert G.same(g.t, w)
    counts = want[3].tolist()
    assert all(0 < c < k for c in counts) if stuff else counts == [k] * B      # some stuff entries were dropped in every image
    for b, c in enumerate(counts):
        assert want[1][b, c:].tolist() == [-1] * (k - c) and want[2][b, c:].tolist() == [-1] * (k - c) and want[0][b, c:].tolist() == [0.0] * (k - c)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_inst_topk_guarded_largest_launch(dev, lead):
    """16384 keys (128 KiB of LDS), as many output rows written in 16 rounds, rows of 257 logits: nothing is filtered, count = k."""
    test_inst_topk_guarded(dev, lead, B=1, Q=64, things=256, stuff=0, k=16384)


@pytest.mark.parametrize('out_w', [64, 61])
@pytest.mark.parametrize('mask_lead', range(16))
def test_inst_paste_guarded(dev, mask_lead, out_w):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    out = (37, out_w)                                                         # three bands, the last one short
    n = len(QUERY)
    logits = torch.from_numpy(R.case_inputs('rescale')[1][:5]).to(dev)
    assert tuple(logits.shape) == (5, *HW)
    query = torch.tensor(QUERY, device=dev)
    cls_scores = torch.linspace(0.9, 0.1, n, device=dev)
    nbytes = lib.bxi_inst_paste_workspace_bytes(n, *out)
    assert nbytes == 16 * n * out[0] and nbytes % 16 == 0

    def call(lg, qu, cs, masks, stats, ms, boxes, ws):
        G.ok(lib.bxi_inst_paste_u8(G.ptr(lg), 5, HW[0], HW[1], G.ptr(qu), G.ptr(cs), n, 4 * HW[0], 4 * HW[1], CROP[0], CROP[1], out[0], out[1],
                                   G.ptr(masks), G.ptr(stats), G.ptr(ms), G.ptr(boxes), G.ptr(ws), nbytes, G.stream(dev)))
    want = [torch.empty((n, *out), dtype=torch.uint8, device=dev), torch.empty((n, 5), dtype=torch.int32, device=dev),
            torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n, 5), dtype=torch.float32, device=dev)]
    call(logits, query, cls_scores, *want, torch.empty(nbytes, dtype=torch.uint8, device=dev))
    lead4 = 1 + mask_lead % 3                                                 # 4, 8, 12 bytes
    gp, gk, gc = G.embed(logits, lead4, G.plane_band(*HW)), G.embed(query, 1), G.embed(cls_scores, lead4)
    gm = G.out((n, *out), torch.uint8, dev, mask_lead, G.plane_band(*out))
    gs, gms, gb = G.out((n, 5), torch.int32, dev, 4 - lead4), G.out((n,), torch.float32, dev, lead4), G.out((n, 5), torch.float32, dev, 4 - lead4)
    ws = G.out(nbytes // 4, torch.int32, dev, 0)                              # 16-byte aligned, exactly the size asked for
    assert gp.ptr() % 16 == 4 * lead4 and gm.ptr() % 16 == mask_lead and gs.ptr() % 16 == 4 * (4 - lead4) and ws.ptr() % 16 == 0
    call(gp, gk, gc, gm, gs, gms, gb, ws)
    G.check_bands(gp, gk, gc, gm, gs, gms, gb, ws)
    G.check_written(gm, gs, gms, gb, ws)
    G.check_unchanged(gp, gk, gc)
    for g, w in zip((gm, gs, gms, gb), want):
        assert G.same(g.t, w)
    assert bool(want[0].any()) and not bool(want[0][2].any()) and want[1][5].tolist() == [0, -1, -1, -1, -1]
    assert want[3][2].tolist() == [0.0] * 5 and float(want[2][5]) == 0.0 and float(want[2][0]) > 0.5
