"""GPU: the kernel-launching entry point of include/boxinst/boxinst_hip_rle.h on misaligned views inside poisoned bands (tests/guarded.py).

``masks`` starts at every byte offset 0..15 inside bands of 0xFF bytes (a band byte that was read is a set pixel: the counts would
differ from the plain call), with rows of 64 and of 61 bytes; ``stats`` sits 4, 8 or 12 bytes off between -1 words.  ``run_offsets``,
``counts``, ``char_offsets``, ``chars`` and ``status`` are exactly as large as the call needs and pre-filled with the 'nobody wrote this'
pattern, and so is the workspace, which is exactly as large as the size query says.  Afterwards the bands are intact, every element of
the outputs is written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors and to the
restatement of tests/rle_ref.py."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import rle_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_family_rle.py checks the table against _lib.RLE_SIGNATURES)
GUARDED = {
    'bxi_mask_rle_u8': 'test_mask_rle_guarded',
}
N, H = 5, 70                                                                  # two word rows, the second one short


def _masks(w):
    rng = np.random.default_rng(w)
    yy, xx = np.mgrid[:H, :w]
    m = np.zeros((N, H, w), np.uint8)
    for i in range(N - 1):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, w), rng.uniform(4, 30)
        m[i] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) & ~((yy - cy) ** 2 + (xx - cx) ** 2 <= (r / 3) ** 2)
    m[1] = 0                                                                  # an empty mask between the others
    m[3, :, w - 1] = 1                                                        # the last column whole: the run ends with the mask
    m[3, H - 1, :] = 1
    return m


def _call(lib, dev, masks, w, stats, cap_runs, cap_chars, ro, counts, co, chars, status, ws, nbytes):
    from boxinstseg_amd import _lib
    rc = lib.bxi_mask_rle_u8(G.ptr(masks), N, H, w, G.ptr(stats), cap_runs, cap_chars, G.ptr(ro), G.ptr(counts), G.ptr(co), G.ptr(chars),
                             G.ptr(status), G.ptr(ws), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


@pytest.mark.parametrize('with_stats', [False, True], ids=['plain', 'stats'])
@pytest.mark.parametrize('w', [64, 61])
@pytest.mark.parametrize('mask_lead', range(16))
def test_mask_rle_guarded(dev, mask_lead, w, with_stats):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    m = _masks(w)
    w_ro, w_counts, w_co, w_chars = R.packed(m)
    cap_runs, cap_chars = len(w_counts), len(w_chars)
    masks = torch.from_numpy(m).to(dev)
    stats = torch.from_numpy(R.stats_of(m)).to(dev) if with_stats else None
    nbytes = lib.bxi_mask_rle_workspace_bytes(N, H, w)
    assert nbytes == (N * 2 * w * 8 + 15) // 16 * 16 + N * w * 16 + (N * w * 4 + 15) // 16 * 16 + (N * 8 + 15) // 16 * 16
    plain = dict(ro=torch.empty(N + 1, dtype=torch.int32, device=dev), counts=torch.empty(cap_runs, dtype=torch.int32, device=dev),
                 co=torch.empty(N + 1, dtype=torch.int32, device=dev), chars=torch.empty(cap_chars, dtype=torch.uint8, device=dev),
                 status=torch.empty(1, dtype=torch.int32, device=dev))
    _call(lib, dev, masks, w, stats, cap_runs, cap_chars, plain['ro'], plain['counts'], plain['co'], plain['chars'], plain['status'],
          torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
    lead4 = 1 + mask_lead % 3                                                 # 4, 8, 12 bytes
    gm = G.embed(masks, mask_lead, G.plane_band(H, w))
    gs = G.embed(stats, lead4) if with_stats else None
    gro, gco = G.out(N + 1, torch.int32, dev, lead4), G.out(N + 1, torch.int32, dev, 4 - lead4)
    gcounts, gchars = G.out(cap_runs, torch.int32, dev, 4 - lead4), G.out(cap_chars, torch.uint8, dev, 15 - mask_lead)
    gstatus = G.out(1, torch.int32, dev, lead4)
    ws = G.out(nbytes // 4, torch.int32, dev, 0)                              # 16-byte aligned, exactly the size asked for
    assert gm.ptr() % 16 == mask_lead and gchars.ptr() % 16 == 15 - mask_lead and gro.ptr() % 16 == 4 * lead4 and ws.ptr() % 16 == 0
    _call(lib, dev, gm, w, gs, cap_runs, cap_chars, gro, gcounts, gco, gchars, gstatus, ws, nbytes)
    G.check_bands(gm, gro, gco, gcounts, gchars, gstatus, ws, *([gs] if with_stats else []))
    G.check_written(gro, gco, gcounts, gstatus)
    G.check_unchanged(gm, *([gs] if with_stats else []))
    for key, g in (('ro', gro), ('counts', gcounts), ('co', gco), ('chars', gchars), ('status', gstatus)):
        assert torch.equal(g.t, plain[key]), key
    assert int(gstatus.t[0]) == 0 and np.array_equal(gro.t.cpu().numpy(), w_ro) and np.array_equal(gco.t.cpu().numpy(), w_co)
    assert np.array_equal(gcounts.t.cpu().numpy().view(np.uint32), w_counts) and np.array_equal(gchars.t.cpu().numpy(), w_chars)
