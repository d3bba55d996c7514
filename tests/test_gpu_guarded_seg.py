"""GPU: the kernel-launching entry point of include/boxinst/boxinst_hip_seg.h on misaligned views inside poisoned bands (tests/guarded.py).

``probs`` starts 4, 8 or 12 bytes past a 16-byte boundary inside NaN bands (a NaN that was read reaches a mask byte's neighbourhood: the
results would differ from the plain call), ``keep_inds`` sits between -1 words; ``masks`` starts at every byte offset 0..15 with rows of
64 and of 61 bytes, ``stats`` 4, 8 or 12 bytes off, all pre-filled with the 'nobody wrote this' pattern, and so is the workspace, which is
exactly as large as the size query says.  Afterwards the bands are intact, every element of ``masks``, ``stats`` and the workspace is
written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import matrix_nms_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.SEG_SIGNATURES)
GUARDED = {
    'bxi_seg_paste_u8': 'test_seg_paste_guarded',
}
HW, CROP = (13, 21), (50, 81)
KEEP = [4, 0, -1, 2, 2, 5]                                   # a repeat and two indices outside [0, 5)


def _call(lib, dev, probs, keep, out, masks, stats, ws, nbytes):
    from boxinstseg_amd import _lib
    rc = lib.bxi_seg_paste_u8(G.ptr(probs), 5, HW[0], HW[1], G.ptr(keep), len(KEEP), 4 * HW[0], 4 * HW[1], CROP[0], CROP[1], out[0], out[1], 0.5,
                              G.ptr(masks), G.ptr(stats), G.ptr(ws), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)


@pytest.mark.parametrize('out_w', [64, 61])
@pytest.mark.parametrize('mask_lead', range(16))
def test_seg_paste_guarded(dev, mask_lead, out_w):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    out = (37, out_w)                                                         # three bands, the last one short
    n = len(KEEP)
    probs = torch.from_numpy(R.disc_probs(np.random.default_rng(1), 5, *HW)).to(dev)
    keep = torch.tensor(KEEP, device=dev)
    nbytes = lib.bxi_seg_paste_workspace_bytes(n, *out)
    assert nbytes == 16 * n * out[0] and nbytes % 16 == 0
    want_m = torch.empty((n, *out), dtype=torch.uint8, device=dev)
    want_s = torch.empty((n, 5), dtype=torch.int32, device=dev)
    _call(lib, dev, probs, keep, out, want_m, want_s, torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
    lead4 = 1 + mask_lead % 3                                                 # 4, 8, 12 bytes
    gp, gk = G.embed(probs, lead4, G.plane_band(*HW)), G.embed(keep, 1)
    gm = G.out((n, *out), torch.uint8, dev, mask_lead, G.plane_band(*out))
    gs = G.out((n, 5), torch.int32, dev, 4 - lead4)
    ws = G.out(nbytes // 4, torch.int32, dev, 0)                              # 16-byte aligned, exactly the size asked for
    assert gp.ptr() % 16 == 4 * lead4 and gm.ptr() % 16 == mask_lead and gs.ptr() % 16 == 4 * (4 - lead4) and ws.ptr() % 16 == 0
    _call(lib, dev, gp, gk, out, gm, gs, ws, nbytes)
    G.check_bands(gp, gk, gm, gs, ws)
    G.check_written(gm, gs, ws)
    G.check_unchanged(gp, gk)
    assert torch.equal(gm.t, want_m) and torch.equal(gs.t, want_s)
    assert bool(want_m.any()) and not bool(want_m[2].any()) and want_s[5].tolist() == [0, -1, -1, -1, -1]
