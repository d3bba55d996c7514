"""Tile waves arrive at the finisher as soon as the pair loop of their last tile is done, ahead of their wait for sum W and their
gradient adds (fused_eval.hip: tile_role / math_tile).  The losses are fixed-point sums and every gradient element still receives at
most two float additions onto 0, so every form must keep giving the bits of the two-launch form; the wrap evaluation keeps the old
order; a wait that fails is loud in the single-launch form too."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from boxinstseg_amd import synthetic
from tests.helpers import grad_report, hip_loss, oracle_path, rel, to_dev
from tests.test_gpu_parity import _loss_with_targets

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _launched(lib, fn):
    """-> (fn(), names of the library's launches meanwhile)."""
    from boxinstseg_amd import _lib
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        out = fn()
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    return out, names


@pytest.mark.parametrize('ipb', [1, 2, 4], ids=['n32', 'n64', 'n128'])
def test_every_form_matches_the_two_launch_form_bit_for_bit(dev, ipb):
    """2 x 800 x 1024 images at 32 / 64 / 128 instances: the single launch (4-row tiles, with and without the stream workgroups staying
    on; at 128 instances its waves walk several tiles), the two-launch form with 4- and 8-row tiles, and the targets-ready evaluation in
    the library's own form and in the long single launch -- the same bits, status 0, within 1e-4 of the oracle."""
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    d = synthetic.cfg2(20 + ipb, inst_per_box=ipb)
    assert d['N'] == 32 * ipb
    with Fh.eval_flags(_lib.EVAL_TWO_LAUNCHES):
        want = hip_loss(d, dev)
    ref = oracle_path(d, want_targets=False)
    assert rel(want[0], ref['loss_prj']) <= TOL and rel(want[1], ref['loss_pairwise']) <= TOL, (want[:2], ref['loss_prj'], ref['loss_pairwise'])
    err, _ = grad_report(want[2], ref['grad'], d['mask_logits'][:, 0])
    assert err <= TOL, err
    one = _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4           # (from 96 instances on the library's own choice is 8-row tiles: two launches)
    forms = [(one, False, 'eval1'), (one | _lib.EVAL_SHARED_DEVICE, False, 'eval1'),
             (_lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_4, False, 'pair'), (_lib.EVAL_TWO_LAUNCHES | _lib.EVAL_TILE_ROWS_8, False, 'pair'),
             (0, True, None), (_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_8, True, 'eval1_ready')]
    for flags, ready, kernel in forms:
        with Fh.eval_flags(flags):
            got, names = _launched(lib, lambda: _loss_with_targets(d, dev) if ready else hip_loss(d, dev))
        assert Fh.last_eval_status()[0] == 0, flags
        if kernel is not None:
            assert kernel in names, (flags, names)
        assert got[0] == want[0] and got[1] == want[1], (flags, got[:2], want[:2])
        assert np.array_equal(got[2], want[2]), flags


@pytest.mark.parametrize('flags', ['single', 'two_launches'])
def test_wrap_evaluation_leaves_a_complete_gradient(dev, flags):
    """The evaluation that draws the last tag (2^28 - 1) zeroes the workspace once every tile wave has arrived; its tile waves arrive
    behind their adds.  At 128 instances (4-row tiles in one launch: waves walk several tiles) it must give the bits of an ordinary
    evaluation -- the whole gradient --, status 0, and leave the workspace all zero."""
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    form = (_lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4) if flags == 'single' else _lib.EVAL_TWO_LAUNCHES
    d = synthetic.cfg2(31, inst_per_box=4)
    t = to_dev(d, dev)
    batch = Fh._Batch(t['imgs'], d['img_metas'], 10)
    inst = Fh._Inst(t['logits'], t['gt_inds'], t['gt_bboxes'], d['H'], d['W'], d['stride'])
    ws = torch.zeros(lib.bxi_boxinst_eval_workspace_bytes(d['B'], d['H'], d['W'], d['stride'], inst.N), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    off = lib.bxi_boxinst_loss_state_status_offset(inst.N, inst.h, inst.w)
    top = (1 << 28) - 1

    def run():
        losses, grad = torch.zeros(2, device=dev), torch.full_like(inst.logits, 7.0)
        state = torch.empty(lib.bxi_boxinst_loss_state_bytes(inst.N, inst.h, inst.w), dtype=torch.uint8, device=dev)
        rc = lib.bxi_boxinst_eval_f32(C.byref(batch.struct), C.byref(inst.struct), 3, 2, 0.3, 1.0, None, None, losses.data_ptr(), grad.data_ptr(),
                                      state.data_ptr(), ws.data_ptr(), ws.numel(), form, st)
        assert rc == 0, _lib.status_string(rc)
        torch.cuda.synchronize()
        assert state[off:off + 4].view(torch.int32).item() == 0
        return losses.cpu().numpy(), grad.cpu().numpy()

    usual = run()
    assert int(ws[:4].view(torch.int32).item()) == 1
    ws[:4].view(torch.int32).fill_(top - 1)                 # the next evaluation draws tag 2^28 - 1
    (wrapped, names) = _launched(lib, run)
    assert ('eval1' if flags == 'single' else 'pair') in names, names
    assert int(ws.view(torch.int32).ne(0).sum().item()) == 0, 'the wrap leaves the workspace all zero'
    assert np.array_equal(wrapped[0], usual[0])
    assert np.array_equal(wrapped[1], usual[1]), 'the wrap evaluation gives the whole gradient'
    after = run()                                           # and the evaluations after it as well
    assert int(ws[:4].view(torch.int32).item()) == 1
    assert np.array_equal(after[0], usual[0]) and np.array_equal(after[1], usual[1])


@pytest.mark.parametrize('ipb', [1, 4], ids=['n32', 'n128'])
def test_waits_that_give_up_are_loud_in_the_single_launch(dev, ipb):
    """BXI_EVAL_WAITS_GIVE_UP in the single-launch form: NaN losses, a non-zero status word and a poisoned gradient; after the workspace is
    zeroed again the evaluation gives its usual bits."""
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    lib = _lib.load()
    d = synthetic.cfg2(40 + ipb, inst_per_box=ipb)
    one = _lib.EVAL_SINGLE_LAUNCH | _lib.EVAL_TILE_ROWS_4
    with Fh.eval_flags(one):
        good = hip_loss(d, dev)
    t = to_dev(d, dev)
    with Fh.eval_flags(one | _lib.EVAL_WAITS_GIVE_UP):
        Fh.DEBUG_KEEP_LAST = True
        x = t['logits'].clone().requires_grad_(True)

        def ev():
            out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], out_stride=d['stride'])
            (out['loss_prj'] + out['loss_pairwise']).backward()
            torch.cuda.synchronize()
            return out
        out, names = _launched(lib, ev)
        assert 'eval1' in names, names
        assert math.isnan(float(out['loss_prj'].detach())) and math.isnan(float(out['loss_pairwise'].detach()))
        assert Fh.last_eval_status()[0] != 0
        assert bool(torch.isnan(x.grad).all())
    Fh.reset_eval_state(drop_workspaces=False)
    with Fh.eval_flags(one):
        again = hip_loss(d, dev)
    assert again[0] == good[0] and again[1] == good[1] and np.array_equal(again[2], good[2])
