"""Where the per-instance table is written in the single launch (fused_eval.hip, eval1_kernel): wave 0 of stream workgroup k -- or, where
the stream workgroups stay on as tile workgroups and the last band of an instance leaves a wave without rows, the last wave of instance
k's last band.  On the smallest shapes at which the placement can go wrong: both sides of the threshold (a last band of 24 and of 25
rows), one and several bands per instance, one, two and three table waves (63 / 64 / 130 instances), one instance, degenerate images,
the shared-device form (nobody stays on: the table stays where it was), a wait that gives up, the wrap evaluation, changing shapes
on one workspace.

Every case asks the library (bxi_dev_eval1_plan through _lib.eval1_plan: the host code that launches) which placement its shape and
flags take and asserts it is the one the case is about, compares losses and gradient bit for bit with the two-launch form (whose table
has workgroups of its own) and with the C oracle within 1e-4, and reads the status word."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

from boxinstseg_amd import synthetic
from tests.helpers import grad_report, hip_loss, oracle_path, rel, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-4
BAND, WAVE_ROWS, WAVES = 32, 8, 4          # rows per stream workgroup, per wave; waves per workgroup (eval_protocol_device.hpp)


def _launched(fn):
    """-> (fn(), names of the library's launches meanwhile: the hook reports each before and after it is enqueued)."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    names = []
    cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: names.append(name.decode()))
    lib.bxi_dev_set_launch_hook(C.cast(cb, C.c_void_p), None)
    try:
        out = fn()
    finally:
        lib.bxi_dev_set_launch_hook(None, None)
    return out, names


def _plan(d, dev, dil=2, flags=0):
    from boxinstseg_amd import _lib
    return _lib.eval1_plan(d['B'], d['N'], d['h'], d['w'], dil, flags, torch.cuda.current_stream(dev).cuda_stream)


def _idle_last_wave(d):
    """The geometry alone: the last band of an instance leaves its last wave without rows."""
    bands = -(-d['h'] // BAND)
    return d['h'] - (bands - 1) * BAND <= (WAVES - 1) * WAVE_ROWS


def _rows(flags):
    from boxinstseg_amd import _lib
    return flags & (_lib.EVAL_TILE_ROWS_4 | _lib.EVAL_TILE_ROWS_8)


_WANT = {}


def _digest(d, dil, flags):
    """What the reference depends on: the batch's bytes, the dilation and the tile rows."""
    crc = 0
    for arr in [d['imgs'], d['mask_logits'], d['gt_inds']] + list(d['gt_bboxes']):
        crc = zlib.crc32(np.ascontiguousarray(arr).tobytes(), crc)
    shapes = tuple(tuple(m['img_shape']) for m in d['img_metas'])
    return crc, shapes, dil, _rows(flags)


def _two_launches_and_oracle(d, dev, dil=2, flags=0):
    """The two-launch form's losses and gradient, checked against the oracle; computed once per (batch, dilation, tile rows) and shared."""
    from boxinstseg_amd import _lib, functional as Fh
    key = _digest(d, dil, flags)
    if key not in _WANT:
        with Fh.eval_flags(_lib.EVAL_TWO_LAUNCHES | _rows(flags)):
            want, names = _launched(lambda: hip_loss(d, dev, pairwise_dilation=dil))
        assert 'pair' in names and 'eval1' not in names, names
        assert Fh.last_eval_status()[0] == 0
        ref = oracle_path(d, want_targets=False, size=3, dil=dil)
        assert rel(want[0], ref['loss_prj']) <= TOL, (want[0], ref['loss_prj'])
        assert rel(want[1], ref['loss_pairwise']) <= TOL or abs(want[1] - ref['loss_pairwise']) < 1e-7, (want[1], ref['loss_pairwise'])
        err, _ = grad_report(want[2], ref['grad'], d['mask_logits'][:, 0])
        assert err <= TOL, err
        _WANT[key] = want
    return _WANT[key]


def _same_bits(got, want, what):
    assert got[0] == want[0] and got[1] == want[1], (what, got[:2], want[:2])
    assert np.array_equal(got[2], want[2]), what


def _single_launch(d, dev, table_last, dil=2, flags=0):
    """One evaluation in the single launch under `flags`, after the plan has said that the table is where the case means it to be:
    status 0, the two-launch form's bits."""
    from boxinstseg_amd import functional as Fh
    p = _plan(d, dev, dil, flags)
    assert p['taken'] == 1 and p['table_last'] == (1 if table_last else 0) and p['merge'] >= p['table_last'], (p, table_last)
    want = _two_launches_and_oracle(d, dev, dil, flags)
    with Fh.eval_flags(flags):
        got, names = _launched(lambda: hip_loss(d, dev, pairwise_dilation=dil))
    assert 'eval1' in names and 'pair' not in names and 'prep' not in names, names
    assert Fh.last_eval_status()[0] == 0
    _same_bits(got, want, (d['N'], d['h'], dil, flags))
    return got


def _canvas(h, boxes_per_img, seed, **kw):
    """B = 2 on a canvas of h x 40 cells whose images differ in shape."""
    H = 4 * h
    kw.setdefault('min_box', 16)
    kw.setdefault('max_box', 120)
    return synthetic.make_batch(B=2, H=H, W=160, boxes_per_img=boxes_per_img, seed=seed, img_shapes=[(H, 160), (H - 8, 150)], **kw)


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('h,last_band', [(24, True), (25, False), (56, True), (57, False)])
def test_both_sides_of_the_threshold(dev, h, last_band, dil):
    """A last band of 24 rows leaves its last wave idle, one of 25 does not; with one band per instance and with two; both dilations
    (the table holds tile counts, which depend on it, and each dilation is a kernel of its own)."""
    d = _canvas(h, 3, 80 + h)
    assert d['h'] == h and _idle_last_wave(d) == last_band
    _single_launch(d, dev, last_band, dil=dil)


def _first_instances(d, n):
    return dict(d, gt_inds=d['gt_inds'][:n], mask_logits=d['mask_logits'][:n], N=n)


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('n,flags', [(1, 0), (63, 0), (64, 0), (130, 'rows4')], ids=['n1', 'n63', 'n64', 'n130'])
def test_one_two_and_three_table_waves(dev, n, flags, dil):
    """Table wave k sits in instance k's last band: one instance; 63 (entry 63 is the total); 64 (a second wave for the total alone); 130."""
    from boxinstseg_amd import _lib
    flags = _lib.EVAL_TILE_ROWS_4 if flags == 'rows4' else 0           # (from 96 instances on the library's own choice is two launches)
    d = _first_instances(_canvas(24, 65, 90, min_box=40, max_box=160), n)
    _single_launch(d, dev, True, dil=dil, flags=flags)


def test_several_bands_two_idle_waves(dev):
    """One image of 804 x 1024 with 32 instances: 201 rows, a last band of 9 (two idle waves), 224 stream workgroups."""
    d = synthetic.make_batch(B=1, H=804, W=1024, boxes_per_img=32, seed=72)
    assert (d['N'], d['h']) == (32, 201) and _idle_last_wave(d)
    _single_launch(d, dev, True)


def test_the_stream_workgroups_must_stay_on(dev):
    """64 instances of 200 rows: the geometry leaves idle waves, but 448 stream workgroups are more than a quarter of the slots -- nobody
    stays on, and the plan keeps the table where it was."""
    d = synthetic.cfg2(78, inst_per_box=2)
    assert (d['N'], d['h']) == (64, 200) and _idle_last_wave(d)
    p = _plan(d, dev)
    assert (p['taken'], p['merge'], p['table_last']) == (1, 0, 0), p
    _single_launch(d, dev, False)


def test_zero_instances(dev):
    """No instances: none of the evaluation's kernels runs (the plan is all zero), both losses are zero."""
    from boxinstseg_amd import _lib, boxinst_mask_loss
    d = _canvas(24, 3, 104)
    assert not any(_lib.eval1_plan(d['B'], 0, d['h'], d['w']).values())
    t = to_dev(d, dev)
    empty = torch.zeros((0, 1, d['h'], d['w']), device=dev, requires_grad=True)
    out, names = _launched(lambda: boxinst_mask_loss(empty, torch.zeros(0, dtype=torch.long, device=dev), t['gt_bboxes'], imgs=t['imgs'],
                                                     img_metas=d['img_metas']))
    assert float(out['loss_prj'].detach()) == 0.0 and float(out['loss_pairwise'].detach()) == 0.0
    assert 'eval1' not in names and 'prep' not in names and 'pair' not in names, names
    (out['loss_prj'] + out['loss_pairwise']).backward()
    torch.cuda.synchronize()


def test_degenerate_images(dev):
    d = _canvas(24, 3, 71)                      # an image without boxes
    d['gt_bboxes'][0] = np.zeros((0, 4), np.float32)
    d['gt_inds'] = np.array([0, 1, 1, 2], np.int64)
    d['mask_logits'] = d['mask_logits'][:4]
    d['N'] = 4
    _single_launch(d, dev, True)
    # an image none of whose rows is valid (8 rows, 10 removed at the bottom)
    d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=2, seed=77, img_shapes=[(96, 160), (8, 160)], min_box=4, max_box=100)
    _single_launch(d, dev, True)


def test_shared_device_keeps_the_table_where_it_was(dev):
    from boxinstseg_amd import _lib
    d = _canvas(24, 3, 104)
    _single_launch(d, dev, True)
    p = _plan(d, dev, 2, _lib.EVAL_SHARED_DEVICE)
    assert (p['taken'], p['merge'], p['table_last']) == (1, 0, 0), p
    _single_launch(d, dev, False, flags=_lib.EVAL_SHARED_DEVICE)


def test_waits_that_give_up_are_loud_and_a_reset_brings_the_bits_back(dev):
    from boxinstseg_amd import _lib, boxinst_mask_loss, functional as Fh
    d = _canvas(24, 3, 104)
    good = _single_launch(d, dev, True)
    assert _plan(d, dev, 2, _lib.EVAL_WAITS_GIVE_UP)['table_last'] == 1
    t = to_dev(d, dev)
    with Fh.eval_flags(_lib.EVAL_WAITS_GIVE_UP):
        Fh.DEBUG_KEEP_LAST = True
        x = t['logits'].clone().requires_grad_(True)

        def ev():
            out = boxinst_mask_loss(x, t['gt_inds'], t['gt_bboxes'], imgs=t['imgs'], img_metas=d['img_metas'], out_stride=d['stride'])
            (out['loss_prj'] + out['loss_pairwise']).backward()
            torch.cuda.synchronize()
            return out
        out, names = _launched(ev)
        assert 'eval1' in names, names
        assert math.isnan(float(out['loss_prj'].detach())) and math.isnan(float(out['loss_pairwise'].detach()))
        assert Fh.last_eval_status()[0] != 0
        assert bool(torch.isnan(x.grad).all())
    Fh.reset_eval_state(drop_workspaces=False)
    with Fh.eval_flags(0):
        again = hip_loss(d, dev)
    assert Fh.last_eval_status()[0] == 0
    _same_bits(again, good, 'after the reset')


def test_wrap_evaluation_zeroes_the_workspace_and_gives_ordinary_bits(dev):
    """The evaluation that draws tag 2^28 - 1 ends by zeroing the workspace: the table's own zeroes and entries are long in memory."""
    from boxinstseg_amd import _lib, functional as Fh
    lib = _lib.load()
    d = _canvas(24, 3, 104)
    assert _plan(d, dev)['table_last'] == 1
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
                                      state.data_ptr(), ws.data_ptr(), ws.numel(), 0, st)
        assert rc == 0, _lib.status_string(rc)
        torch.cuda.synchronize()
        assert state[off:off + 4].view(torch.int32).item() == 0
        return losses.cpu().numpy(), grad.cpu().numpy()

    usual = run()
    want = _two_launches_and_oracle(d, dev)
    assert usual[0][0] == np.float32(want[0]) and usual[0][1] == np.float32(want[1]) and np.array_equal(usual[1][:, 0], want[2])
    assert int(ws[:4].view(torch.int32).item()) == 1
    ws[:4].view(torch.int32).fill_(top - 1)                 # the next evaluation draws tag 2^28 - 1
    wrapped, names = _launched(run)
    assert set(names) == {'eval1'}, names
    assert int(ws.view(torch.int32).ne(0).sum().item()) == 0, 'the wrap leaves the workspace all zero'
    assert np.array_equal(wrapped[0], usual[0]) and np.array_equal(wrapped[1], usual[1])
    after = run()
    assert int(ws[:4].view(torch.int32).item()) == 1
    assert np.array_equal(after[0], usual[0]) and np.array_equal(after[1], usual[1])


def test_changing_shapes_on_one_workspace(dev):
    """Forty evaluations alternating among three instance counts on one canvas -- one workspace (boxinstseg_amd.functional keeps one per
    canvas; the largest count goes first, so it is never replaced), one, two and three table waves: status 0, identical bits on repeats."""
    from boxinstseg_amd import _lib, functional as Fh
    Fh.reset_eval_state()
    base = _canvas(24, 65, 90, min_box=40, max_box=160)
    shapes = []
    for n, flags in ((130, _lib.EVAL_TILE_ROWS_4), (5, 0), (64, 0)):
        d = _first_instances(base, n)
        assert _plan(d, dev, 2, flags)['table_last'] == 1
        shapes.append((n, d, flags))
    first = {}
    ws_ptr = None
    for i in range(40):
        key, d, flags = shapes[i % 3]
        with Fh.eval_flags(flags):
            got = hip_loss(d, dev)
        assert Fh.last_eval_status()[0] == 0, (i, key)
        assert len(Fh._TLS.workspaces) == 1
        ptr = next(iter(Fh._TLS.workspaces.values()))[0].data_ptr()
        assert ws_ptr in (None, ptr), 'one workspace throughout'
        ws_ptr = ptr
        if key in first:
            _same_bits(got, first[key], (i, key))
        else:
            first[key] = got
            _same_bits(got, _two_launches_and_oracle(d, dev, 2, flags), key)
