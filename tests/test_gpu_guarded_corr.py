"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_corr.h on misaligned views inside poisoned bands (tests/guarded.py).

fp32 inputs start 4, 8 or 12 bytes past a 16-byte boundary, int64 labels at 8, int32 lists at 4, surrounded by NaN / -1 (a label or a slot
of -1 that was read would drop an object; a NaN that was read reaches a score, a plane or the loss); outputs are pre-filled with the
'nobody wrote this' pattern, and so is the workspace, which is exactly as large as the size query says.  Afterwards the bands are intact,
every output element is written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import corr_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.CORR_SIGNATURES)
GUARDED = {
    'bxi_corr_plan_f32': 'test_plan_guarded',
    'bxi_corr_retrieve_f32': 'test_retrieve_guarded',
    'bxi_corr_solve_f32': 'test_solve_loss_iiu_guarded',
    'bxi_corr_loss_f32': 'test_solve_loss_iiu_guarded',
    'bxi_corr_iiu_f32': 'test_solve_loss_iiu_guarded',
    'bxi_corr_grad_rescale_f32': 'test_grad_rescale_guarded',
    'bxi_corr_append_f32': 'test_append_guarded',
    'bxi_corr_superres_f32': 'test_superres_guarded',
    'bxi_corr_cu_backward_f32': 'test_cu_backward_guarded',
}
BAND = 4096
NAME = 'in_call'
SPEC = R.load_cases()
CFG, CASE = SPEC['cfg'], SPEC['cases'][NAME]
N, C, L, NC, K = len(CASE['objects']), CASE['C'], CASE['L'], CASE['num_class'], CFG['max_retrieval_objs']
H, W = CASE['out_hw']
THRESH = (CFG['fg_iou_thresh'], CFG['bg_iou_thresh'], CFG['appear_thresh'], CFG['ratio_range'][0], CFG['ratio_range'][1])
_PLAIN = {}


def plain(dev):
    """The fused call on plain tensors, once: inputs, every intermediate list and output."""
    if not _PLAIN:
        from tests.test_gpu_corr import fused
        _PLAIN.update(fused(dev, NAME))
        _PLAIN['before'] = R.inputs_of(np.load(R.GOLDEN), NAME, dev)
    return _PLAIN


def _inputs(dev, lead):
    p = plain(dev)
    b = p['before']
    g = {k: G.embed(b[k], (lead + j) % 4 or 1, BAND) for j, k in enumerate(('s_feat', 's_mask', 't_feat', 't_mask', 'boxes', 'bank_feature', 'bank_mask', 'bank_box'))}
    g['labels'] = G.embed(b['labels'], 1, BAND)
    g['bank_ptr'] = G.embed(b['bank_ptr'], lead, BAND)
    for k in ('obj_slot', 'obj_role', 'ret_slot', 'ret_src', 'count'):
        g[k] = G.embed(p[k], lead, BAND)
    return p, g


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_plan_guarded(dev, lead):
    from boxinstseg_amd import _lib
    p, g = _inputs(dev, lead)
    slot, role = G.out(N, torch.int32, dev, lead), G.out(N, torch.int32, dev, 4 - lead)
    G.ok(_lib.load().bxi_corr_plan_f32(g['boxes'].ptr(), g['labels'].ptr(), g['bank_ptr'].ptr(), N, NC, L, float(CASE['min_size']), slot.ptr(), role.ptr(),
                                       G.stream(dev)))
    G.check_bands(g['boxes'], g['labels'], g['bank_ptr'], slot, role)
    G.check_written(slot, role)
    G.check_unchanged(g['boxes'], g['labels'], g['bank_ptr'])
    assert G.same(slot.t, p['obj_slot']) and G.same(role.t, p['obj_role'])
    assert slot.t.cpu().tolist() == [5, 0, 1] and role.t.cpu().tolist() == [1, 1, 3]      # ptr 5 of 6: the second append wraps


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_retrieve_guarded(dev, lead):
    from boxinstseg_amd import _lib
    p, g = _inputs(dev, lead)
    outs = [G.out((N, L), torch.int32, dev, 4 - lead), G.out((N, K), torch.int32, dev, lead), G.out((N, K), torch.int32, dev, 4 - lead),
            G.out(N, torch.int32, dev, lead), G.out((N, L, 4), torch.float32, dev, lead)]
    ins = [g[k] for k in ('s_feat', 's_mask', 't_feat', 't_mask', 'boxes', 'labels', 'obj_slot', 'bank_feature', 'bank_mask', 'bank_box')]
    G.ok(_lib.load().bxi_corr_retrieve_f32(*(t.ptr() for t in ins[:7]), N, C, *(t.ptr() for t in ins[7:]), NC, L, *THRESH, K, *(o.ptr() for o in outs),
                                           G.stream(dev)))
    G.check_bands(*ins, *outs)
    G.check_written(*outs[:4])                                               # a score may be NaN by itself (an empty slot): compared below
    G.check_unchanged(*ins)
    for o, k in zip(outs[1:], ('ret_slot', 'ret_src', 'count', 'scores')):
        assert G.same(o.t, p[k]), k
    assert outs[0].t.sum(1).cpu().tolist() == [4, 5, 6]                      # object 2 sees six passing slots and keeps five


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_solve_loss_iiu_guarded(dev, lead):
    """bxi_corr_solve_f32, then bxi_corr_loss_f32 and bxi_corr_iiu_f32 on the workspace it left, all three guarded."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    p, g = _inputs(dev, lead)
    nbytes = lib.bxi_corr_workspace_bytes(N, C, K)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = G.out(nbytes // 4, torch.float32, dev, 0, BAND)                     # 16-byte aligned, exactly the size asked for
    Cu, Cm, assign = G.out((N, K, 49, 49), torch.float32, dev, lead), G.out((N, K, 49, 49), torch.float32, dev, 4 - lead), G.out((N, K, 49), torch.int32, dev, lead)
    lists = [g[k] for k in ('ret_slot', 'ret_src', 'count')]
    G.ok(lib.bxi_corr_solve_f32(g['s_feat'].ptr(), g['t_feat'].ptr(), g['labels'].ptr(), N, C, g['bank_feature'].ptr(), NC, L, *(t.ptr() for t in lists), K,
                                CFG['min_objs'], CFG['dist_kernel'], CFG['corr_num_iter'], CFG['corr_num_smooth_iter'], Cu.ptr(), Cm.ptr(), assign.ptr(),
                                ws.ptr(), nbytes, G.stream(dev)))
    G.check_bands(g['s_feat'], g['t_feat'], g['labels'], g['bank_feature'], *lists, Cu, Cm, assign, ws)
    G.check_written(Cu, Cm, assign)
    assert G.same(Cu.t, p['Cu']) and G.same(Cm.t, p['C']) and G.same(assign.t, p['assign'])
    loss, num, grad = G.out(1, torch.float32, dev, lead), G.out(1, torch.int32, dev, lead), G.out((N, C, 7, 7), torch.float32, dev, 4 - lead)
    G.ok(lib.bxi_corr_loss_f32(g['count'].ptr(), N, C, K, CFG['min_objs'], loss.ptr(), num.ptr(), grad.ptr(), ws.ptr(), nbytes, G.stream(dev)))
    G.check_bands(g['count'], loss, num, grad, ws)
    G.check_written(loss, num, grad)
    assert G.same(loss.t.view(()), p['loss']) and int(num.t) == int(p['num_ins']) and G.same(grad.t, p['grad'])
    iiu = G.out((N, 2, H, W), torch.float32, dev, lead, G.plane_band(H, W))
    G.ok(lib.bxi_corr_iiu_f32(g['s_mask'].ptr(), g['t_mask'].ptr(), g['boxes'].ptr(), g['labels'].ptr(), N, C, g['bank_mask'].ptr(), NC, L,
                              *(t.ptr() for t in lists), K, CFG['min_objs'], H, W, iiu.ptr(), ws.ptr(), nbytes, G.stream(dev)))
    G.check_bands(g['s_mask'], g['t_mask'], g['boxes'], g['labels'], g['bank_mask'], *lists, iiu, ws)
    G.check_written(iiu)
    G.check_unchanged(g['s_feat'], g['t_feat'], g['s_mask'], g['t_mask'], g['boxes'], g['labels'], g['bank_feature'], g['bank_mask'], *lists)
    assert G.same(iiu.t, p['iiu']) and bool(torch.isfinite(iiu.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('in_place', [False, True])
def test_grad_rescale_guarded(dev, lead, in_place):
    from boxinstseg_amd import _lib
    p = plain(dev)
    up = torch.tensor([0.375], device=dev)
    gup = G.embed(up, lead, BAND)
    out = G.out(tuple(p['grad'].shape), torch.float32, dev, 4 - lead, BAND)
    src = out if in_place else G.embed(p['grad'], lead, BAND)
    if in_place:
        out.t.copy_(p['grad'])
    G.ok(_lib.load().bxi_corr_grad_rescale_f32(src.ptr(), gup.ptr(), p['grad'].numel(), out.ptr(), G.stream(dev)))
    G.check_bands(gup, out, src)
    G.check_written(out)
    G.check_unchanged(gup)
    if not in_place:
        G.check_unchanged(src)
    assert G.same(out.t, p['grad'] * up[0])


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_append_guarded(dev, lead):
    """bxi_corr_append_f32.  The bank itself is the output: embedded with its contents, the bands around it must survive and the result is the fused call's bank."""
    from boxinstseg_amd import _lib
    p, g = _inputs(dev, lead)
    ins = [g[k] for k in ('t_feat', 't_mask', 'boxes', 'labels', 'obj_slot', 'obj_role')]
    bank = [g[k] for k in ('bank_feature', 'bank_mask', 'bank_box', 'bank_ptr')]
    G.ok(_lib.load().bxi_corr_append_f32(*(t.ptr() for t in ins), N, C, *(t.ptr() for t in bank), NC, L, G.stream(dev)))
    G.check_bands(*ins, *bank)
    G.check_unchanged(*ins)
    for t, want in zip(bank, (p['bank'].feature, p['bank'].mask, p['bank'].box, p['bank'].ptr)):
        assert G.same(t.t, want)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_superres_guarded(dev, lead):
    from boxinstseg_amd import _lib, superres_T
    p = plain(dev)
    T = p['C'][1, :2].contiguous()
    want = superres_T(T)
    gT, out = G.embed(T, lead, BAND), G.out((2, 784, 784), torch.float32, dev, 4 - lead, BAND)
    G.ok(_lib.load().bxi_corr_superres_f32(gT.ptr(), 2, out.ptr(), G.stream(dev)))
    G.check_bands(gT, out)
    G.check_written(out)
    G.check_unchanged(gT)
    assert G.same(out.t, want)


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_cu_backward_guarded(dev, lead):
    from boxinstseg_amd import _lib
    p = plain(dev)
    f0, f1 = p['before']['s_feat'][1].contiguous(), p['before']['bank_feature'][0, 1:5].contiguous()
    dCu = torch.sin(torch.arange(4 * 2401, device=dev, dtype=torch.float32)).view(4, 49, 49)

    def call(a, b, d, o):
        G.ok(_lib.load().bxi_corr_cu_backward_f32(a, b, d, 4, C, o, G.stream(dev)))

    want = torch.empty_like(f0)
    call(f0.data_ptr(), f1.data_ptr(), dCu.data_ptr(), want.data_ptr())
    g0, g1, gd = G.embed(f0, lead, BAND), G.embed(f1, 4 - lead, BAND), G.embed(dCu, lead, BAND)
    out = G.out(tuple(f0.shape), torch.float32, dev, 4 - lead, BAND)
    call(g0.ptr(), g1.ptr(), gd.ptr(), out.ptr())
    G.check_bands(g0, g1, gd, out)
    G.check_written(out)
    G.check_unchanged(g0, g1, gd)
    assert G.same(out.t, want)
