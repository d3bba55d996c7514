"""GPU: the entry points of include/boxinst/boxinst_hip_solo.h on misaligned views inside poisoned bands (tests/guarded.py).

Mask bytes start at every byte offset 1..15 past a 16-byte boundary (the mask pass reads 16-byte vectors between a byte-wise head and
tail), fp32 inputs at 4, 8 and 12 bytes, int64 at 8, surrounded by 0xFF / NaN / -1; outputs and the workspace are pre-filled with the
'nobody wrote this' pattern and the workspace is exactly as large as the size query says.  Afterwards the bands are intact, every output
element is written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import solo_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.SOLO_SIGNATURES)
GUARDED = {
    'bxi_solo_mask_pass_u8': 'test_mask_pass_guarded',
    'bxi_solo_assign_f32': 'test_assign_guarded',
    'bxi_solo_cate_loss_f32': 'test_cate_loss_guarded',
    'bxi_solo_cate_grad_rescale_f32': 'test_cate_grad_rescale_guarded',
}
BAND = 4096
SPEC = R.load_cases()
CASE = SPEC['cases']['mixed']
L, B_IMGS, C = len(SPEC['num_grids']), SPEC['B'], SPEC['num_classes']
OFFSETS = [0, 6, 8, 8]


def _plain(dev, mode):
    import boxinstseg_amd as B
    from boxinstseg_amd import parse_solo_head_cfg
    boxes, labels = R.gt_of(CASE, device=dev)
    masks = [torch.from_numpy(m).to(dev) for m in R.masks_of(CASE)]
    s = parse_solo_head_cfg(R.head_cfg(SPEC, mode))
    if mode == 'discobox':
        return B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **s), s
    return B.box_solov2_targets(boxes, labels, masks, [hw for _, hw in R.level_planes(SPEC, mode)], **s), s


@pytest.mark.parametrize('lead', range(1, 16))
def test_mask_pass_guarded(dev, lead):
    """bxi_solo_mask_pass_u8: the masks of both images at byte offset `lead` (image 1 at 16 - lead) inside 0xFF bytes -- a byte of the band
    that was counted would change a moment, one that was sampled a rescaled pixel; all three factors; every byte of every plane written."""
    from boxinstseg_amd import _lib
    plain, _ = _plain(dev, 'boxlevelset')
    masks = [torch.from_numpy(m).to(dev) for m in R.masks_of(CASE)]
    gm = [G.embed(masks[0], lead, BAND), G.embed(masks[1], 16 - lead, BAND)]
    factors = sorted(plain.masks)
    assert factors == [4, 8, 16]
    gout = [G.out(tuple(plain.masks[f].shape), torch.uint8, dev, (lead + 3 * k) % 16, BAND) for k, f in enumerate(factors)]
    gmom = G.out((8, 3), torch.int64, dev, 1, BAND)
    ia, pa = _lib.int_array, _lib.ptr_array
    rc = _lib.load().bxi_solo_mask_pass_u8(
        pa([gm[0].ptr(), gm[1].ptr(), 0]), ia(OFFSETS), ia([64, 32, 32]), ia([96, 64, 32]), B_IMGS, ia(factors),
        ia([plain.masks[f].shape[1] for f in factors]), ia([plain.masks[f].shape[2] for f in factors]), len(factors), pa([o.ptr() for o in gout]),
        gmom.ptr(), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(*gm, *gout, gmom)
    G.check_written(*gout, gmom)
    G.check_unchanged(*gm)
    assert G.same(gmom.t, plain.moments)
    for o, f in zip(gout, factors):
        assert G.same(o.t, plain.masks[f]), f


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('mode', R.MODES)
def test_assign_guarded(dev, lead, mode):
    """bxi_solo_assign_f32: boxes, labels and moments as misaligned views inside NaN / -1 (a label of -1 that was read would set the
    status word); every element of every output written, the unused tails of the lists included."""
    from boxinstseg_amd import _lib
    plain, s = _plain(dev, mode)
    boxes, labels = R.gt_of(CASE, device=dev)
    gb, gl, gmo = G.embed(torch.cat(boxes), lead, BAND), G.embed(torch.cat(labels), 1, BAND), G.embed(plain.moments, 1, BAND)
    N = plain.flat_cate_labels.shape[0]
    P = _lib.SOLO_PAIRS_PER_INSTANCE * L * 8
    outs = [G.out(N, torch.int64, dev, 1), G.out(N, torch.uint8, dev, lead), G.out(N, torch.int32, dev, lead), G.out(N, torch.int32, dev, 4 - lead),
            G.out(P, torch.int32, dev, lead), G.out(P, torch.int32, dev, 4 - lead), G.out(2 * L * B_IMGS, torch.int32, dev, lead),
            G.out(1, torch.int32, dev, 3), G.out(1, torch.int32, dev, 1)]
    h, w = SPEC['mask_feat_size']
    rc = _lib.load().bxi_solo_assign_f32(
        _lib.SOLO_MODES[mode], B_IMGS, L, _lib.int_array(s['num_grids']), _lib.float_array([v for r in s['scale_ranges'] for v in r]), s['sigma'],
        C, 4 * h, 4 * w, gb.ptr(), gl.ptr(), gmo.ptr(), _lib.int_array(OFFSETS), *(o.ptr() for o in outs), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gb, gl, gmo, *outs)
    G.check_written(*outs)
    G.check_unchanged(gb, gl, gmo)
    cate, ind, owner, sel, pc, pi, counts, num_ins, status = (o.t for o in outs)
    assert G.same(cate, plain.flat_cate_labels) and G.same(ind.bool(), torch.cat(plain.ins_ind_labels)) and G.same(owner, torch.cat(plain.cell_owner))
    assert counts.view(L, B_IMGS, 2).cpu().tolist() == plain.counts and G.same(num_ins, plain.num_ins) and status.cpu().tolist() == [0]
    at = 0
    for l, S in enumerate(s['num_grids']):
        for b in range(B_IMGS):
            p0, (np_, ns) = _lib.SOLO_PAIRS_PER_INSTANCE * (l * 8 + OFFSETS[b]), plain.counts[l][b]
            cap = _lib.SOLO_PAIRS_PER_INSTANCE * (OFFSETS[b + 1] - OFFSETS[b])
            assert G.same(pc[p0:p0 + np_].long(), plain.grid_order[l][b]) and bool((pc[p0 + np_:p0 + cap] == -1).all())
            assert bool((pi[p0 + np_:p0 + cap] == -1).all()) and bool((sel[at + ns:at + S * S] == -1).all())
            at += S * S
        assert G.same(torch.cat([pi[_lib.SOLO_PAIRS_PER_INSTANCE * (l * 8 + OFFSETS[b]):][:plain.counts[l][b][0]] for b in range(B_IMGS)]).long(),
                      plain.pair_inst[l])


def _cate_setup(dev, mode):
    from boxinstseg_amd import _lib
    plain, s = _plain(dev, mode)
    g = np.load(R.GOLDEN)
    preds = [torch.from_numpy(g[f'in_cate{l}']).to(dev) for l in range(L)]
    grids = _lib.int_array(s['num_grids'])
    nbytes = _lib.load().bxi_solo_cate_workspace_bytes(grids, L, B_IMGS, C)
    assert nbytes > 0
    return plain, s, preds, grids, nbytes


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('mode', R.MODES)
def test_cate_loss_guarded(dev, lead, mode):
    """bxi_solo_cate_loss_f32: the five maps, the labels and num_ins as misaligned views (gamma = 2 and the general-gamma kernel); every
    gradient element, the loss and the whole workspace written."""
    from boxinstseg_amd import _lib
    plain, s, preds, grids, nbytes = _cate_setup(dev, mode)
    lib, pa = _lib.load(), _lib.ptr_array

    def call(maps, labels, num_ins, grads, loss, ws):
        rc = lib.bxi_solo_cate_loss_f32(pa(maps), grids, L, B_IMGS, C, labels, num_ins, s['gamma'], s['alpha'], s['loss_weight_cate'], pa(grads), loss,
                                        ws, nbytes, G.stream(dev))
        assert rc == 0, _lib.STATUS.get(rc, rc)

    pg, pl, pw = [torch.empty_like(t) for t in preds], torch.empty(1, device=dev), torch.empty(nbytes // 4, device=dev)
    call([t.data_ptr() for t in preds], plain.flat_cate_labels.data_ptr(), plain.num_ins.data_ptr(), [t.data_ptr() for t in pg], pl.data_ptr(),
         pw.data_ptr())
    gin = [G.embed(t, (lead + l) % 4, BAND) for l, t in enumerate(preds)]
    gout = [G.out(tuple(t.shape), torch.float32, dev, (lead + 1 + l) % 4, BAND) for l, t in enumerate(preds)]
    glab, gnum = G.embed(plain.flat_cate_labels, 1, BAND), G.embed(plain.num_ins, lead, BAND)
    gloss, gw = G.out(1, torch.float32, dev, lead), G.out(nbytes // 4, torch.float32, dev, lead)
    call([t.ptr() for t in gin], glab.ptr(), gnum.ptr(), [t.ptr() for t in gout], gloss.ptr(), gw.ptr())
    G.check_bands(*gin, *gout, glab, gnum, gloss, gw)
    G.check_written(*gout, gloss, gw)
    G.check_unchanged(*gin, glab, gnum)
    assert G.same(gloss.t, pl) and bool(torch.isfinite(gloss.t).all()) and float(gloss.t) > 0
    for got, want in zip(gout, pg):
        assert G.same(got.t, want) and bool(torch.isfinite(got.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('in_place', [False, True])
def test_cate_grad_rescale_guarded(dev, lead, in_place):
    """bxi_solo_cate_grad_rescale_f32: unit gradients and the upstream scalar as misaligned views; every element of every output written."""
    from boxinstseg_amd import _lib
    _, s, preds, grids, _ = _cate_setup(dev, 'discobox')
    up = torch.tensor([0.375], device=dev)
    gup = G.embed(up, lead, BAND)
    if in_place:
        gout = [G.out(tuple(t.shape), torch.float32, dev, (lead + l) % 4, BAND) for l, t in enumerate(preds)]
        for o, t in zip(gout, preds):
            o.t.copy_(t)
        gin = gout
    else:
        gin = [G.embed(t, (lead + l) % 4, BAND) for l, t in enumerate(preds)]
        gout = [G.out(tuple(t.shape), torch.float32, dev, (lead + 2 + l) % 4, BAND) for l, t in enumerate(preds)]
    rc = _lib.load().bxi_solo_cate_grad_rescale_f32(grids, L, B_IMGS, C, _lib.ptr_array([t.ptr() for t in gin]), gup.ptr(),
                                                    _lib.ptr_array([t.ptr() for t in gout]), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gup, *gout)
    G.check_written(*gout)
    G.check_unchanged(gup)
    if not in_place:
        G.check_bands(*gin)
        G.check_unchanged(*gin)
    for got, src in zip(gout, preds):
        assert G.same(got.t, src * up[0])
