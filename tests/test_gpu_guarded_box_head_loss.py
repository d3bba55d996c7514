"""GPU: the entry points of include/boxinst/boxinst_hip_fcos.h on misaligned views inside poisoned bands (tests/guarded.py).

Inputs are views at the element's natural alignment only (fp32 at 4, 8 and 12 bytes past a 16-byte boundary, int64 at 8) surrounded by
NaN / -1; outputs and workspaces are pre-filled with the 'nobody wrote this' pattern and the workspaces are exactly as large as the
size query says.  Afterwards the bands are intact, every output element is written (every gradient element, zeros included), the inputs
are unchanged, and the results are bit-identical to the same call on plain tensors.  The shapes are the fixture's, whose coarsest level
is 3 x 5: a lead of 1..3 elements misaligns its 15-element planes (and every other plane) against the 16-byte vectors."""
import numpy as np
import pytest
import torch

from tests import fcos_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.FCOS_SIGNATURES)
GUARDED = {
    'bxi_fcos_targets_f32': 'test_targets_guarded',
    'bxi_fcos_loss_f32': 'test_loss_guarded',
    'bxi_fcos_grad_rescale_f32': 'test_grad_rescale_guarded',
}
BAND = 4096
SPEC = R.load_cases()
MAPS = ('cls', 'bbox', 'ctr')
B_IMGS, C = 2, SPEC['num_classes']


def _settings(name):
    from boxinstseg_amd import parse_box_head_cfg
    return parse_box_head_cfg(R.head_cfg(SPEC, name))


def _fcos_levels():
    from boxinstseg_amd import _lib
    arr = (_lib.FcosLevel * len(SPEC['levels']))()
    for i, ((h, w), s) in enumerate(zip(SPEC['levels'], SPEC['strides'])):
        arr[i] = _lib.FcosLevel(h, w, s)
    return arr


def _maps(dev):
    g = np.load(R.GOLDEN)
    return {k: [torch.from_numpy(g[f'in_{k}{lv}']).to(dev) for lv in range(len(SPEC['levels']))] for k in MAPS}


def _plain_targets(dev, s):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC, device=dev)
    return B.condinst_box_targets(SPEC['levels'], s['strides'], boxes, labels, regress_ranges=s['regress_ranges'],
                                  center_sampling=s['center_sampling'], center_sample_radius=s['center_sample_radius'],
                                  norm_on_bbox=s['norm_on_bbox'], num_classes=s['num_classes'], B=B_IMGS)


def _grads_array(gs):
    from boxinstseg_amd import _lib
    n = len(SPEC['levels'])
    arr = (_lib.FcosGrads * n)()
    for lv in range(n):
        arr[lv] = _lib.FcosGrads(gs['cls'][lv].ptr(), gs['bbox'][lv].ptr(), gs['ctr'][lv].ptr())
    return arr


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('name', ['cs_norm_giou', 'box_pix_ioulog'])
def test_targets_guarded(dev, lead, name):
    """bxi_fcos_targets_f32: the boxes and labels at misaligned addresses inside NaN / -1 (a NaN box that was read would make NaN targets;
    a label of -1 would set the status word), every row of every output written."""
    from boxinstseg_amd import _lib
    s = _settings(name)
    plain = _plain_targets(dev, s)
    boxes, labels = R.gt_of(SPEC, device=dev)
    gb, gl = G.embed(torch.cat(boxes), lead, BAND), G.embed(torch.cat(labels), 1, BAND)
    N = plain.labels.shape[0]
    outs = [G.out(N, torch.int64, dev, 1), G.out((N, 4), torch.float32, dev, lead), G.out(N, torch.int64, dev, 1), G.out((N, 2), torch.float32, dev, 4 - lead),
            G.out(N, torch.int64, dev, 1), G.out(N, torch.int64, dev, 1), G.out(N, torch.float32, dev, lead), G.out(2, torch.float32, dev, lead),
            G.out(1, torch.int32, dev, 3)]
    lv = _fcos_levels()
    loc_blocks = sum(B_IMGS * ((h * w + _lib.FCOS_LOC_TILE - 1) // _lib.FCOS_LOC_TILE) for h, w in SPEC['levels'])
    nbytes = 16 * loc_blocks                                                   # what this call needs of bxi_fcos_workspace_bytes
    assert nbytes <= _lib.load().bxi_fcos_workspace_bytes(lv, len(SPEC['levels']), B_IMGS, 1)
    gw = G.out(nbytes // 4, torch.int32, dev, lead)
    rc = _lib.load().bxi_fcos_targets_f32(
        lv, len(SPEC['levels']), B_IMGS, _lib.float_array([v for r in s['regress_ranges'] for v in r]), 1 if s['center_sampling'] else 0,
        s['center_sample_radius'], 1 if s['norm_on_bbox'] else 0, C, gb.ptr(), gl.ptr(), _lib.int_array([0, 5, 7]), *(o.ptr() for o in outs),
        gw.ptr(), nbytes, G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    G.check_bands(gb, gl, gw, *outs)
    G.check_written(gw, *outs)
    G.check_unchanged(gb, gl)
    for got, want in zip(outs, plain):
        assert G.same(got.t, want)
        assert not got.t.dtype.is_floating_point or bool(torch.isfinite(got.t).all())
    assert outs[8].t.cpu().tolist() == [0]


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('name', ['cs_norm_giou', 'box_pix_ioulog'])
def test_loss_guarded(dev, lead, name):
    """bxi_fcos_loss_f32: all nine maps, the targets and the normalisers as misaligned views (gamma = 2 and the general-gamma kernel);
    every element of every gradient map, the three losses and the whole workspace written."""
    from boxinstseg_amd import _lib
    s = _settings(name)
    tg = _plain_targets(dev, s)
    maps = _maps(dev)
    n = len(SPEC['levels'])
    kind = _lib.FCOS_BBOX_KINDS[s['bbox_loss_kind']]
    lib = _lib.load()
    nbytes = lib.bxi_fcos_workspace_bytes(_fcos_levels(), n, B_IMGS, C)
    assert nbytes > 0

    def call(levels, grads, labels, bt, ct, norm, losses, ws):
        rc = lib.bxi_fcos_loss_f32(levels, n, B_IMGS, C, labels, bt, ct, norm, s['gamma'], s['alpha'], s['loss_weight_cls'], s['loss_weight_bbox'],
                                   s['loss_weight_centerness'], kind, s['eps'], grads, losses, ws, nbytes, G.stream(dev))
        assert rc == 0, _lib.STATUS.get(rc, rc)

    # plain tensors
    plain_g = {k: [torch.empty_like(t) for t in maps[k]] for k in MAPS}
    plain_l = torch.empty(3, device=dev)
    plain_w = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    lv = (_lib.DetLevel * n)()
    pg = (_lib.FcosGrads * n)()
    for i, ((h, w), st) in enumerate(zip(SPEC['levels'], SPEC['strides'])):
        lv[i] = _lib.DetLevel(maps['cls'][i].data_ptr(), maps['bbox'][i].data_ptr(), maps['ctr'][i].data_ptr(), None, h, w, st)
        pg[i] = _lib.FcosGrads(plain_g['cls'][i].data_ptr(), plain_g['bbox'][i].data_ptr(), plain_g['ctr'][i].data_ptr())
    call(lv, pg, tg.labels.data_ptr(), tg.bbox_targets.data_ptr(), tg.ctr_targets.data_ptr(), tg.stats.data_ptr(), plain_l.data_ptr(), plain_w.data_ptr())
    # guarded
    gin = {k: [G.embed(t, (lead + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
    gout = {k: [G.out(tuple(t.shape), torch.float32, dev, (lead + 1 + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
    glab, gbt, gct = G.embed(tg.labels, 1, BAND), G.embed(tg.bbox_targets, lead, BAND), G.embed(tg.ctr_targets, 4 - lead, BAND)
    gnorm, glosses, gw = G.embed(tg.stats, lead, BAND), G.out(3, torch.float32, dev, lead), G.out(nbytes // 4, torch.int32, dev, lead)
    glv = (_lib.DetLevel * n)()
    for i, ((h, w), st) in enumerate(zip(SPEC['levels'], SPEC['strides'])):
        glv[i] = _lib.DetLevel(gin['cls'][i].ptr(), gin['bbox'][i].ptr(), gin['ctr'][i].ptr(), None, h, w, st)
    call(glv, _grads_array(gout), glab.ptr(), gbt.ptr(), gct.ptr(), gnorm.ptr(), glosses.ptr(), gw.ptr())
    ins = [t for k in MAPS for t in gin[k]] + [glab, gbt, gct, gnorm]
    outs = [t for k in MAPS for t in gout[k]] + [glosses, gw]
    G.check_bands(*ins, *outs)
    G.check_written(*outs)
    G.check_unchanged(*ins)
    assert G.same(glosses.t, plain_l) and bool(torch.isfinite(glosses.t).all()) and float(glosses.t.min()) > 0
    for k in MAPS:
        for got, want in zip(gout[k], plain_g[k]):
            assert G.same(got.t, want) and bool(torch.isfinite(got.t).all())
    assert any(bool((t.t != 0).any()) for t in gout['bbox']) and any(bool((t.t == 0).any()) for t in gout['bbox'])


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('in_place', [False, True])
def test_grad_rescale_guarded(dev, lead, in_place):
    """bxi_fcos_grad_rescale_f32: unit gradients and the three upstream scalars as misaligned views; every element of every output map
    written; in place, the unit gradients themselves are the outputs."""
    from boxinstseg_amd import _lib
    maps = _maps(dev)
    n = len(SPEC['levels'])
    up = torch.tensor([0.5, 3.0, 512.0], device=dev)
    gup = G.embed(up, lead, BAND)
    lib = _lib.load()
    if in_place:
        gout = {k: [G.out(tuple(t.shape), torch.float32, dev, (lead + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
        for k in MAPS:
            for o, t in zip(gout[k], maps[k]):
                o.t.copy_(t)
        gin = gout
    else:
        gin = {k: [G.embed(t, (lead + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
        gout = {k: [G.out(tuple(t.shape), torch.float32, dev, (lead + 2 + j) % 4, BAND) for t in maps[k]] for j, k in enumerate(MAPS)}
    rc = lib.bxi_fcos_grad_rescale_f32(_fcos_levels(), n, B_IMGS, C, _grads_array(gin), gup.ptr(), _grads_array(gout), G.stream(dev))
    assert rc == 0, _lib.STATUS.get(rc, rc)
    outs = [t for k in MAPS for t in gout[k]]
    G.check_bands(gup, *outs)
    G.check_written(*outs)
    G.check_unchanged(gup)
    if not in_place:
        ins = [t for k in MAPS for t in gin[k]]
        G.check_bands(*ins)
        G.check_unchanged(*ins)
    for i, k in enumerate(MAPS):
        for got, src in zip(gout[k], maps[k]):
            assert G.same(got.t, src * up[i])
