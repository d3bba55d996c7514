"""GPU: the training targets of the SOLOv2-style heads and their category loss against the fixture made by the reference's own code
(tests/golden/solo_targets.npz) and against the restatement (tests/solo_ref.py).

Targets are integers: EQUAL, no tolerance.  ``loss_cate`` and its gradient: within 4x the reference's own float32-against-float64
difference recorded in the fixture (``tol_loss_cate``, ``tol_grad_cate``), against the float64 values."""
import numpy as np
import pytest
import torch

from tests import solo_ref as R

pytestmark = pytest.mark.gpu

SPEC = R.load_cases()
CASES = sorted(SPEC['cases'])


def _settings(mode):
    from boxinstseg_amd import parse_solo_head_cfg
    return parse_solo_head_cfg(R.head_cfg(SPEC, mode))


def _run(dev, name, mode, masks_on_host=False):
    import boxinstseg_amd as B
    case = SPEC['cases'][name]
    boxes, labels = R.gt_of(case, device=dev)
    if masks_on_host:
        class Host:                                                   # what the functions use of BitmapMasks
            def __init__(self, m):
                self.m = m

            def to_ndarray(self):
                return self.m
        masks = [Host(m) for m in R.masks_of(case)]
    else:
        masks = [torch.from_numpy(m).to(dev) for m in R.masks_of(case)]
    s = _settings(mode)
    if mode == 'discobox':
        return B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **s)
    return B.box_solov2_targets(boxes, labels, masks, [hw for _, hw in R.level_planes(SPEC, mode)], **s)


def _flat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()


def _check_against(tg, want, key=None, g=None):
    """Every target array of ``tg`` (SoloTargets) equals ``want`` (what tests/solo_ref.py:targets returns)."""
    assert np.array_equal(tg.flat_cate_labels.cpu().numpy(), want['cate_labels'])
    assert np.array_equal(_flat(tg.cate_labels), want['cate_labels'])
    assert np.array_equal(_flat(tg.ins_ind_labels).astype(np.uint8), want['ins_ind_labels']) and tg.ins_ind_labels[0].dtype == torch.bool
    assert np.array_equal(_flat(tg.cell_owner), want['cell_owner'])
    for l in range(len(tg.num_grids)):
        for b in range(tg.B):
            assert np.array_equal(tg.grid_order[l][b].cpu().numpy(), want['grid_order'][l][b]), (l, b)
            assert tg.counts[l][b] == [len(want['grid_order'][l][b]), len(want['sel_inst'][l][b])]
        assert np.array_equal(tg.pair_inst[l].cpu().numpy(), np.concatenate(want['pair_inst'][l])), l
        assert np.array_equal(tg.sel_inst[l].cpu().numpy(), np.concatenate(want['sel_inst'][l])), l
    assert np.array_equal(tg.moments.cpu().numpy(), want['moments'])
    assert tg.num_ins.cpu().tolist() == [want['num_ins']] and tg.status.cpu().tolist() == [0]


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', CASES)
def test_targets_equal_the_fixture(dev, name, mode):
    g = np.load(R.GOLDEN)
    tg = _run(dev, name, mode)
    key = f'{name}_{mode}'
    for k, got in (('cate_labels', tg.flat_cate_labels), ('ins_ind_labels', torch.cat(tg.ins_ind_labels).to(torch.uint8)),
                   ('cell_owner', torch.cat(tg.cell_owner))):
        assert np.array_equal(got.cpu().numpy(), g[f'{key}_{k}']), k
    assert np.array_equal(_flat([o for lv in tg.grid_order for o in lv]), g[f'{key}_grid_order'])
    assert np.array_equal(_flat(tg.pair_inst), g[f'{key}_pair_inst']) and np.array_equal(_flat(tg.sel_inst), g[f'{key}_sel_inst'])
    assert [[c[0] for c in lv] for lv in tg.counts] == g[f'{key}_pair_counts'].tolist()
    assert [[c[1] for c in lv] for lv in tg.counts] == g[f'{key}_set_counts'].tolist()
    assert tg.num_ins.cpu().tolist() == [int(g[f'{key}_num_ins'])] and tg.status.cpu().tolist() == [0]
    # the rescaled masks, the moments, and the planes in the reference's layout
    assert np.array_equal(tg.moments.cpu().numpy(), g[f'{name}_moments'])
    for f, m in tg.masks.items():
        assert m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), g[f'{name}_rescaled_f{f}']), f
    assert sorted(tg.masks) == ([4] if mode == 'discobox' else [4, 8, 16])
    for l, planes in enumerate(tg.ins_labels()):
        assert np.array_equal(planes.cpu().numpy(), g[f'{key}_ins_labels{l}']), l
    # kernel_label_list of the reference: the final label of every pair's cell
    for l, kl in enumerate(tg.kernel_labels()):
        S = SPEC['num_grids'][l]
        lab = tg.cate_labels[l].view(tg.B, S * S).cpu()
        assert torch.equal(kl.cpu(), torch.cat([lab[b][tg.grid_order[l][b].cpu()] for b in range(tg.B)]))


@pytest.mark.parametrize('mode', R.MODES)
def test_two_runs_are_bit_identical_and_host_masks_upload_once(dev, mode):
    a, b, c = _run(dev, 'mixed', mode), _run(dev, 'mixed', mode), _run(dev, 'mixed', mode, masks_on_host=True)
    for other in (b, c):
        assert torch.equal(a.flat_cate_labels, other.flat_cate_labels) and torch.equal(a.moments, other.moments)
        assert torch.equal(torch.cat(a.cell_owner), torch.cat(other.cell_owner)) and a.counts == other.counts
        for f in a.masks:
            assert torch.equal(a.masks[f], other.masks[f])
        for x, y in zip(a.pair_inst + a.sel_inst, other.pair_inst + other.sel_inst):
            assert torch.equal(x, y)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', CASES)
def test_cate_loss_and_gradient(dev, name, mode):
    import boxinstseg_amd as B
    g = np.load(R.GOLDEN)
    key = f'{name}_{mode}'
    tg = _run(dev, name, mode)
    s = _settings(mode)
    preds = [torch.from_numpy(g[f'in_cate{l}']).to(dev).requires_grad_(True) for l in range(len(SPEC['num_grids']))]
    loss = B.solo_cate_loss(preds, tg.flat_cate_labels, tg.num_ins, s['gamma'], s['alpha'], s['loss_weight_cate'])
    again = B.solo_cate_loss([p.detach() for p in preds], tg.cate_labels, tg.num_ins, s['gamma'], s['alpha'], s['loss_weight_cate'])
    assert loss.shape == () and loss.item() == again.item()                      # fixed-order sums: run-to-run identical
    want = float(g[f'{key}_loss64'])
    err = abs(loss.item() - want) / abs(want)
    print(f'{key}: loss {loss.item():.9g} vs {want:.9g}, relative {err:.3e} (allowed {4 * float(g["tol_loss_cate"]):.3e})')
    up = 0.375                                                                   # a non-unit upstream scalar
    (loss * up).backward()
    errs = []
    gmax = max(float(np.abs(g[f'{key}_grad_cate{l}']).max()) for l in range(len(preds)))
    for l, p in enumerate(preds):
        w = g[f'{key}_grad_cate{l}'] * up
        errs.append(float(np.abs(p.grad.cpu().numpy().astype(np.float64) - w).max()) / (gmax * up))
    print(f'{key}: gradient error {max(errs):.3e} (allowed {4 * float(g["tol_grad_cate"]):.3e})')
    assert err <= 4 * float(g['tol_loss_cate'])
    assert max(errs) <= 4 * float(g['tol_grad_cate'])


@pytest.mark.parametrize('mode', R.MODES)
def test_seventy_instances_against_the_restatement(dev, mode):
    """More instances than a wave has lanes, one image on a 128 x 160 canvas.  The moments stay below 2^24 because that is where the
    reference's own fp32 sums stop being exact, not because the library needs it: its moments are exact integers, rounded once.
    Masks whose sums leave 2^24 and 2^32 are checked under that rule, against closed forms, in part C of
    tests/test_gpu_solo_targets_edges.py, and moments no fp32 holds go through the assignment in its large-moment plant."""
    import boxinstseg_amd as B
    boxes, labels, masks = R.random_case(70, 70, 128, 160, 7)
    kw = dict(num_grids=[12, 10, 8, 6, 4], scale_ranges=[(1, 14), (7, 24), (12, 32), (20, 48), (32, 256)], sigma=0.2, num_classes=7)
    want = R.targets(mode, boxes, labels, masks, canvas=(128, 160), **kw)
    assert int(want['moments'].max()) < 2 ** 24 and want['num_ins'] > 64 and sum(len(o) for lv in want['grid_order'] for o in lv) > 70
    db, dl, dm = [b.to(dev) for b in boxes], [t.to(dev) for t in labels], [torch.from_numpy(m).to(dev) for m in masks]
    if mode == 'discobox':
        tg = B.solov2_targets(db, dl, dm, (32, 40), strides=[8, 8, 16, 32, 32], **kw)
    else:
        tg = B.box_solov2_targets(db, dl, dm, [(32, 40), (32, 40), (16, 20), (8, 10), (8, 10)], strides=[8, 8, 16, 32, 32], **kw)
    _check_against(tg, want)
    for f, m in tg.masks.items():
        assert np.array_equal(m.cpu().numpy(), R.rescale(masks[0], f)), f


def test_no_instances_is_all_background(dev):
    import boxinstseg_amd as B
    s = _settings('discobox')
    boxes = [torch.zeros(0, 4, device=dev)] * 2
    labels = [torch.zeros(0, dtype=torch.int64, device=dev)] * 2
    masks = [torch.zeros(0, 64, 96, dtype=torch.uint8, device=dev), torch.zeros(0, 32, 32, dtype=torch.uint8, device=dev)]
    tg = B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **s)
    assert tg.G == 0 and bool((tg.flat_cate_labels == SPEC['num_classes']).all()) and tg.num_ins.cpu().tolist() == [0]
    assert not bool(torch.cat(tg.ins_ind_labels).any()) and bool((torch.cat(tg.cell_owner) == -1).all())
    assert all(p.numel() == 0 for p in tg.pair_inst) and all(p.shape == (0, 16, 24) for p in tg.ins_labels()) and tg.masks[4].shape == (0, 16, 24)
    preds = [torch.from_numpy(p[:2]).to(dev) for p in R.make_cate_inputs(SPEC, 5)]
    loss = B.solo_cate_loss(preds, tg.flat_cate_labels, tg.num_ins, 2.0, 0.25, 1.0)
    want, _ = R.cate_loss([p.cpu().numpy() for p in preds], tg.flat_cate_labels.cpu().numpy(), 0, 2.0, 0.25, 1.0)
    assert abs(loss.item() - float(want)) <= 1e-5 * float(want)


def test_b_zero_is_a_no_op(dev):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    ia, pa = _lib.int_array, _lib.ptr_array
    st = torch.cuda.current_stream(dev).cuda_stream
    assert lib.bxi_solo_mask_pass_u8(pa([]), ia([0]), ia([]), ia([]), 0, ia([4]), ia([16]), ia([24]), 1, pa([0]), None, st) == 0
    assert lib.bxi_solo_assign_f32(0, 0, 5, ia(SPEC['num_grids']), _lib.float_array([0] * 10), 0.2, 5, 64, 96, *([None] * 3), ia([0]), *([None] * 9), st) == 0
    assert lib.bxi_solo_cate_loss_f32(pa([0] * 5), ia(SPEC['num_grids']), 5, 0, 5, None, None, 2.0, 0.25, 1.0, pa([0] * 5), None, None, 0, st) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', R.MODES)
def test_bad_label_sets_the_status_word(dev, mode):
    import boxinstseg_amd as B
    from boxinstseg_amd import _lib
    case = SPEC['cases']['mixed']
    boxes, labels = R.gt_of(case, device=dev)
    labels[0] = labels[0].clone()
    labels[0][4] = SPEC['num_classes']                                           # instance 4 hits levels 1 and 2
    masks = [torch.from_numpy(m).to(dev) for m in R.masks_of(case)]
    s = _settings(mode)
    if mode == 'discobox':
        tg = B.solov2_targets(boxes, labels, masks, SPEC['mask_feat_size'], **s)
    else:
        tg = B.box_solov2_targets(boxes, labels, masks, [hw for _, hw in R.level_planes(SPEC, mode)], **s)
    assert tg.status.cpu().tolist() == [_lib.SOLO_STATUS_BAD_LABEL]
    assert not any(4 in p.cpu().tolist() for p in tg.pair_inst) and not bool((torch.cat(tg.cell_owner) == 4).any())   # such an instance is skipped
    assert int(tg.flat_cate_labels.max()) == SPEC['num_classes'] and int(tg.flat_cate_labels.min()) >= 0
