"""GPU: the box head's training step (csrc/fcos_loss.hip) against what the reference's own code computed (tests/golden/box_head_loss.npz)
and against the restatement tests/fcos_ref.py.

Targets take no tolerance: they are bit-equal to the reference's float32 run.  Losses and gradients are compared with the reference's
float64 run, within 4x the float32-vs-float64 difference the generator measured on the reference itself (the `tol_*` keys)."""
import functools

import numpy as np
import pytest
import torch

from tests import fcos_ref as R

pytestmark = pytest.mark.gpu

SPEC = R.load_cases()
MAPS = ('cls', 'bbox', 'ctr')
CASES = sorted(SPEC['cases'])


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(R.GOLDEN)
    return {k: g[k] for k in g.files}


def tol(k):
    return 4.0 * float(golden()[k])


def settings(name, **over):
    from boxinstseg_amd import parse_box_head_cfg
    cfg = R.head_cfg(SPEC, name)
    cfg.update(over)
    return parse_box_head_cfg(cfg)


def maps_np(B=2):
    g = golden()
    m = {k: [g[f'in_{k}{lv}'] for lv in range(len(SPEC['levels']))] for k in MAPS}
    if B == 1:
        return {k: [a[:1] for a in v] for k, v in m.items()}
    if B == 3:
        return {k: [np.concatenate([a, a[:1]]) for a in v] for k, v in m.items()}
    return m


def on(dev, maps, grad=False):
    return {k: [torch.as_tensor(a).to(dev).clone().requires_grad_(grad) for a in v] for k, v in maps.items()}


def lib_targets(dev, s, boxes, labels, sizes=None, strides=None):
    import boxinstseg_amd as B
    return B.condinst_box_targets(SPEC['levels'] if sizes is None else sizes, s['strides'] if strides is None else strides,
                                  [b.to(dev) for b in boxes], [t.to(dev) for t in labels], regress_ranges=s['regress_ranges'],
                                  center_sampling=s['center_sampling'], center_sample_radius=s['center_sample_radius'],
                                  norm_on_bbox=s['norm_on_bbox'], num_classes=s['num_classes'], B=len(boxes))


def ref_targets(s, boxes, labels, dtype=torch.float32, sizes=None, strides=None):
    return R.targets(SPEC['levels'] if sizes is None else sizes, s['strides'] if strides is None else strides, [b.to(dtype) for b in boxes], labels,
                     s['regress_ranges'], s['center_sampling'], s['center_sample_radius'], s['norm_on_bbox'], s['num_classes'], dtype)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), torch.as_tensor(b).contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def assert_targets_equal(tg, want, stats64):
    for k in R.TARGET_KEYS:
        assert same_bits(getattr(tg, k), want[k]), k
    stats = tg.stats.cpu().double().numpy()
    print('stats', stats, 'want', stats64)
    assert stats[0] == stats64[0]
    assert abs(stats[1] - stats64[1]) <= tol('tol_stats') * abs(stats64[1])
    assert tg.status.cpu().tolist() == [0]


def run_loss(dev, m_np, boxes, labels, s, upstream=(1.0, 1.0, 1.0)):
    """The library's losses [3] and the gradients of sum(upstream * loss) w.r.t. every map."""
    import boxinstseg_amd as B
    m = on(dev, m_np, grad=True)
    out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], [b.to(dev) for b in boxes], [t.to(dev) for t in labels], None, s)
    losses = out[0]
    total = upstream[0] * losses['loss_cls'] + upstream[1] * losses['loss_bbox'] + upstream[2] * losses['loss_centerness']
    total.backward()
    vals = torch.stack([losses['loss_cls'], losses['loss_bbox'], losses['loss_centerness']]).detach()
    return vals, {k: [t.grad for t in m[k]] for k in MAPS}, out[1:]


def assert_close(vals, grads, want_losses, want_grads, what='', bbox_scale=None):
    """want_*: float64.  Losses relative, each gradient kind relative to its largest float64 element over the levels (``bbox_scale``: the
    size to take for the distance gradients instead, where the true gradient is zero by symmetry)."""
    got = vals.cpu().double().numpy()
    want_losses = np.asarray(want_losses, np.float64)
    err = np.abs(got - want_losses)
    print(what, 'losses', got, 'want', want_losses, 'rel err', err / np.maximum(np.abs(want_losses), 1e-300), 'allowed', tol('tol_losses'))
    assert np.isfinite(got).all()
    assert (err <= tol('tol_losses') * np.abs(want_losses)).all(), (got, want_losses)
    for k in MAPS:
        scale = max(float(np.abs(np.asarray(w)).max()) for w in want_grads[k])
        if k == 'bbox' and bbox_scale is not None:
            scale = bbox_scale
        worst = max(float(np.abs(g.cpu().double().numpy() - np.asarray(w)).max()) for g, w in zip(grads[k], want_grads[k]))
        print(what, f'grad_{k}: max err {worst:.3e}, max |g64| {scale:.3e}, rel {worst / max(scale, 1e-300):.3e}, allowed {tol("tol_grad_" + k):.3e}')
        assert all(bool(torch.isfinite(g).all()) for g in grads[k])
        assert worst <= tol('tol_grad_' + k) * scale, k


def restated(m_np, boxes, labels, s):
    """The restatement in float64 (targets in float64 as well): losses [3] and gradients per kind."""
    tg = ref_targets(s, boxes, labels, torch.float64)
    vals, gc, gb, gn = R.losses_and_grads(m_np, tg, s, torch.float64)
    return vals.numpy(), {'cls': [g.numpy() for g in gc], 'bbox': [g.numpy() for g in gb], 'ctr': [g.numpy() for g in gn]}


# ---- targets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_targets_are_bit_equal_to_the_reference(dev, name):
    g = golden()
    boxes, labels = R.gt_of(SPEC)
    tg = lib_targets(dev, settings(name), boxes, labels)
    assert_targets_equal(tg, {k: g[f'{name}_{k}'] for k in R.TARGET_KEYS}, g[f'{name}_stats64'])


def test_equal_area_tie_goes_to_the_lower_index(dev):
    boxes, labels = R.gt_of(SPEC)
    tg = lib_targets(dev, settings('cs_norm_giou'), boxes, labels)
    img1 = tg.gt_inds[tg.img_inds == 1].cpu()
    assert int((img1 >= 0).sum()) == SPEC['positives_image1'] and set(img1[img1 >= 0].tolist()) == {5}
    # swapped, the other box is the lower index and wins the same locations
    swapped = [boxes[0], boxes[1].flip(0)]
    tg2 = lib_targets(dev, settings('cs_norm_giou'), swapped, labels)
    assert torch.equal(tg2.gt_inds, tg.gt_inds) and torch.equal(tg2.labels, tg.labels)
    assert not torch.equal(tg2.bbox_targets, tg.bbox_targets)
    want = ref_targets(settings('cs_norm_giou'), swapped, labels)
    for k in R.TARGET_KEYS:
        assert same_bits(getattr(tg2, k), want[k]), k


@pytest.mark.parametrize('arrangement', ['winner_in_last_chunk', 'tie_across_the_boundary'])
def test_more_boxes_than_one_chunk(dev, arrangement):
    from boxinstseg_amd import box_head_loss
    n = box_head_loss.GT_CHUNK + 1
    b = np.tile(np.array([[0, 0, 160, 96]], np.float32), (n, 1))
    if arrangement == 'winner_in_last_chunk':
        b[n - 1] = [1, 1, 159, 95]
        winner = n - 1
    else:
        b[n - 2], b[n - 1] = [2, 1, 158, 95], [3, 1, 159, 95]               # equal areas, one on either side of the chunk boundary
        winner = n - 2
    boxes, labels = [torch.from_numpy(b)], [torch.arange(n) % 5]
    s = dict(settings('box_pix_ioulog'), regress_ranges=((-1.0, 1e8),), strides=[32])
    tg = lib_targets(dev, s, boxes, labels, sizes=[(3, 5)], strides=[32])
    want = ref_targets(s, boxes, labels, sizes=[(3, 5)], strides=[32])
    assert want['gt_inds'].tolist() == [winner] * 15
    for k in R.TARGET_KEYS:
        assert same_bits(getattr(tg, k), want[k]), k
    assert tg.stats.cpu().tolist()[0] == 15.0 and tg.status.cpu().tolist() == [0]


@pytest.mark.parametrize('batch', ['empty_image_in_the_middle', 'no_boxes_at_all', 'one_image'])
def test_images_without_boxes(dev, batch):
    boxes, labels = R.gt_of(SPEC)
    none_b, none_l = torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64)
    if batch == 'empty_image_in_the_middle':
        boxes, labels, B = [boxes[0], none_b, boxes[1]], [labels[0], none_l, labels[1]], 3
    elif batch == 'no_boxes_at_all':
        boxes, labels, B = [none_b, none_b], [none_l, none_l], 2
    else:
        boxes, labels, B = boxes[:1], labels[:1], 1
    s = settings('cs_norm_giou')
    m = maps_np(B)
    tg = lib_targets(dev, s, boxes, labels)
    want = ref_targets(s, boxes, labels)
    assert_targets_equal(tg, want, ref_targets(s, boxes, labels, torch.float64)['stats'].numpy())
    vals, grads, _ = run_loss(dev, m, boxes, labels, s)
    want_l, want_g = restated(m, boxes, labels, s)
    if batch == 'no_boxes_at_all':
        assert vals[1].item() == 0.0 and vals[2].item() == 0.0 and want_l[1] == 0.0 and want_l[2] == 0.0
        assert all(bool((g == 0).all()) for k in ('bbox', 'ctr') for g in grads[k])
        assert tg.stats.cpu().tolist() == [0.0, 0.0] and bool((tg.labels == 5).all()) and bool((tg.gt_inds == -1).all())
        assert bool((tg.bbox_targets == 0).all())
    if batch == 'empty_image_in_the_middle':
        mid = tg.img_inds == 1
        assert bool((tg.labels[mid] == 5).all()) and bool((tg.gt_inds[mid] == -1).all()) and bool((tg.bbox_targets[mid] == 0).all())
        assert all(bool((g[1] == 0).all()) for k in ('bbox', 'ctr') for g in grads[k])
        last = tg.gt_inds[(tg.img_inds == 2) & (tg.gt_inds >= 0)]
        assert set(last.cpu().tolist()) == {5}              # image 2's boxes follow image 0's five: indices 5 and 6, the tie goes to 5
    assert_close(vals, grads, want_l, want_g, batch)


# ---- losses and gradients -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_losses_and_gradients_match_the_reference(dev, name):
    g = golden()
    boxes, labels = R.gt_of(SPEC)
    vals, grads, rest = run_loss(dev, maps_np(), boxes, labels, R.head_cfg(SPEC, name))
    want_g = {k: [g[f'{name}_grad_{k}{lv}'] for lv in range(len(SPEC['levels']))] for k in MAPS}
    assert_close(vals, grads, g[f'{name}_losses64'], want_g, name)
    for got, key in zip(rest, ('points', 'level_inds', 'img_inds', 'gt_inds')):
        assert same_bits(got, g[f'{name}_{key}']), key


@pytest.mark.parametrize('mode', ['linear', 'square'])
@pytest.mark.parametrize('norm_on_bbox', [True, False])
def test_iou_linear_and_square(dev, mode, norm_on_bbox):
    boxes, labels = R.gt_of(SPEC)
    s = settings('box_norm_ioulog', loss_bbox=dict(type='IoULoss', mode=mode, loss_weight=1.5), norm_on_bbox=norm_on_bbox)
    assert s['bbox_loss_kind'] == 'iou_' + mode
    vals, grads, _ = run_loss(dev, maps_np(), boxes, labels, s)
    assert_close(vals, grads, *restated(maps_np(), boxes, labels, s), what=mode)


def _maps_from_targets(tg, m_np, dev):
    """bbox maps that predict exactly the target on every location."""
    out, at = [], 0
    for (h, w) in SPEC['levels']:
        n = 2 * h * w
        out.append(tg.bbox_targets[at:at + n].view(2, h * w, 4).permute(0, 2, 1).reshape(2, 4, h, w).contiguous().cpu().numpy())
        at += n
    return dict(m_np, bbox=out)


@pytest.mark.parametrize('name', ['cs_norm_giou', 'box_pix_ioulog'])
@pytest.mark.parametrize('planted', ['all_distances_zero', 'prediction_equals_target'])
def test_planted_edges(dev, name, planted):
    boxes, labels = R.gt_of(SPEC)
    s = settings(name)
    m = maps_np()
    if planted == 'all_distances_zero':
        m = dict(m, bbox=[np.zeros_like(a) for a in m['bbox']])
    else:
        m = _maps_from_targets(lib_targets(dev, s, boxes, labels), m, dev)
    vals, grads, _ = run_loss(dev, m, boxes, labels, s)
    # the float32 targets, so that prediction and target are the same numbers in the restatement too (ties on all four edges)
    tg = ref_targets(s, boxes, labels, torch.float32)
    want_l, gc, gb, gn = R.losses_and_grads(m, tg, s, torch.float64)
    want_g = {'cls': [t.numpy() for t in gc], 'bbox': [t.numpy() for t in gb], 'ctr': [t.numpy() for t in gn]}
    bbox_scale = None
    if planted == 'prediction_equals_target':
        assert want_l[1].item() == 0.0 and vals[1].item() == 0.0                 # IoU = GIoU = 1
        # Every edge is tied, so every min / max hands half of its gradient to the prediction, and the halves of the overlap, the union
        # and the enclosing box cancel: the true gradient is zero, and what float64 autograd leaves is its own rounding.  Each half
        # carries the rounding error of a one-sided derivative, so the error is bounded relative to THAT size: the largest gradient
        # of the same positives with every predicted distance a quarter larger (no edge tied, the outer side of all four).
        one_sided = dict(m, bbox=[a * 1.25 for a in m['bbox']])
        bbox_scale = max(float(t.abs().max()) for t in R.losses_and_grads(one_sided, tg, s, torch.float64)[2])
        assert bbox_scale > 0 and max(float(np.abs(t).max()) for t in want_g['bbox']) <= 1e-12 * bbox_scale
    else:
        assert np.isfinite(want_l.numpy()).all() and want_l[1].item() > 0
    assert_close(vals, grads, want_l.numpy(), want_g, planted, bbox_scale)


def test_upstream_gradients_scale_the_three_parts(dev):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC)
    cfg = R.head_cfg(SPEC, 'cs_norm_giou')
    _, unit, _ = run_loss(dev, maps_np(), boxes, labels, cfg)
    up = (0.5, 3.0, 512.0)
    m = on(dev, maps_np(), grad=True)
    out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], [b.to(dev) for b in boxes], [t.to(dev) for t in labels], None, cfg)[0]
    total = up[0] * out['loss_cls'] + up[1] * out['loss_bbox'] + up[2] * out['loss_centerness']
    flat = m['cls'] + m['bbox'] + m['ctr']
    first = torch.autograd.grad(total, flat, retain_graph=True)
    second = torch.autograd.grad(total, flat)
    n = len(SPEC['levels'])
    for i, k in enumerate(MAPS):
        for lv in range(n):
            want = unit[k][lv] * up[i]                                            # powers of two and 3: one rounding at the most
            assert torch.allclose(first[i * n + lv], want, rtol=2e-7, atol=0), (k, lv)
            assert same_bits(second[i * n + lv], first[i * n + lv].cpu()), (k, lv)
    # one loss alone leaves the other maps' gradients at zero
    m = on(dev, maps_np(), grad=True)
    out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], [b.to(dev) for b in boxes], [t.to(dev) for t in labels], None, cfg)[0]
    out['loss_bbox'].backward()
    assert all(bool((t.grad == 0).all()) for t in m['cls'] + m['ctr']) and any(bool((t.grad != 0).any()) for t in m['bbox'])
    assert all(same_bits(t.grad, u.cpu()) for t, u in zip(m['bbox'], unit['bbox']))


def test_half_precision_maps_are_taken_as_float(dev):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC)
    cfg = R.head_cfg(SPEC, 'cs_norm_giou')
    half = {k: [torch.as_tensor(a).to(dev).half().requires_grad_(True) for a in v] for k, v in maps_np().items()}
    out = B.condinst_box_loss(half['cls'], half['bbox'], half['ctr'], [b.to(dev) for b in boxes], [t.to(dev) for t in labels], None, cfg)[0]
    (out['loss_cls'] + out['loss_bbox'] + out['loss_centerness']).backward()
    as_float = {k: [t.detach().float().cpu().numpy() for t in v] for k, v in half.items()}
    vals, grads, _ = run_loss(dev, as_float, boxes, labels, cfg)
    assert same_bits(torch.stack([out['loss_cls'], out['loss_bbox'], out['loss_centerness']]), vals.cpu())
    for k in MAPS:
        for h, g in zip(half[k], grads[k]):
            assert h.grad.dtype == torch.float16 and torch.equal(h.grad, g.half())


def test_run_to_run_bit_identity(dev):
    boxes, labels = R.gt_of(SPEC)
    runs = [run_loss(dev, maps_np(), boxes, labels, R.head_cfg(SPEC, 'box_pix_ioulog'), (0.5, 3.0, 512.0)) for _ in range(3)]
    for vals, grads, _ in runs[1:]:
        assert same_bits(vals, runs[0][0].cpu())
        for k in MAPS:
            assert all(same_bits(a, b.cpu()) for a, b in zip(grads[k], runs[0][1][k]))


def test_no_host_synchronisation(dev):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC)
    cfg = settings('cs_norm_giou')
    m = on(dev, maps_np(), grad=True)
    gb, gl = [b.to(dev) for b in boxes], [t.to(dev) for t in labels]
    want, _, _ = run_loss(dev, maps_np(), boxes, labels, cfg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], gb, gl, None, cfg)
        (out[0]['loss_cls'] + out[0]['loss_bbox'] + out[0]['loss_centerness']).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert same_bits(torch.stack([out[0]['loss_cls'], out[0]['loss_bbox'], out[0]['loss_centerness']]), want.cpu())


def test_captured_graph_follows_its_inputs(dev):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC)
    cfg = settings('cs_norm_giou')
    m = on(dev, maps_np())
    gb, gl = [b.to(dev) for b in boxes], [t.to(dev) for t in labels]
    flat = m['cls'] + m['bbox'] + m['ctr']
    for t in flat:
        t.requires_grad_(True)

    def step():
        out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], gb, gl, None, cfg)
        total = out[0]['loss_cls'] + out[0]['loss_bbox'] + out[0]['loss_centerness']
        return torch.stack(list(out[0].values())).detach(), torch.autograd.grad(total, flat), out[4]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vals, grads, gt_inds = step()
    # new predictions and new boxes, in place
    with torch.no_grad():
        for t in flat:
            t.mul_(0.75).add_(0.125)
        gb[0][1] += torch.tensor([4.0, -2.0, 6.0, 3.0], device=dev)
        gb[1].copy_(gb[1].flip(0))
    graph.replay()
    torch.cuda.synchronize()
    new_np = {k: [t.detach().cpu().numpy() for t in m[k]] for k in MAPS}
    new_boxes = [b.cpu() for b in gb]
    want_v, want_g, rest = run_loss(dev, new_np, new_boxes, labels, cfg)
    assert same_bits(vals, want_v.cpu()) and torch.equal(gt_inds, rest[3])
    n = len(SPEC['levels'])
    for i, k in enumerate(MAPS):
        assert all(same_bits(grads[i * n + lv], want_g[k][lv].cpu()) for lv in range(n)), k
    old_v, _, _ = run_loss(dev, maps_np(), boxes, labels, cfg)
    assert not same_bits(vals, old_v.cpu())


def test_out_of_range_label_sets_the_status_word(dev):
    from boxinstseg_amd import _lib
    boxes, labels = R.gt_of(SPEC)
    bad = [labels[0].clone(), labels[1]]
    bad[0][2] = 5                                                               # num_classes itself; the big box of image 0
    s = settings('cs_norm_giou')
    tg = lib_targets(dev, s, boxes, bad)
    assert tg.status.cpu().tolist() == [_lib.FCOS_STATUS_BAD_LABEL]
    good = lib_targets(dev, s, boxes, labels)
    lost = good.gt_inds == 2
    assert int(lost.sum()) > 0
    assert bool((tg.labels[lost] == 5).all()) and bool((tg.gt_inds[lost] == -1).all()) and bool((tg.ctr_targets[lost] == 0).all())
    assert torch.equal(tg.labels[~lost], good.labels[~lost]) and torch.equal(tg.gt_inds[~lost], good.gt_inds[~lost])
    assert tg.stats.cpu().tolist()[0] == good.stats.cpu().tolist()[0] - int(lost.sum())
    for t in (tg.bbox_targets, tg.ctr_targets, tg.points, tg.stats):
        assert bool(torch.isfinite(t).all())
    bad[0][2] = -3
    assert lib_targets(dev, s, boxes, bad).status.cpu().tolist() == [_lib.FCOS_STATUS_BAD_LABEL]
    vals, grads, _ = run_loss(dev, maps_np(), boxes, bad, s)
    assert bool(torch.isfinite(vals).all()) and all(bool(torch.isfinite(g).all()) for k in MAPS for g in grads[k])


def test_outputs_feed_training_sample(dev):
    import boxinstseg_amd as B
    boxes, labels = R.gt_of(SPEC)
    cfg = settings('cs_norm_giou')
    m = on(dev, maps_np())
    rng = np.random.default_rng(5)
    params = [torch.from_numpy(rng.standard_normal((2, 7, h, w)).astype(np.float32)).to(dev) for h, w in SPEC['levels']]
    head = B.CondInstMaskHead(in_channels=16, boxinst_enabled=True, topk_per_img=6, max_proposals=-1).to(dev)
    out = B.condinst_box_loss(m['cls'], m['bbox'], m['ctr'], [b.to(dev) for b in boxes], [t.to(dev) for t in labels], None, cfg)
    got = head.training_sample(m['cls'], m['ctr'], params, *out[1:])
    want_t = ref_targets(cfg, boxes, labels)
    want = head.training_sample(m['cls'], m['ctr'], params, *(want_t[k].to(dev) for k in ('points', 'level_inds', 'img_inds', 'gt_inds')))
    assert got[0].shape[0] > 0 and len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
