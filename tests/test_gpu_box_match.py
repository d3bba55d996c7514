"""GPU: the Box2Mask target assignment (csrc/box_match.hip) against what the reference's own code computed
(tests/golden/box_match.npz, written by tests/golden/make_golden_box_match.py from the case table of tests/box_match_ref.py).

Tolerances
  cost          within 4 x ``tol`` of the reference's fp64 cost, ``tol`` = max |reference fp32 - reference fp64| of the case, measured by
                the generator and stored in the fixture (r4 2.9e-6, frac 5.0e-7, down 7.0e-7, wide 1.3e-7, batch 1.3e-6, coco 1.5e-6,
                crowd 1.7e-6, c65 1.7e-7).  The 64-problem batch is not stored: its tol is the same difference of the restatement
                (tests/box_match_ref.py) evaluated in fp32 and in fp64, measured by the test.
  projections   against the reference's fp64 projections.  The kernel forms the source coordinate in fp32 as ATen does, so the
                bilinear weights differ from the fp64 ones by at most 3 roundings of a number below max(h, w): 3 * 2^-24 * max(h, w);
                two weights act on differences of at most 2 max|x|, and the four-term value adds 4 roundings of at most max|x|:
                |d logit| <= 2^-24 max|x| (12 max(h, w) + 4).  The sigmoid has slope <= 1/4 and its fp32 evaluation (expf, add, divide)
                adds 4 * 2^-24.
  assignment    index for index: the generator rejects a seed unless every optimum is separated by more than 100 x tol.
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import box_match_ref as R
from tests.test_host_box_match import GOLDEN, N_RAND, N_TIES, limit_uniform_pinned

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
NAMES = sorted(R.CASES)


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(golden, name, dev):
    _, hw, HW, Q, counts, pset, C = R.CASES[name]
    images = R.load_case(golden, name)
    tens = [{k: _t(v, dev) for k, v in im.items()} for im in images]
    return images, tens, hw, HW, Q, counts, R.PARAMS[pset], C


def _assigner(prm):
    import boxinstseg_amd as B
    return B.MaskHungarianAssigner(cls_cost=dict(type='ClassificationCost', weight=prm['w_cls']),
                                   dice_cost=dict(type='BoxMatchingCost', weight=prm['w_dice'], pred_act=prm['pred_act'], eps=prm['eps']))


def proj_tol(logits, act):
    """The bound of the module docstring for one plane stack."""
    finite = np.abs(logits[np.isfinite(logits)])
    t = EPS32 * float(finite.max()) * (12 * max(logits.shape[-2:]) + 4)
    return 0.25 * t + 4 * EPS32 if act else t


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.parametrize('name', NAMES)
def test_projections_match_the_reference(dev, golden, name):
    from boxinstseg_amd import box_match as M
    images, tens, (h, w), (H, W), Q, counts, prm, _ = _case(golden, name, dev)
    for i, (im, tn) in enumerate(zip(images, tens)):
        k = f'{name}{i}'
        rows, cols, sumsq = (t.cpu().numpy() for t in M.project_pred(tn['logits'], (H, W), prm['pred_act']))
        want_r, want_c = golden[f'{k}_proj_rows64'], golden[f'{k}_proj_cols64']
        tol = proj_tol(im['logits'], prm['pred_act'])
        err = max(np.abs(rows - want_r).max(), np.abs(cols - want_c).max())
        print(f'{k}: projections max error {err:.3e} (bound {tol:.3e})')
        assert rows.shape == (Q, H) and cols.shape == (Q, W) and err <= tol
        for side, want in enumerate((want_r, want_c)):
            sq = (want ** 2).sum(1)
            bound = 2 * np.abs(want).max() * tol * want.shape[1] + 2 * EPS32 * sq
            assert (np.abs(sumsq[:, side] - sq) <= bound).all(), (k, side)
        # the ground truths: exact
        m = im['masks']
        for view in (tn['masks'], tn['masks'].bool(), tn['masks'].float() * 0.5):
            gr, gc, gs = (t.cpu().numpy() for t in M.project_gt(view))
            scale = 0.5 if view.dtype == torch.float32 else 1.0
            assert gr.shape == (counts[i], H) and gc.shape == (counts[i], W) and gs.shape == (counts[i], 2)
            if counts[i]:
                assert np.array_equal(gr, m.max(2) * scale) and np.array_equal(gc, m.max(1) * scale)
                assert np.array_equal(gs, np.stack([((m.max(2) * scale) ** 2).sum(1), ((m.max(1) * scale) ** 2).sum(1)], 1))
    if name == 'r4':        # the all-negative query: a maximum that started at 0 would give sigmoid(0) = 0.5
        assert rows[0].max() < 0.5 and cols[0].max() < 0.5
        assert np.allclose(rows[1], 1 / (1 + np.exp(-0.75)), rtol=0, atol=4 * EPS32) and np.allclose(cols[1], rows[1][0], rtol=0, atol=0)


def test_projection_nan_in_nan_out_and_same_size(dev, golden):
    from boxinstseg_amd import box_match as M
    images, tens, (h, w), (H, W), Q, counts, prm, _ = _case(golden, 'r4', dev)
    x = images[0]['logits'].copy()
    x[2, 5, 3] = np.nan                                   # an interior sample: its neighbours' rows and columns turn NaN, nothing else
    x[3] = np.nan
    want_r, want_c = R.pred_projections(x, H, W, True)
    assert 0 < np.isnan(want_r[2]).sum() < H and 0 < np.isnan(want_c[2]).sum() < W and np.isnan(want_r[3]).all()
    rows, cols, sumsq = (t.cpu().numpy() for t in M.project_pred(_t(x, dev), (H, W), True))
    tol = proj_tol(x, True)
    for got, want in ((rows, want_r), (cols, want_c)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.nanmax(np.abs(got - want)) <= tol
    assert np.isnan(sumsq[2]).all() and np.isnan(sumsq[3]).all() and np.isfinite(sumsq[[0, 1, 4]]).all()
    # predictions already at the target size (what the reference hands to its assigner): read as they are
    for act in (True, False):
        rows, cols, _ = (t.cpu().numpy() for t in M.project_pred(_t(x, dev), None, act))
        plain = 1.0 / (1.0 + np.exp(-x.astype(np.float64))) if act else x.astype(np.float64)       # no resampling: 0 * NaN never happens
        want_r, want_c = plain.max(axis=2), plain.max(axis=1)
        assert np.isnan(want_r[2]).sum() == 1 and np.isnan(want_c[2]).sum() == 1
        for got, want in ((rows, want_r), (cols, want_c)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.nanmax(np.abs(got - want)) <= (4 * EPS32 if act else 0.0)


@pytest.mark.parametrize('name', NAMES)
def test_cost_within_the_measured_tolerance(dev, golden, name):
    import boxinstseg_amd as B
    from boxinstseg_amd import box_match as M
    images, tens, (h, w), (H, W), Q, counts, prm, _ = _case(golden, name, dev)
    tol = float(golden[f'{name}_tol'])
    pred = M.project_pred(torch.cat([t['logits'] for t in tens]), (H, W), prm['pred_act'])
    gt = M._project_gt_list([t['masks'] for t in tens], H, W, dev)
    cost, status = M.match_cost(torch.cat([t['cls'] for t in tens]), torch.cat([t['labels'] for t in tens]), pred, gt, Q, counts,
                                prm['w_cls'], prm['w_dice'], prm['eps'])
    assert status.cpu().tolist() == [0] * len(counts) and cost.numel() == Q * sum(counts)
    cost, at = cost.cpu().numpy(), 0
    for i, G in enumerate(counts):
        k = f'{name}{i}'
        got = cost[at * Q:(at + G) * Q].reshape(Q, G)
        at += G
        if not G:
            continue
        err = float(np.abs(got - golden[f'{k}_cost64']).max())
        print(f'{k}: cost max error against the fp64 reference {err:.3e} (reference fp32: {tol:.3e}, bound {4 * tol:.3e})')
        assert err <= 4 * tol
        # the two classes on their own: the reference's [num_query, num_gt] tensors; their sum carries one more fp32 rounding of each
        tn = tens[i]
        c_cls = B.ClassificationCost(weight=prm['w_cls'])(tn['cls'], tn['labels'])
        dice = B.BoxMatchingCost(weight=prm['w_dice'], pred_act=prm['pred_act'], eps=prm['eps'])
        c_dice = dice(tn['logits'][:, None], tn['masks'][:, None], target_shape=(H, W))
        assert c_cls.shape == c_dice.shape == (Q, G)
        both = (c_cls.double() + c_dice.double()).cpu().numpy()
        assert np.abs(both - golden[f'{k}_cost64']).max() <= 4 * tol + 2 * EPS32 * np.abs(golden[f'{k}_cost64']).max()
        want_cls = R.class_cost(images[i]['cls'], images[i]['labels'], prm['w_cls'])
        assert np.abs(c_cls.cpu().numpy() - want_cls).max() <= prm['w_cls'] * (images[i]['cls'].shape[1] + 8) * EPS32
        if name in ('down', 'frac'):     # the four-dimensional inputs of match_cost.py:400-425, up-sampled by the caller
            up = F.interpolate(tn['logits'][:, None], (H, W), mode='bilinear', align_corners=False)
            c_up = dice(up, tn['masks'][:, None])
            assert c_up.shape == (Q, G) and np.abs((c_cls.double() + c_up.double()).cpu().numpy() - golden[f'{k}_cost64']).max() <= \
                4 * tol + 2 * EPS32 * np.abs(golden[f'{k}_cost64']).max()


@pytest.mark.parametrize('name', NAMES)
def test_assignment_equals_scipy(dev, golden, name):
    images, tens, (h, w), (H, W), Q, counts, prm, _ = _case(golden, name, dev)
    a = _assigner(prm)
    gt_inds, labels, pos, pos_gt, got_counts = a.assign_batch(torch.stack([t['cls'] for t in tens]), torch.stack([t['logits'] for t in tens]),
                                                              [t['labels'] for t in tens], [t['masks'] for t in tens])
    assert got_counts == list(counts) and gt_inds.shape == labels.shape == (len(counts), Q)
    assert [s.cpu().tolist() for s in a.last_status] == [[0] * len(counts)] * 2
    at = 0
    for i, G in enumerate(counts):
        k, npos = f'{name}{i}', min(Q, G)
        assert np.array_equal(gt_inds[i].cpu().numpy(), golden[f'{k}_gt_inds']), k
        assert np.array_equal(labels[i].cpu().numpy(), golden[f'{k}_assigned_labels']), k
        assert np.array_equal(pos[at:at + npos].cpu().numpy(), golden[f'{k}_rows']), k
        assert np.array_equal(pos_gt[at:at + npos].cpu().numpy(), golden[f'{k}_cols']), k
        at += npos
        # one image through assign(): at prediction size with target_shape, and up-sampled by the caller as the reference does
        tn = tens[i]
        res = a.assign(tn['cls'], tn['logits'], tn['labels'], tn['masks'], None, target_shape=(H, W))
        assert res.num_gts == G and res.max_overlaps is None
        assert np.array_equal(res.gt_inds.cpu().numpy(), golden[f'{k}_gt_inds']) and np.array_equal(res.labels.cpu().numpy(), golden[f'{k}_assigned_labels'])
        up = F.interpolate(tn['logits'][:, None], (H, W), mode='bilinear', align_corners=False)
        res = a.assign(tn['cls'], up, tn['labels'], tn['masks'][:, None], None)
        assert np.array_equal(res.gt_inds.cpu().numpy(), golden[f'{k}_gt_inds']) and np.array_equal(res.labels.cpu().numpy(), golden[f'{k}_assigned_labels'])
    assert at == pos.numel() == pos_gt.numel()


def test_solver_on_stored_random_matrices(dev, golden):
    """Unique optima: the indices are scipy's.  Every shape alone, and the two one-query matrices as one batch."""
    from boxinstseg_amd import box_match as M
    for n in range(N_RAND):
        c = golden[f'lsa_rand{n}_cost']
        Q, G = c.shape
        labels = torch.arange(G, device=dev) + 100
        gt_inds, lab, pos, pos_gt, status = M.linear_sum_assignment(_t(c, dev), labels, Q, [G])
        rows, cols = golden[f'lsa_rand{n}_rows'], golden[f'lsa_rand{n}_cols']
        assert status.cpu().tolist() == [0]
        assert np.array_equal(pos.cpu().numpy(), rows) and np.array_equal(pos_gt.cpu().numpy(), cols), (n, Q, G)
        want = np.zeros(Q, np.int64)
        want[rows] = cols + 1
        assert np.array_equal(gt_inds[0].cpu().numpy(), want) and np.array_equal(lab[0].cpu().numpy(), np.where(want > 0, want + 99, -1))
    a, b = golden['lsa_rand5_cost'], golden['lsa_rand6_cost']
    assert a.shape == (1, 1) and b.shape == (1, 4)
    flat = torch.cat([_t(a, dev).flatten(), _t(b, dev).flatten()])
    gt_inds, _, pos, pos_gt, _ = M.linear_sum_assignment(flat, torch.arange(5, device=dev), 1, [1, 4])
    assert pos.cpu().tolist() == [0, 0] and pos_gt.cpu().tolist() == [0, int(golden['lsa_rand6_cols'][0])]


def test_solver_on_stored_matrices_full_of_ties(dev, golden):
    """Many optimal assignments: a valid one-to-one matching of min(Q, G) pairs whose total is scipy's, exactly (small integers)."""
    from boxinstseg_amd import box_match as M
    for n in range(N_TIES):
        c = golden[f'lsa_ties{n}_cost']
        Q, G = c.shape
        gt_inds, _, pos, pos_gt, status = M.linear_sum_assignment(_t(c.astype(np.float32), dev), torch.zeros(G, dtype=torch.long, device=dev), Q, [G])
        pos, pos_gt = pos.cpu().numpy(), pos_gt.cpu().numpy()
        assert status.cpu().tolist() == [0] and R.is_matching(pos, pos_gt, Q, G) and (np.diff(pos) > 0).all(), n
        assert int(c[pos, pos_gt].astype(np.int64).sum()) == int(golden[f'lsa_ties{n}_total']), n
        assert np.array_equal(np.flatnonzero(gt_inds[0].cpu().numpy()), pos)


def _solve_timed(dev, c, labels, Q, counts, what):
    from boxinstseg_amd import box_match as M
    cost = _t(c, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = M.linear_sum_assignment(cost, labels, Q, counts)
    torch.cuda.synchronize()
    print(f'{what}: launch to completion {1e3 * (time.perf_counter() - t0):.1f} ms')            # printed, never asserted
    return out


@pytest.mark.parametrize('Q,G', [(1024, 1024), (1024, 8), (8, 1024)], ids=['square', 'tall', 'flat'])
def test_solver_at_the_limit_uniform(dev, golden, Q, G):
    """BXI_MATCH_MAX_SIDE on one or both sides (every LDS array at its full length, 16 trips of every lane loop): index for index the
    restatement's assignment, computed here because a 4 MB matrix is not stored.  The square matrix is pinned by the fixture's CRC32 of
    its bytes; when it is the generator's matrix the restatement is first held against scipy's stored indices."""
    c = R.limit_uniform(Q, G)
    labels = np.arange(G, dtype=np.int64) + 100
    want_gi, want_lab, want_pos, want_gt = R.assign(c.astype(np.float64), labels)
    if Q == G:
        _, pinned = limit_uniform_pinned(golden)
        print(f'the uniform matrix {"is" if pinned else "is NOT"} the one the fixture pins')
        if pinned:
            assert np.array_equal(want_gt, golden['lsa_limit_cols'])
    gt_inds, lab, pos, pos_gt, status = _solve_timed(dev, c, _t(labels, dev), Q, [G], f'uniform {Q}x{G}')
    assert status.cpu().tolist() == [0]
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(pos_gt.cpu().numpy(), want_gt)
    assert np.array_equal(gt_inds[0].cpu().numpy(), want_gi) and np.array_equal(lab[0].cpu().numpy(), want_lab)
    assert len(want_pos) == min(Q, G) and R.is_matching(want_pos, want_gt, Q, G)


def test_solver_at_the_limit_full_of_ties(dev, golden):
    """1024 x 1024 exact small integers with many optimal assignments: a one-to-one matching of all 1024 rows whose total is the
    restatement's (and scipy's stored one), as an integer."""
    c = R.limit_ties()
    Q, G = c.shape
    rows, cols = R.linear_sum_assignment(c)
    want = int(c[rows, cols].astype(np.int64).sum())
    assert want == int(golden['lsa_limit_ties_total'])
    gt_inds, _, pos, pos_gt, status = _solve_timed(dev, c, torch.zeros(G, dtype=torch.long, device=dev), Q, [G], f'ties {Q}x{G}')
    pos, pos_gt = pos.cpu().numpy(), pos_gt.cpu().numpy()
    assert status.cpu().tolist() == [0] and R.is_matching(pos, pos_gt, Q, G) and (np.diff(pos) > 0).all()
    assert int(c[pos, pos_gt].astype(np.int64).sum()) == want
    assert np.array_equal(np.flatnonzero(gt_inds[0].cpu().numpy()), pos)


def test_one_past_the_limit_is_refused_before_any_launch(dev):
    """Q = 1025, and G = 1025 in one problem of two: BXI_ERR_UNSUPPORTED, as the wrapper's exception; no output element is written,
    the status words and the other problem's rows included."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd import box_match as M
    side = _lib.MATCH_MAX_SIDE + 1
    assert side == R.LIMIT_SIDE + 1 == 1025
    for Q, counts in ((side, [2]), (4, [3, side])):
        total, npos = sum(counts), sum(min(Q, g) for g in counts)
        cost, labels = torch.rand(total * Q, device=dev), torch.zeros(total, dtype=torch.long, device=dev)
        with pytest.raises(_lib.BoxInstHipError, match='BXI_ERR_UNSUPPORTED') as e:
            M.linear_sum_assignment(cost, labels, Q, counts)
        assert e.value.status == _lib.BXI_ERR_UNSUPPORTED
        outs = [torch.full((len(counts), Q), -7, dtype=torch.int64, device=dev), torch.full((len(counts), Q), -7, dtype=torch.int64, device=dev),
                torch.full((npos,), -7, dtype=torch.int64, device=dev), torch.full((npos,), -7, dtype=torch.int64, device=dev),
                torch.full((len(counts),), -7, dtype=torch.int32, device=dev)]
        rc = _lib.load().bxi_linear_sum_assignment_f32(cost.data_ptr(), labels.data_ptr(), len(counts), Q, _lib.int_array(M._offsets(counts)),
                                                       *[t.data_ptr() for t in outs], torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert rc == _lib.BXI_ERR_UNSUPPORTED and all(bool((t == -7).all()) for t in outs)


BATCH_Q, BATCH_COUNTS = 9, [p % 12 for p in range(64)]             # BXI_MAX_IMAGES problems: empty ones, G < Q, G = Q and G > Q, mixed


def test_sixty_four_problems_in_one_solver_call(dev):
    """Every slot of first[] in the kernel arguments, the compacted-slot prefix summed over up to 63 earlier problems: problems 0..62
    equal the restatement of their own block index for index, at their prefix offsets; problem 63 carries a planted NaN and comes back
    all background.  One problem more is the documented shape error."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd import box_match as M
    Q, counts = BATCH_Q, BATCH_COUNTS
    assert len(counts) == _lib.BXI_MAX_IMAGES == 64 and counts[63] == 3 and {0, Q - 1, Q, Q + 1} <= set(counts)
    rng = np.random.default_rng(64)
    off = M._offsets(counts)
    cost = rng.uniform(0, 10, off[-1] * Q).astype(np.float32)
    labels = rng.integers(0, 9, off[-1]).astype(np.int64)
    cost[off[63] * Q + 5] = np.nan
    gt_inds, lab, pos, pos_gt, status = (t.cpu().numpy() for t in M.linear_sum_assignment(_t(cost, dev), _t(labels, dev), Q, counts))
    assert status.tolist() == [0] * 63 + [_lib.MATCH_STATUS_NONFINITE]
    slot = 0
    for p, G in enumerate(counts[:63]):
        block = cost[off[p] * Q:off[p + 1] * Q].reshape(Q, G).astype(np.float64)
        want_gi, want_lab, want_pos, want_gt = R.assign(block, labels[off[p]:off[p + 1]])
        npos = min(Q, G)
        assert len(want_pos) == npos
        assert np.array_equal(gt_inds[p], want_gi) and np.array_equal(lab[p], want_lab), p
        assert np.array_equal(pos[slot:slot + npos], want_pos) and np.array_equal(pos_gt[slot:slot + npos], want_gt), p
        slot += npos
    assert gt_inds[63].tolist() == [0] * Q and lab[63].tolist() == [-1] * Q
    assert slot + 3 == len(pos) == len(pos_gt) and pos[slot:].tolist() == [-1] * 3 and pos_gt[slot:].tolist() == [-1] * 3
    with pytest.raises(_lib.BoxInstHipError, match='BXI_ERR_BAD_SHAPE'):
        M.linear_sum_assignment(_t(np.append(cost[:off[63] * Q], np.zeros(4 * Q, np.float32)), dev), _t(np.append(labels[:off[63]], [0] * 4), dev),
                                Q, counts[:63] + [2, 2])


def test_sixty_four_problems_in_one_cost_call(dev):
    """The same 64 problems through match_cost, on projections built directly (H = W = 4): every block against bin_dice / class_cost in
    fp64 within 4 x the fp32-against-fp64 difference of the same restatement evaluated in fp32 on the same inputs (the rule of the
    stored cases, measured here instead of by the generator)."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd import box_match as M
    Q, counts, C, H, W = BATCH_Q, BATCH_COUNTS, 6, 4, 4
    P, off, prm = len(counts), M._offsets(counts), R.CFG
    rng = np.random.default_rng(65)
    cls = rng.normal(0, 1.5, (P * Q, C + 1)).astype(np.float32)
    labels = rng.integers(0, C, off[-1]).astype(np.int64)
    pr, pc = rng.uniform(0, 1, (P * Q, H)).astype(np.float32), rng.uniform(0, 1, (P * Q, W)).astype(np.float32)
    tr, tc = (rng.uniform(size=(off[-1], H)) < 0.6).astype(np.float32), (rng.uniform(size=(off[-1], W)) < 0.6).astype(np.float32)
    sq = lambda a, b: np.stack([(a.astype(np.float64) ** 2).sum(1), (b.astype(np.float64) ** 2).sum(1)], 1).astype(np.float32)   # noqa: E731
    cost, status = M.match_cost(_t(cls, dev), _t(labels, dev), tuple(_t(a, dev) for a in (pr, pc, sq(pr, pc))),
                                tuple(_t(a, dev) for a in (tr, tc, sq(tr, tc))), Q, counts, prm['w_cls'], prm['w_dice'], prm['eps'])
    assert status.cpu().tolist() == [0] * P and cost.numel() == Q * off[-1]
    cost = cost.cpu().numpy()

    def restated(p, dt):
        q, g = slice(p * Q, (p + 1) * Q), slice(off[p], off[p + 1])
        dice = R.bin_dice(pr[q].astype(dt), tr[g].astype(dt), prm['eps']) + R.bin_dice(pc[q].astype(dt), tc[g].astype(dt), prm['eps'])
        out = R.class_cost(cls[q], labels[g], prm['w_cls'], dt) + prm['w_dice'] * dice
        assert out.dtype == dt
        return out
    live = [p for p in range(P) if counts[p]]
    want = {p: restated(p, np.float64) for p in live}
    tol = max(float(np.abs(restated(p, np.float32) - want[p]).max()) for p in live)
    err = max(float(np.abs(cost[off[p] * Q:off[p + 1] * Q].reshape(Q, counts[p]) - want[p]).max()) for p in live)
    print(f'64 problems: cost max error against the fp64 restatement {err:.3e} (restatement in fp32: {tol:.3e}, bound {4 * tol:.3e})')
    assert tol > 0 and err <= 4 * tol
    with pytest.raises(_lib.BoxInstHipError, match='BXI_ERR_BAD_SHAPE'):
        M.match_cost(_t(cls, dev), _t(labels, dev), None, None, Q, counts + [0], prm['w_cls'], 0.0, prm['eps'])


def _stored_targets(golden, name, H, W):
    out = []
    for i, G in enumerate(R.CASES[name][4]):
        k = f'{name}{i}'
        npos = len(golden[f'{k}_t_pos_inds'])
        packed = golden[f'{k}_t_mask_targets']
        out.append(dict(labels=golden[f'{k}_t_labels'], label_weights=golden[f'{k}_t_label_weights'], mask_weights=golden[f'{k}_t_mask_weights'],
                        mask_targets=np.unpackbits(packed, axis=1)[:, :H * W].reshape(npos, 1, H, W) if npos else np.zeros((0, 1, H, W), np.uint8),
                        npos=npos))
    return out


def _check_targets(got, want, Q):
    labels, label_weights, mask_targets, mask_weights, num_pos, num_neg = got
    assert num_pos == sum(t['npos'] for t in want) and num_neg == Q * len(want) - num_pos
    for i, t in enumerate(want):
        assert labels[i].dtype == torch.int64 and np.array_equal(labels[i].cpu().numpy(), t['labels'])
        assert label_weights[i].dtype == torch.int64 and np.array_equal(label_weights[i].cpu().numpy(), t['label_weights'])
        assert mask_weights[i].dtype == torch.float32 and np.array_equal(mask_weights[i].cpu().numpy(), t['mask_weights'])
        assert tuple(mask_targets[i].shape) == t['mask_targets'].shape and np.array_equal(mask_targets[i].cpu().numpy(), t['mask_targets'])


def test_get_targets_batch_without_a_sync(dev, golden):
    """box2mask_get_targets on the three-problem batch against what _get_target_single returned, under sync_debug_mode('error')."""
    import boxinstseg_amd as B
    images, tens, (h, w), (H, W), Q, counts, prm, C = _case(golden, 'batch', dev)
    a = _assigner(prm)
    cls, logits = torch.stack([t['cls'] for t in tens]), torch.stack([t['logits'] for t in tens])
    labels, masks = [t['labels'] for t in tens], [t['masks'] for t in tens]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = B.box2mask_get_targets(cls, logits, labels, masks, a, C)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert isinstance(got[4], int) and isinstance(got[5], int)
    _check_targets(got, _stored_targets(golden, 'batch', H, W), Q)


def test_get_targets_never_holds_the_upsampled_predictions(dev):
    """Q * H * W floats of ONE image would be 26 MB here; the whole call stays below its inputs plus 4 MiB (the projection workspace
    of 200 planes, 0.6 MB, the projections, 0.4 MB, the gathered mask targets, 0.5 MB, and the allocator's rounding)."""
    import boxinstseg_amd as B
    B_, Q, h, H, C, counts = 2, 100, 64, 256, 7, (3, 5)
    gen = torch.Generator(device='cpu').manual_seed(5)
    logits = torch.randn(B_, Q, h, h, generator=gen).to(dev)
    cls = torch.randn(B_, Q, C + 1, generator=gen).to(dev)
    labels = [torch.randint(0, C, (g,), generator=gen).to(dev) for g in counts]
    masks = []
    for g in counts:
        m = torch.zeros(g, H, H, dtype=torch.uint8)
        for j in range(g):
            y, x = (int(v) for v in torch.randint(0, H - 40, (2,), generator=gen))
            m[j, y:y + 20 + 5 * j, x:x + 30] = 1
        masks.append(m.to(dev))
    a = _assigner(R.CFG)
    inputs = sum(t.numel() * t.element_size() for t in [logits, cls] + labels + masks)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = B.box2mask_get_targets(cls, logits, labels, masks, a, C)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    print(f'peak extra memory {extra / 2**20:.2f} MiB, inputs {inputs / 2**20:.2f} MiB, one up-sampled image {Q * H * H * 4 / 2**20:.1f} MiB')
    assert extra <= inputs + 4 * 2 ** 20 < Q * H * H * 4
    assert got[4] == 8 and got[5] == 192 and [int(w_.sum()) for w_ in got[3]] == [3, 5] and [tuple(m.shape) for m in got[2]] == [(3, 1, H, H), (5, 1, H, H)]
    assert a.last_status[1].cpu().tolist() == [0, 0]


def test_status_words_and_a_planted_nan(dev, golden):
    """A NaN in one problem's cost: that problem comes back all background with -1 in its slots and a non-zero status; the others are what
    they were.  A label outside the classes does the same through the cost's own status word, and nothing is read out of range."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd import box_match as M
    images, tens, (h, w), (H, W), Q, counts, prm, C = _case(golden, 'batch', dev)
    labels = torch.cat([t['labels'] for t in tens])
    cost = np.concatenate([golden[f'batch{i}_cost32'].ravel() for i in range(3)])
    clean = M.linear_sum_assignment(_t(cost, dev), labels, Q, counts)
    bad = cost.copy()
    bad[4 * Q + 9] = np.nan                                # inside problem 2 (problem 1 owns the first 4 * Q elements)
    for planted in (np.nan, np.inf, -np.inf):
        bad[4 * Q + 9] = planted
        gt_inds, lab, pos, pos_gt, status = M.linear_sum_assignment(_t(bad, dev), labels, Q, counts)
        assert status.cpu().tolist() == [0, 0, _lib.MATCH_STATUS_NONFINITE]
        assert torch.equal(gt_inds[:2], clean[0][:2]) and torch.equal(lab[:2], clean[1][:2])
        assert torch.equal(pos[:4], clean[2][:4]) and torch.equal(pos_gt[:4], clean[3][:4])
        assert gt_inds[2].cpu().tolist() == [0] * Q and lab[2].cpu().tolist() == [-1] * Q
        assert pos[4:].cpu().tolist() == [-1] * 7 and pos_gt[4:].cpu().tolist() == [-1] * 7
    assert np.array_equal(clean[0][2].cpu().numpy(), golden['batch2_gt_inds']) and clean[4].cpu().tolist() == [0, 0, 0]
    # a label outside [0, C + 1) in problem 1
    wrong = labels.clone()
    wrong[1] = C + 1
    pred = M.project_pred(torch.cat([t['logits'] for t in tens]), (H, W), prm['pred_act'])
    gt = M._project_gt_list([t['masks'] for t in tens], H, W, dev)
    c, status = M.match_cost(torch.cat([t['cls'] for t in tens]), wrong, pred, gt, Q, counts, prm['w_cls'], prm['w_dice'], prm['eps'])
    assert status.cpu().tolist() == [0, _lib.MATCH_STATUS_BAD_LABEL, 0]
    block = c[:4 * Q].view(Q, 4).cpu().numpy()
    assert np.isnan(block[:, 1]).all() and np.isfinite(np.delete(block, 1, axis=1)).all() and np.isfinite(c[4 * Q:].cpu().numpy()).all()
    gt_inds, _, _, _, status = M.linear_sum_assignment(c, wrong, Q, counts)
    assert status.cpu().tolist() == [0, _lib.MATCH_STATUS_NONFINITE, 0] and gt_inds[1].cpu().tolist() == [0] * Q
    assert np.array_equal(gt_inds[2].cpu().numpy(), golden['batch2_gt_inds'])


def test_launches_are_bit_identical_from_run_to_run(dev, golden):
    from boxinstseg_amd import box_match as M
    images, tens, (h, w), (H, W), Q, counts, prm, _ = _case(golden, 'r4', dev)
    tn = tens[0]

    def run():
        pred = M.project_pred(tn['logits'], (H, W), prm['pred_act'])
        gt = M.project_gt(tn['masks'])
        cost, _ = M.match_cost(tn['cls'], tn['labels'], pred, gt, Q, counts, prm['w_cls'], prm['w_dice'], prm['eps'])
        return list(pred) + list(gt) + [cost] + list(M.linear_sum_assignment(cost, tn['labels'], Q, counts))
    first = run()
    for _ in range(3):
        for a, b in zip(first, run()):
            assert torch.equal(_bits(a), _bits(b))


def test_graph_capture_of_the_whole_builder(dev, golden):
    """One stream, a linear chain: capture box2mask_get_targets, replay it on the stored batch, then on the same batch with its queries
    permuted -- the assignment (a separated optimum) moves with the queries."""
    import boxinstseg_amd as B
    images, tens, (h, w), (H, W), Q, counts, prm, C = _case(golden, 'batch', dev)
    a = _assigner(prm)
    cls0, logits0 = torch.stack([t['cls'] for t in tens]), torch.stack([t['logits'] for t in tens])
    cls, logits = torch.zeros_like(cls0), torch.zeros_like(logits0)
    labels, masks = [t['labels'] for t in tens], [t['masks'] for t in tens]

    def step():
        return B.box2mask_get_targets(cls, logits, labels, masks, a, C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    want = _stored_targets(golden, 'batch', H, W)
    cls.copy_(cls0)
    logits.copy_(logits0)
    graph.replay()
    torch.cuda.synchronize()
    _check_targets(out, want, Q)
    perm = torch.randperm(Q, generator=torch.Generator().manual_seed(3)).to(dev)
    cls.copy_(cls0[:, perm])
    logits.copy_(logits0[:, perm])
    graph.replay()
    torch.cuda.synchronize()
    p = perm.cpu().numpy()
    for i, t in enumerate(want):
        assert np.array_equal(out[0][i].cpu().numpy(), t['labels'][p]) and np.array_equal(out[3][i].cpu().numpy(), t['mask_weights'][p])
        assert int(out[3][i].sum()) == t['npos']
