"""CPU: every case of tests/corr_edges.py is what it claims to be.  No kernel runs here: each figure below comes from the restatement
(tests/corr_ref.py) or from plain arithmetic on the case's inputs, and is printed before it is asserted.

The conditions under which the GPU test may compare arg-maxes and retrieved slots exactly (``E.assert_conditions``: no row of a running
plane of C is a near tie, no score lies near its threshold) are asserted for every fused case, with no row left out; so are the counts,
``num_ins`` and ``ret_src`` lists that the docstrings state; the bounds that the GPU test derives from the restatement are printed."""
import numpy as np
import pytest
import torch

from tests import corr_edges as E
from tests import corr_ref as R

CHUNK, GROUPS, PLAN_THREADS, COMPACT_BLOCK, PASTE_TILE, RETRIEVE_WAVES = 16, 5, 256, 64, 4096, 4       # csrc/corr.hip


def test_kernel_constants_are_the_source():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'boxinstseg_amd', 'csrc', 'corr.hip')) as fh:
        code = fh.read()
    assert int(re.search(r'constexpr int kChunk = (\d+)', code).group(1)) == CHUNK
    assert int(re.search(r'constexpr int kPasteTile = (\d+)', code).group(1)) == PASTE_TILE
    assert 'ch += 5' in code and 'dpart[5]' in code and 'blockIdx.y * 4 + wave' in code
    assert re.search(r'__launch_bounds__\(256\) void corr_plan_kernel', code) and re.search(r'__launch_bounds__\(64\) void corr_compact_kernel', code)
    with open(os.path.join(root, 'include', 'boxinst', 'boxinst_hip_corr.h')) as fh:
        assert int(re.search(r'#define BXI_CORR_MAX_OBJS (\d+)', fh.read()).group(1)) == 8 == E.case('queue100')['cfg']['max_retrieval_objs']


@pytest.mark.parametrize('name', E.FUSED + ('labels', 'labels_removed'))
def test_conditions_hold(name):
    E.assert_conditions(name)
    c, w = E.case(name), E.want(name)
    K = c['cfg']['max_retrieval_objs']
    assert 1 <= c['cfg']['min_objs'] <= K <= 8 and w['ret_slot'].shape[1] == K
    for k, v in c['inp'].items():
        if v.dtype == np.float32:
            assert np.array_equal(R.half(v), v), k                               # float16 holds every input
    ran = [i for i, n in enumerate(w['count'].tolist()) if n >= c['cfg']['min_objs']]
    assert w['num_ins'] == len(ran) and all(bool((w['assign'][i, :int(w['count'][i])] >= 0).all()) for i in ran)


def test_the_recorded_sources_are_the_fixtures():
    """``ret_src`` of the restatement (the shadow table) against the census that the fixture recorded for 'in_call'."""
    g, spec = np.load(R.GOLDEN), R.load_cases()
    inp = R.inputs_of(g, 'in_call', dtype=torch.float64)
    out = R.corr_objects(inp, dict(spec['cfg'], min_size=spec['cases']['in_call']['min_size']), spec['cases']['in_call']['out_hw'], record=True)
    cs = spec['cases']['in_call']['census']
    assert out['ret_src'][0].tolist() == [-1, -1, -1, -1, -1] and out['ret_src'][1].tolist() == cs['src1'] and out['ret_src'][2].tolist() == cs['src2']
    assert tuple(out['scores'].shape) == (3, 6, 4) and bool(torch.isfinite(out['scores'][:, 1:5]).all())


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
def _simulate_appends(labels, boxes, ptr, L, min_size, inclusive=False):
    """Who wrote each slot last (-1: the stored entry stays) and ptr afterwards, by the loop's rule alone."""
    writer = -np.ones((len(ptr), L), np.int64)
    ptr = list(ptr)
    for j, (c, b) in enumerate(zip(labels, boxes)):
        w, h = b[2] - b[0], b[3] - b[1]
        if (w >= min_size and h >= min_size) if inclusive else (w > min_size and h > min_size):
            writer[c, ptr[c]] = j
            ptr[c] = (ptr[c] + 1) % L
    return writer, ptr


def test_many_objects_short_queue():
    c, w = E.case('many'), E.want('many')
    inp, cfg = c['inp'], c['cfg']
    N, L = len(inp['labels']), inp['bank_feature'].shape[1]
    assert N == 300 > PLAN_THREADS and (N + COMPACT_BLOCK - 1) // COMPACT_BLOCK == 5 and L == 3 < RETRIEVE_WAVES and inp['s_feat'].shape[1] == 17
    good = np.nonzero(inp['labels'] == 0)[0].tolist()
    assert good == [0, 63, 64, 65, 255, 256, 299] == list(E.MANY_GOOD)
    rest = np.setdiff1d(np.arange(N), good)
    assert not inp['s_mask'][rest].any() and not inp['t_mask'][rest].any() and set(inp['labels'][rest].tolist()) == {1, 2}
    assert len({inp['t_feat'][j].tobytes() for j in range(N)}) == N
    wd, ht = inp['boxes'][:, 2] - inp['boxes'][:, 0], inp['boxes'][:, 3] - inp['boxes'][:, 1]
    on = [int(((wd == cfg['min_size']) & (inp['labels'] == k)).sum()) for k in range(3)]
    flagged = [int(((wd > cfg['min_size']) & (ht > cfg['min_size']) & (inp['labels'] == k)).sum()) for k in range(3)]
    print(f'objects exactly min_size wide per class {on}, flagged per class {flagged}')
    assert on[0] == 0 and on[1] >= 20 and on[2] >= 20 and bool((ht > cfg['min_size']).all()) and min(flagged) > L
    writer, ptr = _simulate_appends(inp['labels'], inp['boxes'], E.MANY_PTR, L, cfg['min_size'])
    writer_ge, ptr_ge = _simulate_appends(inp['labels'], inp['boxes'], E.MANY_PTR, L, cfg['min_size'], inclusive=True)
    print(f'ptr afterwards {ptr} (with >= it would be {ptr_ge}); last writers {writer.tolist()} (with >=: {writer_ge.tolist()})')
    assert w['after_ptr'].tolist() == ptr == [(p + f) % L for p, f in zip(E.MANY_PTR, flagged)]
    assert all((writer[k] != writer_ge[k]).any() for k in (1, 2))                # the bank afterwards tells > from >=
    assert bool((writer >= 0).all())                                             # every stored entry is overwritten: the role rule decides all
    for k in range(3):
        for s in range(L):
            j = int(writer[k, s])
            assert np.array_equal(w['after_feature'][k, s].numpy(), inp['t_feat'][j]) and np.array_equal(w['after_box'][k, s].numpy(), inp['boxes'][j])
            assert np.array_equal(w['after_mask'][k, s].numpy(), inp['t_mask'][j])
    # the counts and sources the builder's docstring promises
    assert w['count'][good].tolist() == [2, 3, 3, 3, 3, 3, 3] and w['num_ins'] == 7 and int(w['count'].sum()) == 20
    assert w['ret_slot'][good].tolist() == [[0, 1, -1]] + [[0, 1, 2]] * 6
    assert w['ret_src'][good].tolist() == [[-1, -1, -1], [-1, -1, 0], [63, -1, 0], [63, 64, 0], [63, 64, 65], [255, 64, 65], [255, 256, 65]]
    assert bool((w['iiu'][rest] == 0).all()) and all(bool((w['iiu'][g] != 0).any()) for g in good)
    # the reduced call (the good objects alone), on which the seeds were chosen, is the same computation
    r = E.want('many_reduced')
    assert torch.equal(r['C'], w['C'][good]) and torch.equal(r['count'], w['count'][good])


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
def test_queue_cases():
    c, w = E.case('queue100'), E.want('queue100')
    L = c['inp']['bank_feature'].shape[1]
    groups = sorted({s // RETRIEVE_WAVES for s in E.QUEUE_SLOTS})
    assert L == 100 and (L + RETRIEVE_WAVES - 1) // RETRIEVE_WAVES == 25 and groups == [0, 1, 15, 16, 24]
    assert w['count'].tolist() == [8, 1, 0] and w['num_ins'] == 2 and w['ret_slot'][0].tolist() == list(E.QUEUE_SLOTS[:8]) and w['ret_slot'][1, 0] == 7
    assert bool((w['ret_src'] == -1).all()) and w['after_ptr'].tolist() == [7, 0, 1]          # class 1's ptr wraps from 99
    assert bool((w['after_feature'][2, 0].float() == torch.from_numpy(c['inp']['t_feat'][2])).all())
    want_src = {1: [[-1], [0], [1]], 2: [[-1], [-1, 0], [1, 0]], 3: [[-1], [-1, 0], [-1, 0, 1]]}
    for L in (1, 2, 3):
        a, b = E.want(f'queue{L}'), E.want(f'queue{L}_one_class')
        assert E.case(f'queue{L}')['inp']['bank_feature'].shape[1] == L < RETRIEVE_WAVES      # 4 - L waves of the workgroup are dead
        for k in ('s_feat', 's_mask', 't_feat', 't_mask', 'boxes'):
            assert np.array_equal(E.case(f'queue{L}')['inp'][k], c['inp'][k]) and np.array_equal(E.case(f'queue{L}_one_class')['inp'][k], c['inp'][k])
        assert a['count'].tolist() == [1, 1, 0] and a['num_ins'] == 2 and bool((a['ret_src'] == -1).all())
        assert b['count'].tolist() == [1, min(2, L), L] and b['num_ins'] == 3
        assert [b['ret_src'][i, :int(b['count'][i])].tolist() for i in range(3)] == want_src[L]
        print(f'L = {L}: one class: counts {b["count"].tolist()}, sources {want_src[L]}, ptr afterwards {b["after_ptr"].tolist()}')
        assert b['after_ptr'].tolist() == [(1 % L + 3) % L, 0, 0]


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
def test_solver_cases():
    stages = {C: [min(CHUNK, C - c0) for c0 in range(0, C, CHUNK)] for C in (15, 16, 17)}
    assert stages == {15: [15], 16: [16], 17: [16, 1]} and stages[17][-1] < GROUPS
    fixture = {k: E.CFG[k] for k in ('corr_num_iter', 'corr_num_smooth_iter', 'dist_kernel')}
    assert fixture == dict(corr_num_iter=10, corr_num_smooth_iter=1, dist_kernel=9)
    want_settings = dict(c15=(10, 1, 9), c16=(10, 1, 9), c17=(10, 1, 9), zero_cells=(10, 1, 9), iter0=(0, 1, 9), smooth0=(2, 0, 9), dist1=(10, 1, 1),
                         dist13=(10, 1, 13), it1sm3d3=(1, 3, 3), dist1_it1=(1, 1, 1), dist13_it1=(1, 1, 13))
    for name, st in want_settings.items():
        c, w = E.case(name), E.want(name)
        assert (c['cfg']['corr_num_iter'], c['cfg']['corr_num_smooth_iter'], c['cfg']['dist_kernel']) == st, name
        assert c['inp']['s_feat'].shape[1] == (int(name[1:]) if name in ('c15', 'c16', 'c17') else 17)
        assert w['count'].tolist() == [2, 3] and w['num_ins'] == 2 and w['ret_slot'].tolist() == [[1, 3, -1], [1, 3, 4]]
        assert w['ret_src'].tolist() == [[-1, -1, -1], [-1, -1, 0]] and w['after_ptr'].tolist() == [1]
        cells = [float(np.abs(c['inp'][k]).sum(-3).min()) for k in ('s_feat', 't_feat')] + [float(np.abs(c['inp']['bank_feature'][0, [1, 3]]).sum(1).min())]
        assert (min(cells) == 0) == (name == 'zero_cells'), name                  # zero cells only where they are planted
    c, w = E.case('zero_cells'), E.want('zero_cells')
    o, y, x = E.ZERO_S
    s, y2, x2 = E.ZERO_BANK
    assert not c['inp']['s_feat'][o, :, y, x].any() and not c['inp']['bank_feature'][0, s, :, y2, x2].any()
    assert bool((w['Cu'][o, :, 7 * y + x] == 0).all()) and bool((w['Cu'][:, 0, :, 7 * y2 + x2] == 0).all()) and w['ret_slot'][0, 0] == s
    assert bool((w['grad'][o, :, y, x].abs() > 100 * w['grad'][0].abs().max()).any())     # 1 / (0 + 1e-4): the zero cell's gradient
    # ten rounds forget dist_kernel; one round does not
    same = float((E.want('dist1')['C'] - E.want('dist13')['C']).abs().max() / E.want('dist13')['C'].abs().max())
    apart = float((E.want('dist1_it1')['C'] - E.want('dist13_it1')['C']).abs().max() / E.want('dist13_it1')['C'].abs().max())
    apart0 = float((E.want('iter0')['C'] - E.want('iter0')['Cu']).abs().max())
    print(f'C at dist_kernel 1 against 13: after ten rounds {same:.3e}, after one {apart:.3e}; C against Cu without a round {apart0:.3e}')
    assert same < 1e-9 and apart > 0.1 and apart0 > 0.1


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------
def test_paste_and_clip_cases():
    c, w = E.case('paste'), E.want('paste')
    H, W = c['hw']
    assert H * W == 6336 and (H * W + PASTE_TILE - 1) // PASTE_TILE == 2 and divmod(PASTE_TILE, W) == (46, 48)
    b = c['inp']['boxes']
    ints = lambda v: [int(x) for x in v]  # noqa: E731
    x1, y1, x2, y2 = ints(b[0])
    assert (x2 - x1, y2 - y1) == (70, 60) and y1 < 46 < y2 and x1 <= 48 < x2                  # over the tile edge, inside a row
    assert 28.0 / 60 * 0.5 - 0.5 < 0 and 28.0 / 70 * 0.5 - 0.5 < 0                            # upsampling: the first tap's source is negative
    assert b[1].tolist() == [3.75, 2.5, 24.75, 21.5] and int(b[1][2]) - int(b[1][0]) == int(b[1][2] - b[1][0]) == 21
    assert int(b[1][3]) - int(b[1][1]) == int(b[1][3] - b[1][1]) == 19
    assert (b[2][2] - b[2][0], b[2][3] - b[2][1]) == (1, 25) and (b[3][2], b[3][3]) == (W, H)
    assert w['count'].tolist() == [2, 3, 2, 3] and w['num_ins'] == 4 and w['ret_src'].tolist() == [[-1, -1, -1], [-1, -1, 0], [-1, -1, -1], [1, -1, -1]]
    for i in range(4):
        x1, y1, x2, y2 = ints(b[i])
        inside = torch.zeros(H, W, dtype=torch.bool)
        inside[y1:y2, x1:x2] = True
        assert bool((w['iiu'][i][:, ~inside] == 0).all()) and bool((w['iiu'][i][:, inside] != 0).any(1).all())
    assert bool((w['iiu'][0].reshape(2, -1)[:, PASTE_TILE:] != 0).any()) and bool((w['iiu'][3].reshape(2, -1)[:, -1] != 0).any())
    # clipping
    cb = np.asarray(E.CLIP_BOXES)
    assert np.array_equal(cb, cb.astype(np.int64)) and cb[0, 0] < 0 < cb[0, 2] and cb[1, 1] < 0 < cb[1, 3] and cb[2, 0] < W < cb[2, 2] and cb[3, 1] < H < cb[3, 3]
    assert cb[4, 0] >= W and (cb + E.PAD).min() >= 0 and (cb[:, 2] + E.PAD).max() <= W + 2 * E.PAD and (cb[:, 3] + E.PAD).max() <= H + 2 * E.PAD
    assert np.array_equal(E.case('clip')['inp']['boxes'] + E.PAD, E.case('clip_padded')['inp']['boxes'])
    for k in R.INPUT_KEYS:
        if k != 'boxes':
            assert np.array_equal(E.case('clip')['inp'][k], E.case('clip_padded')['inp'][k])
    wc, wp = E.want('clip'), E.want('clip_padded')
    assert tuple(wc['iiu'].shape) == (5, 2, H, W) and wc['count'].tolist() == [2, 3, 3, 3, 3] and wc['num_ins'] == 5
    kept = [int((wc['iiu'][i] != 0).sum()) for i in range(5)]
    whole = [int((wp['iiu'][i] != 0).sum()) for i in range(5)]
    print(f'non-zero iiu elements inside the canvas {kept}, of the whole box {whole}')
    assert all(0 < k < f for k, f in zip(kept[:4], whole[:4])) and kept[4] == 0 < whole[4]
    assert bool((wc['iiu'][0][:, :, 0] != 0).any()) and bool((wc['iiu'][1][:, 0] != 0).any()) and bool((wc['iiu'][2][:, :, -1] != 0).any())
    assert bool((wc['iiu'][3][:, -1] != 0).any())


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------
def test_labels_case():
    a, b = E.want('labels'), E.want('labels_removed')
    lab = E.case('labels')['inp']['labels'].tolist()
    assert [lab[i] for i in E.BAD_LABELS] == [-1, E.case('labels')['inp']['bank_feature'].shape[0]]
    keep = [i for i in range(len(lab)) if i not in E.BAD_LABELS]
    plain = R.load_cases()['cases']['plain']['census']
    assert plain['count'][1] > 0 and 3 in plain['ran']                                        # both objects mattered before
    for i in E.BAD_LABELS:
        assert int(a['count'][i]) == 0 and bool((a['ret_slot'][i] == -1).all()) and bool((a['iiu'][i] == 0).all()) and bool((a['grad'][i] == 0).all())
    for k in ('count', 'ret_slot', 'ret_src', 'assign', 'Cu', 'C', 'iiu', 'grad', 'scores', 'after_feature', 'after_mask', 'after_box', 'after_ptr'):
        x, y = (a[k][keep] if k[:5] != 'after' else a[k]), b[k]
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), k
    assert a['num_ins'] == b['num_ins'] == 2 and a['count'].tolist() == [5, 0, 5, 0, 3, 0]


# ---- exact scores ------------------------------------------------------------------------------------------------------------------------
def test_exact_scores_are_exact():
    for zero_query in (False, True):
        inp = E.exact_case(zero_query)['inp']
        for k in ('s_mask', 'bank_mask'):
            blocks = inp[k].reshape(-1, 7, 4, 7, 4)
            assert set(np.unique(inp[k]).tolist()) <= {0.0, 1.0} and bool((blocks == blocks[:, :, :1, :, :1]).all())
        for k in ('s_feat', 'bank_feature'):
            assert np.array_equal(inp[k] * 8, np.round(inp[k] * 8)) and inp[k].max() <= 1
        s32, s64 = E.exact_scores(torch.float32, zero_query), E.exact_scores(torch.float64, zero_query)
        for col in (0, 1, 3):
            assert torch.equal(s32[:, col].view(torch.int32), s64[:, col].float().view(torch.int32)), col
        # appearance: integer numerators over 64 and integer denominators, and the fp32 quotient of the fp32 operands
        t = E.as_torch(inp)
        m0, m1 = R.down7(t['s_mask']), R.down7(t['bank_mask'][0])
        num = (t['s_feat'][0][None] * t['bank_feature'][0] * m0[:, None] * m1[:, None]).sum((1, 2, 3))
        den = (m0 * m1).sum((1, 2))
        assert torch.equal(num * 64, (num * 64).round()) and torch.equal(den, den.round()) and float(num.max()) * 64 < 2 ** 24
        by_hand = num.float().numpy() / (den.float().numpy() + np.float32(1e-6))
        assert by_hand.dtype == np.float32 and np.array_equal(by_hand.view(np.int32), s32[:, 2].numpy().view(np.int32))
        print(f'zero query {zero_query}: scores {s32.tolist()}')
    s = E.exact_scores()
    assert s[E.EXACT_EMPTY].tolist() == [0.0, float(np.float32(24 * 16) / np.float32(784)), 0.0, float('inf')]
    assert s[:, 3].tolist() == [1.0, 1.0, float('inf'), 1.0, 2.0, 0.5] and s[0, 0] == np.float32(2) / np.float32(3) and s[3, 1] == np.float32(5) / np.float32(11)
    z = E.exact_scores(zero_query=True)
    assert bool(torch.isnan(z[E.EXACT_EMPTY, 0])) and bool((z[[0, 1, 3, 4, 5], 0] == 0).all())
    assert E.exact_passing(E.WIDE) == [0, 1, 2, 3, 4, 5]                         # what the restatement says of the empty slot: 0 > -inf
    assert E.exact_passing(E.WIDE, zero_query=True) == [0, 1, 3, 4, 5]           # and 0 / 0 passes nothing


def test_thresholds_sit_on_the_scores():
    st = E.threshold_settings()
    assert len(st) == 1 + 3 * 2 + 2 * 3
    for name, (th, slot, passes) in st.items():
        got = E.exact_passing(th)
        print(f'{name}: passing {got}')
        if slot is not None:
            assert (slot in got) == passes, name
    s = E.exact_scores()
    assert st['fg_iou_thresh_equal'][0]['fg_iou_thresh'] == float(s[0, 0]) > st['fg_iou_thresh_ulp_below'][0]['fg_iou_thresh']
    assert np.float32(st['fg_iou_thresh_ulp_below'][0]['fg_iou_thresh']) == np.nextafter(np.float32(s[0, 0]), np.float32(0))


# ---- stand-alone entry points ------------------------------------------------------------------------------------------------------------
def test_bounds_from_the_restatement():
    tols = E.score_tols()
    print('scores (fg, bg, appearance, ratio): fp32 against fp64 restatement ' + ', '.join(f'{t:.3e}' for t in tols) + f'; the bound is {E.MARGIN:g} times that')
    assert all(0 < t < 1e-6 for t in tols)
    for K in E.SUPERRES_KS:
        t = E.superres_tol(K)
        print(f'superres_T K = {K}: {t:.3e} (largest magnitude {float(E.superres_want(K).abs().max()):.3e})')
        assert 0 < t < 1e-6 and float(E.superres_T(K).min()) >= 0
    for run in E.SOLVE_RUNS:
        t = E.solve_tol(run)
        print(f'Cu gradient K, C, zero cell = {run}: {t:.3e} (largest magnitude {float(E.solve_want(*run)[1].abs().max()):.3e})')
        assert 0 < t < (1e-3 if run[1] == 1 else 1e-5)
    assert sorted({r[0] for r in E.SOLVE_RUNS[:-1]}) == [1, 8] and sorted({r[1] for r in E.SOLVE_RUNS}) == [1, 4, 15, 16, 17]
    f0, f1, _ = E.solve_inputs(*E.SOLVE_RUNS[-1])
    assert float(np.abs(f0).sum(1).min()) == 0 and all(float(np.abs(a).sum(1).min()) > 0 for r in E.SOLVE_RUNS[:-1] for a in E.solve_inputs(*r)[:2])
    y, x = E.SOLVE_ZERO
    assert bool((E.solve_want(*E.SOLVE_RUNS[-1])[0][:, 7 * y + x] == 0).all())
    # the one-hot planes: every output is a product of two 7 -> 28 tap weights (eighths) over 16, the same in fp32 and fp64
    T = torch.from_numpy(E.onehot_T())
    a, b = R.superres(T), R.superres(T.double())
    assert torch.equal(a.double(), b) and int((b != 0).sum()) > 0
    U = R.up_matrix(torch.zeros(1, dtype=torch.float64))
    assert torch.equal(U * 64, (U * 64).round())
    for k, (p, q) in enumerate(E.ONEHOT):
        assert torch.equal(b[k], torch.outer(U[:, p], U[:, q]) / 16)
