"""CPU: every case of tests/solo_edges.py reaches the path it was planted for.  No kernel runs here: each count below comes from the
restatement (tests/solo_ref.py) alone, and is printed before it is asserted.

The vectorised forms the GPU tests compare against (``solo_edges.windows``, ``solo_edges.targets_from_moments``) are shown equal to
``R._window`` / ``R.targets``, instance by instance, on full sweep calls in both modes."""
import numpy as np
import pytest
import torch

from tests import solo_edges as E
from tests import solo_ref as R

TILE = 1024                      # BXI_FCOS_ELEM_TILE
PAIRS = 9                        # BXI_SOLO_PAIRS_PER_INSTANCE


def test_constants_are_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'boxinst', 'boxinst_hip_fcos.h')) as fh:
        assert int(re.search(r'#define BXI_FCOS_ELEM_TILE (\d+)', fh.read()).group(1)) == TILE
    with open(os.path.join(root, 'include', 'boxinst', 'boxinst_hip_solo.h')) as fh:
        text = fh.read()
    assert int(re.search(r'#define BXI_SOLO_PAIRS_PER_INSTANCE (\d+)', text).group(1)) == PAIRS
    assert int(re.search(r'#define BXI_SOLO_MAX_GRID (\d+)', text).group(1)) == 64 == max(E.GRIDS64)
    assert int(re.search(r'#define BXI_SOLO_MAX_FACTORS (\d+)', text).group(1)) == 4


# ---- A -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
def test_big_batch_crosses_both_256_edges(mode):
    want = E.big_want(mode, E.N_BIG)
    off = 3                                                                  # image 1's first global index
    S0 = E.GRIDS[0]
    # per level, image 1's owners (flat order: level, image, cell)
    at, own = 0, []
    for S in E.GRIDS:
        own.append(want['cell_owner'][at + S * S:at + 2 * S * S])
        at += 2 * S * S
    late_owned = sum(int((o - off >= 256).sum()) for o in own)
    contested = 0
    for l, S in enumerate(E.GRIDS):
        cells, inst = want['grid_order'][l][1], want['pair_inst'][l][1] - off
        early, late = np.zeros(S * S, bool), np.zeros(S * S, bool)
        early[cells[inst < 256]] = True
        late[cells[inst >= 256]] = True
        both = early & late
        assert bool((own[l][both] - off >= 256).all())                       # the later claimant owns it
        contested += int(both.sum())
    chunks0 = sorted(set((np.nonzero(own[0] >= 0)[0] // 256).tolist()))
    sel0 = want['sel_inst'][0][1]
    pairs = [len(want['grid_order'][l][1]) for l in range(len(E.GRIDS))]
    print(f'{mode}: num_ins {want["num_ins"]}, cells owned by a local index >= 256: {late_owned}, cells claimed from both sides of 256: '
          f'{contested}, level-0 chunks with a set cell: {chunks0} ({len(sel0)} set cells), pairs per level {pairs}')
    assert late_owned > 0 and contested > 0
    assert chunks0 == list(range((S0 * S0 + 255) // 256)) and len(sel0) >= 3
    assert max(pairs) > 256
    w64 = E.big_want(mode, E.N_BIG, True)
    top = int((w64['cell_owner'][4096:2 * 4096][3840:] >= 0).sum())
    print(f'{mode}: S = 64, set cells of image 1 at 3840 and above: {top}; set cells in all {int((w64["cell_owner"][4096:8192] >= 0).sum())}')
    assert top > 0
    assert int(want['moments'].max()) < 2 ** 24                              # the reference's own fp32 sums are exact on this batch
    # the cuts sit on both sides of the instance chunk's edge and every one of them changes the result
    assert E.CUTS == (255, 256, 257, 300)
    nums = [E.big_want(mode, n)['num_ins'] for n in E.CUTS]
    print(f'{mode}: num_ins at cuts {E.CUTS}: {nums}')
    assert len(set(nums)) > 1


# ---- B -----------------------------------------------------------------------------------------------------------------------
def _against_targets(name, mode, keep=None):
    c = E.planted_cases()[name]
    idx = np.arange(len(c['mom'])) if keep is None else keep
    boxes, labels, mom = c['boxes'][idx], c['labels'][idx], c['mom'][idx]
    kw = dict(num_grids=c['num_grids'], scale_ranges=c['scale_ranges'], sigma=c['sigma'], num_classes=c['num_classes'], canvas=c['canvas'])
    r = R.targets(mode, [boxes], [labels], None, mom=[mom], **kw)
    w = E.targets_from_moments(mode, boxes, labels, mom, **kw)
    assert np.array_equal(np.concatenate(w['cate_labels']), r['cate_labels']) and np.array_equal(np.concatenate(w['cell_owner']), r['cell_owner'])
    for l in range(len(c['num_grids'])):
        assert np.array_equal(w['pair_cell'][l], r['grid_order'][l][0]) and np.array_equal(w['pair_inst'][l], r['pair_inst'][l][0]), l
        assert np.array_equal(w['sel_inst'][l], r['sel_inst'][l][0]), l
    assert w['num_ins'] == r['num_ins'] > 0
    return c, w


@pytest.mark.parametrize('mode', R.MODES)
def test_vectorised_windows_equal_the_restatement(mode):
    """R.targets and, one by one, R._window on every instance of a full sweep call (S = 1..8); R.targets on every instance of the range
    and large-moment plants, on every fourth of the calls that hold S = 36 and 40 and on every tenth of the window plant."""
    fourth = np.arange(0, len(E.sweep_case((2520, 2520), E.SWEEP_GROUPS[4])['mom']), 4)
    for name, keep in (('sweep_800x1344_S1-8', None), ('sweep_800x1344_S33-40', fourth), ('sweep_2520x2520_S33-40', fourth + 1), ('ranges', None),
                       ('large_moments', None), ('windows', np.arange(0, len(E.window_case()['mom']), 10))):
        c, w = _against_targets(name, mode, keep)
        if name != 'sweep_800x1344_S1-8':
            continue
        for l, S in enumerate(c['num_grids']):
            win = w['windows'][l]
            for n, i in enumerate(w['hit'][l]):
                got = tuple(int(win[k][n]) for k in ('top', 'down', 'left', 'right'))
                assert got == R._window(mode, c['boxes'][i], c['mom'][i], S, c['canvas'], c['sigma']), (name, l, i)


def _census(mode):
    """Counts over every planted case of part B, from the restatement."""
    n = dict(naive_differs=0, naive_changes_window=0, negative=0, zero=0, clip_low=0, clip_high=0, sign_fix=0, zero_branch=0, half_correction=0, divisions=0)
    for name, c in E.planted_cases().items():
        w = E.planted_want(name, mode)
        for l, S in enumerate(c['num_grids']):
            win = w['windows'][l]
            for num, coord in ((win['num_w'], win['coord_w']), (win['num_h'], win['coord_h'])):
                n['naive_differs'] += int((np.floor(num.astype(np.float64) * S) != coord).sum())
                q, br = E.floor_div_branches(num, 1. / S)
                assert np.array_equal(q.astype(np.int64), coord)                     # the census restates the operator it counts
                n['sign_fix'] += br['sign_fix']; n['zero_branch'] += br['zero']; n['half_correction'] += br['half_correction']
                n['negative'] += int((num < 0).sum()); n['zero'] += int((num == 0).sum()); n['divisions'] += num.size
            nw, nh = np.floor(win['num_w'].astype(np.float64) * S).astype(np.int64), np.floor(win['num_h'].astype(np.float64) * S).astype(np.int64)
            tb, db, lb, rb = win['box']
            n['naive_changes_window'] += int(((np.maximum(tb, nh - 1) != win['top']) | (np.minimum(db, nh + 1) != win['down']) |
                                              (np.maximum(nw - 1, lb) != win['left']) | (np.minimum(rb, nw + 1) != win['right'])).sum())
            raw, br = E.floor_div_branches(win['edge'], 1. / S)
            assert np.array_equal(raw, (torch.from_numpy(win['edge']) // (1. / S)).numpy())
            n['sign_fix'] += br['sign_fix']; n['zero_branch'] += br['zero']; n['half_correction'] += br['half_correction']
            n['negative'] += int((win['edge'] < 0).sum()); n['zero'] += int((win['edge'] == 0).sum()); n['divisions'] += raw.size
            n['clip_low'] += int((raw[[0, 2]] < 0).sum())
            n['clip_high'] += int((raw[[1, 3]] > S - 1).sum())
    return n


@pytest.mark.parametrize('mode', R.MODES)
def test_planted_moments_reach_every_edge(mode):
    n = _census(mode)
    print(f'{mode}: ' + ', '.join(f'{k} {v}' for k, v in n.items()))
    assert n['naive_differs'] >= 100
    assert n['naive_changes_window'] >= 100     # instances whose window a multiplying kernel would get wrong through the centre alone
    assert n['negative'] >= 1 and n['zero'] >= 1 and n['clip_low'] >= 1 and n['clip_high'] >= 1
    # all three arithmetic branches of the floor division are taken (the GPU test's docstring says what is left)
    assert n['sign_fix'] >= 1 and n['zero_branch'] >= 1 and n['half_correction'] >= 1


def test_the_two_precisions_are_told_apart():
    """Centres whose cell differs between fp32 (DiscoBox) and double (BoxLevelSet), and among them windows that differ."""
    cells, wins = 0, 0
    for name, c in E.planted_cases().items():
        a, b = E.planted_want(name, 'discobox'), E.planted_want(name, 'boxlevelset')
        for l in range(len(c['num_grids'])):
            assert np.array_equal(a['hit'][l], b['hit'][l])
            wa, wb = a['windows'][l], b['windows'][l]
            differ = (wa['coord_w'] != wb['coord_w']) | (wa['coord_h'] != wb['coord_h'])
            window = np.zeros_like(differ)
            for k in ('top', 'down', 'left', 'right'):
                window |= wa[k] != wb[k]
            cells += int(differ.sum())
            wins += int((differ & window).sum())
    print(f'centres whose fp32 and double cells differ: {cells}; of these with different windows: {wins}')
    assert cells >= 1 and wins >= 1


def test_range_plant_sits_on_and_beside_the_bounds():
    c = E.range_case()
    areas = E.gt_areas(c['boxes']).numpy()
    f32 = np.float32
    on, below, above, both = 0, 0, 0, 0
    for lo, hi in c['scale_ranges']:
        lo, hi = f32(lo), f32(hi)
        on += int((areas == lo).sum()) + int((areas == hi).sum())
        below += int((areas == np.nextafter(lo, f32(-np.inf))).sum())
        above += int((areas == np.nextafter(hi, f32(np.inf))).sum())
    hits = np.stack([(areas >= f32(lo)) & (areas <= f32(hi)) for lo, hi in c['scale_ranges']])
    both = int((hits.sum(0) >= 2).sum())
    prod = ((c['boxes'][:, 2] - c['boxes'][:, 0]) * (c['boxes'][:, 3] - c['boxes'][:, 1])).double().numpy()
    inexact = (areas.astype(np.float64) ** 2 != prod)
    on_inexact = int((inexact & ((areas == f32(E.ROOT77)) | (areas == f32(E.ROOT1001)))).sum())
    print(f'areas on a bound {on}, one fp32 step below a lower bound {below}, one above an upper bound {above}, in two or more levels {both}, '
          f'on a bound that is an inexact root {on_inexact}')
    assert on >= 8 and below >= 2 and above >= 2 and both >= 4 and on_inexact >= 4
    assert float(E.ROOT77) ** 2 != 77.0 and float(E.ROOT1001) ** 2 != 1001.0 and float(f32(9.) * f32(16.)) == 144.0


def test_large_moments_are_large():
    c = E.large_moment_case()
    m = c['mom']
    f = m.astype(np.float64).astype(np.float32).astype(np.float64)
    print(f'moments that no fp32 holds: m00 {int((f[:, 0] != m[:, 0]).sum())}, m10 {int((f[:, 1] != m[:, 1]).sum())}; above 2^32: {int((m[:, 1] > 2 ** 32).sum())}')
    assert int((f[:, 0] != m[:, 0]).sum()) > 0 and int((f[:, 1] != m[:, 1]).sum()) > 0 and int((m[:, 1:] > 2 ** 32).sum()) > 0
    assert int(m.max()) < 2 ** 53
    # fp32 ties: 2^25 + 2 lies halfway between two fp32 values and goes to the even one
    assert float(np.float32(2 ** 25 + 2)) == 2 ** 25 and float(np.float32(2 ** 25 + 6)) == 2 ** 25 + 8 and float(np.float32(2 ** 24 + 1)) == 2 ** 24
    assert (m[:, 1] / m[:, 0] <= c['canvas'][1]).all() and (m[:, 2] / m[:, 0] <= c['canvas'][0]).all()


def test_pair_capacity_and_grid_limits():
    for name, c in E.planted_cases().items():
        assert len(c['num_grids']) == 8 and all(1 <= s <= 64 for s in c['num_grids'])
        for mode in R.MODES:
            w = E.planted_want(name, mode)
            for l in range(8):
                assert len(w['pair_cell'][l]) <= PAIRS * len(c['mom'])
    assert sorted(s for g in E.SWEEP_GROUPS for s in g) == list(range(1, 65))


# ---- C -----------------------------------------------------------------------------------------------------------------------
def test_mask_cases_reach_their_paths():
    cases = E.mask_cases()
    c = cases['second_trip']
    m = c['images'][0]
    band = E.mask_pass_band(c['factors'])
    assert band == 16 and band * m.shape[2] // 16 > 256                                   # more vectors than threads: a second trip
    flat = m[0].reshape(-1, band * m.shape[2])
    assert not flat[:, :4096].any() and flat[:, 4096:].all() and flat.shape[0] == 2       # ones only where the second trip reads
    assert R.moments(m)[0, 0] == 2 * (band * m.shape[2] - 4096) and m[1].all()
    for H in (16, 32):
        for W in (4, 8, 12):
            mm = cases[f'narrow_{H}x{W}']['images'][0]
            assert mm.shape[1:] == (H, W) and 16 // W + (1 if 16 % W else 0) >= 2          # a 16-byte vector spans two rows or more
            assert mm[3].all() and 0 < mm[0].sum() < H * W
    c = cases['half_band']
    band = E.mask_pass_band(c['factors'])
    hs = [m.shape[1] for m in c['images']]
    assert band == 16 and hs[0] % band == 8 and (max(hs) + band - 1) // band - (hs[0] + band - 1) // band >= 1
    assert [E.mask_pass_band(f) for f in ([2], [2, 4, 8, 16], [32, 64])] == [16, 16, 64]
    for key in ('factors_2', 'factors_2_4_8_16', 'factors_32_64'):
        c = cases[key]
        for f, (h, w) in zip(c['factors'], c['planes']):
            assert all(h > m.shape[1] // f and w > m.shape[2] // f and m.shape[1] % max(c['factors']) == 0 for m in c['images'])
        mom, planes = E.mask_want(c)
        assert all(p.any() for p in planes) and all(not p[:, -1].any() and not p[:, :, -1].any() for p in planes)
    assert len(cases['factors_2_4_8_16']['factors']) == 4
    (H, W, f), (H2, W2, f2) = E.LARGE_MASKS
    want = E.large_mask_moments(H, W)
    print(f'{H} x {W}: moments {want[0]}')
    assert want[0][1] > 2 ** 32 and want[0][2] > 2 ** 32 and want[0][0] < 2 ** 31
    # the wide one: a single band; the band's m10 and the share of every one of 256 threads (vectors tid, tid + 256, ...) leave 32 bits
    assert E.mask_pass_band([f2]) == H2 == 64 and (H2 * W2) % 16 == 0 and H2 * W2 < 2 ** 31
    per_vec = (np.arange(H2 * W2, dtype=np.int64) % W2).reshape(-1, 16).sum(1)
    per_thread = np.bincount(np.arange(per_vec.size) % 256, weights=per_vec.astype(np.float64))
    print(f'{H2} x {W2}: band m10 {int(per_vec.sum())}, smallest per-thread share {int(per_thread.min())}')
    assert int(per_vec.sum()) == E.large_mask_moments(H2, W2)[0][1] > 2 ** 32 and per_thread.min() > 2 ** 32
    # the closed form on a small full mask
    small = R.moments(np.ones((1, 6, 10), np.uint8))[0].tolist()
    assert small == [60, 6 * (10 * 9 // 2), 10 * (6 * 5 // 2)]


# ---- E -----------------------------------------------------------------------------------------------------------------------
def test_cate_case_spans_tiles_and_tiny_levels():
    c = E.cate_case()
    B, C, grids = E.CATE_SPEC['B'], E.CATE_SPEC['num_classes'], E.CATE_SPEC['num_grids']
    counts = [B * C * s * s for s in grids]
    assert counts[:2] == [9600, 7776] and counts[0] // TILE >= 2 and counts[0] % TILE and counts[1] % TILE and grids[2] ** 2 < 4 and grids[3] ** 2 == 4
    hw = grids[0] ** 2
    lab = c['labels'][:B * hw].reshape(B, hw)
    b, yx = np.nonzero(lab < C)
    elem = (b * C + lab[b, yx]) * hw + yx
    tiles = sorted(set((elem // TILE).tolist()))
    print(f'level 0: {len(elem)} positive elements in tiles {tiles}; num_ins {c["num_ins"]}')
    assert any(t > 0 for t in tiles)
    at = 0
    positives = []
    for s in grids:
        positives.append(int((c['labels'][at:at + B * s * s] < C).sum()))
        at += B * s * s
    print(f'positive cells per level {positives}')
    assert positives[0] > 0 and positives[1] > 0 and at == len(c['labels'])
    seen = {(v, pos) for _, _, _, _, v, pos in c['planted']}
    assert seen == {(v, p) for v in E.CATE_PLANTS for p in (True, False)}
    for l, b, ch, yx, v, pos in c['planted']:
        assert c['preds'][l].reshape(B, C, -1)[b, ch, yx] == v
    for gamma, alpha in E.CATE_SETTINGS:
        l32, g32 = R.cate_loss(c['preds'], c['labels'], c['num_ins'], gamma, alpha, E.CATE_LOSS_WEIGHT, dtype=torch.float32)
        l64, g64 = R.cate_loss(c['preds'], c['labels'], c['num_ins'], gamma, alpha, E.CATE_LOSS_WEIGHT)
        assert bool(torch.isfinite(l32)) and bool(torch.isfinite(l64)) and all(bool(torch.isfinite(g).all()) for g in g32 + g64)
        print(f'gamma {gamma}: loss {float(l64):.9g}, fp32 against fp64 {abs(float(l32) - float(l64)) / float(l64):.3e}')
