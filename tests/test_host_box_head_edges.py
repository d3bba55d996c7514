"""CPU: every case of tests/fcos_edges.py reaches the path it is named for.  No kernel runs here: each count below comes from the
restatement (tests/fcos_ref.py) and the tile formulas of the header alone, and is printed before it is asserted."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fcos_edges as E
from tests import fcos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def test_constants_are_the_headers():
    with open(os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_fcos.h')) as fh:
        text = fh.read()
    for macro, value in (('BXI_FCOS_LOC_TILE', E.LOC_TILE), ('BXI_FCOS_ELEM_TILE', E.ELEM_TILE), ('BXI_FCOS_GT_CHUNK', E.GT_CHUNK)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', text).group(1)) == value, macro
    with open(os.path.join(ROOT, 'include', 'boxinst_hip.h')) as fh:
        assert int(re.search(r'#define BXI_MAX_IMAGES (\d+)', fh.read()).group(1)) == E.MAX_IMAGES
    with open(os.path.join(ROOT, 'boxinstseg_amd', 'csrc', 'fcos_loss.hip')) as fh:
        assert f'i += {E.FINISH_THREADS})' in fh.read()
    from boxinstseg_amd import _lib
    lib = _lib.load()
    for sizes, B, C in ((E.SIZES_A, 4, 5), (E.SIZES_TILE, 3, 5), ([E.CHUNK_SIZE], 1, 5), (E.SIZES_MANY, E.MAX_IMAGES, 5)):
        arr = (_lib.FcosLevel * len(sizes))()
        for i, (h, w) in enumerate(sizes):
            arr[i] = _lib.FcosLevel(h, w, 8)
        assert lib.bxi_fcos_workspace_bytes(arr, len(sizes), B, C) == 16 * (E.loc_workgroups(sizes, B) + E.focal_workgroups(sizes, B, C))


# ---- A -----------------------------------------------------------------------------------------------------------------------
def test_config_sizes_are_the_issue_s():
    c = E.config_case()
    assert E.tiles(E.SIZES_A) == [60, 15, 4, 1, 1] and E.loc_workgroups(E.SIZES_A, c['B']) == 324
    assert sum(h * w for h, w in E.SIZES_A) * c['B'] == 81068
    assert 100 * 152 - 59 * E.LOC_TILE == 96 and 50 * 76 - 14 * E.LOC_TILE == 216
    assert [len(b) for b in c['boxes']] == [70, 3, 0, 1] and c['boxes'][3].tolist() == [[0.5, 0.25, 1215.5, 799.75]]
    assert all(b.dtype == torch.float32 for b in c['boxes']) and c['labels'][0].tolist() == [i % 5 for i in range(70)]
    side = torch.stack([c['boxes'][0][:, 2] - c['boxes'][0][:, 0], c['boxes'][0][:, 3] - c['boxes'][0][:, 1]], 1)
    big = side.min(1)[0]
    assert int((big >= 399).sum()) == 5 and int((side.max(1)[0] < 121).sum()) == 50
    for b in c['boxes']:
        assert bool((b[:, 0] >= 0).all()) and bool((b[:, 2] <= 1216).all()) and bool((b[:, 1] >= 0).all()) and bool((b[:, 3] <= 800).all())
    assert [(E.config_settings(n)['center_sampling'], E.config_settings(n)['norm_on_bbox']) for n in E.COMBOS] == \
        [(False, True), (False, False), (True, True), (True, False)]


@pytest.mark.parametrize('name', E.COMBOS)
def test_config_case_reaches_every_tile_trip_and_chunk(name):
    c = E.config_case()
    B = c['B']
    w = E.config_want(name)
    gi, img, lvl = w['gt_inds'].numpy(), w['img_inds'].numpy(), w['level_inds'].numpy()
    pos = gi >= 0
    wg, tile, _ = E.workgroup_of(E.SIZES_A, B)
    per_level = [int((pos & (lvl == l)).sum()) for l in range(5)]
    per_image = [int((pos & (img == b)).sum()) for b in range(B)]
    late_wg = int((pos & (wg >= E.FINISH_THREADS)).sum())
    second_chunk = pos & (lvl == 0) & (img == 0) & (tile >= 1) & (gi >= E.GT_CHUNK)
    ct = w['ctr_targets'].numpy()
    print(f'{name}: tiles per level {E.tiles(E.SIZES_A)}, workgroups {E.loc_workgroups(E.SIZES_A, B)}, positives {int(pos.sum())}, per level '
          f'{per_level}, per image {per_image}, in workgroups >= 256: {late_wg} (workgroups with positives: {len(set(wg[pos].tolist()))}), on level 0 in '
          f'tiles >= 1 won by a box of index >= 64: {int(second_chunk.sum())} (boxes {sorted(set(gi[second_chunk].tolist()))}), smallest positive '
          f'centerness target {ct[pos].min():.6g}')
    assert all(n > 0 for n in per_level)
    assert per_image[2] == 0 and all(per_image[b] > 0 for b in (0, 1, 3))
    assert late_wg > 0 and int(second_chunk.sum()) > 0
    # what makes the centerness sum exact in any order: every term a multiple of 2^-40, every partial sum below 2^12
    assert float(ct[pos].min()) >= 2.0 ** -17 and int(pos.sum()) < 2 ** 12 and bool((ct[~pos] == 0).all()) and float(ct.max()) <= 1.0
    total = w['ctr_targets'].double().sum()
    for order in (np.arange(len(ct))[::-1], np.random.default_rng(0).permutation(len(ct))):
        assert float(torch.from_numpy(ct[order].copy()).double().cumsum(0)[-1]) == float(total)
    assert E.stats_of(w) == (float(pos.sum()), float(np.float32(float(total))))
    # the same targets whatever norm_on_bbox says, but for the distances' unit
    other = E.config_want({'cs_norm_giou': 'cs_pix_giou_w', 'cs_pix_giou_w': 'cs_norm_giou', 'box_norm_ioulog': 'box_pix_ioulog',
                           'box_pix_ioulog': 'box_norm_ioulog'}[name])
    assert torch.equal(other['gt_inds'], w['gt_inds']) and not torch.equal(other['bbox_targets'], w['bbox_targets'])


# ---- B -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_on_bbox', [True, False])
def test_tile_case_sits_on_the_tile_edges(norm_on_bbox):
    c = E.tile_case()
    assert [h * w for h, w in E.SIZES_TILE] == [256, 257, 255, 512, 511] and E.tiles(E.SIZES_TILE) == [1, 2, 1, 2, 2]
    w = E.ref_targets(c, E.tile_settings(norm_on_bbox))
    gi, img, lvl = w['gt_inds'].numpy(), w['img_inds'].numpy(), w['level_inds'].numpy()
    _, tile, _ = E.workgroup_of(E.SIZES_TILE, c['B'])
    assert bool((gi[img == 0] == 0).all()) and bool((gi[img == 1] == -1).all()) and bool((gi[img == 2] >= 1).all())
    bt = w['bbox_targets'].numpy()[img == 0]
    rows = {tuple(r) for r in bt.tolist()}
    split = {(l, t): sorted(set(gi[(img == 2) & (lvl == l) & (tile == t)].tolist())) for l in range(5) for t in range(E.tiles(E.SIZES_TILE)[l])}
    print(f'norm_on_bbox {norm_on_bbox}: locations {len(gi)}, distinct bbox_targets in image 0: {len(rows)} of {len(bt)}; image 2, boxes per '
          f'(level, tile): {split}')
    # every location of a level has its own distances: a location written to another's row shows
    at = 0
    for h, wd in E.SIZES_TILE:
        assert len({tuple(r) for r in bt[at:at + h * wd].tolist()}) == h * wd
        at += h * wd
    assert set(gi[img == 2].tolist()) == {1, 2}
    assert split[(1, 0)] == [1, 2] and split[(3, 0)] == [1, 2] and split[(3, 1)] == [1, 2] and split[(4, 0)] == [1, 2] and split[(4, 1)] == [1]


@pytest.mark.parametrize('arrangement', E.CHUNK_ARRANGEMENTS)
def test_chunk_case_winners(arrangement):
    c = E.chunk_case(arrangement)
    n = len(c['boxes'][0])
    w = E.ref_targets(c, E.chunk_settings())
    gi = w['gt_inds'].numpy()
    T = E.tiles([E.CHUNK_SIZE])[0]
    per_tile = [sorted(set((gi[t * E.LOC_TILE:(t + 1) * E.LOC_TILE] // E.GT_CHUNK).tolist())) for t in range(T)]
    print(f'{arrangement}: {n} boxes, {T} tiles (the last holds {len(gi) - (T - 1) * E.LOC_TILE}), winning chunks per tile {per_tile}, winning boxes '
          f'{sorted(set(gi.tolist()))}')
    assert T == 7 and len(gi) - 6 * E.LOC_TILE == 64
    b = c['boxes'][0]
    assert not bool((b == b.round()).all(1).any())
    if arrangement == 'winner_in_last_chunk':
        assert n == E.GT_CHUNK + 1 and set(gi.tolist()) == {n - 1}
    elif arrangement == 'tie_across_the_boundary':
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        assert n == E.GT_CHUNK + 1 and float(area[n - 2]) == float(area[n - 1]) < float(area[0]) and set(gi.tolist()) == {n - 2}
        assert (n - 2) // E.GT_CHUNK == 0 and (n - 1) // E.GT_CHUNK == 1
    else:
        assert n == 2 * E.GT_CHUNK + 3 and per_tile == [[k] for k in E.ALTERNATING_CHUNKS] and {0, 1, 2} == set(E.ALTERNATING_CHUNKS)
        assert {63, 64, 127, 128, 130} <= set(gi.tolist())                  # the first and the last slot of a chunk win somewhere


def test_many_images_case_fills_the_offset_table():
    c = E.many_images_case()
    assert c['B'] == E.MAX_IMAGES == 64 and E.tiles(E.SIZES_MANY) == [1, 2]
    assert [i for i, b in enumerate(c['boxes']) if len(b)] == list(E.IMAGES_WITH_BOXES)
    w = E.ref_targets(c, E.many_images_settings())
    gi, img = w['gt_inds'].numpy(), w['img_inds'].numpy()
    per = {b: sorted(set(gi[(img == b) & (gi >= 0)].tolist())) for b in E.IMAGES_WITH_BOXES}
    print(f'B = {c["B"]}: workgroups {E.loc_workgroups(E.SIZES_MANY, c["B"])}, winning global box indices per image {per}, positives '
          f'{ {b: int(((img == b) & (gi >= 0)).sum()) for b in E.IMAGES_WITH_BOXES} }')
    assert per == {0: [0, 1], 31: [2, 3, 4], 63: [5, 6]}
    assert set(img[gi >= 0].tolist()) == set(E.IMAGES_WITH_BOXES)


# ---- C -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.LOSS_CASES)
def test_loss_case_plants_and_trips(name):
    c = E.config_case()
    B, C = c['B'], c['C']
    lc = E.loss_case(name)
    s = E.config_settings(name)
    assert (s['gamma'], s['bbox_loss_kind']) == {'cs_norm_giou': (2.0, 'giou'), 'box_pix_ioulog': (1.5, 'iou_log')}[name] and s['gamma'] >= 1
    n_part = E.loc_workgroups(E.SIZES_A, B) + E.focal_workgroups(E.SIZES_A, B, C)
    assert E.focal_workgroups(E.SIZES_A, B, C) == 398 and n_part == 722 and (n_part + E.FINISH_THREADS - 1) // E.FINISH_THREADS == 3
    labels = E.config_want(name)['labels'].numpy()
    slices = E.level_slices(E.SIZES_A, B)
    seen = {}
    for l, e, v, positive in lc['planted']:
        hw = E.SIZES_A[l][0] * E.SIZES_A[l][1]
        b, cc, yx = e // (C * hw), (e // hw) % C, e % hw
        assert float(lc['maps']['cls'][l].reshape(-1)[e]) == v == float(lc['maps']['cls'][l][b, cc].reshape(-1)[yx])
        assert (int(labels[slices[l]].reshape(B, hw)[b, yx]) == cc) == positive
        seen.setdefault((l, positive), set()).add(v)
    elems = {l: sorted(e for ll, e, _, _ in lc['planted'] if ll == l) for l in (0, 1)}
    print(f'{name}: partials {n_part} (three trips of the finish kernel), planted elements per level {elems}; focal tiles holding a plant: '
          f'{ {l: sorted(set(e // E.ELEM_TILE for e in v)) for l, v in elems.items()} }')
    for l in (0, 1):
        hw = E.SIZES_A[l][0] * E.SIZES_A[l][1]
        assert seen[(l, True)] == set(E.PLANTS) and seen[(l, False)] == set(E.PLANTS)
        assert {0, E.ELEM_TILE - 1, E.ELEM_TILE, B * C * hw - 1, C * hw - 1, C * hw} <= set(elems[l])
    # seeded maps of the recipe, exact zeros among the distances
    made = R.make_inputs(dict(levels=E.SIZES_A, num_classes=C, gt_bboxes=[None] * B), E.SEED_MAPS)
    for k in ('bbox', 'ctr'):
        assert all(np.array_equal(a, b) for a, b in zip(lc['maps'][k], made[k]))
    assert sum(int((a != b).sum()) for a, b in zip(lc['maps']['cls'], made['cls'])) == len(lc['planted'])
    assert any((m == 0).any() for m in lc['maps']['bbox'])
    # both runs of the restatement are finite on the planted maps
    tg = E.config_want(name)
    for dtype in (torch.float32, torch.float64):
        out = R.losses_and_grads(lc['maps'], tg, s, dtype)
        assert bool(torch.isfinite(out[0]).all()) and all(bool(torch.isfinite(g).all()) for part in out[1:] for g in part)


def test_maps_from_targets_round_trip():
    c = E.config_case()
    bt = E.config_want('cs_norm_giou')['bbox_targets']
    maps = E.maps_from_targets(bt.numpy(), E.SIZES_A, c['B'])
    assert [m.shape for m in maps] == [(c['B'], 4, h, w) for h, w in E.SIZES_A]
    assert torch.equal(R.flatten_maps([torch.from_numpy(m) for m in maps]), bt)
