"""CPU: the host side of Matrix NMS and mask scoring (no kernel is launched here).

* tests/matrix_nms_ref.py, the float64 restatement the GPU tests compare against, reproduces what the reference's own
  mask_matrix_nms and BoxSOLOv2Head.get_seg_single computed (tests/golden/matrix_nms.npz, make_golden_matrix_nms.py);
* include/boxinst/boxinst_hip_post.h, the library's exports and _lib.POST_SIGNATURES name the same entry points, and each is
  run by a named guarded test or is a size query;
* CPU tensors fail loudly, and the entry points validate their arguments before anything touches a device."""
import os

import numpy as np
import pytest
import torch

from tests import matrix_nms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'matrix_nms.npz')
CASES = ('g20', 'g05', 'lin', 'cut')
SCORE_RTOL = 2e-6


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def golden_case(g, name):
    h, w = (int(v) for v in g[f'{name}_hw'])
    packed = g[f'{name}_masks']
    masks = np.unpackbits(packed, axis=1)[:, :h * w].reshape(len(packed), h, w).astype(bool)
    return dict(masks=masks, labels=g[f'{name}_labels'], scores=g[f'{name}_scores'],
                kernel='gaussian' if int(g[f'{name}_kernel']) == 0 else 'linear', sigma=float(g[f'{name}_sigma']),
                nms_pre=int(g[f'{name}_nms_pre']), filter_thr=float(g[f'{name}_filter_thr']), max_num=int(g[f'{name}_max_num']))


def golden_seg(g):
    """The get_seg_single fixture and the candidates the reference's method selects from it (box_solov2_head.py:525-546)."""
    score_thr, mask_thr, filter_thr, nms_pre, max_per_img, sigma = (float(v) for v in g['seg_cfg'])
    cfg = dict(score_thr=score_thr, mask_thr=mask_thr, filter_thr=filter_thr, nms_pre=int(nms_pre), max_per_img=int(max_per_img),
               kernel='gaussian', sigma=sigma)
    cate = g['seg_cate']
    idx = np.argwhere(cate > np.float32(score_thr))
    level = np.repeat(g['seg_strides'], g['seg_grids'] ** 2).astype(np.float64)
    return cfg, idx, cate[cate > np.float32(score_thr)], level[idx[:, 0]]


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(name):
    g = np.load(GOLDEN)
    c = golden_case(g, name)
    r = R.matrix_nms_ref(c['masks'], c['labels'], c['scores'], c['filter_thr'], c['nms_pre'], c['max_num'], c['kernel'], c['sigma'])
    assert R.min_rel_gap(r['decayed'], (c['filter_thr'],)) > 1e-4            # the order of the fixture is not a coin toss
    assert np.array_equal(r['keep_inds'], g[f'{name}_keep_inds'])
    assert np.array_equal(r['labels'], g[f'{name}_out_labels'])
    assert np.allclose(r['scores'], g[f'{name}_out_scores'], rtol=SCORE_RTOL, atol=0)
    assert (r['decayed'] < c['scores'].astype(np.float64)[r['order']] * (1 - 1e-6)).mean() > 0.8      # most candidates are decayed


def test_restatement_reproduces_get_seg_single():
    g = np.load(GOLDEN)
    cfg, idx, cate_scores, level = golden_seg(g)
    r = R.seg_nms_ref(g['seg_probs'][idx[:, 0]], idx[:, 1], cate_scores, level, cfg['mask_thr'], cfg['filter_thr'], cfg['nms_pre'],
                      cfg['max_per_img'], cfg['kernel'], cfg['sigma'])
    assert 0 < len(r['kept']) < len(idx), 'the per-level area filter must drop some candidates and keep some'
    assert len(set(level.tolist())) == 2
    assert R.min_rel_gap(r['decayed'], (cfg['filter_thr'],)) > 1e-4 and R.min_rel_gap(r['scores_in']) > 1e-4
    assert np.array_equal(r['labels'], g['seg_out_labels'])
    assert np.allclose(r['scores'], g['seg_out_scores'], rtol=SCORE_RTOL, atol=0)


def test_restatement_hand_cases():
    """Three identical masks of one label (the values of the reference, matrix_nms.py:88-99, by hand)."""
    m = np.ones((3, 4, 5), bool)
    lab, s = np.zeros(3, np.int64), np.array([0.9, 0.8, 0.7], np.float32)
    r = R.matrix_nms_ref(m, lab, s)
    # column 1: exp(-2) / 1; column 2: min(exp(-2) / 1, exp(-2) / exp(-2)) = exp(-2)
    assert np.allclose(r['scores'], [np.float32(0.9), np.float32(0.8) * np.exp(-2.0), np.float32(0.7) * np.exp(-2.0)], rtol=1e-12)
    assert np.allclose(r['scores'], [0.9, 0.1083, 0.0947], atol=5e-5)
    r = R.matrix_nms_ref(m, lab, s, kernel='linear')
    assert np.isnan(r['scores'][0]) and np.allclose(r['scores'][1:], [0.9, 0.0], rtol=1e-7) and r['keep_inds'].tolist() == [2, 0, 1]
    r = R.matrix_nms_ref(m, lab, s, kernel='linear', filter_thr=0.05)
    assert r['keep_inds'].tolist() == [0]
    # tied scores: the lower index first
    r = R.matrix_nms_ref(R.disc_masks(np.random.default_rng(0), 6, 7, 9), np.zeros(6, np.int64), np.full(6, 0.5, np.float32))
    assert r['order'].tolist() == list(range(6))


def test_cpu_tensors_fail_loudly():
    import boxinstseg_amd as B
    from boxinstseg_amd import matrix_nms as M
    masks, lab, s = torch.ones(3, 4, 5, dtype=torch.bool), torch.zeros(3, dtype=torch.long), torch.tensor([0.9, 0.8, 0.7])
    cfg = dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0)
    meta = dict(img_shape=(16, 20, 3), ori_shape=(16, 20, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.mask_matrix_nms(masks, lab, s)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.mask_matrix_nms(masks[:0], lab[:0], s[:0])
    with pytest.raises(RuntimeError, match='CUDA'):
        B.seg_nms(torch.rand(3, 4, 5), lab, s, torch.ones(3), cfg)
    with pytest.raises(RuntimeError, match='CUDA'):
        M.pack_probs(torch.rand(3, 4, 5), 0.5)
    with pytest.raises(RuntimeError, match='CUDA'):
        M.pack_masks(masks)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box_solov2_get_seg_single(torch.rand(5, 2), torch.rand(5, 4, 5), (4, 5), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(RuntimeError, match='CUDA'):
        B.discobox_get_seg_single(torch.rand(5, 2), torch.rand(1, 3, 4, 5), torch.rand(5, 3), (4, 5), meta, cfg, [2, 1], [8, 16])
    with pytest.raises(NotImplementedError, match='not supported in matrix nms'):
        B.mask_matrix_nms(masks, lab, s, kernel='cosine')
    with pytest.raises(NotImplementedError):
        B.seg_nms(torch.rand(3, 4, 5), lab, s, torch.ones(3), dict(cfg, kernel='cosine'))


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000                                           # a non-NULL value no call below dereferences: every one fails before its launch
    # pack: n_all == 0 is a no-op; bad shapes; h*w at the fp32-exact limit; NULL pointers
    assert lib.bxi_mask_pack_f32(None, 0, 4, 5, 0.5, None, None, None, None) == 0
    assert lib.bxi_mask_pack_u8(None, 0, 4, 5, None, None, None) == 0
    assert lib.bxi_mask_pack_f32(X, -1, 4, 5, 0.5, X, X, X, None) == -2
    assert lib.bxi_mask_pack_f32(X, 3, 0, 5, 0.5, X, X, X, None) == -2
    assert lib.bxi_mask_pack_u8(X, 3, 4, 0, X, X, None) == -2
    assert lib.bxi_mask_pack_f32(X, 3, 4096, 4096, 0.5, X, X, X, None) == -2
    assert lib.bxi_mask_pack_u8(X, 3, 4096, 4096, X, X, None) == -2
    assert lib.bxi_mask_pack_f32(None, 3, 4, 5, 0.5, X, X, X, None) == -1
    assert lib.bxi_mask_pack_f32(X, 3, 4, 5, 0.5, X, X, None, None) == -1
    assert lib.bxi_mask_pack_u8(X, 3, 4, 5, None, X, None) == -1
    assert lib.bxi_mask_pack_u8(X, 3, 4, 5, X, None, None) == -1
    # workspace size: compensate [n] + one row of column maxima per 32 candidates
    assert lib.bxi_matrix_nms_workspace_bytes(0) == 0 and lib.bxi_matrix_nms_workspace_bytes(2049) == 0
    assert lib.bxi_matrix_nms_workspace_bytes(1) == 8 and lib.bxi_matrix_nms_workspace_bytes(33) == 4 * 33 * 3
    assert lib.bxi_matrix_nms_workspace_bytes(2048) == 4 * 2048 * 65
    big = 1 << 30

    def nms(bits=X, area=X, labels=X, order=X, scores=X, n_all=50, n=40, h=24, w=40, kernel=0, sigma=2.0, decayed=X, iou=X, ws=X, ws_bytes=big):
        return lib.bxi_matrix_nms_f32(bits, area, labels, order, scores, n_all, n, h, w, kernel, sigma, decayed, iou, ws, ws_bytes, None)
    assert nms(n_all=0) == -2 and nms(h=0) == -2 and nms(h=4096, w=4096) == -2
    assert nms(n=0) == -4 and nms(n=2049) == -4
    assert nms(kernel=2) == -3 and nms(kernel=-1) == -3 and nms(sigma=float('nan')) == -3
    for name in ('bits', 'area', 'labels', 'order', 'scores', 'decayed', 'iou'):
        assert nms(**{name: None}) == -1, name
    assert nms(ws=None) == -5
    assert nms(ws_bytes=lib.bxi_matrix_nms_workspace_bytes(40) - 1) == -5
    assert nms(ws=X + 2) == -5                            # fp32 workspace: 4-byte aligned
    assert _lib.status_string(-5)
