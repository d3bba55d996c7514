"""CPU: the host side of the Box2Mask target assignment (no kernel is launched here).

* tests/box_match_ref.py, the float64 restatement the GPU tests lean on, reproduces what the reference's own code computed
  (tests/golden/box_match.npz, make_golden_box_match.py); with the reference and scipy present the fixture's expectations are
  regenerated live and compared with the stored ones;
* include/boxinst/boxinst_hip_assign.h, the library's exports and _lib.ASSIGN_SIGNATURES name the same entry points, and each is
  run by a named guarded test or is a size query;
* the registries build the assigner from the reference's own config block;
* CPU tensors fail loudly, and the entry points validate their arguments before anything touches a device."""
import importlib.util
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import box_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'box_match.npz')
CFG_JSON = os.path.join(ROOT, 'tests', 'golden', 'box_match_assigner_cfg.json')
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_box_match.py')
HEADER = os.path.join(ROOT, 'include', 'boxinst', 'boxinst_hip_assign.h')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
N_RAND, N_TIES = 12, 5


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _generator():
    pytest.importorskip('scipy')
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/core/bbox/match_costs/match_cost.py')):
        pytest.skip('the upstream checkout is not here')
    spec = importlib.util.spec_from_file_location('make_golden_box_match', GENERATOR)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_restatement_reproduces_the_reference(name):
    g = np.load(GOLDEN)
    _, (h, w), (H, W), Q, counts, pset, C = R.CASES[name]
    prm = R.PARAMS[pset]
    tol = float(g[f'{name}_tol'])
    stored, made = R.load_case(g, name), R.make_inputs(name)
    for i, (im, G) in enumerate(zip(stored, counts)):
        k = f'{name}{i}'
        for key in im:
            assert np.array_equal(im[key], made[i][key]), f'{k}: the stored {key} are not the inputs of the case table'
        pr, pc = R.pred_projections(im['logits'], H, W, prm['pred_act'])
        assert np.allclose(pr, g[f'{k}_proj_rows64'], rtol=0, atol=1e-12) and np.allclose(pc, g[f'{k}_proj_cols64'], rtol=0, atol=1e-12)
        cost = R.match_cost(im, H, W, **prm)
        assert cost.shape == (Q, G) == g[f'{k}_cost64'].shape
        if G:
            assert np.abs(cost - g[f'{k}_cost64']).max() <= 1e-11           # fp64 against fp64: summation order only
            assert np.abs(g[f'{k}_cost32'] - g[f'{k}_cost64']).max() <= tol and tol > 0
        gt_inds, labels, pos, pos_gt = R.assign(g[f'{k}_cost32'].astype(np.float64), im['labels'])
        assert np.array_equal(pos, g[f'{k}_rows']) and np.array_equal(pos_gt, g[f'{k}_cols'])
        assert np.array_equal(gt_inds, g[f'{k}_gt_inds']) and np.array_equal(labels, g[f'{k}_assigned_labels'])
        # the same assignment from the fp64 cost: the optimum is separated by far more than the two costs differ
        assert np.array_equal(R.assign(cost, im['labels'])[0], gt_inds)
        # what _get_target_single made of it (box2mask_head.py:176-189)
        assert np.array_equal(np.where(gt_inds > 0, labels, C), g[f'{k}_t_labels'])
        assert np.array_equal(g[f'{k}_t_label_weights'], np.ones(Q, np.int64))
        assert np.array_equal((gt_inds > 0).astype(np.float32), g[f'{k}_t_mask_weights'])
        assert np.array_equal(pos, g[f'{k}_t_pos_inds']) and np.array_equal(np.flatnonzero(gt_inds == 0), g[f'{k}_t_neg_inds'])
        targets = np.unpackbits(g[f'{k}_t_mask_targets'], axis=1)[:, :H * W].reshape(len(pos), H, W) if len(pos) else np.zeros((0, H, W))
        assert np.array_equal(targets, im['masks'][pos_gt])
    if name == 'r4':
        assert (stored[0]['logits'][0] < 0).all() and len(np.unique(stored[0]['logits'][1])) == 1


def test_restatement_solver_on_the_stored_matrices():
    g = np.load(GOLDEN)
    for n in range(N_RAND):
        c = g[f'lsa_rand{n}_cost']
        rows, cols = R.linear_sum_assignment(c)
        assert np.array_equal(rows, g[f'lsa_rand{n}_rows']) and np.array_equal(cols, g[f'lsa_rand{n}_cols']), n
    for n in range(N_TIES):
        c = g[f'lsa_ties{n}_cost'].astype(np.float64)
        rows, cols = R.linear_sum_assignment(c)
        assert R.is_matching(rows, cols, *c.shape) and c[rows, cols].sum() == int(g[f'lsa_ties{n}_total']) > 0, n
    assert f'lsa_rand{N_RAND}_cost' not in g and f'lsa_ties{N_TIES}_cost' not in g
    # by hand: the greedy choice (0,0) is wrong here
    rows, cols = R.linear_sum_assignment(np.array([[1.0, 2.0], [1.5, 9.0]]))
    assert rows.tolist() == [0, 1] and cols.tolist() == [1, 0]
    assert not R.is_matching(np.array([0, 0]), np.array([0, 1]), 2, 2) and R.is_matching(np.array([1, 0]), np.array([0, 1]), 2, 2)


def limit_uniform_pinned(g):
    """The 1024 x 1024 uniform matrix and whether it is the one the generator saw (a numpy whose stream differs gives another)."""
    c = R.limit_uniform(R.LIMIT_SIDE, R.LIMIT_SIDE)
    return c, zlib.crc32(c.tobytes()) == int(g['lsa_limit_crc'])


def test_restatement_solver_at_the_limit():
    """The matrices of the GPU limit cases, built here as there: on the pinned uniform one the restatement's indices are scipy's stored
    ones; on the tied one its total is scipy's."""
    g = np.load(GOLDEN)
    c, pinned = limit_uniform_pinned(g)
    assert c.shape == (R.LIMIT_SIDE, R.LIMIT_SIDE) == (1024, 1024) and c.dtype == np.float32
    rows, cols = R.linear_sum_assignment(c)
    assert R.is_matching(rows, cols, *c.shape) and np.array_equal(rows, np.arange(R.LIMIT_SIDE))
    if pinned:
        assert g['lsa_limit_cols'].dtype == np.int16 and np.array_equal(cols, g['lsa_limit_cols'])
    t = R.limit_ties()
    assert t.dtype == np.float32 and np.array_equal(t, np.round(t)) and 0 <= t.min() and t.max() <= 1008
    rows, cols = R.linear_sum_assignment(t)
    assert R.is_matching(rows, cols, *t.shape) and int(t[rows, cols].astype(np.int64).sum()) == int(g['lsa_limit_ties_total']) == 1532


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_fixture_is_what_the_reference_computes_now(name):
    """Live: the reference's code, loaded where it lies, gives the stored expectations again."""
    gen = _generator()
    g = np.load(GOLDEN)
    live = gen.reference_case(name)
    assert live, name
    for key, want in live.items():
        assert key in g, key
        got = g[key]
        if want.dtype.kind == 'f':
            assert np.allclose(got, want, rtol=0, atol=1e-6 if want.dtype == np.float32 else 1e-12), key
        else:
            assert np.array_equal(got, want), key


def test_header_exports_and_signatures_agree():
    """(declarations, exports and ctypes signatures: tests/test_abi_families.py)"""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    with open(HEADER) as fh:
        text = fh.read()
    assert int(re.search(r'#define BXI_MATCH_MAX_SIDE (\d+)', text).group(1)) == _lib.MATCH_MAX_SIDE
    assert lib.bxi_abi_version() == _lib.BXI_ABI_VERSION == 7                # additive: the version stays


def _reference_assigner_cfg():
    path = os.path.join(REFERENCE, 'configs/box2mask/box2mask_r50_lsj_8x2_50e_coco.py')
    with open(CFG_JSON) as fh:
        stored = json.load(fh)
    if os.path.exists(path):
        import ast
        with open(path) as fh:
            tree = ast.parse(fh.read())
        node = next(n for n in ast.walk(tree) if isinstance(n, ast.keyword) and n.arg == 'assigner')
        live = eval(compile(ast.Expression(node.value), path, 'eval'), {'dict': dict})
        assert live == stored, 'tests/golden/box_match_assigner_cfg.json is not the config block of the reference any more'
    return stored


def test_registries_build_the_assigner_from_the_reference_config():
    import boxinstseg_amd as B
    from boxinstseg_amd import box_match, registry
    cfg = _reference_assigner_cfg()
    assert cfg['type'] == 'MaskHungarianAssigner' and 'mask_cost' not in cfg
    a = registry.build_assigner(cfg)
    assert type(a) is box_match.MaskHungarianAssigner is B.MaskHungarianAssigner is registry.BBOX_ASSIGNERS.get('MaskHungarianAssigner')
    assert type(a.cls_cost) is B.ClassificationCost and a.cls_cost.weight == R.CFG['w_cls']
    assert type(a.dice_cost) is B.BoxMatchingCost
    assert (a.dice_cost.weight, a.dice_cost.pred_act, a.dice_cost.eps) == (R.CFG['w_dice'], R.CFG['pred_act'], R.CFG['eps'])
    assert a.mask_cost.weight == 0
    d = B.build_match_cost(dict(type='BoxMatchingCost'))
    assert (d.weight, d.pred_act, d.eps) == (R.DEFAULTS['w_dice'], R.DEFAULTS['pred_act'], R.DEFAULTS['eps'])
    assert B.build_match_cost(dict(type='ClassificationCost')).weight == R.DEFAULTS['w_cls']
    assert registry.MATCH_COST.get('BoxMatchingCost') is B.BoxMatchingCost
    with pytest.raises(TypeError, match='BoxMatchingCost'):
        B.MaskHungarianAssigner(dice_cost=dict(type='DiceCost', weight=1.0))
    with pytest.raises(TypeError, match='weight=0.0'):
        B.MaskHungarianAssigner(mask_cost=dict(type='FocalLossCost', weight=1.0, binary_input=True))
    with pytest.raises(KeyError):
        B.build_match_cost(dict(type='DiceCost'))


def test_cpu_tensors_fail_loudly():
    import boxinstseg_amd as B
    from boxinstseg_amd import box_match as M
    a = B.MaskHungarianAssigner()
    cls, pred = torch.randn(5, 4), torch.randn(5, 6, 7)
    labels, masks = torch.tensor([0, 2]), torch.ones(2, 12, 14, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.ClassificationCost()(cls, labels)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.BoxMatchingCost()(pred[:, None], masks[:, None, :6, :7])
    with pytest.raises(RuntimeError, match='CUDA'):
        a.assign(cls, pred, labels, masks, None, target_shape=(12, 14))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box2mask_get_targets(cls[None], pred[None], [labels], [masks], a, 3)
    with pytest.raises(RuntimeError, match='CUDA'):
        M.project_pred(pred, (12, 14))
    with pytest.raises(RuntimeError, match='CUDA'):
        M.project_gt(masks)
    with pytest.raises(RuntimeError, match='CUDA'):
        M.linear_sum_assignment(torch.rand(5, 2), labels, 5, [2])


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000                                           # a non-NULL value no call below dereferences: every one fails before its launch
    big = 1 << 40
    ws = lib.bxi_box_match_workspace_bytes
    assert ws(0, 8, 8) == 0 and ws(3, 0, 8) == 0 and ws(3, 8, 0) == 0 and ws(1, 65536, 65536) == 0
    assert ws(3, 20, 30) == 4 * 3 * (20 + 30)                                # one column tile, one row band
    assert ws(2, 129, 1025) == 4 * 2 * (2 * 129 + 2 * 1025)                  # two of each
    assert ws(200, 1024, 1024) == 4 * 200 * (1024 + 8 * 1024)

    def pred(src=X, n=3, h=7, w=9, H=20, W=30, act=1, rows=X, cols=X, sq=X, wsp=X, nbytes=big):
        return lib.bxi_match_project_pred_f32(src, n, h, w, H, W, act, rows, cols, sq, wsp, nbytes, None)
    assert pred(n=0, src=None, rows=None, cols=None, sq=None, wsp=None, nbytes=0) == 0
    assert pred(n=-1) == -2 and pred(h=0) == -2 and pred(W=0) == -2 and pred(H=65536, W=65536) == -2 and pred(h=65536, w=65536) == -2
    for name in ('src', 'rows', 'cols', 'sq'):
        assert pred(**{name: None}) == -1, name
    assert pred(wsp=None) == -5 and pred(nbytes=ws(3, 20, 30) - 1) == -5 and pred(wsp=X + 2) == -5
    assert pred(h=20, w=30, nbytes=ws(3, 20, 30) - 1) == -5                  # the same checks on the path without resampling
    for fn in (lib.bxi_match_project_gt_u8, lib.bxi_match_project_gt_f32):
        assert fn(None, 0, 20, 30, None, None, None, None, 0, None) == 0
        assert fn(X, -1, 20, 30, X, X, X, X, big, None) == -2 and fn(X, 2, 0, 30, X, X, X, X, big, None) == -2
        assert fn(None, 2, 20, 30, X, X, X, X, big, None) == -1 and fn(X, 2, 20, 30, X, X, None, X, big, None) == -1
        assert fn(X, 2, 20, 30, X, X, X, None, big, None) == -5 and fn(X, 2, 20, 30, X, X, X, X, ws(2, 20, 30) - 1, None) == -5

    def cost(cls=X, C=4, labels=X, pr=X, pc=X, ps=X, tr=X, tc=X, ts=X, P=2, Q=5, off=(0, 2, 5), H=20, W=30, wc=2.0, wd=5.0, eps=1.0, out=X, st=X):
        return lib.bxi_match_cost_f32(cls, C, labels, pr, pc, ps, tr, tc, ts, P, Q, None if off is None else _lib.int_array(off), H, W, wc, wd,
                                      eps, out, st, None)
    assert cost(P=0, off=None) == 0
    assert cost(P=-1) == -2 and cost(P=65, off=tuple(range(66))) == -2 and cost(Q=0) == -2 and cost(H=0) == -2 and cost(C=0) == -2
    assert cost(off=None) == -1 and cost(off=(1, 2, 5)) == -3 and cost(off=(0, 3, 2)) == -3
    assert cost(wc=float('nan')) == -3 and cost(wd=float('nan')) == -3 and cost(eps=float('nan')) == -3
    for name in ('labels', 'pr', 'pc', 'ps', 'tr', 'tc', 'ts', 'out', 'st'):
        assert cost(**{name: None}) == -1, name

    def lsa(c=X, labels=X, P=2, Q=5, off=(0, 2, 5), gi=X, lab=X, pos=X, pgt=X, st=X):
        return lib.bxi_linear_sum_assignment_f32(c, labels, P, Q, None if off is None else _lib.int_array(off), gi, lab, pos, pgt, st, None)
    assert lsa(P=0, off=None) == 0
    assert lsa(P=-1) == -2 and lsa(P=65, off=tuple(range(66))) == -2
    assert lsa(Q=0) == -4 and lsa(Q=1025) == -4 and lsa(off=(0, 1025, 1026)) == -4
    assert lsa(off=None) == -1 and lsa(off=(1, 2, 5)) == -3 and lsa(off=(0, 3, 2)) == -3
    for name in ('c', 'labels', 'gi', 'lab', 'pos', 'pgt', 'st'):
        assert lsa(**{name: None}) == -1, name
