"""CPU: the host side of DiscoBox's cross-image correspondence (no kernel is launched here).

* tests/corr_ref.py, the restatement the GPU tests lean on, reproduces what the reference's own code computed (tests/golden/corr.npz,
  corr_planes_<case>.npz, make_golden_corr.py); with the reference present each case is regenerated live and compared;
* the limits of include/boxinst/boxinst_hip_corr.h are those of _lib, and INTEGRATION.md names the feature (the header against
  _lib.CORR_SIGNATURES, the exports and the guarded tests: tests/test_abi_families.py);
* the loss_corr block of every configs/discobox file is accepted (tests/golden/corr_cfg.json);
* CPU tensors, wrong sizes and max_retrieval_objs > 8 fail before any launch."""
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import corr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_corr.py')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
SPEC = R.load_cases()
CFG = SPEC['cfg']
NAMES = list(SPEC['cases'])


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _planes(name):
    return np.load(R.GOLDEN.replace('corr.npz', f'corr_planes_{name}.npz'))


@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_fixture(name):
    g, case = np.load(R.GOLDEN), SPEC['cases'][name]
    inp = R.inputs_of(g, name, dtype=torch.float64)
    inp['s_feat'].requires_grad_(True)
    out = R.corr_objects(inp, dict(CFG, min_size=case['min_size']), case['out_hw'], record=True)
    for k in ('ret_slot', 'count', 'assign'):
        assert np.array_equal(out[k].numpy(), g[f'{name}_{k}']), k
    assert out['num_ins'] == int(g[f'{name}_num_ins']) == len(case['census']['ran']) and out['count'].tolist() == case['census']['count']
    for mine, key in ((inp['bank_feature'], 'after_feature'), (inp['bank_mask'], 'after_mask'), (inp['bank_box'], 'after_box')):
        assert np.array_equal(mine.float().numpy(), g[f'{name}_{key}'].astype(np.float32)), key
    assert np.array_equal(inp['bank_ptr'].numpy(), g[f'{name}_after_ptr'])
    grad = torch.autograd.grad(out['loss_sum'], inp['s_feat'])[0] if out['num_ins'] else torch.zeros_like(inp['s_feat'])
    planes = _planes(name)
    for mine, want in ((out['Cu'].numpy(), planes['Cu']), (out['C'].numpy(), planes['C']), (grad.numpy(), g[f'{name}_grad']),
                       (out['iiu'].numpy(), g[f'{name}_iiu']), (float(out['loss_sum']), float(g[f'{name}_loss_sum']))):
        assert np.allclose(mine, want, rtol=1e-9, atol=1e-12)
    zero = np.unpackbits(g[f'{name}_iiu_zero'])[:out['iiu'].numel()].astype(bool).reshape(tuple(out['iiu'].shape))
    assert np.array_equal(out['iiu'].numpy() == 0, zero)
    for k in R.TOLERANCED:
        assert 0 < float(g[f'tol_{k}']) < 1e-5, k                    # measured, positive, of the size of float32 rounding


def test_restatement_rules_by_hand():
    # 28 -> 7: the mean of the middle 2 x 2 of each 4 x 4 block
    m = torch.arange(784.).view(1, 28, 28)
    assert torch.equal(R.down7(m)[0, 0, 0], m[0, 1:3, 1:3].mean()) and torch.equal(R.down7(m)[0, 6, 3], m[0, 25:27, 13:15].mean())
    # dist_kernel = 9 keeps Chebyshev distance <= 4: 1849 of the 2401 pairs
    assert int(R.dist_mask(9, torch.zeros(1)).sum()) == 1849 and int(R.dist_mask(1, torch.zeros(1)).sum()) == 49
    # pass_message: a corner pair has 4 in-range shifts, a centre pair 9; a constant stays constant
    T = torch.ones(1, 49, 49, dtype=torch.float64)
    assert torch.allclose(R.pass_message(T.clone()), T)
    one = torch.zeros(1, 49, 49, dtype=torch.float64)
    one[0, 0, 0] = 1.0                                   # (0,0) -> (0,0): votes for (1,1) -> (1,1) with shift (1,1); that pair has 9 shifts
    assert float(R.pass_message(one.clone())[0, 8, 8]) == pytest.approx(1 / 9) and float(R.pass_message(one.clone())[0, 0, 0]) == pytest.approx(1 / 4)
    # superres keeps the mass of T up to the 49 / 784 factor: rows of the bilinear matrix add up to 1
    U = R.up_matrix(torch.zeros(1, dtype=torch.float64))
    assert tuple(U.shape) == (784, 49) and torch.allclose(U.sum(1), torch.ones(784, dtype=torch.float64)) and int((U > 0).sum(1).max()) == 4
    # a zero slot fails every predicate through 0/0 and x/0
    q = torch.full((28, 28), 0.5)
    sc = R.slot_scores(q, torch.ones(4, 7, 7), torch.tensor([0., 0., 10., 10.]), torch.zeros(1, 28, 28), torch.zeros(1, 4, 7, 7), torch.zeros(1, 4))
    assert not bool(R.passing(sc, CFG).any()) and bool(torch.isnan(sc[0]).all()) and bool(torch.isinf(sc[3]).all())


@pytest.mark.parametrize('name', NAMES)
def test_fixture_is_what_the_reference_computes_now(name):
    """Live: the reference's code, loaded where it lies, gives the stored expectations again."""
    if not os.path.exists(os.path.join(REFERENCE, 'mmdet/models/dense_heads/discobox_head.py')):
        pytest.skip('the upstream checkout is not here')
    spec = importlib.util.spec_from_file_location('make_golden_corr', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert json.loads(json.dumps(dict(cfg=gen.CFG, kinds=gen.KINDS, cases=gen.SPEC))) == SPEC
    g = np.load(R.GOLDEN)
    live, planes, tol = gen.case_arrays(gen.load_reference(), name, gen.SPEC[name])
    for key, want in live.items():
        assert key in g, key
        if want.dtype.kind != 'f' or want.dtype == np.float16:
            assert np.array_equal(g[key], want), key
        else:               # exp and log may differ by an ulp between builds of torch
            assert np.allclose(g[key], want, rtol=1e-11, atol=1e-13), key
    stored = _planes(name)
    assert np.allclose(stored['Cu'], planes['Cu'], rtol=1e-11, atol=1e-13) and np.allclose(stored['C'], planes['C'], rtol=1e-11, atol=1e-13)
    for k, v in tol.items():
        assert v <= float(g[f'tol_{k}']) * 1.5, k
    if name == NAMES[0]:
        with open(os.path.join(ROOT, 'tests', 'golden', 'corr_cfg.json')) as fh:
            assert json.load(fh) == json.loads(json.dumps(gen.config_blocks())), 'tests/golden/corr_cfg.json is not what the configs of the reference give'


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[corr]."""
    from boxinstseg_amd import _lib
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_corr.h')) as fh:
        code = fh.read()
    for macro, value in (('BXI_CORR_FEAT', _lib.CORR_FEAT), ('BXI_CORR_MASK', _lib.CORR_MASK), ('BXI_CORR_MAX_OBJS', _lib.CORR_MAX_OBJS),
                         ('BXI_CORR_MAX_QUEUE', _lib.CORR_MAX_QUEUE)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', code).group(1)) == value, macro
    assert (R.FEAT, R.MASK) == (_lib.CORR_FEAT, _lib.CORR_MASK)
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3g', 'RoIAlign', '430 MB', 'num_gpu_bank', 'create_one', 'save_corr_img', 'perform_sinkhorn', 'corr_objects', 'bxi_corr_solve_f32'):
        assert word in integration, word


def test_reference_corr_blocks_are_accepted():
    import boxinstseg_amd as B
    from boxinstseg_amd import corr
    with open(os.path.join(ROOT, 'tests', 'golden', 'corr_cfg.json')) as fh:
        stored = json.load(fh)
    with open(os.path.join(ROOT, 'tests', 'golden', 'solo_head_cfg.json')) as fh:
        blocks = {k: v for k, v in json.load(fh).items() if k.startswith('discobox/')}
    assert len(stored) == 4 and sorted(stored) == sorted(blocks)
    for fname, block in blocks.items():
        s = B.parse_corr_cfg(block)
        assert s == stored[fname]
        assert s['bank'] == dict(num_class=block['num_classes'], len_queue=100, fg_iou_thresh=0.7, bg_iou_thresh=0.7, ratio_range=[0.9, 1.2], appear_thresh=0.7,
                                 max_retrieval_objs=5)
        assert s['solver'] == dict(exp=1.0, eps=0.05, gaussian_filter_size=3, low_score=0.3, num_iter=10, num_smooth_iter=1, dist_kernel=9)
        assert (s['min_size'], s['loss_weight'], s['min_objs']) == (32.0, 1.0, 5)
        ns = types.SimpleNamespace(**{k: v for k, v in block.items()})
        assert B.parse_corr_cfg(ns) == s
        bank, solver = B.ObjectBank(**s['bank']), B.SemanticCorrSolver(**s['solver'])
        assert bank.feature is None and bank.len_queue == 100 and solver.dist_kernel == 9
    block = next(iter(blocks.values()))
    lc = block['loss_corr']
    with pytest.raises(TypeError, match='loss_corr'):
        B.parse_corr_cfg({k: v for k, v in block.items() if k != 'loss_corr'})
    with pytest.raises(NotImplementedError, match='save_corr_img'):
        B.parse_corr_cfg(dict(block, loss_corr=dict(lc, save_corr_img=True)))
    with pytest.raises(NotImplementedError, match='size'):
        B.parse_corr_cfg(dict(block, loss_corr=dict(lc, obj_bank=dict(lc['obj_bank'], feat_height=14))))
    for name in ('ObjectBank', 'SemanticCorrSolver', 'superres_T', 'corr_objects', 'parse_corr_cfg'):
        assert name in B.__all__ and getattr(B, name) is getattr(corr, name) and name in B.__doc__


def test_cpu_tensors_and_bad_arguments_fail_loudly():
    import boxinstseg_amd as B
    kw = dict(num_class=2, len_queue=4, fg_iou_thresh=0.7, bg_iou_thresh=0.7, ratio_range=[0.9, 1.2], appear_thresh=0.7)
    with pytest.raises(ValueError, match='max_retrieval_objs'):
        B.ObjectBank(max_retrieval_objs=9, **kw)
    with pytest.raises(ValueError, match='len_queue'):
        B.ObjectBank(max_retrieval_objs=5, **dict(kw, len_queue=2000))
    with pytest.raises(ValueError, match='dist_kernel'):
        B.SemanticCorrSolver(1.0, 0.05, 3, 0.3, 10, 1, dist_kernel=8)
    with pytest.raises(ValueError, match='num_iter'):
        B.SemanticCorrSolver(1.0, 0.05, 3, 0.3, -1, 1, dist_kernel=9)
    bank, solver = B.ObjectBank(max_retrieval_objs=5, **kw), B.SemanticCorrSolver(1.0, 0.05, 3, 0.3, 10, 1, 9)
    f, m, b, lab = torch.zeros(2, 8, 7, 7), torch.zeros(2, 28, 28), torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.corr_objects(f, m, f, m, b, lab, bank, solver, (8, 8), 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.superres_T(torch.zeros(1, 49, 49))
    with pytest.raises(RuntimeError, match='CUDA'):
        bank.append(0, 0, f, m, b)
    with pytest.raises(RuntimeError, match='CUDA'):
        bank.get_similar_obj(types.SimpleNamespace(mask=m[:1], feature=f[:1], box=b[:1], category=0))
    with pytest.raises(RuntimeError, match='CUDA'):
        solver.solve(types.SimpleNamespace(mask=m[:1]), dict(feature=f, mask=m), f[:1])
    assert bank.feature is None                                              # nothing was allocated on the way


def test_abi_validation_without_device():
    """Every call fails before its launch: X is a non-NULL value that nothing dereferences."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X, nan = 0x1000, float('nan')
    assert lib.bxi_corr_workspace_bytes(4, 32, 9) == 0 and lib.bxi_corr_workspace_bytes(-1, 32, 5) == 0 and lib.bxi_corr_workspace_bytes(4, 0, 5) == 0
    assert lib.bxi_corr_workspace_bytes(0, 32, 5) == 16
    need = lib.bxi_corr_workspace_bytes(4, 32, 5)
    assert need == 4 * 5 * (2401 * 4 + 32 * 49 * 4 + 2 * 784 * 4 + 8) and need % 16 == 0
    assert lib.bxi_corr_plan_f32(X, X, X, 2, 2, 2000, 8.0, X, X, None) == -2
    assert lib.bxi_corr_plan_f32(X, X, X, 2, 2, 8, nan, X, X, None) == -3
    assert lib.bxi_corr_plan_f32(X, X, None, 2, 2, 8, 8.0, X, X, None) == -1
    retrieve = lambda **k: lib.bxi_corr_retrieve_f32(X, X, X, X, X, X, X, 2, k.get('C', 32), X, X, X, 2, 8, k.get('fg', 0.7), 0.7, 0.7, 0.9, 1.2, k.get('K', 5),  # noqa: E731
                                                     X, X, X, k.get('count', X), None, None)
    assert retrieve(K=9) == -2 and retrieve(K=0) == -2 and retrieve(C=0) == -2 and retrieve(fg=nan) == -3 and retrieve(count=None) == -1
    solve = lambda **k: lib.bxi_corr_solve_f32(X, X, X, 2, 32, X, 2, 8, X, X, X, k.get('K', 5), k.get('min_objs', 5), k.get('dist', 9), k.get('it', 10), 1, X, X, X,  # noqa: E731
                                               k.get('ws', X), k.get('bytes', 1 << 30), None)
    assert solve(K=9) == -2 and solve(dist=8) == -3 and solve(dist=0) == -3 and solve(it=-1) == -3 and solve(min_objs=0) == -3
    assert solve(ws=None) == -5 and solve(bytes=16) == -5 and solve(ws=X + 4) == -5
    assert lib.bxi_corr_loss_f32(X, 2, 32, 5, 0, X, X, X, X, 1 << 30, None) == -3
    assert lib.bxi_corr_loss_f32(X, 2, 32, 5, 5, X, X, X, X, 16, None) == -5
    assert lib.bxi_corr_loss_f32(X, 2, 32, 5, 5, None, X, X, X, 1 << 30, None) == -1
    assert lib.bxi_corr_grad_rescale_f32(X, X, -1, X, None) == -2 and lib.bxi_corr_grad_rescale_f32(X, None, 4, X, None) == -1
    iiu = lambda **k: lib.bxi_corr_iiu_f32(X, X, X, X, 2, 32, X, 2, 8, X, X, X, 5, 5, k.get('H', 8), 8, X, X, k.get('bytes', 1 << 30), None)  # noqa: E731
    assert iiu(H=0) == -2 and iiu(H=1 << 30) == -2 and iiu(bytes=16) == -5
    assert lib.bxi_corr_append_f32(X, X, X, X, X, X, 2, 32, X, X, X, None, 2, 8, None) == -1
    assert lib.bxi_corr_append_f32(X, X, X, X, X, X, 2, 32, X, X, X, X, 2, 0, None) == -2
    assert lib.bxi_corr_superres_f32(X, -1, X, None) == -2 and lib.bxi_corr_superres_f32(X, 4000, X, None) == -2 and lib.bxi_corr_superres_f32(None, 1, X, None) == -1
    assert lib.bxi_corr_cu_backward_f32(X, X, X, 9, 32, X, None) == -2 and lib.bxi_corr_cu_backward_f32(X, X, X, 0, 32, X, None) == -2
    assert lib.bxi_corr_cu_backward_f32(X, X, None, 5, 32, X, None) == -1
