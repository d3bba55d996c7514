"""CPU: the host side of multi-scale deformable attention (no kernel is launched here).

* the two restatements of tests/msda_ref.py -- mmcv's op never ran here, its arithmetic is unpinned -- agree forward and in every gradient,
  and obey rules checked by hand;
* the fixture is what the restatement computes now, its inputs keep off the grid, its tolerances are of the size of fp32 rounding;
* the limits of include/boxinst/boxinst_hip_msda.h are those of _lib, and INTEGRATION.md names the feature (the header against
  _lib.MSDA_SIGNATURES, the exports and the guarded tests: tests/test_abi_families.py);
* the attn_cfgs block of the reference's Box2Mask configs builds the module; its state-dict keys and init_weights are the restated module's;
* bad arguments, CPU tensors, half precision and shapes outside the support set fail before any launch;
* the premise of tests/test_gpu_msda_fixed_point.py holds for the restatement alone: on the dyadic cases fp32 and fp64 give the same bits;
  cell_hits counts a case counted by hand."""
import importlib
import importlib.util
import inspect
import json
import math
import os
import re

import pytest
import torch

from tests import msda_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, 'tests', 'golden', 'make_golden_msda.py')
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
SPEC = R.load_cases()
GRADIENT_CASES = [n for n in SPEC['cases'] if n != 'edges']


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize('name', GRADIENT_CASES)
def test_the_two_restatements_agree(name):
    t, spec = R.case_tensors(name, torch.float64)
    a, b = R.run_case(t, spec), R.run_case(t, spec, core=R.msda_grid_sample)
    assert sorted(a) == sorted(b) and len(a) == 4
    for k in a:
        assert _rel(a[k], b[k]) < 1e-12, k


def _one(value, shape, x, y, dtype=torch.float64):
    """One sample at (x, y) with weight 1 on a single level: out [D], d out.sum() / d (x, y)."""
    H, W = shape
    v = value.to(dtype).view(1, H * W, 1, -1)
    loc = torch.tensor([x, y], dtype=dtype).view(1, 1, 1, 1, 1, 2).requires_grad_(True)
    out = R.msda_scalar(v, [shape], loc, torch.ones(1, 1, 1, 1, 1, dtype=dtype))
    g, = torch.autograd.grad(out.sum(), loc)
    return out.detach().view(-1), g.view(2)


def test_restatement_rules_by_hand():
    torch.manual_seed(5)
    H, W, D = 4, 8, 3
    value = torch.randn(H * W, D, dtype=torch.float64)
    img = value.view(H, W, D)
    # a sample on a pixel centre returns that pixel
    out, _ = _one(value, (H, W), 2.5 / W, 1.5 / H)
    assert torch.equal(out, img[1, 2])
    # h = -1 exactly: strict inequality, zero output and a zero gradient (grid_sample has a non-zero one there)
    out, g = _one(value, (H, W), 2.7 / W, -0.5 / H)
    assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    out, g = _one(value, (H, W), -0.5 / W, 1.7 / H)
    assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    # just inside: only the first row, with a weight of 1/1024
    out, g = _one(value, (H, W), 2.5 / W, (-1 + 1 / 1024 + 0.5) / H)
    assert torch.allclose(out, img[0, 2] / 1024, rtol=1e-12) and torch.allclose(g[1], img[0, 2].sum() * H, rtol=1e-12)
    # wholly outside, NaN and infinity: zero, zero gradient
    for x, y in ((5.0, -3.0), (0.5, 1.0 + 0.5 / H), (float('nan'), 0.5), (0.5, float('inf'))):
        out, g = _one(value, (H, W), x, y)
        assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0, (x, y)
    # one row out: h = -0.5 takes half of row 0 and nothing else
    out, _ = _one(value, (H, W), 2.5 / W, 0.0)
    assert torch.allclose(out, 0.5 * img[0, 2], rtol=1e-13)
    # a 1 x 1 level: the pixel at its centre, a quarter of it on its corner, gradient -+ pixel / 2 there
    one = torch.tensor([[3.0, -2.0]], dtype=torch.float64)
    out, _ = _one(one, (1, 1), 0.5, 0.5)
    assert torch.equal(out, one[0])
    out, g = _one(one, (1, 1), 1.0, 1.0)
    assert torch.allclose(out, one[0] / 4, rtol=1e-13) and torch.allclose(g, torch.full((2,), -0.5, dtype=torch.float64), rtol=1e-13)
    # (W, H) order of the normaliser on a non-square level: an offset of (1, 0) pixels moves one COLUMN
    ref = torch.tensor([2.5 / W, 1.5 / H], dtype=torch.float64).view(1, 1, 1, 2)
    off = torch.tensor([1.0, 0.0], dtype=torch.float64).view(1, 1, 1, 1, 1, 2)
    loc, w = R.fused_to_plain([(H, W)], ref, off, torch.zeros(1, 1, 1, 1, dtype=torch.float64))
    assert float(w) == 1.0
    out = R.msda_scalar(value.view(1, H * W, 1, D), [(H, W)], loc, w)
    assert torch.allclose(out.view(-1), img[1, 3], rtol=1e-12)
    off = torch.tensor([0.0, 1.0], dtype=torch.float64).view(1, 1, 1, 1, 1, 2)
    out = R.msda_scalar(value.view(1, H * W, 1, D), [(H, W)], R.fused_to_plain([(H, W)], ref, off, torch.zeros(1, 1, 1, 1, dtype=torch.float64))[0], w)
    assert torch.allclose(out.view(-1), img[2, 2], rtol=1e-12)


def test_fixture_self_check():
    g = R.golden()
    assert SPEC['factor'] == 4 and SPEC['margin'] == R.MARGIN
    want_names = {'plain', 'decoder_small', 'edges', 'hot_cell', 'heads_d8_l1_p1', 'heads_d8_l8_p8', 'heads_d16_l8_p1', 'heads_d16_l1_p8',
                  'heads_d64_l1_p8', 'heads_d64_l8_p1'}
    assert set(SPEC['cases']) == want_names
    for name, spec in SPEC['cases'].items():
        t, _ = R.case_tensors(name, torch.float64)
        assert R.off_grid(t, spec, t.get('boundary')), name                      # the condition on the inputs
        assert sum(h * w for h, w in spec['shapes']) == t['value'].shape[1]
        got, want = R.run_case(t, spec), R.expected(name)
        assert sorted(got) == sorted(want)
        for k in want:
            assert want[k].dtype == torch.float64 and _rel(got[k], want[k]) < 1e-11, (name, k)
        assert spec['fixed_point_ratio'] <= 2 ** 16                           # csrc/msda.hip: the fixed-point error stays below 2^-25 max|grad_value|
    d = SPEC['cases']['decoder_small']
    assert (d['M'], d['D'], d['P'], d['Q'], d['shapes'], d['fused']) == (8, 32, 4, 126, [[2, 3], [4, 6], [8, 12]], True)
    p = SPEC['cases']['plain']
    assert (p['B'], p['M'], p['D'], p['Q'], p['P'], p['shapes']) == (2, 2, 32, 11, 2, [[5, 7], [3, 4]])
    h = SPEC['cases']['hot_cell']
    t, _ = R.case_tensors('hot_cell', torch.float64)
    hh, ww = R.case_hw(t, h)
    assert h['Q'] == 300 and bool(((hh > 1) & (hh < 2) & (ww > 2) & (ww < 3)).all())          # one cell
    assert float(t['w'].abs().max()) > 45 and float(t['grad_out'].abs().max()) > 500 and float(t['grad_out'].abs().min()) < 1e-5
    e, _ = R.case_tensors('edges')
    want = R.expected('edges')
    assert int(e['zero'].sum()) >= 10 and bool(torch.isnan(e['loc']).any())
    assert float(want['grad_loc'][e['zero']].abs().max()) == 0.0 and float(want['grad_attn'][e['zero']].abs().max()) == 0.0
    for q in R.QUANTITIES:
        assert 0 < R.tol(q) < 1e-4, q                                            # measured, positive, of the size of float32 rounding
    assert sorted(k for k in g if k.startswith('tol_')) == sorted(f'tol_{q}' for q in R.QUANTITIES)
    for f in (R.GOLDEN, R.GOLDEN_DECODER, R.GOLDEN_DECODER_IN):
        assert os.path.getsize(f) < 1 << 20, f


def test_fixture_tolerances_are_what_the_generator_measures():
    spec = importlib.util.spec_from_file_location('make_golden_msda', GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.FACTOR == SPEC['factor'] and gen.MODULE_CFG == SPEC['module']['cfg']
    for t, s in gen.all_cases():
        stored, _ = R.case_tensors(s['name'])
        for k, v in stored.items():
            assert torch.equal(torch.nan_to_num(t[k].float(), nan=7.0), torch.nan_to_num(v.float(), nan=7.0)), (s['name'], k)


def _module_pair():
    import boxinstseg_amd as B
    cfg, g = SPEC['module']['cfg'], R.golden()
    mine, ref = B.MultiScaleDeformableAttention(**cfg), R.RefMSDA(**cfg)
    state = {k[len('module_param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('module_param_')}
    return mine, ref, state


def test_module_state_dict_and_init_weights():
    import boxinstseg_amd as B
    torch.manual_seed(0)
    mine, ref, state = _module_pair()
    keys = sorted(f'{n}.{p}' for n in ('sampling_offsets', 'attention_weights', 'value_proj', 'output_proj') for p in ('weight', 'bias'))
    assert sorted(mine.state_dict()) == sorted(ref.state_dict()) == sorted(state) == keys
    assert all(mine.state_dict()[k].shape == ref.state_dict()[k].shape for k in keys)
    mine.load_state_dict(state)                                                                    # strict
    for cfg in (SPEC['module']['cfg'], dict(embed_dims=256, num_heads=8, num_levels=3, num_points=4)):
        a, b = B.MultiScaleDeformableAttention(**cfg), R.RefMSDA(**cfg)
        assert torch.allclose(a.sampling_offsets.bias, b.sampling_offsets.bias, rtol=0, atol=1e-6)
        M, L, P = cfg['num_heads'], cfg['num_levels'], cfg['num_points']
        grid = a.sampling_offsets.bias.view(M, L, P, 2)
        assert torch.allclose(grid[0, :, :, 0], torch.arange(1., P + 1).expand(L, P)) and float(grid[0, :, :, 1].abs().max()) < 1e-6     # head 0 looks along +x
        assert float(grid[:, :, 0].abs().amax(-1).sub(1).abs().max()) < 1e-6                     # the larger component of point 0 is 1
        for m in (a.sampling_offsets.weight, a.attention_weights.weight, a.attention_weights.bias, a.value_proj.bias, a.output_proj.bias):
            assert float(m.abs().max()) == 0.0
        for proj in (a.value_proj, a.output_proj):
            bound = math.sqrt(6.0 / (2 * cfg['embed_dims']))
            assert float(proj.weight.abs().max()) <= bound and float(proj.weight.std()) == pytest.approx(bound / math.sqrt(3), rel=0.1)
    assert isinstance(mine.dropout, torch.nn.Dropout) and mine.dropout.p == 0.0 and B.MultiScaleDeformableAttention().dropout.p == 0.1
    assert inspect.signature(B.MultiScaleDeformableAttention.__init__).parameters.keys() == inspect.signature(R.RefMSDA.__init__).parameters.keys() - {'core'}
    fwd = list(inspect.signature(B.MultiScaleDeformableAttention.forward).parameters)
    assert fwd == ['self', 'query', 'key', 'value', 'identity', 'query_pos', 'key_padding_mask', 'reference_points', 'spatial_shapes', 'level_start_index', 'kwargs']
    assert list(inspect.signature(B.multi_scale_deformable_attn).parameters) == ['value', 'spatial_shapes', 'level_start_index', 'sampling_locations',
                                                                                 'attention_weights', 'im2col_step']


def test_reference_config_block_builds_the_module():
    import boxinstseg_amd as B
    with open(R.CFG_JSON) as fh:
        stored = json.load(fh)
    configs = os.path.join(REFERENCE, 'configs/box2mask')
    if os.path.isdir(configs):
        for f in sorted(os.listdir(configs)):
            layer = B.load_config(os.path.join(configs, f))['model']['panoptic_head']['pixel_decoder']['encoder']['transformerlayers']
            assert layer['attn_cfgs'] == stored['attn_cfgs'], f'tests/golden/msda_cfg.json is not the attn_cfgs block of {f} any more'
    cfg = stored['attn_cfgs']
    assert cfg['type'] == 'MultiScaleDeformableAttention' and B.ATTENTION.get(cfg['type']) is B.MultiScaleDeformableAttention
    m = B.build_attention(cfg)
    assert isinstance(m, B.MultiScaleDeformableAttention) and isinstance(m, torch.nn.Module)
    assert (m.embed_dims, m.num_heads, m.num_levels, m.num_points, m.im2col_step, m.batch_first, m.dropout.p) == (256, 8, 3, 4, 64, False, 0.0)
    assert m.sampling_offsets.out_features == 8 * 3 * 4 * 2 and m.attention_weights.out_features == 8 * 3 * 4
    for name in ('multi_scale_deformable_attn', 'multi_scale_deformable_attn_fused', 'MultiScaleDeformableAttention', 'ATTENTION', 'build_attention'):
        assert name in B.__all__ and name in B.__doc__


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[msda]."""
    from boxinstseg_amd import _lib
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_msda.h')) as fh:
        code = fh.read()
    for macro, value in (('BXI_MSDA_MAX_LEVELS', _lib.MSDA_MAX_LEVELS), ('BXI_MSDA_MAX_POINTS', _lib.MSDA_MAX_POINTS),
                         ('BXI_MSDA_MIN_HEAD_DIM', _lib.MSDA_MIN_HEAD_DIM), ('BXI_MSDA_MAX_HEAD_DIM', _lib.MSDA_MAX_HEAD_DIM),
                         ('BXI_MSDA_FUSED', _lib.MSDA_FUSED), ('BXI_MSDA_MAX_CELL_SAMPLES', _lib.MSDA_MAX_CELL_SAMPLES)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', code).group(1)) == value, macro
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3i', 'multi_scale_deformable_attn_fused', 'unpinned', 'h = -1', 'grid_sample', 'build_attention', 'fixed point'):
        assert word in integration, word


def test_cpu_tensors_and_bad_arguments_fail_loudly():
    import boxinstseg_amd as B
    v, ss, ls = torch.zeros(1, 6, 2, 8), torch.tensor([[2, 3]]), torch.tensor([0])
    loc, w = torch.zeros(1, 4, 2, 1, 2, 2), torch.zeros(1, 4, 2, 1, 2)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.multi_scale_deformable_attn(v, ss, ls, loc, w)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.multi_scale_deformable_attn_fused(v, ss, ls, torch.zeros(1, 4, 1, 2), loc, torch.zeros(1, 4, 2, 2))
    m = B.MultiScaleDeformableAttention(embed_dims=16, num_heads=2, num_levels=1, num_points=2)
    with pytest.raises(RuntimeError, match='CUDA'):
        m(torch.zeros(6, 1, 16), reference_points=torch.zeros(1, 6, 1, 2), spatial_shapes=ss, level_start_index=ls, key_pos=None, attn_mask=None)
    with pytest.raises(ValueError, match='2 or 4'):
        m(torch.zeros(6, 1, 16), reference_points=torch.zeros(1, 6, 1, 3), spatial_shapes=ss, level_start_index=ls)
    with pytest.raises(RuntimeError, match='required'):
        m(torch.zeros(6, 1, 16))
    with pytest.raises(ValueError, match='divisible'):
        B.MultiScaleDeformableAttention(embed_dims=30, num_heads=4)
    for kw in (dict(embed_dims=24, num_heads=2), dict(embed_dims=8, num_heads=2), dict(embed_dims=256, num_heads=2),
               dict(num_levels=9), dict(num_points=9), dict(num_levels=0)):
        with pytest.raises(NotImplementedError, match='power of two'):
            B.MultiScaleDeformableAttention(**kw)
    # the checks that need no device run in front of the device check only where they can: exercise them through a fake `is_cuda`-free path
    from boxinstseg_amd import msda
    with pytest.raises(RuntimeError, match='add up'):
        msda._levels(torch.tensor([[2, 3], [1, 1]]), torch.tensor([0, 6]), 6, 'cpu')
    with pytest.raises(RuntimeError, match='running sum'):
        msda._levels(torch.tensor([[2, 3], [1, 1]]), torch.tensor([0, 5]), 7, 'cpu')
    with pytest.raises(RuntimeError, match='positive'):
        msda._levels(torch.tensor([[0, 3]]), torch.tensor([0]), 0, 'cpu')
    with pytest.raises(RuntimeError, match=r'\[L,2\]'):
        msda._levels(torch.tensor([2, 3]), torch.tensor([0]), 6, 'cpu')
    with pytest.raises(RuntimeError, match='level_start_index'):
        msda._levels(torch.tensor([[2, 3]]), torch.tensor([0, 1]), 6, 'cpu')
    assert msda._levels([(2, 3)], [0], 6, 'cpu')[2] == 1
    with pytest.raises(NotImplementedError, match='power of two'):
        msda._unsupported(2, 12, 1, 1)


def test_unsupported_status_names_the_header():
    from boxinstseg_amd import _lib, msda
    msda._status('bxi_msda_forward_f32', 0)
    with pytest.raises(NotImplementedError, match='^bxi_msda_forward_f32: outside the support set of include/boxinst/boxinst_hip_msda.h$'):
        msda._status('bxi_msda_forward_f32', _lib.BXI_ERR_UNSUPPORTED)
    with pytest.raises(_lib.BoxInstHipError, match='^bxi_msda_forward_f32: BXI_ERR_BAD_SHAPE -- '):
        msda._status('bxi_msda_forward_f32', -2)


def test_abi_validation_without_device():
    """Every call fails before its launch: X is a non-NULL value that nothing dereferences."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X, U = 0x1000, _lib.BXI_ERR_UNSUPPORTED
    fwd = lambda **k: lib.bxi_msda_forward_f32(k.get('v', X), X, k.get('st', X), X, k.get('off', X), X, k.get('B', 2), k.get('S', 47), k.get('M', 2),  # noqa: E731
                                               k.get('D', 32), k.get('Q', 11), k.get('L', 2), k.get('P', 2), k.get('flags', 0), k.get('out', X), None)
    assert fwd(B=-1) == -2 and fwd(S=-1) == -2 and fwd(M=0) == -2 and fwd(Q=-1) == -2 and fwd(L=0) == -2 and fwd(P=0) == -2 and fwd(D=0) == -2
    assert fwd(D=4) == U and fwd(D=24) == U and fwd(D=128) == U and fwd(L=9) == U and fwd(P=9) == U
    assert fwd(flags=2) == -3 and fwd(S=1 << 26) == -2 and fwd(Q=1 << 27) == -2
    assert fwd(v=None) == -1 and fwd(st=None) == -1 and fwd(out=None) == -1 and fwd(flags=1, off=None) == -1 and fwd(off=None, Q=0) == 0
    assert fwd(Q=0, out=None) == 0 and fwd(B=0, v=None, out=None) == 0                                      # no-ops: nothing is touched
    q = lib.bxi_msda_backward_workspace_bytes
    assert q(2, 47, 2, 32, 11, 2, 2) == 2 * 256 * 4 + 2 * 47 * 2 * 32 * 8 and q(2, 47, 2, 32, 0, 2, 2) == q(2, 47, 2, 32, 11, 2, 2)
    assert q(1, 0, 2, 32, 0, 2, 2) == 2048 and q(2, 47, 2, 24, 11, 2, 2) == 0 and q(2, 47, 2, 32, 11, 9, 2) == 0 and q(-1, 47, 2, 32, 11, 2, 2) == 0
    assert q(1, 47, 2, 32, (1 << 22) // 4, 2, 2) == 0 and q(1, 47, 2, 32, (1 << 22) // 4 - 1, 2, 2) > 0       # Q * L * P < 2^22
    need = q(2, 47, 2, 32, 11, 2, 2)
    bwd = lambda **k: lib.bxi_msda_backward_f32(k.get('g', X), X, X, X, X, k.get('off', X), X, 2, 47, 2, k.get('D', 32), k.get('Q', 11), 2, 2,  # noqa: E731
                                                k.get('flags', 0), k.get('gv', X), k.get('ga', X), X, k.get('ws', X), k.get('bytes', need), None)
    assert bwd(D=12) == U and bwd(flags=4) == -3 and bwd(Q=-1) == -2
    assert bwd(ws=None) == -5 and bwd(bytes=need - 1) == -5 and bwd(ws=X + 8) == -5
    assert bwd(gv=None) == -1 and bwd(g=None) == -1 and bwd(ga=None) == -1 and bwd(flags=1, off=None) == -1


@pytest.mark.parametrize('name,gmax,scale_b1', sorted(set(R.DYADIC_EXACT + R.DYADIC_BOUND)))
def test_dyadic_cases_are_exact_in_fp32(name, gmax, scale_b1):
    """The premise of the GPU file, for the restatement alone: every intermediate is exact in fp32, so the fp32 run IS the fp64 run."""
    t, spec = R.dyadic(name, gmax, scale_b1)
    arg = R.DYADIC[name]
    assert (spec['B'], spec['Q'], spec['M'], spec['D'], spec['P']) == (arg['B'], arg['Q'], arg['M'], arg['D'], arg['P'])
    assert all(v.dtype == torch.float32 for v in t.values()) and float(t['grad_out'].abs().max()) == gmax == float(t['grad_out'][0].abs().max())
    assert R.fixed_point_mx(t, spec) == gmax
    if scale_b1:
        assert 0 < float(t['grad_out'][1].abs().max()) <= gmax * 2.0 ** -scale_b1
    if spec['fused']:
        assert bool(((t['logits'] == 0).sum(-1) == 4).all()) and bool(((t['logits'] == 0) | (t['logits'] == float('-inf'))).all())
    else:
        assert float(t['w'].abs().max()) == 1.0
    r32, r64 = R.run_case(t, spec), R.run_case({k: v.double() for k, v in t.items()}, spec)
    assert sorted(r32) == sorted(r64) and len(r64) == 4
    for k in r64:
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
        assert bool(torch.isfinite(r64[k]).all()) and float(r64[k].abs().max()) > 0, k
        assert torch.equal(r64[k].float().double(), r64[k]), f'{k}: not representable in fp32'
        assert torch.equal(r32[k].view(torch.int32), r64[k].float().view(torch.int32)), k
    # some sample of every case is outside, some cell is hit more than once, and an Mx of 8 really is a power of two
    n = R.cell_hits([tuple(s) for s in spec['shapes']], R.plain_locations(t, spec), spec['B'], t['value'].shape[1], spec['M'])
    assert int(n.max()) > 1 and int(n.sum()) < 4 * spec['B'] * spec['Q'] * spec['M'] * len(spec['shapes']) * spec['P']


def test_cell_hits_by_hand():
    """Two levels, 2 x 2 and 1 x 1, one (b, q, m), six samples each.
    level 0: (.5, .5) h = w = .5, four corners inside -> cells 0 1 2 3;  (.25, .25) h = w = 0 on a pixel centre: the four corners still land
             inside (three of weight 0: an upper bound) -> 0 1 2 3;  (0, 0) h = w = -.5: only (0, 0) -> cell 0;  (-.25, .5) w = -1: does not
             count;  NaN: does not count;  (1, .25) w = 1.5, h = 0: (0, 1) and (1, 1) -> cells 1 3.          totals 3 3 2 3
    level 1: (.5, .5) h = w = 0: only (0, 0) -> cell 4;  (1, 1) h = w = .5: only (0, 0) -> cell 4;  (1.5, .5) w = 1 = W: does not count;
             (-.5, .5) w = -1: does not count;  (5, 5), (inf, .5): do not count.                                total 2"""
    nan, inf = float('nan'), float('inf')
    loc = torch.tensor([[(.5, .5), (.25, .25), (0., 0.), (-.25, .5), (nan, .5), (1., .25)],
                        [(.5, .5), (1., 1.), (1.5, .5), (-.5, .5), (5., 5.), (inf, .5)]], dtype=torch.float64).view(1, 1, 1, 2, 6, 2)
    n = R.cell_hits([(2, 2), (1, 1)], loc, 1, 5, 1)
    assert n.dtype == torch.int64 and tuple(n.shape) == (1, 5, 1) and n.view(-1).tolist() == [3, 3, 2, 3, 2]
    # B and M index the count: the same samples in batch 1, head 2 of a [2, 5, 3] count land there and nowhere else
    big = torch.full((2, 1, 3, 2, 6, 2), 9.0, dtype=torch.float64)
    big[1, 0, 2] = loc[0, 0, 0]
    n = R.cell_hits([(2, 2), (1, 1)], big, 2, 5, 3)
    assert n[1, :, 2].tolist() == [3, 3, 2, 3, 2] and int(n.sum()) == 13
    # fp32 locations count the same
    assert torch.equal(R.cell_hits([(2, 2), (1, 1)], loc.float(), 1, 5, 1), R.cell_hits([(2, 2), (1, 1)], loc, 1, 5, 1))
