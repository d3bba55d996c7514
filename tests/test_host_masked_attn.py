"""CPU: the host side of the masked attention (no kernel is launched here).

* statement (i) of tests/masked_attn_ref.py (torch's nn.MultiheadAttention) and its per-head restatement (ii) agree within 1e-12 in fp64, with
  identity and with random projections, with a 3-D, a 2-D and no mask;
* the fixture is what the restated statements of box2mask_head.py give now; its planted rows are what they were planted for;
* the limits of include/boxinst/boxinst_hip_attn.h are those of _lib, and INTEGRATION.md names the feature (the header against
  _lib.ATTN_SIGNATURES, the exports and the guarded tests: tests/test_abi_families.py);
* the attn_cfgs block of the transformer decoder of the reference's Box2Mask configs builds the module; its state-dict keys and shapes are
  those of nn.MultiheadAttention(256, 8) under ``attn.``;
* unsupported arguments fail before any launch."""
import inspect
import json
import os
import re

import pytest
import torch
from torch import nn

from tests import masked_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


@pytest.mark.parametrize('mask', ['3d', '2d', 'none'])
@pytest.mark.parametrize('params', ['identity', 'random'])
def test_the_two_statements_agree(params, mask):
    t = R.make_case(3, Q=9, S=37, D=16, B=2, M=2, mask=mask != 'none')
    m = t.get('mask')
    if mask == '2d':
        m = m[0]
    q, k, v = (t[n].double() for n in ('q', 'k', 'v'))
    p = R.identity_params(32) if params == 'identity' else R.random_params(32, 5)
    a, b = R.mha_torch(q, k, v, m, 2, p), R.attention_heads(q, k, v, m, 2, p)
    assert a.dtype == torch.float64 and float((a - b).abs().max()) < 1e-12 * max(1.0, float(a.abs().max()))
    if params == 'identity' and mask == 'none':                       # identity projections are exact: (i) is the core alone
        q32 = t['q']
        assert torch.equal(nn.functional.linear(q32, p['in_proj_weight'][:32].float(), p['in_proj_bias'][:32].float()), q32)


def test_fixture_is_what_the_statements_give_now():
    g = R.golden()
    assert os.path.getsize(R.GOLDEN) < 1 << 20
    pred, planted = torch.from_numpy(g['mask_pred']), torch.from_numpy(g['planted']).float()
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (2, 5, 64, 64) and torch.equal(planted, R.planted_mask_pred())
    assert sorted(k for k in g if k.startswith('bits_')) == sorted(f'bits_{n}' for n in R.MASK_CASES) and 'planted_bits_f8' in g
    for name, (H, W, h, w) in R.MASK_CASES.items():
        want = torch.from_numpy(g[f'bits_{name}'])
        got = R.pack_bits(R.box2mask_mask(pred, (h, w), R.MASK_HEADS))
        assert want.dtype == torch.int32 and tuple(want.shape) == (2 * R.MASK_HEADS, 5, (h * w + 31) // 32) and torch.equal(got, want), name
        if (h * w) % 32:
            assert bool((R.unpack_bits(want, want.shape[-1] * 32)[..., h * w:] == 0).all())      # tail bits clear
    want = R.unpack_bits(torch.from_numpy(g['planted_bits_f8']), 64).view(2, R.MASK_HEADS, 5, 64)
    assert torch.equal(R.pack_bits(R.box2mask_mask(planted, (8, 8), R.MASK_HEADS)), torch.from_numpy(g['planted_bits_f8']))
    v = R.resized(planted.double(), (8, 8))
    assert torch.equal(v, R.resized(planted, (8, 8)).double())      # weights 1/2 * 1/2 on integers: fp32 is exact
    assert bool((v[0, 1] < 0).all()) and not bool(want[0, :, 1].any())              # all negative: repaired to all clear
    assert float(v[0, 2, 0]) == 0.0 and float(v[0, 2, 8]) == 0.0 and not bool(want[0, 0, 2, 0]) and not bool(want[0, 0, 2, 8])     # exactly 0: kept
    assert not bool(want[1, :, 3].any()) and bool(want.any())
    assert torch.equal(want[:, 0], (v < 0) & ~(v < 0).all(-1, keepdim=True))      # on exact values the rule v < 0 IS the reference's


def test_pack_bits_by_hand():
    m = torch.zeros(2, 35, dtype=torch.bool)
    m[0, 0] = m[0, 31] = m[0, 32] = m[1, 34] = True
    b = R.pack_bits(m)
    assert b.tolist() == [[1 - 2 ** 31, 1], [0, 4]] and torch.equal(R.unpack_bits(b, 35), m)


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[attn]."""
    from boxinstseg_amd import _lib
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_attn.h')) as fh:
        code = fh.read()
    assert len(_lib.ATTN_SIGNATURES) == 6
    for macro, value in (('BXI_ATTN_SPAN', _lib.ATTN_SPAN), ('BXI_ATTN_MAX_Q', _lib.ATTN_MAX_Q), ('BXI_ATTN_MAX_S', _lib.ATTN_MAX_S),
                         ('BXI_ATTN_MAX_HEADS', _lib.ATTN_MAX_HEADS)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', code).group(1)) == value, macro
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        integration = fh.read()
    for word in ('Level 3l', 'box2mask_attn_mask', 'masked_attention', 'v < 0', 'not repeated', 'unpinned', 'build_attention', 'key_padding_mask'):
        assert word in integration, word
    assert 'v < 0' in code


def test_reference_config_block_builds_the_module():
    import boxinstseg_amd as B
    with open(R.CFG_JSON) as fh:
        stored = json.load(fh)
    configs = os.path.join(REFERENCE, 'configs/box2mask')
    if os.path.isdir(configs):
        for f in sorted(os.listdir(configs)):
            layer = B.load_config(os.path.join(configs, f))['model']['panoptic_head']['transformer_decoder']['transformerlayers']
            assert layer['attn_cfgs'] == stored['attn_cfgs'], f'tests/golden/masked_attn_cfg.json is not the attn_cfgs block of {f} any more'
    cfg = stored['attn_cfgs']
    assert cfg == dict(type='MultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.0, proj_drop=0.0, dropout_layer=None, batch_first=False)
    assert B.ATTENTION.get(cfg['type']) is B.MultiheadAttention
    m = B.build_attention(cfg)
    assert isinstance(m, B.MultiheadAttention) and isinstance(m, nn.Module) and isinstance(m.dropout_layer, nn.Identity)
    assert (m.embed_dims, m.num_heads, m.batch_first, m.proj_drop.p, m.attn.dropout) == (256, 8, False, 0.0, 0.0)
    want = nn.MultiheadAttention(256, 8).state_dict()
    got = m.state_dict()
    assert sorted(got) == sorted(f'attn.{k}' for k in want) == ['attn.in_proj_bias', 'attn.in_proj_weight', 'attn.out_proj.bias', 'attn.out_proj.weight']
    assert all(got[f'attn.{k}'].shape == want[k].shape for k in want)
    m.load_state_dict({f'attn.{k}': v for k, v in want.items()})              # strict
    ref = R.RefMultiheadAttention(**{k: v for k, v in cfg.items() if k != 'type'})
    assert sorted(ref.state_dict()) == sorted(got)
    assert float(m.attn.in_proj_bias.abs().max()) == 0.0 and float(m.attn.out_proj.bias.abs().max()) == 0.0     # torch's initialisation
    default = B.MultiheadAttention(64, 2)
    assert isinstance(default.dropout_layer, nn.Dropout) and default.dropout_layer.p == 0.0
    assert list(inspect.signature(B.MultiheadAttention.__init__).parameters) == list(inspect.signature(R.RefMultiheadAttention.__init__).parameters) == \
        ['self', 'embed_dims', 'num_heads', 'attn_drop', 'proj_drop', 'dropout_layer', 'init_cfg', 'batch_first', 'kwargs']
    assert list(inspect.signature(B.MultiheadAttention.forward).parameters) == \
        ['self', 'query', 'key', 'value', 'identity', 'query_pos', 'key_pos', 'attn_mask', 'key_padding_mask', 'kwargs']
    for name in ('PackedAttnMask', 'attn_mask_bits', 'box2mask_attn_mask', 'pack_attn_mask', 'masked_attention', 'MultiheadAttention'):
        assert name in B.__all__ and name in B.__doc__, name


def test_unsupported_arguments_fail_before_any_launch():
    import boxinstseg_amd as B
    with pytest.raises(ValueError, match='divisible'):
        B.MultiheadAttention(30, 4)
    for kw in (dict(embed_dims=24, num_heads=2), dict(embed_dims=256, num_heads=2), dict(embed_dims=16, num_heads=2)):
        with pytest.raises(NotImplementedError, match='head dimension'):
            B.MultiheadAttention(**kw)
    with pytest.raises(NotImplementedError, match='Dropout'):
        B.MultiheadAttention(64, 2, dropout_layer=dict(type='DropPath', drop_prob=0.1))
    with pytest.raises(NotImplementedError, match='kdim'):
        B.MultiheadAttention(64, 2, kdim=32)
    m = B.MultiheadAttention(64, 2)
    x, mem = torch.zeros(5, 1, 64), torch.zeros(7, 1, 64)
    with pytest.raises(NotImplementedError, match='CPU'):
        m(x, mem, mem)
    with pytest.raises(NotImplementedError, match='bool'):
        m(x, mem, mem, attn_mask=torch.zeros(5, 7))
    with pytest.raises(NotImplementedError, match='key_padding_mask'):
        m(x, mem, mem, key_padding_mask=torch.zeros(1, 7, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='half'):
        m.half()(x.half(), mem.half(), mem.half())
    drop = B.MultiheadAttention(64, 2, attn_drop=0.1)
    with pytest.raises(NotImplementedError, match='dropout'):
        drop(x, mem, mem)
    with pytest.raises(NotImplementedError, match='CPU'):             # in eval mode attention dropout is the identity: only the device is wrong
        drop.eval()(x, mem, mem)
    with pytest.raises(NotImplementedError, match='CPU'):
        B.masked_attention(x, mem, mem, None, 2)
    with pytest.raises(NotImplementedError, match='CPU'):
        B.attn_mask_bits(torch.zeros(1, 2, 8, 8), (4, 4))
    with pytest.raises(NotImplementedError, match='CPU'):
        B.pack_attn_mask(torch.zeros(5, 7, dtype=torch.bool), 2)
    with pytest.raises(NotImplementedError, match='bool'):
        B.pack_attn_mask(torch.zeros(5, 7), 2)


def test_unsupported_status_names_the_header():
    from boxinstseg_amd import _lib, masked_attn
    masked_attn._status('bxi_masked_attn_forward_f32', 0)
    with pytest.raises(NotImplementedError, match='^bxi_masked_attn_forward_f32: outside the support set of include/boxinst/boxinst_hip_attn.h$'):
        masked_attn._status('bxi_masked_attn_forward_f32', _lib.BXI_ERR_UNSUPPORTED)
    with pytest.raises(_lib.BoxInstHipError, match='^bxi_masked_attn_forward_f32: BXI_ERR_BAD_SHAPE -- '):
        masked_attn._status('bxi_masked_attn_forward_f32', -2)


def test_abi_validation_without_device():
    """Every call fails before its launch: X is a non-NULL value that nothing dereferences."""
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X, U = 0x1000, _lib.BXI_ERR_UNSUPPORTED
    fq, bq = lib.bxi_masked_attn_forward_workspace_bytes, lib.bxi_masked_attn_backward_workspace_bytes
    assert fq(2, 8, 100, 16384, 32) == 4 * 64 * 16 * 100 * 34 and bq(2, 8, 100, 16384, 32) == 4 * (16 * 100 + 64 * 16 * 100 * 32)
    assert fq(2, 2, 100, 35, 16) == 4 * 1 * 4 * 100 * 18 and fq(2, 2, 1, 257, 64) == 4 * 2 * 4 * 66
    assert fq(2, 2, 100, 35, 24) == 0 and bq(2, 2, 100, 35, 8) == 0 and fq(0, 2, 100, 35, 32) == 0 and bq(2, 2, 0, 35, 32) == 0 and fq(2, 2, 100, 0, 32) == 0
    assert fq(1, 1, _lib.ATTN_MAX_Q + 1, 35, 16) == 0 and fq(1, 1, 1, _lib.ATTN_MAX_S + 1, 16) == 0 and fq(256, 256, 1, 35, 16) == 0
    need = fq(2, 2, 100, 35, 32)
    fwd = lambda **k: lib.bxi_masked_attn_forward_f32(k.get('q', X), X, X, k.get('bits', X), k.get('ph', 0), 2, 2, k.get('Q', 100), k.get('S', 35),  # noqa: E731
                                                      k.get('D', 32), 0.25, k.get('out', X), X, k.get('ws', X), k.get('bytes', need), None)
    assert fwd(D=8) == U and fwd(D=48) == U and fwd(D=128) == U and fwd(Q=0) == -2 and fwd(S=0) == -2 and fwd(D=0) == -2 and fwd(ph=2) == -3
    assert fwd(q=None) == -1 and fwd(out=None) == -1 and fwd(ws=None) == -5 and fwd(bytes=need - 1) == -5 and fwd(ws=X + 8) == -5
    need = bq(2, 2, 100, 35, 32)
    bwd = lambda **k: lib.bxi_masked_attn_backward_f32(k.get('g', X), X, X, X, X, k.get('ph', 1), X, k.get('lse', X), 2, 2, k.get('Q', 100), 35,  # noqa: E731
                                                       k.get('D', 32), 0.25, k.get('dq', X), X, X, k.get('ws', X), k.get('bytes', need), None)
    assert bwd(D=12) == U and bwd(Q=-1) == -2 and bwd(ph=-1) == -3 and bwd(g=None) == -1 and bwd(lse=None) == -1 and bwd(dq=None) == -1
    assert bwd(ws=None) == -5 and bwd(bytes=need - 1) == -5 and bwd(ws=X + 4) == -5
    bits = lambda **k: lib.bxi_attn_mask_bits_f32(k.get('p', X), 2, k.get('Q', 5), 64, 64, k.get('h', 8), k.get('w', 8), k.get('bits', X), None)  # noqa: E731
    assert bits(Q=0) == -2 and bits(h=0) == -2 and bits(h=8192, w=4096) == -2 and bits(p=None) == -1 and bits(bits=None) == -1
    pack = lambda **k: lib.bxi_attn_pack_mask_u8(k.get('m', X), k.get('rows', 10), k.get('S', 35), k.get('bits', X), None)  # noqa: E731
    assert pack(rows=0) == -2 and pack(S=0) == -2 and pack(S=_lib.ATTN_MAX_S + 1) == -2 and pack(m=None) == -1 and pack(bits=None) == -1
