"""CPU: the host side of the half-precision dynamic mask convolution (no kernel is launched here).

* the constants of include/boxinst/boxinst_hip_dconv16.h are those of _lib, _lib.DCONV16_SIGNATURES holds exactly the four entry points
  and the build lists the source and the header;
* bxi_solo_dconv16_forward / _backward validate their arguments before anything touches a device, in the stated order: every call below
  fails (or is a no-op) with pointers nothing dereferences;
* the workspace sizes are monotone in N, 0 for N == 0 and for refused sizes;
* the Python surface raises on CPU tensors, on fp32 input with compute='half', on mixed dtypes and on an unknown compute or conv; the
  defaults are unchanged; the documents point to the new path."""
import inspect
import os
import re

import pytest
import torch

from tests import solo_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000                                                                    # a pointer nothing dereferences


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _callers():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    d = dict(feat=X, dtype=0, B=2, E=5, H=7, W=9, maps=[X, X], grids=[3, 2], L=2, layout=0, cells=X, counts=[2, 1, 0, 1], N=4, act=1, out=X,
             odt=0, img=X, status=X, gout=X, gfeat=X, gmaps=[X, X], ws=X)
    need = lib.bxi_solo_dconv16_backward_workspace_bytes(4, 2, 5, 7, 9)
    need_fwd = lib.bxi_solo_dconv16_forward_workspace_bytes(4, 2, 5)

    def arrays(a):
        maps = None if a['maps'] is None else _lib.ptr_array([m or 0 for m in a['maps']])
        grids = None if a['grids'] is None else _lib.int_array(a['grids'])
        counts = None if a['counts'] is None else _lib.int_array(a['counts'])
        return maps, grids, counts

    def fwd(**k):
        a = {**d, 'bytes': need_fwd, **k}
        maps, grids, counts = arrays(a)
        return lib.bxi_solo_dconv16_forward(a['feat'], a['dtype'], a['B'], a['E'], a['H'], a['W'], maps, grids, a['L'], a['layout'], a['cells'], counts,
                                            a['N'], a['act'], a['out'], a['odt'], a['img'], a['status'], a['ws'], a['bytes'], None)

    def bwd(**k):
        a = {**d, 'bytes': need, **k}
        maps, grids, counts = arrays(a)
        gmaps = None if a['gmaps'] is None else _lib.ptr_array([m or 0 for m in a['gmaps']])
        return lib.bxi_solo_dconv16_backward(a['feat'], a['dtype'], a['B'], a['E'], a['H'], a['W'], maps, grids, a['L'], a['layout'], a['cells'], counts,
                                             a['N'], a['act'], a['out'], a['gout'], a['odt'], a['gfeat'], gmaps, a['status'], a['ws'], a['bytes'], None)
    return lib, fwd, bwd, need, need_fwd


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib, fwd, bwd, need, need_fwd = _callers()
    assert need_fwd == 2 * (2 * 16 * 32) and _lib.DCONV16_TILE == 64          # 4 / 32 + 2 chunks of 32 rows x 16 (E = 5 rounded up to 16)
    assert need == need_fwd + 4 * (1 * 4 * 5 + 4 * 5)                         # 63 pixels: one tile of partial sums, then the sums
    for call in (fwd, bwd):
        for key in ('maps', 'grids', 'counts'):                               # the host arrays first, before the shape and the types
            assert call(**{key: None}) == -1 and call(**{key: None}, E=0, dtype=7) == -1, key
        assert call(B=0) == -2 and call(B=_lib.BXI_MAX_IMAGES + 1, counts=[0] * 130) == -2
        assert call(L=0) == -2 and call(L=9, maps=[X] * 9, grids=[2] * 9, counts=[0] * 18) == -2
        assert call(E=0) == -2 and call(E=1025) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(N=-1) == -2
        assert call(E=1024, H=1024, W=1024) == -2 and call(H=1 << 16, W=1 << 15) == -2
        assert call(grids=[0, 2]) == -2 and call(counts=[2, 1, -1, 2]) == -2 and call(counts=[2, 1, 0, 0]) == -2 and call(N=5) == -2
        assert call(layout=2) == -3 and call(act=2) == -3 and call(act=-1) == -3
        assert call(layout=1) == -2 and call(layout=1, L=1, maps=[X], grids=[12], counts=[4, 0]) == -2
        # the shape is answered before the types, the types before the device pointers and the workspace
        assert call(E=0, dtype=7) == -2 and call(layout=2, dtype=7) == -3
        for bad in (dict(dtype=-1), dict(dtype=2), dict(dtype=3), dict(odt=-1), dict(odt=3), dict(dtype=0, odt=1), dict(dtype=1, odt=0)):
            assert call(**bad) == -3 and call(**bad, out=None, ws=None) == -3, bad
        for good in (dict(dtype=0, odt=0), dict(dtype=0, odt=2), dict(dtype=1, odt=1), dict(dtype=1, odt=2)):
            assert call(**good, out=None) == -1 and call(**good, ws=None) == -5, good
        for key in ('out', 'status', 'cells'):
            assert call(**{key: None}) == -1, key
        assert call(maps=[X, None]) == -1
    assert fwd(E=1024, out=None) == -1 and fwd(feat=None) == -1
    rows = dict(layout=1, L=1, B=1, maps=[X], grids=[12], counts=[4], gmaps=[X])
    assert fwd(**rows, cells=None, out=None) == -1 and fwd(**rows, cells=None, ws=None) == -5 and bwd(**rows, cells=None, ws=None) == -5
    # N == 0 touches nothing forward, whatever the pointers are -- but the types are still checked
    zero = dict(N=0, counts=[0, 0, 0, 0])
    assert fwd(**zero, feat=None, cells=None, out=None, img=None, status=None, maps=[None, None], ws=None, bytes=0) == 0
    assert fwd(**zero, E=0) == -2 and fwd(**zero, act=5) == -3 and fwd(**zero, dtype=5) == -3
    assert bwd(gfeat=None, gmaps=None, out=None, gout=None, ws=None, bytes=0) == 0 and bwd(gfeat=None, gmaps=None, odt=5) == -3
    assert bwd(out=None) == -1 and bwd(gout=None) == -1 and bwd(gmaps=[X, None]) == -1
    assert bwd(feat=None) == -1 and bwd(feat=None, gmaps=None, gout=None) == -1          # grad_feat alone does not read the feature
    for call, size in ((fwd, need_fwd), (bwd, need)):
        assert call(ws=None) == -5 and call(bytes=size - 1) == -5 and call(ws=X + 8) == -5 and call(ws=X + 2) == -5 and call(bytes=0) == -5
    assert bwd(ws=None, gmaps=None) == -5 and bwd(ws=None, gout=None) == -1
    assert bwd(N=0, counts=[0, 0, 0, 0], ws=None, bytes=0, gmaps=None, gfeat=None) == 0


def test_workspace_size():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    qf, q = lib.bxi_solo_dconv16_forward_workspace_bytes, lib.bxi_solo_dconv16_backward_workspace_bytes
    # forward: N / 32 + B chunks of 32 rows x E rounded up to 16 halves; backward adds one fp32 N x E block per tile of 64 pixels and one more
    assert qf(1, 1, 1) == 2 * 16 * 32 and qf(31, 1, 5) == 2 * 16 * 32 and qf(32, 1, 5) == 2 * 2 * 16 * 32 and qf(65, 3, 17) == 2 * 5 * 32 * 32
    assert q(1, 1, 1, 1, 1) == qf(1, 1, 1) + 8 and q(4, 2, 5, 7, 9) == qf(4, 2, 5) + 160 and q(4, 2, 5, 8, 8) == q(4, 2, 5, 7, 9)
    assert q(4, 2, 5, 5, 13) == qf(4, 2, 5) + 4 * 4 * 5 * 3
    by_n = [q(n, 2, 16, 24, 40) for n in range(0, 70)]
    assert by_n[0] == 0 and all(b > a for a, b in zip(by_n, by_n[1:]))
    fwd_by_n = [qf(n, 2, 16) for n in range(0, 70)]
    assert fwd_by_n[0] == 0 and all(b >= a for a, b in zip(fwd_by_n[1:], fwd_by_n[2:])) and fwd_by_n[69] > fwd_by_n[1]
    assert q(40, 2, 256, 200, 336) == 2 * 3 * 256 * 32 + 4 * 40 * 256 * (1050 + 1)
    assert qf(40, 2, 256) * 2 == lib.bxi_solo_dconv_forward_workspace_bytes(40, 2, 256)                   # half the fp32 family's bytes
    for bad in ((0, 2, 5, 7, 9), (-1, 2, 5, 7, 9), (4, 0, 5, 7, 9), (4, 65, 5, 7, 9), (4, 2, 0, 7, 9), (4, 2, 1025, 7, 9), (4, 2, 5, 0, 9), (4, 2, 5, 7, 0),
                (1, 1, 5, 1 << 16, 1 << 15), (128, 1, 1, 1 << 12, 1 << 12)):
        assert q(*bad) == 0, bad
    assert qf(0, 2, 5) == 0 and qf(-1, 2, 5) == 0 and qf(4, 0, 5) == 0 and qf(4, 65, 5) == 0 and qf(4, 2, 0) == 0 and qf(4, 2, 1025) == 0


def test_header_table_and_build_agree():
    from boxinstseg_amd import _lib, build
    assert sorted(_lib.DCONV16_SIGNATURES) == ['bxi_solo_dconv16_backward', 'bxi_solo_dconv16_backward_workspace_bytes',
                                               'bxi_solo_dconv16_forward', 'bxi_solo_dconv16_forward_workspace_bytes']
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_dconv16.h')) as fh:
        text = fh.read()
    for name in ('DCONV16_F16', 'DCONV16_BF16', 'DCONV16_OUT_F32', 'DCONV16_TILE'):
        assert re.search(r'#define BXI_' + name + r' (\d+)', text).group(1) == str(getattr(_lib, name)), name
    assert len({_lib.DCONV16_F16, _lib.DCONV16_BF16, _lib.DCONV16_OUT_F32}) == 3
    for word in ('autocast', 'fmaf chain', 'subnormal', 'v_mfma_f32_32x32x16', 'depends only on its own kernel values'):
        assert word in text, word
    assert 'solo_dconv16.hip' in build.SOURCES and any(h.endswith('boxinst_hip_dconv16.h') for h in build.HEADERS)
    assert 'solo_dconv_device.hpp' in build.HEADERS and all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)


class _FakeCuda:
    """What need_cuda and len() ask of a tensor: the ``conv`` keyword is checked right behind them."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def __len__(self):
        return self.shape[0]


def test_the_python_surface_raises():
    import boxinstseg_amd as B
    case = R.make_case(1, 2, 5, 7, 9, [3], [[1, 1]])
    for dtype in (torch.float16, torch.bfloat16):
        feat, maps, order, _ = R.to_torch(case, dtype)
        with pytest.raises(RuntimeError, match='CUDA'):                       # half tensors on the CPU: there is no fallback
            B.solo_dynamic_masks(maps, order, feat, compute='half')
        with pytest.raises(RuntimeError, match='CUDA'):
            B.solo_dynamic_masks_pair(maps, maps, order, feat, feat, compute='half')
        with pytest.raises(RuntimeError, match='CUDA'):
            B.solo_candidate_masks(feat[:1], torch.rand(4, 5).to(dtype), torch.tensor([0, 1]), compute='half')
        # mixed dtypes: said before a device is asked for; nothing is cast
        other = torch.float32 if dtype == torch.float16 else torch.float16
        with pytest.raises(RuntimeError, match='one half dtype'):
            B.solo_dynamic_masks([m.to(other) for m in maps], order, feat, compute='half')
        with pytest.raises(RuntimeError, match='one half dtype'):
            B.solo_dynamic_masks_pair(maps, maps, order, feat, feat.to(other), compute='half')
        with pytest.raises(RuntimeError, match='one half dtype'):
            B.solo_candidate_masks(feat[:1], torch.rand(4, 5).to(other), compute='half')
        with pytest.raises(RuntimeError, match='out_dtype'):
            B.solo_dynamic_masks(maps, order, feat, compute='half', out_dtype=torch.float64)
        with pytest.raises(RuntimeError, match='out_dtype'):
            B.solo_dynamic_masks(maps, order, feat, compute='half', out_dtype=torch.bfloat16 if dtype == torch.float16 else torch.float16)
    feat, maps, order, _ = R.to_torch(case, torch.float32)
    with pytest.raises(RuntimeError, match='one half dtype'):                 # fp32 input: no silent cast
        B.solo_dynamic_masks(maps, order, feat, compute='half')
    with pytest.raises(RuntimeError, match='one half dtype'):
        B.solo_candidate_masks(torch.rand(1, 5, 7, 9), torch.rand(4, 5), compute='half')
    with pytest.raises(RuntimeError, match='out_dtype'):
        B.solo_dynamic_masks(maps, order, feat, out_dtype=torch.float16)
    for call in (lambda: B.solo_dynamic_masks(maps, order, feat, compute='fp16'),
                 lambda: B.solo_dynamic_masks_pair(maps, maps, order, feat, feat, compute='bf16'),
                 lambda: B.solo_candidate_masks(torch.rand(1, 5, 7, 9), torch.rand(4, 5), compute=None)):
        with pytest.raises(ValueError, match='compute'):
            call()
    with pytest.raises(ValueError, match='conv'):
        B.discobox_get_seg_single(_FakeCuda(4, 2), _FakeCuda(1, 5, 7, 9), _FakeCuda(4, 5), (7, 9), {}, {}, [2], [8], conv='half')


def test_defaults_and_documents():
    import boxinstseg_amd as B
    from boxinstseg_amd import solo_conv
    for fn in (B.solo_dynamic_masks, B.solo_dynamic_masks_pair, B.solo_candidate_masks):
        p = inspect.signature(fn).parameters
        assert p['compute'].default == 'fp32' and p['out_dtype'].default is None
    assert inspect.signature(B.discobox_get_seg_single).parameters['conv'].default == 'torch'
    assert "compute='half'" in solo_conv.__doc__ and 'solo_dconv16' in solo_conv.__doc__ and 'solo_dconv16' in B.__doc__
    for rel, words in (('README.md', ('solo_dconv16', "compute='half'")), ('DESIGN_NEXT_ROWS.md', ('solo_dconv16',)),
                       ('INTEGRATION.md', ("compute='half'", "conv='hip_half'")), ('profiles/NOTES.md', ('R26-1', 'solo_dconv16')),
                       ('include/boxinst/boxinst_hip_dconv.h', ('boxinst_hip_dconv16.h',)), ('tools/README.md', ('solo_dconv16_bench.py',))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)
