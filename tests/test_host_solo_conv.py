"""CPU: the host side of the dynamic mask convolution of the SOLOv2-style heads (no kernel is launched here).

* bxi_solo_dconv_forward_f32 / _backward_f32 validate their arguments before anything touches a device: every call below fails (or is a
  no-op) with pointers nothing dereferences -- every limit of the header, the NULL combinations, the workspace NULL / short / misaligned;
* the workspace size is monotone in N and in the tiles and 0 for what the entry point refuses;
* the constants of include/boxinst/boxinst_hip_dconv.h are those of _lib, _lib.DCONV_SIGNATURES holds the four entry points and the build
  lists the sources (the header against the table, the exports and the guarded tests: tests/test_abi_families.py);
* CPU tensors raise; the documents name the feature;
* tests/solo_conv_ref.py reproduces tests/golden/solo_conv.npz (which its generator ties to the reference's statements) and a case counted
  by hand."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import solo_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'solo_conv.npz')
X = 0x1000                                                                    # a pointer nothing dereferences


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _callers():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    d = dict(feat=X, B=2, E=5, H=7, W=9, maps=[X, X], grids=[3, 2], L=2, layout=0, cells=X, counts=[2, 1, 0, 1], N=4, act=1, out=X, img=X,
             status=X, gout=X, gfeat=X, gmaps=[X, X], ws=X)
    need = lib.bxi_solo_dconv_backward_workspace_bytes(4, 2, 5, 7, 9)
    need_fwd = lib.bxi_solo_dconv_forward_workspace_bytes(4, 2, 5)

    def arrays(a):
        maps = None if a['maps'] is None else _lib.ptr_array([m or 0 for m in a['maps']])
        grids = None if a['grids'] is None else _lib.int_array(a['grids'])
        counts = None if a['counts'] is None else _lib.int_array(a['counts'])
        return maps, grids, counts

    def fwd(**k):
        a = {**d, 'bytes': need_fwd, **k}
        maps, grids, counts = arrays(a)
        return lib.bxi_solo_dconv_forward_f32(a['feat'], a['B'], a['E'], a['H'], a['W'], maps, grids, a['L'], a['layout'], a['cells'], counts, a['N'],
                                              a['act'], a['out'], a['img'], a['status'], a['ws'], a['bytes'], None)

    def bwd(**k):
        a = {**d, 'bytes': need, **k}
        maps, grids, counts = arrays(a)
        gmaps = None if a['gmaps'] is None else _lib.ptr_array([m or 0 for m in a['gmaps']])
        return lib.bxi_solo_dconv_backward_f32(a['feat'], a['B'], a['E'], a['H'], a['W'], maps, grids, a['L'], a['layout'], a['cells'], counts, a['N'],
                                               a['act'], a['out'], a['gout'], a['gfeat'], gmaps, a['status'], a['ws'], a['bytes'], None)
    return lib, fwd, bwd, need, need_fwd


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib, fwd, bwd, need, need_fwd = _callers()
    assert need_fwd == 4 * (2 * 8 * 32) and _lib.DCONV_TILE == 64             # 4 / 32 + 2 chunks of 32 rows x 8 (E = 5 rounded up to 8)
    assert need == need_fwd + 4 * (1 * 4 * 5 + 4 * 5)                         # 63 pixels: one tile of partial sums, then the sums
    for call in (fwd, bwd):
        # the host arrays first
        for key in ('maps', 'grids', 'counts'):
            assert call(**{key: None}) == -1, key
        # 1 <= B <= BXI_MAX_IMAGES, 1 <= L <= 8, 1 <= E <= 1024, H, W >= 1, N >= 0
        assert call(B=0) == -2 and call(B=-1) == -2 and call(B=_lib.BXI_MAX_IMAGES + 1, counts=[0] * 130) == -2
        assert call(L=0) == -2 and call(L=9, maps=[X] * 9, grids=[2] * 9, counts=[0] * 18) == -2
        assert call(E=0) == -2 and call(E=1025) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(H=-7) == -2 and call(N=-1) == -2
        # B*E*H*W and N*H*W below 2^31; a map below 2^31 elements
        assert call(E=1024, H=1024, W=1024) == -2 and call(H=1 << 16, W=1 << 15) == -2
        assert call(E=1, H=1 << 12, W=1 << 12, N=128, counts=[128, 0, 0, 0]) == -2
        assert call(E=1024, grids=[1 << 10, 2]) == -2 and call(grids=[1 << 16, 2]) == -2
        # a grid below 1, a negative count, counts that do not sum to N
        assert call(grids=[0, 2]) == -2 and call(grids=[3, -2]) == -2
        assert call(counts=[2, 1, -1, 2]) == -2 and call(counts=[2, 1, 0, 0]) == -2 and call(N=5) == -2
        # layout and activation
        assert call(layout=2) == -3 and call(layout=-1) == -3 and call(act=2) == -3 and call(act=-1) == -3
        # the test-time layout is one matrix and one image
        assert call(layout=1) == -2 and call(layout=1, L=1, maps=[X], grids=[12], counts=[4, 0]) == -2
        # NULL device pointers, N > 0
        for key in ('out', 'status', 'cells'):
            assert call(**{key: None}) == -1, key
        assert call(maps=[X, None]) == -1
    # the limits themselves pass the shape checks: the next check answers
    assert fwd(E=1024, out=None) == -1 and fwd(B=_lib.BXI_MAX_IMAGES, counts=[4] + [0] * 127, out=None) == -1
    assert fwd(L=8, maps=[X] * 8, grids=[2] * 8, counts=[4] + [0] * 15, out=None) == -1 and fwd(E=1, H=1, W=1, out=None) == -1
    assert fwd(feat=None) == -1
    # the test-time layout needs no cells
    rows = dict(layout=1, L=1, B=1, maps=[X], grids=[12], counts=[4], gmaps=[X])
    assert fwd(**rows, cells=None, out=None) == -1 and fwd(**rows, cells=None, ws=None) == -5 and bwd(**rows, cells=None, ws=None) == -5
    # N == 0 touches nothing forward, whatever the pointers are
    zero = dict(N=0, counts=[0, 0, 0, 0])
    assert fwd(**zero, feat=None, cells=None, out=None, img=None, status=None, maps=[None, None], ws=None, bytes=0) == 0
    assert fwd(**zero, E=0) == -2 and fwd(**zero, act=5) == -3
    # backward: both gradients NULL is a checked no-op; the saved output and the upstream gradient; a NULL gradient map
    assert bwd(gfeat=None, gmaps=None, out=None, gout=None, ws=None, bytes=0) == 0 and bwd(gfeat=None, gmaps=None, E=0) == -2
    assert bwd(out=None) == -1 and bwd(gout=None) == -1 and bwd(gmaps=[X, None]) == -1
    assert bwd(feat=None) == -1 and bwd(feat=None, gmaps=None, gout=None) == -1          # grad_feat alone does not read the feature
    # the workspace: NULL, too small, not 16-byte aligned -- with N > 0, after the pointers
    for call, size in ((fwd, need_fwd), (bwd, need)):
        assert call(ws=None) == -5 and call(bytes=size - 1) == -5 and call(ws=X + 8) == -5 and call(ws=X + 4) == -5 and call(bytes=0) == -5
    assert bwd(ws=None, gmaps=None) == -5 and bwd(ws=None, gout=None) == -1
    assert bwd(N=0, counts=[0, 0, 0, 0], ws=None, bytes=0, gmaps=None, gfeat=None) == 0


def test_workspace_size():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    qf, q = lib.bxi_solo_dconv_forward_workspace_bytes, lib.bxi_solo_dconv_backward_workspace_bytes
    # forward: N / 32 + B chunks of 32 rows x E rounded up to a multiple of 8; backward adds one N x E block per tile of 64 pixels and one more
    assert qf(1, 1, 1) == 4 * 1 * 8 * 32 and qf(31, 1, 5) == 4 * 1 * 8 * 32 and qf(32, 1, 5) == 4 * 2 * 8 * 32 and qf(65, 3, 16) == 4 * 5 * 16 * 32
    assert q(1, 1, 1, 1, 1) == qf(1, 1, 1) + 8 and q(4, 2, 5, 7, 9) == qf(4, 2, 5) + 160 and q(4, 2, 5, 8, 8) == q(4, 2, 5, 7, 9)
    assert q(4, 2, 5, 5, 13) == qf(4, 2, 5) + 4 * 4 * 5 * 3
    by_n = [q(n, 2, 16, 24, 40) for n in range(0, 70)]
    assert by_n[0] == 0 and all(b > a for a, b in zip(by_n, by_n[1:]))
    fwd_by_n = [qf(n, 2, 16) for n in range(0, 70)]
    assert fwd_by_n[0] == 0 and all(b >= a for a, b in zip(fwd_by_n[1:], fwd_by_n[2:])) and fwd_by_n[69] > fwd_by_n[1]
    by_tiles = [q(7, 2, 16, h, 64) for h in range(1, 40)]
    assert all(b > a for a, b in zip(by_tiles, by_tiles[1:]))
    assert q(40, 2, 256, 200, 336) == 4 * (3 * 256 * 32 + 40 * 256 * (1050 + 1))
    for bad in ((0, 2, 5, 7, 9), (-1, 2, 5, 7, 9), (4, 0, 5, 7, 9), (4, 65, 5, 7, 9), (4, 2, 0, 7, 9), (4, 2, 1025, 7, 9), (4, 2, 5, 0, 9), (4, 2, 5, 7, 0),
                (1, 1, 5, 1 << 16, 1 << 15), (128, 1, 1, 1 << 12, 1 << 12)):
        assert q(*bad) == 0, bad
    assert qf(0, 2, 5) == 0 and qf(-1, 2, 5) == 0 and qf(4, 0, 5) == 0 and qf(4, 65, 5) == 0 and qf(4, 2, 0) == 0 and qf(4, 2, 1025) == 0


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[dconv]."""
    from boxinstseg_amd import _lib
    assert sorted(_lib.DCONV_SIGNATURES) == [
        'bxi_solo_dconv_backward_f32', 'bxi_solo_dconv_backward_workspace_bytes', 'bxi_solo_dconv_forward_f32', 'bxi_solo_dconv_forward_workspace_bytes']
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_dconv.h')) as fh:
        text = fh.read()
    for name in ('DCONV_MAPS', 'DCONV_ROWS', 'DCONV_NONE', 'DCONV_SIGMOID', 'DCONV_MAX_LEVELS', 'DCONV_MAX_E', 'DCONV_TILE', 'DCONV_STATUS_BAD_CELL'):
        assert re.search(r'#define BXI_' + name + r' (\d+)', text).group(1) == str(getattr(_lib, name)), name
    assert 'DEVIATION' in text and 'autocast' in text
    from boxinstseg_amd import build
    assert 'solo_dconv.hip' in build.SOURCES and any(h.endswith('boxinst_hip_dconv.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_documents_name_the_feature():
    import boxinstseg_amd as B
    for name in ('solo_dynamic_masks', 'solo_dynamic_masks_pair', 'solo_candidate_masks'):
        assert name in B.__all__ and name in B.__doc__ and callable(getattr(B, name))
    for rel, words in (('README.md', ('solo_dynamic_masks', 'solo_dconv')), ('DESIGN_NEXT_ROWS.md', ('solo_dconv', 'solo_dynamic_masks')),
                       ('INTEGRATION.md', ('solo_dynamic_masks', 'solo_dynamic_masks_pair', 'solo_candidate_masks', "conv='hip'", 'autocast')),
                       ('profiles/NOTES.md', ('R19-1', 'solo_dconv')), ('tools/README.md', ('solo_dconv_bench.py',))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert re.search(r'^#+ Level 3k.*solo_dynamic_masks', fh.read(), flags=re.M), 'INTEGRATION.md has no "Level 3k" heading for solo_dynamic_masks'
    assert inspect.signature(B.discobox_get_seg_single).parameters['conv'].default == 'torch'


def test_cpu_tensors_raise():
    import boxinstseg_amd as B
    case = R.make_case(1, 2, 5, 7, 9, [3], [[1, 1]])
    feat, maps, order, _ = R.to_torch(case, torch.float32)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_dynamic_masks(maps, order, feat)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_dynamic_masks_pair(maps, maps, order, feat, feat)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_candidate_masks(torch.rand(1, 5, 7, 9), torch.rand(4, 5), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match='conv'):
        B.discobox_get_seg_single(_FakeCuda(4, 2), _FakeCuda(1, 5, 7, 9), _FakeCuda(4, 5), (7, 9), {}, {}, [2], [8], conv='eager')


class _FakeCuda:
    """What need_cuda and len() ask of a tensor: the ``conv`` keyword is checked right behind them."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def __len__(self):
        return self.shape[0]


def test_restatement_reproduces_the_fixture():
    """The generator held tests/solo_conv_ref.py equal to the reference's statements, bit for bit, when it wrote the fixture; here the
    restatement must still give the fixture's fp64 values (1e-12: another BLAS may order a sum differently) from the fixture's inputs, the
    inputs must be what make_case draws, and the recorded bounds must be the rule's."""
    M = R
    z = np.load(GOLDEN)
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-13)                                        # noqa: E731
    for name, spec in M.CASES.items():
        case = R.make_case(**spec)
        assert np.array_equal(case['feat'], z[f'{name}/feat']) and np.array_equal(case['g'], z[f'{name}/g'])
        for l, m in enumerate(case['maps']):
            assert np.array_equal(m, z[f'{name}/map{l}'])
            for b, o in enumerate(case['order'][l]):
                assert np.array_equal(o, z[f'{name}/order{l}_{b}'])
        for sigmoid, tag in ((True, 'sig'), (False, 'lin')):
            out, gfeat, gmaps = R.run_ref(case, torch.float64, sigmoid)
            assert close(out, z[f'{name}/{tag}/out']) and close(gfeat, z[f'{name}/{tag}/gfeat'])
            assert all(close(gm, z[f'{name}/{tag}/gmap{l}']) for l, gm in enumerate(gmaps))
            for key in ('tol_out', 'tol_gfeat', 'tol_gmap'):
                assert 1e-8 < float(z[f'{name}/{tag}/{key}']) < 2e-6, key                # 4 x an fp32 rounding error, never a loose number
    assert int(sum(map(sum, M.CASES['b']['counts']))) == z['b/g'].shape[0] and len(set(z['b/order0_0'].tolist())) == 2    # the duplicate cell
    assert z['b/order0_1'].size == 0 and z['b/order1_1'].size == 0 and not z['b/sig/gfeat'][1].any()      # the image without instances
    seg, kern, rows = torch.from_numpy(z['test/seg']).double(), torch.from_numpy(z['test/kernels']).double(), torch.from_numpy(z['test/rows'])
    assert close(R.candidate_masks(seg, kern[rows]).numpy(), z['test/out']) and 1e-8 < float(z['test/tol_out']) < 2e-6
    # the training restatement and the test-time one are the same product
    feat, maps, order, _ = R.to_torch(R.make_case(**M.CASES['a']), torch.float64)
    lvl0 = R.dynamic_masks(maps, order, feat)[0][0]
    k0 = maps[0][0].view(5, -1)[:, order[0][0]].t()
    assert close(lvl0[:2].numpy(), R.candidate_masks(feat[:1], k0.contiguous()).numpy())


def test_a_case_counted_by_hand():
    """E = 2, one image of 1 x 2 pixels, one level with S = 1: logits = 5 [1, 2] - 6 [3, 4] = [-13, -14]; with the upstream gradient [1, -2]
    grad_feat = [[5, -10], [-6, 12]] and grad_kernel = [1 - 4, 3 - 8] = [-3, -5].  fp32 and fp64 agree exactly: integers."""
    case = dict(feat=np.array([[[[1, 2]], [[3, 4]]]], np.float32), maps=[np.array([[[[5]], [[-6]]]], np.float32)], order=[[np.array([0])]],
                g=np.array([[[1, -2]]], np.float32), grids=[1], N=1)
    for dtype in (torch.float32, torch.float64):
        out, gfeat, gmaps = R.run_ref(case, dtype, sigmoid=False)
        assert out.tolist() == [[[-13, -14]]] and gfeat.tolist() == [[[[5, -10]], [[-6, 12]]]] and gmaps[0].tolist() == [[[[-3]], [[-5]]]]
    # the same cell twice: two equal rows, and the cell's gradient is the sum of both rows'
    case['order'], case['g'], case['N'] = [[np.array([0, 0])]], np.array([[[1, -2]], [[2, 1]]], np.float32), 2
    out, gfeat, gmaps = R.run_ref(case, torch.float32, sigmoid=False)
    assert out.tolist() == [[[-13, -14]], [[-13, -14]]] and gmaps[0].tolist() == [[[[-3 + 4]], [[-5 + 10]]]]
    assert gfeat.tolist() == [[[[15, -5]], [[-18, 6]]]]
    # the exact cases of the GPU file stay below 2^24 whatever the order: 1024 * 15 * 15 and 2^14 * 15 * 7
    assert 1024 * 15 * 15 < 1 << 24 and (1 << 14) * 15 * 7 < 1 << 24 and 65 * 15 * 7 < 1 << 24
