"""CPU: the host side of the final-mask kernel of the SOLOv2-style heads (no kernel is launched here).

* bxi_seg_paste_u8 validates its arguments before anything touches a device: every call below fails (or is a no-op) with pointers nothing
  dereferences;
* the workspace size is one 16-byte record per mask, output row and chunk of 1024 columns, monotone in n, 0 for what the entry point refuses;
* _lib.SEG_SIGNATURES holds the two entry points and the build lists the sources (include/boxinst/boxinst_hip_seg.h against the table,
  the exports and the guarded tests: tests/test_abi_families.py);
* the documents name the feature; CPU tensors raise; the two restatements of tests/seg_paste_ref.py agree with torch's own fp32 composition
  under the tie rule and with a count by hand."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import matrix_nms_ref as R
from tests import seg_paste_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000
    d = dict(probs=X, n_all=5, h=13, w=21, keep=X, n=4, up_h=52, up_w=84, crop_h=50, crop_w=81, out_h=37, out_w=61, thr=0.5, masks=X, stats=X, ws=X)
    need = lib.bxi_seg_paste_workspace_bytes(4, 37, 61)
    assert need == 16 * 4 * 37

    def call(**k):
        a = {**d, 'bytes': need, **k}
        return lib.bxi_seg_paste_u8(a['probs'], a['n_all'], a['h'], a['w'], a['keep'], a['n'], a['up_h'], a['up_w'], a['crop_h'], a['crop_w'],
                                    a['out_h'], a['out_w'], a['thr'], a['masks'], a['stats'], a['ws'], a['bytes'], None)
    # a non-positive size, crop > up, n < 0
    for key in ('n_all', 'h', 'w', 'up_h', 'up_w', 'crop_h', 'crop_w', 'out_h', 'out_w'):
        assert call(**{key: 0}) == -2 and call(**{key: -3}) == -2, key
    assert call(crop_h=53) == -2 and call(crop_w=85) == -2 and call(n=-1) == -2
    assert call(crop_h=52, crop_w=84, ws=None) == -5                          # crop == up is fine: the next check answers
    # n * bands * chunks >= 2^31, n_all * h * w >= 2^31, out_h * out_w >= 2^31
    assert call(n=1 << 27, out_h=256, out_w=61) == -2 and call(n=1 << 20, out_h=1 << 14, out_w=2048) == -2
    assert call(n_all=1 << 23, h=16, w=16) == -2 and call(n_all=(1 << 23) - 1, h=16, w=16, ws=None) == -5
    assert call(out_h=1 << 16, out_w=1 << 15) == -2
    # a NaN threshold; n == 0 touches nothing, whatever the pointers are
    assert call(thr=float('nan')) == -3 and call(thr=float('nan'), n=0) == -3
    assert call(n=0, probs=None, keep=None, masks=None, stats=None, ws=None, bytes=0) == 0
    for key in ('probs', 'keep', 'masks', 'stats'):
        assert call(**{key: None}) == -1, key
    # the workspace: NULL, too small, not 16-byte aligned
    assert call(ws=None) == -5 and call(bytes=need - 1) == -5 and call(ws=X + 8) == -5
    # source rows that do not fit the staging buffer even for single output rows
    assert call(w=9000, up_w=36000, crop_w=81) == _lib.BXI_ERR_UNSUPPORTED


def test_workspace_size():
    from boxinstseg_amd import _lib
    q = _lib.load().bxi_seg_paste_workspace_bytes
    assert q(0, 37, 61) == 0 and q(1, 37, 61) == 16 * 37 and q(1, 37, 1024) == 16 * 37 and q(1, 37, 1025) == 2 * 16 * 37
    sizes = [q(n, 427, 640) for n in range(0, 130)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[100] == 100 * 427 * 16
    assert q(-1, 37, 61) == 0 and q(4, 0, 61) == 0 and q(4, 37, 0) == 0 and q(1 << 27, 256, 61) == 0 and q(1, 1 << 16, 1 << 15) == 0


def test_header_exports_and_signatures_agree():
    """The family's own half; the header against the table and the exports is tests/test_abi_families.py[seg]."""
    from boxinstseg_amd import _lib, build
    assert sorted(_lib.SEG_SIGNATURES) == ['bxi_seg_paste_u8', 'bxi_seg_paste_workspace_bytes']
    assert 'seg_paste.hip' in build.SOURCES and 'paste_device.hpp' in build.HEADERS


def test_documents_name_the_feature():
    import boxinstseg_amd as B
    for name in ('seg_paste', 'solo_get_seg', 'solo_format_results'):
        assert name in B.__all__ and name in B.__doc__ and callable(getattr(B, name))
    for rel, words in (('README.md', ('seg_paste',)), ('DESIGN_NEXT_ROWS.md', ('seg_paste',)),
                       ('INTEGRATION.md', ('seg_paste', 'solo_get_seg', 'solo_format_results', 'mask_stats')), ('profiles/NOTES.md', ('R18-1', 'seg_paste'))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert re.search(r'^#+ Level \w+.*seg_paste', fh.read(), flags=re.M), 'INTEGRATION.md has no "Level" heading for seg_paste'
    with open(os.path.join(ROOT, 'DESIGN_NEXT_ROWS.md')) as fh:
        assert 'A fused resize of the kept masks is not built' not in fh.read()


def test_cpu_tensors_raise():
    import types
    import boxinstseg_amd as B
    meta = dict(img_shape=(27, 33, 3), ori_shape=(40, 51, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.seg_paste(torch.rand(3, 7, 9), torch.tensor([0, 1]), (7, 9), meta, 0.5)
    res = types.SimpleNamespace(scores=torch.rand(2), labels=torch.tensor([0, 1]), masks=torch.zeros(2, 40, 51, dtype=torch.bool),
                                mask_stats=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_format_results(res, 2)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.solo_get_seg([torch.rand(1, 2, 2, 3)], None, [torch.rand(1, 4, 7, 9)], [meta],
                       dict(score_thr=0.1, mask_thr=0.5, filter_thr=0.05, nms_pre=500, max_per_img=100, kernel='gaussian', sigma=2.0), [2], [8], 3)


def test_the_restatements_agree_with_torch_fp32():
    """grid64 carries torch's own fp32 composition under the tie rule with no pixel in the band (what the parity cases of the GPU file rely
    on), the band against p64 has to be widened, and the count / box restatement matches a case counted by hand."""
    worst = 0.0
    for hw, crop, out in (((7, 9), (27, 33), (40, 51)), ((25, 38), (97, 150), (61, 93)), ((13, 21), (52, 84), (131, 200))):
        probs = R.disc_probs(np.random.default_rng(1), 4, *hw)
        keep, up = np.array([2, 0, 3]), (4 * hw[0], 4 * hw[1])
        x = F.interpolate(torch.from_numpy(probs[keep])[None], size=up, mode='bilinear')[:, :, :crop[0], :crop[1]]
        m32 = (F.interpolate(x, size=out, mode='bilinear')[0] > 0.5).numpy().astype(np.uint8)
        pg = S.check_tie(m32, probs, keep, up, crop, out, 0.5, str(hw), cap=1.0)
        worst = max(worst, float(np.abs(pg - S.p64(probs, keep, up, crop, out)).max()))
    assert 1e-6 < worst < 1e-5                                                # the fp32 tap positions alone move p by more than the plain band
    assert np.array_equal(S.p64(probs, [-1, 9], up, crop, out), np.zeros((2, *out)))          # an index outside the candidates: a zero plane
    m = np.zeros((3, 5, 7), np.uint8)
    m[1, 2:4, 3:6] = 1
    m[2, 4, 0] = 1
    assert S.stats_of(m).tolist() == [[0, -1, -1, -1, -1], [6, 3, 2, 5, 3], [1, 0, 4, 0, 4]]
    boxes, (masks, scores) = S.format_results(torch.tensor([1, 1, 0]), torch.tensor([0.5, 0.25, 0.125]), torch.from_numpy(m).bool(), 3)
    assert boxes[0].tolist() == [[0, 4, 1, 5, 0.125]] and boxes[1].tolist() == [[3, 2, 6, 4, 0.25]] and boxes[2].shape == (0, 5)
    assert [len(x) for x in masks] == [1, 1, 0] and float(scores[1][0]) == 0.25
