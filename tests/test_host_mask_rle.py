"""CPU: COCO's run-length encoding as tests/rle_ref.py restates it, the host half of boxinstseg_amd.mask_rle (rle_decode, the capacity
rule, the shape check) and the argument checks of bxi_mask_rle_u8 (no kernel is launched here).

The restatement is UNPINNED -- pycocotools never ran next to it -- so the hand cases below, worked out from the published algorithm, are
what holds it: single counts at the 1 / 2 / 3 character thresholds, a negative delta, and the 2 x 4 mask 0000 / 0101."""
import os

import numpy as np
import pytest
import torch

from tests import rle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _blobs(rng, n, h, w):
    """Seeded masks: unions of a few discs, some with a hole."""
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, max(2, min(h, w) / 2))
            d = (yy - cy) ** 2 + (xx - cx) ** 2
            out[i] |= (d <= r * r).astype(np.uint8)
            if rng.random() < 0.5:
                out[i] &= ~(d <= (r / 3) ** 2)
    return out


def test_hand_cases():
    for cnts, s in (([6], b'6'), ([0, 6], b'06'), ([15], b'?'), ([16], b'`0'), ([31], b'o0'), ([3, 1, 3, 1], b'3130')):
        assert R.rle_to_string(cnts) == s, cnts
        assert R.rle_from_string(s) == cnts
    # a delta of -1: the fourth count is one less than the second
    assert R.rle_to_string([5, 5, 5, 4]) == b'555O' and R.rle_from_string(b'555O') == [5, 5, 5, 4]
    m = np.array([[0, 0, 0, 0], [0, 1, 0, 1]], np.uint8)
    assert R.rle_counts(m) == [3, 1, 3, 1] and R.encode(m) == {'size': [2, 4], 'counts': b'3130'}
    assert R.rle_counts(np.zeros((2, 3))) == [6] and R.rle_counts(np.ones((2, 3))) == [0, 6]
    one = np.zeros((3, 2), np.uint8)
    one[0, 0] = 1
    assert R.rle_counts(one) == [0, 1, 5]
    one[:] = 0
    one[2, 1] = 7                                                             # any non-zero byte is a set pixel
    assert R.rle_counts(one) == [5, 1]


def test_character_thresholds():
    """A value needs k characters while it fits k 5-bit groups with a sign bit to spare: 1 up to 15, 2 up to 511, 3 up to 16383."""
    for v, k in ((15, 1), (16, 2), (511, 2), (512, 3), (16383, 3), (16384, 4), ((1 << 29) - 1, 6)):
        s = R.rle_to_string([v])
        assert len(s) == k and R.rle_from_string(s) == [v], v
    for d, k in ((-1, 1), (-16, 1), (-17, 2), (-512, 2), (-513, 3), (-16384, 3), (-16385, 4)):
        cnts = [1, 20000, 1, 20000 + d]
        s = R.rle_to_string(cnts)
        assert len(s) == 1 + 4 + 1 + k and R.rle_from_string(s) == cnts, d


def test_round_trip_and_sums():
    from boxinstseg_amd import rle_decode
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 9), (9, 1), (7, 5), (64, 3), (65, 66), (40, 56)):
        masks = np.concatenate([_blobs(rng, 4, h, w), (rng.random((2, h, w)) < 0.5).astype(np.uint8), np.zeros((1, h, w), np.uint8),
                                np.ones((1, h, w), np.uint8)])
        rles = []
        for m in masks:
            cnts = R.rle_counts(m)
            assert cnts == R.rle_counts_fast(m) and sum(cnts) == h * w and all(c > 0 for c in cnts[1:])
            rle = R.encode(m)
            assert np.array_equal(R.decode(rle), m != 0)
            rles.append(rle)
        got = rle_decode(rles)
        assert got.dtype == np.bool_ and got.shape == masks.shape and np.array_equal(got, masks != 0)
        assert np.array_equal(rle_decode([dict(r, counts=r['counts'].decode()) for r in rles]), masks != 0)     # str counts, as json gives them
    assert rle_decode([]).shape == (0, 0, 0)
    with pytest.raises(RuntimeError, match='do not tile'):
        rle_decode([{'size': [2, 4], 'counts': b'313'}])
    with pytest.raises(RuntimeError, match='sizes differ'):
        rle_decode([{'size': [2, 4], 'counts': b'3130'}, {'size': [4, 2], 'counts': b'3130'}])


def test_packed_and_stats_helpers():
    m = np.zeros((3, 5, 7), np.uint8)
    m[1, 2:4, 3:6] = 1
    m[2, 4, 0] = 1
    ro, counts, co, chars = R.packed(m)
    assert ro.tolist() == [0, 1, 8, 11] and counts.tolist() == [35, 17, 2, 3, 2, 3, 2, 6, 4, 1, 30]
    mid = R.rle_to_string([17, 2, 3, 2, 3, 2, 6])
    assert mid == b'a0230003' and co.tolist() == [0, 2, 10, 14] and bytes(chars) == b'S1' + mid + b'41n0'     # 17 and 30 carry bit 4: two characters
    assert R.stats_of(m).tolist() == [[0, -1, -1, -1, -1], [6, 3, 2, 5, 3], [1, 0, 4, 0, 4]]


def test_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000
    need = lib.bxi_mask_rle_workspace_bytes(3, 65, 70)
    r16 = lambda b: (b + 15) // 16 * 16                                       # every array starts on a multiple of 16 bytes
    assert need == r16(3 * 2 * 70 * 8) + 3 * 70 * 16 + r16(3 * 70 * 4) + r16(3 * 8) and need % 16 == 0      # bit words, column records, first characters, totals

    def call(**k):
        a = dict(masks=X, n=3, h=65, w=70, stats=None, cap_runs=10, cap_chars=10, ro=X, counts=X, co=X, chars=X, status=X, ws=X, bytes=need)
        a.update(k)
        return lib.bxi_mask_rle_u8(a['masks'], a['n'], a['h'], a['w'], a['stats'], a['cap_runs'], a['cap_chars'], a['ro'], a['counts'], a['co'],
                                   a['chars'], a['status'], a['ws'], a['bytes'], None)
    assert call(n=-1) == -2 and call(h=0) == -2 and call(w=0) == -2 and call(cap_runs=-1) == -2 and call(cap_chars=-1) == -2
    # h * w >= 2^29 is refused by argument alone; so is a batch whose worst case leaves an int32 offset
    assert call(n=1, h=1 << 15, w=1 << 14) == _lib.BXI_ERR_UNSUPPORTED and call(n=1, h=1 << 29, w=1) == _lib.BXI_ERR_UNSUPPORTED
    assert call(n=0, h=1 << 15, w=1 << 14) == _lib.BXI_ERR_UNSUPPORTED
    assert call(n=1200, h=480, w=640) == _lib.BXI_ERR_UNSUPPORTED
    assert lib.bxi_mask_rle_workspace_bytes(1, 1 << 15, 1 << 14) == 0 and lib.bxi_mask_rle_workspace_bytes(-1, 4, 4) == 0
    for key in ('masks', 'ro', 'counts', 'co', 'chars', 'status'):
        assert call(**{key: None}) == -1, key
    assert call(ws=None) == -5 and call(bytes=need - 1) == -5 and call(ws=X + 8) == -5
    # capacities of zero need no buffers: the next check answers
    assert call(cap_runs=0, counts=None, cap_chars=0, chars=None, ws=None) == -5
    sizes = [lib.bxi_mask_rle_workspace_bytes(n, 480, 640) for n in range(0, 110)]
    assert sizes[0] == 0 and all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[100] == 100 * (8 * 640 * 8 + 640 * 20 + 8)


def test_surface_without_device():
    import boxinstseg_amd as B
    from boxinstseg_amd import _lib, build, mask_rle
    assert sorted(_lib.RLE_SIGNATURES) == ['bxi_mask_rle_u8', 'bxi_mask_rle_workspace_bytes']
    assert 'mask_rle.hip' in build.SOURCES and any(h.endswith('boxinst_hip_rle.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, p)) for p in build.SOURCES + build.HEADERS)
    for name in ('rle_encode', 'rle_decode', 'solo_encode_results', 'box2mask_encode_results'):
        assert name in B.__all__ and name in B.__doc__ and getattr(B, name) is getattr(mask_rle, name), name
    # the capacity rule as documented, and the refusal before anything is allocated
    assert mask_rle.default_capacities(100, 480, 640) == (100 * 1282, 2 * 100 * 1282) and mask_rle.default_capacities(3, 1, 1) == (6, 12)
    assert mask_rle.default_capacities(0, 5, 5) == (0, 0)
    with pytest.raises(NotImplementedError, match='boxinst_hip_rle.h'):
        mask_rle.check_shape(1, 1 << 15, 1 << 14)
    with pytest.raises(NotImplementedError):
        mask_rle.check_shape(1200, 480, 640)
    mask_rle.check_shape(100, 480, 640)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.rle_encode(torch.zeros(2, 4, 4, dtype=torch.uint8))
    for rel, words in (('README.md', ('rle_encode',)), ('INTEGRATION.md', ('rle_encode', 'solo_encode_results', 'box2mask_encode_results', 'unpinned')),
                       ('tools/README.md', ('mask_rle_bench',)), ('profiles/NOTES.md', ('R28-1', 'rle_encode'))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)
