"""CPU: the host side of the test-time mask paste (no kernel is launched here).

* bxi_mask_paste_u8 validates its arguments before anything touches a device;
* the class-grouped order and byte offsets that boxinstseg_amd.dynamic.paste_masks computes with torch ops reproduce the
  reference's per image ``masks[labels == c]`` order (condinst_head.py:1281-1285)."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def _dims(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


def test_mask_paste_abi_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    ok = _dims([(41, 70, 60, 101)])
    # N == 0: a no-op, whatever the device pointers
    assert lib.bxi_mask_paste_u8(None, 0, 12, 18, 4, None, None, 1, ok, 0.5, None, None) == 0
    # NULL pointers
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, ok, 0.5, None, None) == -1
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, None, 0.5, None, None) == -1
    # bad dims: negative N, empty logits, factor < 1, a crop larger than the canvas, dims < 1, B outside 1..64
    assert lib.bxi_mask_paste_u8(None, -1, 12, 18, 4, None, None, 1, ok, 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 0, 18, 4, None, None, 1, ok, 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 0, None, None, 1, ok, 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, _dims([(49, 70, 60, 101)]), 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, _dims([(48, 73, 60, 101)]), 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, _dims([(41, 70, 0, 101)]), 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 0, ok, 0.5, None, None) == -2
    many = _dims([(41, 70, 60, 101)] * 65)
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 65, many, 0.5, None, None) == -2
    assert lib.bxi_mask_paste_u8(None, 0, 12, 18, 4, None, None, 65, many, 0.5, None, None) == -2
    # a NaN threshold
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 1, ok, float('nan'), None, None) == -3
    # the same dims are fine up to the device pointers: 64 images, a crop equal to the canvas
    assert lib.bxi_mask_paste_u8(None, 3, 12, 18, 4, None, None, 64, _dims([(48, 72, 1, 1)] * 64), 0.5, None, None) == -1


@pytest.mark.parametrize('seed', range(6))
def test_grouped_order_matches_reference_selection(seed):
    """Instance j writes its own id into its block; reading the blocks back class by class gives, per image and class, the ids
    of ``np.nonzero(labels_i == c)`` in detection order -- the reference's ``masks[labels == c]``."""
    from boxinstseg_amd.dynamic import paste_order
    rng = np.random.default_rng(300 + seed)
    B = int(rng.integers(1, 5))
    ncls = int(rng.choice([1, 3, 80]))
    counts = [int(rng.integers(0, 12)) for _ in range(B)]
    counts[int(rng.integers(0, B))] += 1
    hw = [int(rng.integers(1, 7)) * int(rng.integers(1, 5)) for _ in range(B)]
    labels = [rng.integers(0, ncls, size=c) if seed != 3 else np.full(c, ncls - 1) for c in counts]      # seed 3: one class
    img = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
    lab = torch.from_numpy(np.concatenate(labels).astype(np.int64))
    off, key = paste_order(img, lab, counts, hw, ncls)
    total = sum(c * s for c, s in zip(counts, hw))
    buf = np.full(total, -1, np.int64)
    for j, o in enumerate(off.tolist()):
        s = hw[int(img[j])]
        assert 0 <= o and o + s <= total
        assert (buf[o:o + s] == -1).all(), 'two instances share bytes'
        buf[o:o + s] = j
    assert (buf >= 0).all(), 'a byte is written by no instance'
    per_class = np.bincount(key.numpy(), minlength=B * (ncls + 1)).reshape(B, ncls + 1)
    pos, first = 0, 0
    for i in range(B):
        for c in range(ncls):
            n = int(per_class[i, c])
            got = buf[pos:pos + n * hw[i]].reshape(n, hw[i])[:, 0] - first
            want = np.nonzero(labels[i] == c)[0]
            assert np.array_equal(got, want), (i, c)
            pos += n * hw[i]
        first += counts[i]
    assert pos == total


def test_detection_order_offsets_and_foreign_labels():
    """Without classes the blocks stay in detection order; labels outside 0..num_classes-1 go last in their image."""
    from boxinstseg_amd.dynamic import paste_order
    img = torch.tensor([0, 0, 1, 1, 1])
    off, _ = paste_order(img, None, [2, 3], [6, 10])
    assert off.tolist() == [0, 6, 12, 22, 32]
    off, key = paste_order(img, torch.tensor([5, 1, 0, -1, 0]), [2, 3], [6, 10], 2)
    assert off.tolist() == [6, 0, 12, 32, 22]
    assert key.tolist() == [2, 1, 3, 5, 3]
