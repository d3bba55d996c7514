"""COCO's run-length encoding of a binary mask, restated from the published algorithm of cocoapi's maskApi.c (rleEncode, rleToString,
rleFrString, rleDecode) as literal loops in Python / numpy -- the yardstick of boxinstseg_amd.mask_rle.  UNPINNED: pycocotools never ran
next to it; the hand cases of tests/test_host_mask_rle.py are what holds it.  A plain module, no fixtures, nothing from the reference."""
from __future__ import annotations

import numpy as np


def rle_counts(mask) -> list:
    """rleEncode of one [h, w] mask: walk it in column-major order, j = x * h + y; any non-zero element is a set pixel."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    flat = m.T.reshape(-1).tolist()                       # column-major
    cnts, p, c = [], 0, 0
    for v in flat:
        if v != p:
            cnts.append(c)
            c = 0
            p = v
        c += 1
    cnts.append(c)
    return cnts


def rle_counts_fast(mask) -> list:
    """The same counts from numpy's diff (for the larger cases; test_host_mask_rle.py holds the two together)."""
    m = (np.asarray(mask) != 0).astype(np.int8)
    flat = np.concatenate([[0], m.T.reshape(-1)])
    pos = np.flatnonzero(np.diff(flat))
    edges = np.concatenate([[0], pos, [m.size]])
    return np.diff(edges).tolist()


def rle_to_string(cnts) -> bytes:
    """rleToString: every count, from the fourth on its difference to the count two before, in 5-bit groups with a continuation bit."""
    out = bytearray()
    for i, x in enumerate(cnts):
        x = int(x)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                       # arithmetic: python's >> floors
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


def rle_from_string(s) -> list:
    """rleFrString: the inverse of rle_to_string."""
    s = bytes(s)
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def rle_decode_counts(cnts, h, w) -> np.ndarray:
    """rleDecode: alternating runs of zeros and ones, column-major -> bool [h, w]."""
    flat = np.zeros(h * w, dtype=bool)
    at, v = 0, False
    for c in cnts:
        flat[at:at + c] = v
        at += c
        v = not v
    assert at == h * w, (at, h, w)
    return flat.reshape(w, h).T.copy()


def encode(mask, fast=False) -> dict:
    """What ``mask_util.encode(np.array(mask[:, :, None], order='F', dtype='uint8'))[0]`` returns."""
    h, w = np.asarray(mask).shape
    return {'size': [int(h), int(w)], 'counts': rle_to_string(rle_counts_fast(mask) if fast else rle_counts(mask))}


def decode(rle) -> np.ndarray:
    h, w = rle['size']
    return rle_decode_counts(rle_from_string(rle['counts']), h, w)


def packed(masks, fast=True):
    """[n, h, w] (or a list of [h, w] of one size) -> what bxi_mask_rle_u8 writes with sufficient capacities: run_offsets int32 [n+1],
    counts uint32, char_offsets int32 [n+1], chars uint8."""
    ro, co, counts, chars = [0], [0], [], bytearray()
    for m in masks:
        c = rle_counts_fast(m) if fast else rle_counts(m)
        counts += c
        chars += rle_to_string(c)
        ro.append(len(counts))
        co.append(len(chars))
    return (np.array(ro, np.int32), np.array(counts, np.uint32), np.array(co, np.int32), np.frombuffer(bytes(chars), np.uint8).copy())


def stats_of(masks) -> np.ndarray:
    """area, x_min, y_min, x_max, y_max per mask; (0, -1, -1, -1, -1) for an empty one (the layout of seg_paste's statistics)."""
    out = []
    for m in masks:
        ys, xs = np.nonzero(np.asarray(m))
        out.append([len(ys), xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0, -1, -1, -1, -1])
    return np.array(out, np.int32).reshape(-1, 5)
