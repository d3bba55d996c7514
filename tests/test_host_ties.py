"""Inputs whose projection lines are TIED, and the expectation they are checked against (no GPU needed).

The projection term sends each row's and each column's whole gradient to one pixel, the arg-max; DESIGN.md section 1 documents
"the first index of the largest logit".  This module holds
  - the tie inputs (`tie_logits`) and the shapes (`SHAPES`) that tests/test_gpu_ties.py feeds to the kernels, and
  - the host checks of tests/helpers.py:project_term_f64, the float64 restatement the GPU tests compare with: against the C oracle
    where the two rules cannot differ, and against what each input is built to produce (which lines are tied, where the first
    index of the largest logit lies).
"""
import numpy as np
import pytest

from boxinstseg_amd import synthetic
from oracle import c_oracle
from tests.helpers import instance_bitmasks, project_term_f64

# name -> batch.  Each crosses one structure of the kernels that the parity suite names.
SHAPES = {
    'scalar_w51': lambda: synthetic.make_batch(B=2, H=72, W=204, boxes_per_img=2, seed=27, min_box=16, max_box=120),        # w = 51, h = 18 (not 8k)
    'odd_19x40': lambda: synthetic.make_batch(B=1, H=76, W=160, boxes_per_img=3, seed=8, min_box=24, max_box=100),          # h = 19
    'two_chunks_272x336': lambda: synthetic.make_batch(B=1, H=1088, W=1344, boxes_per_img=3, seed=22, min_box=200, max_box=900),
    'n300': lambda: synthetic.make_batch(B=3, H=64, W=96, boxes_per_img=5, inst_per_box=20, seed=21, min_box=12, max_box=60),
    'cfg1': lambda: synthetic.cfg1(3),
    'headline': lambda: synthetic.cfg2(0),                                                                                   # 2 x 800 x 1024, 32 instances
}
KINDS = ['constant', 'nine_levels', 'planted', 'bf16_rounded', 'fp16_rounded', 'saturated']
MERGE_WIDTHS = (4, 8, 16, 64, 256)          # 4-wide vectors, 8-row waves, 16-row tiles, 64 lanes, 256-column / 256-row chunks
PLANT = np.float32(5.0)


def _round_to(x, kind):
    import torch
    dt = torch.bfloat16 if kind == 'bf16' else torch.float16
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).float().numpy()


def _adjacent_pairs(L):
    """(0, last) and (kB - 1, kB), B in MERGE_WIDTHS, k = 1 and the last that fits."""
    pairs = [(0, L - 1)] if L > 1 else []
    for B in MERGE_WIDTHS:
        for k in sorted({1, (L - 1) // B}):
            if k >= 1 and k * B < L:
                pairs.append((k * B - 1, k * B))
    return pairs


def plant_pairs(L, lo, hi, crosses, n):
    """Per line i of length L the two positions (p < q) that receive PLANT, a multiple of one of MERGE_WIDTHS in (p, q].  [lo, hi] is the
    box's extent along the line, `crosses[i]` whether line i meets the box.  Lines that meet it alternate: p inside and q outside (q the
    first multiple of B beyond the box), then p outside (kB - 1, the last before the box) and q inside; where the box leaves no room on
    that side the other form is taken, and lines that do not meet the box (or a box that spans the line) take the adjacent pairs."""
    adj = _adjacent_pairs(L)
    out = []
    for i in range(len(crosses)):
        B = MERGE_WIDTHS[(i // 2 + n) % len(MERGE_WIDTHS)]
        pair = None
        if crosses[i] and L > 1:
            forms = ('in_out', 'out_in') if i % 2 == 0 else ('out_in', 'in_out')
            for form in forms:
                if form == 'in_out' and hi < L - 1:
                    p, q = max(lo, hi - (i // 2) % 3), min((hi // B + 1) * B, L - 1)
                    if (q // 4) * 4 > p:                               # (q capped at the last position: still a multiple of 4 in (p, q])
                        pair = (p, q)
                        break
                if form == 'out_in' and lo > 0:
                    p = (lo // B) * B - 1
                    if p < 0:
                        p = (lo // 4) * 4 - 1
                    if p >= 0:
                        pair = (p, min(hi, lo + (i // 2) % 3))
                        break
        if pair is None:
            pair = adj[(i + n) % len(adj)] if adj else (0, 0)
        out.append(pair)
    return out


def tie_logits(kind, d, seed=0):
    """-> logits [N,1,h,w] float32 for the batch `d` (its boxes decide what is inside / outside)."""
    N, h, w = d['N'], d['h'], d['w']
    rng = np.random.default_rng(7700 + seed)
    if kind == 'constant':
        x = np.full((N, h, w), 1.5, np.float32)
    elif kind == 'nine_levels':
        x = rng.integers(-4, 5, size=(N, h, w)).astype(np.float32)
    elif kind in ('bf16_rounded', 'fp16_rounded'):
        x = _round_to(2.0 * rng.standard_normal((N, h, w)), kind[:4])
    elif kind == 'saturated':
        x = (d['mask_logits'][:, 0] * 40.0).astype(np.float32)
    elif kind == 'planted':
        x = rng.uniform(-4.0, 4.0, size=(N, h, w)).astype(np.float32)
        bm = instance_bitmasks(d)
        for n in range(N):
            rows, cols = np.flatnonzero(bm[n].any(1)), np.flatnonzero(bm[n].any(0))
            r_lo, r_hi = (rows[0], rows[-1]) if rows.size else (0, -1)
            c_lo, c_hi = (cols[0], cols[-1]) if cols.size else (0, -1)
            if n % 2 == 0:          # every ROW tied (columns p, q of those rows tie over many rows: the first row wins)
                for r, (p, q) in enumerate(plant_pairs(w, c_lo, c_hi, bm[n].any(1), n)):
                    x[n, r, p] = x[n, r, q] = PLANT
            else:                   # every COLUMN tied
                for c, (p, q) in enumerate(plant_pairs(h, r_lo, r_hi, bm[n].any(0), n)):
                    x[n, p, c] = x[n, q, c] = PLANT
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x[:, None], dtype=np.float32)


def tied_lines(x):
    """x [N,h,w] -> (tied columns [N,w], tied rows [N,h]): lines whose largest fp32 logit occurs more than once."""
    return ((x == x.max(1, keepdims=True)).sum(1) > 1), ((x == x.max(2, keepdims=True)).sum(2) > 1)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# Restatement (float64) against the C oracle (fp32): the difference is the ORACLE's rounding -- its fp32 expf sigmoid, 1 - s near
# s = 1, and its fp32 dice sums over up to 336 terms --, nothing of the code under test.  Largest measured gradient difference over
# max|g|: 1.88e-6 (tie-free headline batch), 1.82e-6 (constant map at 272 x 336); largest loss difference 7.0e-7 relative.  The
# bound is 4 x 1.9e-6 for both.
RESTATEMENT_BOUND = 4 * 1.9e-6


@pytest.mark.parametrize('shape', list(SHAPES))
def test_restatement_equals_the_c_oracle_where_no_line_is_tied(shape):
    """project_term_f64 against c_oracle.project_term on the synthetic logits of every shape, restricted to what both rules agree on:
    the batches are tie-free in the logits AND in the oracle's fp32 sigmoid (asserted: 'sigma_first' picks the same pixels).
    Measured gradient differences / max|g|: scalar_w51 2.4e-7, odd_19x40 6.3e-7, two_chunks_272x336 1.63e-6, n300 5.1e-7,
    cfg1 7.1e-7, headline 1.88e-6 (loss differences 3.7e-8 .. 1.5e-7 relative); bound = 4 x 1.9e-6 = 7.6e-6."""
    d = SHAPES[shape]()
    x = d['mask_logits'][:, 0]
    bm = instance_bitmasks(d)
    tc, tr = tied_lines(x)
    assert not tc.any() and not tr.any()
    for g in (1.0, 0.5):
        want_l, want_g = c_oracle.project_term(x, bm, g_out=g)
        loss, grad, arg = project_term_f64(x, bm, 'logit_first', g_out=g)
        sig = project_term_f64(x, bm, 'sigma_first', g_out=g)
        assert np.array_equal(sig[2][0], arg[0]) and np.array_equal(sig[2][1], arg[1])       # tie-free in the fp32 sigmoid as well
        err = _rel(grad, want_g.astype(np.float64))
        print(f'{shape} g_out {g}: grad {err:.2e}  loss {abs(loss.mean() - want_l) / want_l:.2e}')
        assert err <= RESTATEMENT_BOUND, err
        assert abs(loss.mean() - want_l) <= RESTATEMENT_BOUND * want_l
        assert np.count_nonzero(grad) <= d['N'] * (d['h'] + d['w'])


@pytest.mark.parametrize('kind', ['nine_levels', 'constant'])
@pytest.mark.parametrize('shape', ['scalar_w51', 'two_chunks_272x336', 'cfg1'])
def test_restatement_equals_the_c_oracle_where_equal_sigmoids_are_equal_logits(shape, kind):
    """On the nine-level and the constant maps every line is tied, yet distinct logits have distinct fp32 sigmoids, so the oracle's
    'first maximum of sigma' IS the first index of the largest logit: restatement and oracle must agree here as well.
    Measured / max|g|: nine levels 1.03e-6 .. 1.55e-6, constant 2.3e-7 .. 1.82e-6 (losses 2.4e-7 .. 7.0e-7); same bound."""
    d = SHAPES[shape]()
    x = tie_logits(kind, d)[:, 0]
    bm = instance_bitmasks(d)
    want_l, want_g = c_oracle.project_term(x, bm)
    loss, grad, _ = project_term_f64(x, bm, 'logit_first')
    err = _rel(grad, want_g.astype(np.float64))
    print(f'{shape} {kind}: grad {err:.2e}  loss {abs(loss.mean() - want_l) / want_l:.2e}')
    assert err <= RESTATEMENT_BOUND, err
    assert abs(loss.mean() - want_l) <= RESTATEMENT_BOUND * want_l
    # and the rule matters on these maps: the last index is a different gradient altogether
    assert _rel(project_term_f64(x, bm, 'logit_last')[1], grad) > 0.1


@pytest.mark.parametrize('shape', list(SHAPES))
def test_tie_inputs_are_tied_where_they_say(shape):
    """Each input documents itself: which lines are tied, and where the first index of the largest logit lies."""
    d = SHAPES[shape]()
    N, h, w = d['N'], d['h'], d['w']
    bm = instance_bitmasks(d)
    # constant: every line tied; every column's pixel is row 0, every row's column 0; (0, 0) takes a row and a column at once; with a
    # box that does not touch row 0 / column 0 all of these lie outside the box
    x = tie_logits('constant', d)[:, 0]
    tc, tr = tied_lines(x)
    assert tc.all() and tr.all()
    _, grad, (ca, ra) = project_term_f64(x, bm)
    assert not ca.any() and not ra.any()
    assert np.count_nonzero(grad[:, 1:, 1:]) == 0
    corner = grad[:, 0, 0]
    _, g_last, _ = project_term_f64(x, bm, 'logit_last')
    assert np.count_nonzero(g_last[:, :-1, :-1]) == 0
    assert np.all(corner != 0.0)
    off_hull = [n for n in range(N) if not bm[n, 0].any() and not bm[n, :, 0].any()]        # every arg-max pixel outside the box hull
    print(f'{shape}: {len(off_hull)} of {N} instances with every arg-max pixel of the constant map outside the box hull')
    assert len(off_hull) >= 1
    # nine levels: ties on nearly every line, at scattered positions
    x = tie_logits('nine_levels', d)[:, 0]
    tc, tr = tied_lines(x)
    assert tc.mean() > 0.5 and tr.mean() > 0.5           # (lines of 16 .. 19 pixels: two thirds; of 200 and more: all)
    _, _, (ca, ra) = project_term_f64(x, bm)
    assert len(np.unique(ca)) > min(h, 8) // 2 and len(np.unique(ra)) > min(w, 8) // 2
    # planted: even instances have EVERY row tied between exactly two columns (p, q), p the expected pixel; odd instances every column
    x = tie_logits('planted', d)[:, 0]
    tc, tr = tied_lines(x)
    _, _, (ca, ra) = project_term_f64(x, bm)
    straddled = {B: 0 for B in MERGE_WIDTHS}
    in_out = out_in = 0
    for n in range(N):
        rows, cols = np.flatnonzero(bm[n].any(1)), np.flatnonzero(bm[n].any(0))
        if n % 2 == 0:
            assert tr[n].all() and ((x[n] == PLANT).sum(1) == 2).all()
            pairs = plant_pairs(w, cols[0] if cols.size else 0, cols[-1] if cols.size else -1, bm[n].any(1), n)
            assert np.array_equal(ra[n], [p for p, _ in pairs])
            inside = lambda r, c: bool(bm[n, r, c])
            for r, (p, q) in enumerate(pairs):
                in_out += inside(r, p) and not inside(r, q)
                out_in += inside(r, q) and not inside(r, p)
        else:
            assert tc[n].all() and ((x[n] == PLANT).sum(0) == 2).all()
            pairs = plant_pairs(h, rows[0] if rows.size else 0, rows[-1] if rows.size else -1, bm[n].any(0), n)
            assert np.array_equal(ca[n], [p for p, _ in pairs])
            for c, (p, q) in enumerate(pairs):
                in_out += bool(bm[n, p, c]) and not bool(bm[n, q, c])
                out_in += bool(bm[n, q, c]) and not bool(bm[n, p, c])
        for p, q in pairs:
            assert p < q
            for B in MERGE_WIDTHS:
                straddled[B] += any(p < m <= q for m in range(B, max(h, w), B))
    assert all(straddled[B] > 0 for B in MERGE_WIDTHS if B < min(h, w)), straddled
    assert in_out > 0 and out_in > 0 and 0.25 <= in_out / (in_out + out_in) <= 0.75, (in_out, out_in)
    # reduced-precision roundings: the line maximum of 2 N(0,1) lies in [4, 8), where bf16 steps by 1/32 and fp16 by 1/256: about 2 % and
    # 0.2 % of the lines are tied (counted: headline 325 and 32 of 14 592, n300 99 and 14 of 12 000)
    for kind, share in (('bf16_rounded', 5e-3), ('fp16_rounded', 5e-4)):
        x = tie_logits(kind, d)[:, 0]
        assert np.array_equal(x, _round_to(x, kind[:4]))
        tc, tr = tied_lines(x)
        print(f'{shape} {kind}: {int(tc.sum() + tr.sum())} of {tc.size + tr.size} lines tied')
        assert tc.sum() + tr.sum() >= max(1 if tc.size + tr.size >= 4000 else 0, int(share * (tc.size + tr.size))), (kind, tc.mean(), tr.mean())
    # saturated: distinct logits, but the fp32 sigmoid is 1.0 on several pixels of almost every line
    x = tie_logits('saturated', d)[:, 0]
    tc, tr = tied_lines(x)
    assert not tc.any() and not tr.any()
    s32 = (np.float32(1) / (np.float32(1) + np.exp(-np.clip(x, -80, 80)))).astype(np.float32)
    sc, sr = tied_lines(s32)
    assert sc.mean() > 0.5 and sr.mean() > 0.5           # (short lines: three quarters; cfg1, as counted for test_loss_extreme_logits: 511 of 512)
