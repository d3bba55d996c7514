"""Float64 restatement of the end of get_seg_single of the SOLOv2-style heads and of the detectors' format_results (a plain module:
numpy and CPU torch only), shared by tests/test_gpu_seg_paste.py, tests/test_gpu_guarded_seg.py and tools/seg_paste_bench.py.

    p64(probs, keep, up, crop, out)     box_solov2_head.py:576-588 / discobox_head.py:1641-1655 in float64 on the CPU:
                                        F.interpolate(seg_preds[keep], size=up, 'bilinear')[:, :, :crop_h, :crop_w] -> F.interpolate(., size=out)
    grid64(probs, keep, up, crop, out)  the same composition in float64 ON THE FP32 SAMPLING GRID: the taps and weights are the ones ATen's
                                        fp32 kernel computes (src = max(scale (dst + 0.5) - 0.5, 0) with scale = fp32(in) / fp32(out) and fp32
                                        arithmetic), only the products and sums are float64 -- what tests/test_gpu_mask_paste.py does for its
                                        composition.  At a source coordinate of a few hundred the fp32 tap position is up to ~1e-5 pixel
                                        away from where float64 places it, which moves p by as much: that is the grid, not the kernel.
    assert_tie_rule / check_tie         a byte may differ from ``grid64 > thr`` only where |grid64 - thr| <= 1e-6; against p64 the band is
                                        widened, pixel by pixel, by |grid64 - p64|.  `cap`: the share of pixels outside the band (the
                                        parity tests ask for >= 99 %, so the rule cannot hide a failure).
    format_results(...)                 single_stage_ts.py:88-103 / single_stage_boxseg.py:75-90 on CPU tensors, restated.
    stats_of(masks)                     numpy's count and np.where bounds of uint8 / bool masks [n,H,W] -> int32 [n,5], (0,-1,-1,-1,-1) if empty.

A keep index outside [0, n_all) stands for an all-zero plane (the library's rule; the reference would raise).
"""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
TIE = 1e-6


def _rows(probs, keep):
    probs, keep = np.asarray(probs), np.asarray(keep, np.int64)
    ok = (keep >= 0) & (keep < len(probs))
    x = np.zeros((len(keep),) + probs.shape[1:], np.float64)
    x[ok] = probs[keep[ok]]
    return x


def p64(probs, keep, up, crop, out):
    """-> float64 [n, out_h, out_w]."""
    x = torch.from_numpy(_rows(probs, keep)).unsqueeze(0)
    if x.shape[1] == 0:
        return np.zeros((0,) + tuple(out))
    x = F.interpolate(x, size=tuple(up), mode='bilinear')[:, :, :crop[0], :crop[1]]
    return F.interpolate(x, size=tuple(out), mode='bilinear').squeeze(0).numpy()


def taps_resize(n_out, n_in):
    """F.interpolate(bilinear, align_corners=False, size) as ATen's fp32 kernel places the taps: (i0, i1, l0, l1) per output index."""
    dst = np.arange(n_out)
    if n_in == n_out:
        return dst, dst, np.ones(n_out, f32), np.zeros(n_out, f32)
    scale = f32(n_in) / f32(n_out)
    src = np.maximum(scale * (dst.astype(f32) + f32(0.5)) - f32(0.5), f32(0))
    assert src.dtype == f32
    i0 = src.astype(np.int64)
    l1 = src - i0.astype(f32)
    return i0, i0 + (i0 < n_in - 1), f32(1) - l1, l1


def axis_matrix(n_out, crop, up, n):
    """[n_out, n] float64: output index -> weights over source indices through both stages (stage 2 clamps at the crop's edge, stage 1 at
    the source's), fp32 taps and weights."""
    o0, o1, L0, L1 = taps_resize(n_out, crop)
    a0, a1, l0, l1 = taps_resize(up, n)
    m = np.zeros((n_out, n))
    rows = np.arange(n_out)
    for oi, ow in ((o0, L0), (o1, L1)):
        np.add.at(m, (rows, a0[oi]), ow.astype(np.float64) * l0[oi])
        np.add.at(m, (rows, a1[oi]), ow.astype(np.float64) * l1[oi])
    return m


def grid64(probs, keep, up, crop, out):
    """-> float64 [n, out_h, out_w]."""
    x = _rows(probs, keep)
    ry, rx = axis_matrix(out[0], crop[0], up[0], x.shape[1]), axis_matrix(out[1], crop[1], up[1], x.shape[2])
    return np.einsum('yr,nrc,xc->nyx', ry, x, rx, optimize=True)


def assert_tie_rule(got, p, thr, tol, what='', cap=None):
    got = np.asarray(got)
    assert got.shape == p.shape and got.dtype == np.uint8, (what, got.shape, p.shape, got.dtype)
    assert set(np.unique(got).tolist()) <= {0, 1}, what
    with np.errstate(invalid='ignore'):
        outside = ~(np.abs(p - thr) <= tol)                       # a NaN probability is outside: its byte must be 0
        bad = (got != (p > thr)) & outside
    assert not bad.any(), f'{what}: {int(bad.sum())} pixels off outside the tie band, e.g. p = {p[bad][:4]}'
    if cap is not None and got.size:
        assert outside.mean() >= cap, f'{what}: only {outside.mean():.4f} of the pixels lie outside the band'


def check_tie(got, probs, keep, up, crop, out, thr, what='', cap=0.99):
    """The tie rule against grid64, and against p64 with the band widened by |grid64 - p64|.  `thr` as the kernel compares: fp32."""
    pg, pp = grid64(probs, keep, up, crop, out), p64(probs, keep, up, crop, out)
    thr = float(f32(thr))
    assert_tie_rule(got, pg, thr, TIE, f'{what} vs grid64', cap)
    assert_tie_rule(got, pp, thr, TIE + np.abs(pg - pp), f'{what} vs fp64', cap)
    return pg


def stats_of(masks):
    masks = np.asarray(masks).astype(bool)
    out = np.full((len(masks), 5), -1, np.int32)
    for i, m in enumerate(masks):
        ys, xs = np.where(m)
        out[i, 0] = int(m.sum())
        if len(ys):
            out[i, 1:] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def format_results(labels, scores, masks, num_classes):
    """What single_stage_ts.py:88-103 returns for CPU tensors (labels int64 [n], scores [n], masks bool [n,H,W]), restated: a mask with no
    set pixel is dropped (:94); a kept one goes to its class's mask list, its score to the score list (:95-96), and the extremes of
    torch.where(mask) give the row [x_min, y_min, x_max + 1, y_max + 1, score] (:97-99); np.array turns a class's rows into float64 [k,5],
    a class without rows is np.zeros((0, 5)) (:101)."""
    per_class = [dict(rows=[], masks=[], scores=[]) for _ in range(num_classes)]
    for i in range(len(masks)):
        mask = masks[i].cpu()
        if int(mask.sum()) == 0:
            continue
        into = per_class[int(labels[i])]
        score = scores[i].cpu()
        ys, xs = torch.where(mask)
        into['masks'].append(mask)
        into['scores'].append(score)
        into['rows'].append([xs.min().numpy(), ys.min().numpy(), xs.max().numpy() + 1, ys.max().numpy() + 1, score.numpy()])
    boxes = [np.array(c['rows']) if c['rows'] else np.zeros((0, 5)) for c in per_class]
    return boxes, ([c['masks'] for c in per_class], [c['scores'] for c in per_class])
