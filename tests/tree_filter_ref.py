"""fp64 references around oracle/tree_filter_oracle.py (tfo) for the tree-filter tests: the gradient of TreeFilter2D with respect to
its embedding, the whole module per image and group, and the edge weights at which the kernels' arithmetic is exact or extreme
(exact 0, exact 1, fp32 subnormals).  numpy only; tests/test_host_tree_filter.py checks everything here without a device.

Reference: mmdet/ops/tree_filter/modules/tree_filter.py:90-150 (build_edge_weight, split_group, forward),
functions/refine.py:32-41 (no weight gradient on the low-level tree)."""
import zlib

import numpy as np

from oracle import tree_filter_oracle as tfo


def embed_grad(embed, gw, si, sp, low_tree, sigma=0.02):
    """d loss / d embed [Ce,V] (vertex order) from d loss / d w = gw [V] (sorted order), through build_edge_weight:
    w_i = exp(-|e_i - e_parent(i)|^2 / s), s = sigma on the low-level tree and 1 otherwise.  Position i receives its own edge's term
    and, with the opposite sign, the term of every edge to one of its children."""
    embed = np.asarray(embed, np.float64)
    e = embed[:, si]
    diff = e - e[:, sp]
    w = tfo.edge_weights(embed, si, sp, low_tree, sigma)
    s = sigma if low_tree else 1.0
    t = np.asarray(gw, np.float64)[None] * (-w[None] / s) * 2.0 * diff
    t[:, 0] = 0.0
    r = t.copy()
    for c in range(r.shape[0]):
        np.subtract.at(r[c], sp[1:], t[c, 1:])
    out = np.empty_like(r)
    out[:, si] = r
    return out


def module_reference(feat, emb, trees, groups, low_tree, sigma, gout, info=None):
    """TreeFilter2D(groups, sigma)(feat [B,C,H,W], emb [B,Ce,H,W], trees [B,V-1,2], low_tree) and its backward on gout, per image and
    group: row b*G + g filters feature channels [g C/G, (g+1) C/G) with the weights of embedding channels [g Ce/G, (g+1) Ce/G)
    (tree_filter.py:99-100, 110-119).  -> (out, d feat, d emb), fp64, shaped like the inputs; d emb is None on the low-level tree.
    `info`, if a dict, receives 'gw_absmax' [B,G]: max |d loss / d w| of each image and group (what the embedding tolerance scales with)."""
    feat, emb, gout = (np.asarray(a, np.float64) for a in (feat, emb, gout))
    B, C, H, W = feat.shape
    Ce, V, G = emb.shape[1], H * W, groups
    cg, eg = C // G, Ce // G
    out, dfeat = np.empty((B, C, V)), np.empty((B, C, V))
    demb = None if low_tree else np.empty((B, Ce, V))
    gmax = np.zeros((B, G))
    orders = {}
    for b in range(B):
        t = np.ascontiguousarray(trees[b])
        key = t.tobytes()
        if key not in orders:                       # Box2Mask repeats one tree per instance
            orders[key] = tfo.bfs_order(t, V)
        si, sp, sc = orders[key]
        for g in range(G):
            fs, es = slice(g * cg, (g + 1) * cg), slice(g * eg, (g + 1) * eg)
            e = emb[b, es].reshape(eg, V)
            x = feat[b, fs].reshape(cg, V)
            go = gout[b, fs].reshape(cg, V)
            w = tfo.edge_weights(e, si, sp, low_tree, sigma)
            out[b, fs], saved = tfo.refine_forward(x, w, si, sp, sc)
            dfeat[b, fs] = tfo.refine_backward_feature(go, w, si, sp, sc, saved)
            if not low_tree:
                gw = tfo.refine_backward_weight(x, go, w, si, sp, sc, saved)
                gmax[b, g] = np.abs(gw).max()
                demb[b, es] = embed_grad(e, gw, si, sp, False, sigma)
    if info is not None:
        info['gw_absmax'] = gmax
    shape = lambda a, c: None if a is None else a.reshape(B, c, H, W)
    return shape(out, C), shape(dfeat, C), shape(demb, Ce)


def components(w, sp):
    """component id per sorted position when every edge with w != 1 is cut: position i joins its parent's component iff w[i] == 1"""
    comp = np.zeros(len(w), np.int64)
    n = 1
    for i in range(1, len(w)):
        if w[i] == 1:
            comp[i] = comp[sp[i]]
        else:
            comp[i] = n
            n += 1
    return comp


def component_mean_f32(x_sorted, comp):
    """x_sorted [..., V] of integers (sorted order) -> [..., n_components] float32: the exact integer sum of each component, divided by its
    size in float32 (one IEEE division: the only rounding a kernel may make on weights of exactly 0 and 1)"""
    x = np.asarray(x_sorted, np.float64)
    n = int(comp.max()) + 1
    s = np.zeros(x.shape[:-1] + (n,))
    flat, sf = x.reshape(-1, x.shape[-1]), s.reshape(-1, n)
    for c in range(flat.shape[0]):
        np.add.at(sf[c], comp, flat[c])
    assert (s == np.round(s)).all() and np.abs(s).max() < 2 ** 24
    return s.astype(np.float32) / np.bincount(comp, minlength=n).astype(np.float32)


REGIMES = ('ones', 'zeros', 'cut', 'mixed')
MIXED_VALUES = (0.0, 1e-45, 1e-40, 1e-30, 1e-10, 0.5, 1.0)      # 1e-45 rounds to the smallest fp32 subnormal, 1e-40 is subnormal too


def regime_weights(name, V, rng):
    """float32 edge weights [V] (sorted order; slot 0 is unused by the kernels and filled like the rest)"""
    if name == 'ones':
        return np.ones(V, np.float32)
    if name == 'zeros':
        return np.zeros(V, np.float32)
    if name == 'cut':
        return (rng.random(V) < 0.8).astype(np.float32)
    if name == 'mixed':
        return np.asarray(MIXED_VALUES, np.float64)[rng.integers(0, len(MIXED_VALUES), V)].astype(np.float32)
    raise ValueError(name)


def regime_inputs(name, V, B=2, C=2):
    """The draw test_refine_weight_regimes runs (and the host test checks the preconditions of): integer x, g [B,C,V] in [-8, 8] as float32
    and B different weight draws [B,V]."""
    rng = np.random.default_rng(zlib.crc32(f'{name}-{V}'.encode()))
    x = rng.integers(-8, 9, (B, C, V)).astype(np.float32)
    g = rng.integers(-8, 9, (B, C, V)).astype(np.float32)
    w = np.stack([regime_weights(name, V, rng) for _ in range(B)])
    return x, g, w


def image_like_embedding(B, Ce, H, W, rng):
    """An embedding with the edge weights Box2Mask's first filter really sees (exp(-d / 0.02) on a normalised image): a block of exactly
    equal pixels (w == 1 inside), a step of 2.0 across the map (w underflows to 0 on every edge that crosses it), 0.05-sigma noise elsewhere."""
    e = rng.standard_normal((B, Ce, H, W)) * 0.05
    e[:, :, : H // 2, : W // 3] = 0.25                                   # flat / padded region
    e[:, :, :, W // 2:] += 2.0                                           # an object edge
    return e.astype(np.float32)
