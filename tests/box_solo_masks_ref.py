"""BoxLevelSet's mask predictions as the reference states them (mmdet/models/dense_heads/box_solov2_head.py), restated statement by
statement, plus the seeded cases and the tolerance rule of the box_solo_masks tests.

    ins_preds_all     :205-216 of ``forward`` with ``eval=False``: per level the grouped convolution of the mask feature with the kernels of
                      EVERY cell and the bilinear resize of the whole result
    select            :317-320 of ``loss``: the rows of the set cells, level by level, images concatenated
    rows_ref          the two together; ``resized_first`` is the composition in the other order (resize the feature, then multiply the
                      set cells' kernels), which is how the kernels work
    taps              the bilinear weights of ``F.interpolate(size=..., mode='bilinear')`` as include/boxinst/boxinst_hip_dconvl.h states them

All run in the dtype of their inputs.  The tolerance rule is the project's (tests/solo_conv_ref.py: ``bound``, ``assert_within``)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.solo_conv_ref import assert_within, bound  # noqa: F401  (re-exported: one rule)


def ins_preds_all(kernel_pred, feature_pred, level_sizes, seg_num_grids):
    """Per level [B, S_l^2, oh_l, ow_l]: every cell's mask logits, resized."""
    N, c, h, w = feature_pred.shape
    feature_pred = feature_pred.view(-1, h, w).unsqueeze(0)
    ins_pred = []
    for i in range(len(kernel_pred)):
        kernel = kernel_pred[i].permute(0, 2, 3, 1).contiguous().view(-1, c).unsqueeze(-1).unsqueeze(-1)
        ins_i = F.conv2d(feature_pred, kernel, groups=N).view(N, seg_num_grids[i] ** 2, h, w)
        ins_i = F.interpolate(ins_i, size=(level_sizes[i][0], level_sizes[i][1]), mode='bilinear')
        ins_pred.append(ins_i)
    return ins_pred


def select(ins_preds, ins_ind_labels):
    """``ins_ind_labels[l][b]`` bool [S_l^2]  ->  per level [N_l, oh_l, ow_l]."""
    return [torch.cat([ins_preds_level_img[ins_ind_labels_level_img, ...]
                       for ins_preds_level_img, ins_ind_labels_level_img in zip(ins_preds_level, ins_ind_labels_level)], 0)
            for ins_preds_level, ins_ind_labels_level in zip(ins_preds, ins_ind_labels)]


def rows_ref(kernel_pred, feature_pred, ins_ind_labels, level_sizes):
    return select(ins_preds_all(kernel_pred, feature_pred, level_sizes, [int(k.shape[-1]) for k in kernel_pred]), ins_ind_labels)


def resized_first(kernel_pred, feature_pred, ins_ind_labels, level_sizes):
    """The other order: the feature resized to the level's size, then the set cells' kernels times it."""
    out = []
    B, E = feature_pred.shape[:2]
    for k, labels, (oh, ow) in zip(kernel_pred, ins_ind_labels, level_sizes):
        f = F.interpolate(feature_pred, size=(oh, ow), mode='bilinear')
        rows = [torch.einsum('en,ehw->nhw', k[b].reshape(E, -1)[:, labels[b]], f[b]) for b in range(B)]
        out.append(torch.cat(rows, 0))
    return out


def taps(n_in, n_out, dtype=torch.float64):
    """(i0, i1, l0, l1) of every output index of one axis: scale = in / out; src = max(scale * (dst + 0.5) - 0.5, 0); i0 = floor(src);
    i1 = min(i0 + 1, in - 1); l1 = src - i0; l0 = 1 - l1."""
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    src = (scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def resize_by_taps(x, oh, ow):
    """``F.interpolate(x, size=(oh, ow), mode='bilinear')`` of [..., h, w] written out with ``taps``."""
    y0, y1, h0, h1 = taps(x.shape[-2], oh, x.dtype)
    x0, x1, w0, w1 = taps(x.shape[-1], ow, x.dtype)
    top = w0 * x[..., y0, :][..., x0] + w1 * x[..., y0, :][..., x1]
    bot = w0 * x[..., y1, :][..., x0] + w1 * x[..., y1, :][..., x1]
    return h0[:, None] * top + h1[:, None] * bot


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
# name -> make_case arguments; counts[l][b] = set cells of (level, image)
CASES = {
    # one (level, image) without rows (1, 0); level 3 without rows in any image; image 1 without rows in the whole group {2}
    'ratios124': dict(seed=21, B=2, E=12, H=16, W=24, sizes=[(16, 24), (16, 24), (8, 12), (4, 6), (4, 6)], grids=[4, 3, 3, 2, 2],
                      counts=[[3, 2], [0, 4], [2, 0], [0, 0], [1, 2]]),
    # non-integer ratios, a slight up-size, clamped edge taps
    'odd': dict(seed=22, B=1, E=8, H=13, W=19, sizes=[(12, 18), (14, 20), (7, 10), (4, 5), (3, 5)], grids=[3, 3, 2, 2, 2],
                counts=[[2], [3], [2], [1], [2]]),
    # tiles that straddle rows; 34 set cells in one (level, image): more than a chunk of 32
    'wide': dict(seed=23, B=1, E=72, H=8, W=70, sizes=[(8, 70), (8, 70), (4, 35), (2, 18), (2, 17)], grids=[6, 3, 3, 2, 2],
                 counts=[[34], [2], [3], [1], [2]]),
    # a single output pixel
    'point': dict(seed=24, B=1, E=8, H=5, W=7, sizes=[(5, 7), (5, 7), (1, 1), (1, 1), (1, 1)], grids=[2, 2, 2, 1, 1],
                  counts=[[1], [2], [2], [1], [0]]),
}
# the ratios124 shape on integers: feature in [-4, 4], kernels in [-3, 3], upstream gradient in [-3, 3].  At ratios 1, 2 and 4 every
# bilinear weight is 1 or 1/2 per axis, every value a multiple of 1/16 and every partial sum far below 2^24: fp32 is exact in any order
EXACT_CASES = {
    'exact_a': dict(CASES['ratios124'], seed=31, integers=True),
    'exact_b': dict(CASES['ratios124'], seed=32, integers=True, counts=[[16, 0], [9, 9], [0, 3], [4, 0], [0, 4]]),
}


def make_case(seed, B, E, H, W, sizes, grids, counts, integers=False):
    """Seeded inputs of one case as numpy arrays: ``feat`` [B,E,H,W], ``maps[l]`` [B,E,S,S], ``labels[l]`` bool [B,S^2] with
    ``counts[l][b]`` set cells, ``g[l]`` [N_l,oh,ow]."""
    rng = np.random.default_rng(seed)
    if integers:
        feat = rng.integers(-4, 5, size=(B, E, H, W)).astype(np.float32)
        maps = [rng.integers(-3, 4, size=(B, E, S, S)).astype(np.float32) for S in grids]
    else:
        feat = (0.5 * rng.standard_normal((B, E, H, W))).astype(np.float32)
        maps = [(rng.standard_normal((B, E, S, S)) / np.sqrt(E)).astype(np.float32) for S in grids]
    labels = []
    for l, S in enumerate(grids):
        lab = np.zeros((B, S * S), bool)
        for b in range(B):
            assert 0 <= counts[l][b] <= S * S
            lab[b, rng.permutation(S * S)[:counts[l][b]]] = True
        labels.append(lab)
    g = []
    for l, (oh, ow) in enumerate(sizes):
        n = int(sum(counts[l]))
        g.append(rng.integers(-3, 4, size=(n, oh, ow)).astype(np.float32) if integers else rng.standard_normal((n, oh, ow)).astype(np.float32))
    return dict(feat=feat, maps=maps, labels=labels, g=g, sizes=[tuple(s) for s in sizes], grids=list(grids), counts=[list(c) for c in counts])


def to_torch(case, dtype=torch.float64, device='cpu', requires_grad=False):
    feat = torch.from_numpy(case['feat']).to(device=device, dtype=dtype).requires_grad_(requires_grad)
    maps = [torch.from_numpy(m).to(device=device, dtype=dtype).requires_grad_(requires_grad) for m in case['maps']]
    labels = [torch.from_numpy(lab).to(device) for lab in case['labels']]
    g = [torch.from_numpy(x).to(device=device, dtype=dtype) for x in case['g']]
    return feat, maps, labels, g


def cells_of(case, device='cpu'):
    """``cells[l][b]``: the set cells, ascending, as int64 tensors."""
    return [[torch.from_numpy(np.flatnonzero(lab[b]).astype(np.int64)).to(device) for b in range(lab.shape[0])] for lab in case['labels']]


def run_ref(case, dtype, fn=rows_ref):
    """``fn`` on the CPU in ``dtype`` with the case's upstream gradient: ([rows per level], grad_feat, [grad_map per level]) as float64
    numpy arrays, gradients of ``sum_l (rows_l * g_l).sum()``."""
    feat, maps, labels, g = to_torch(case, dtype, requires_grad=True)
    rows = fn(maps, feat, labels, case['sizes'])
    sum((r * x).sum() for r, x in zip(rows, g)).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                                    # noqa: E731
    return [r.detach().double().numpy() for r in rows], zero(feat).double().numpy(), [zero(m).double().numpy() for m in maps]


def flat(arrays):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays]) if len(arrays) else np.zeros(0)
