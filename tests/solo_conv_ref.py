"""The dynamic mask convolution of DiscoBoxSOLOv2Head as the reference states it (mmdet/models/dense_heads/discobox_head.py), restated
statement by statement, plus the seeded cases and the tolerance rule of the solo_conv tests.

    dynamic_masks     :1180-1246 of ``loss`` (the per-level gather ``kernel_pred.view(E, -1)[:, grid_order]``, one ``F.conv2d`` per
                      (level, image) with a non-empty order, the ``cat``s) and the ``sigmoid`` at :1275; ``corr_loss`` :936-1022 is the same
    candidate_masks   :1606-1608 of ``get_seg_single``

Both run in the dtype of their inputs.  ``grid_order`` is [level][image] here (the reference zips its [image][level] list).

The tolerance rule of the project: for every quantity the bound is 4 x the restatement's own fp32-against-fp64 difference on the CPU,
relative to the largest fp64 value (``bound``); ``assert_within`` holds a result against the fp64 values under it."""
import numpy as np
import torch
import torch.nn.functional as F


def dynamic_masks(kernel_preds_raw, grid_order, ins_pred, sigmoid=True):
    """Returns (ins_pred_list, img_ind_list): per level the masks [N_l,H,W] and ``torch.ones(n) * idx`` per image, None for an empty level."""
    kernel_preds = [[kernel_preds_level_img.view(kernel_preds_level_img.shape[0], -1)[:, grid_orders_level_img]
                     for kernel_preds_level_img, grid_orders_level_img in zip(kernel_preds_level, grid_orders_level)]
                    for kernel_preds_level, grid_orders_level in zip(kernel_preds_raw, grid_order)]
    ins_pred_list = []
    img_ind_list = []
    for b_kernel_pred in kernel_preds:
        b_mask_pred = []
        b_img_inds = []
        for idx, kernel_pred in enumerate(b_kernel_pred):
            if kernel_pred.size()[-1] == 0:
                continue
            cur_ins_pred = ins_pred[idx, ...]
            H, W = cur_ins_pred.shape[-2:]
            N, I = kernel_pred.shape
            cur_ins_pred = cur_ins_pred.unsqueeze(0)
            kernel_pred = kernel_pred.permute(1, 0).view(I, -1, 1, 1)
            cur_ins_pred = F.conv2d(cur_ins_pred, kernel_pred, stride=1).view(-1, H, W)
            b_mask_pred.append(cur_ins_pred)
            b_img_inds.append(torch.ones(cur_ins_pred.shape[0]) * idx)
        if len(b_mask_pred) == 0:
            b_mask_pred = None
            b_img_inds = None
        else:
            b_mask_pred = torch.cat(b_mask_pred, 0)
            b_img_inds = torch.cat(b_img_inds, 0)
        ins_pred_list.append(b_mask_pred)
        img_ind_list.append(b_img_inds)
    if sigmoid:
        ins_pred_list = [None if s_input is None else torch.sigmoid(s_input) for s_input in ins_pred_list]
    return ins_pred_list, img_ind_list


def candidate_masks(seg_preds, kernel_preds, sigmoid=True):
    """``seg_preds`` [1,E,h,w], ``kernel_preds`` [I,E] (already gathered, I >= 1) -> [I,h,w]."""
    I, N = kernel_preds.shape
    kernel_preds = kernel_preds.view(I, N, 1, 1)
    seg_preds = F.conv2d(seg_preds, kernel_preds, stride=1).squeeze(0)
    return seg_preds.sigmoid() if sigmoid else seg_preds


# the fixture's cases (tests/golden/make_golden_solo_conv.py), name -> make_case arguments: an S = 1 level and a level nobody uses; an image
# without instances and a cell named twice.  TEST_CASE: the test-time product on gathered rows.
CASES = {
    'a': dict(seed=11, B=2, E=5, H=7, W=9, grids=[3, 1, 2], counts=[[2, 1], [1, 0], [0, 0]]),
    'b': dict(seed=12, B=3, E=16, H=13, W=21, grids=[4, 2], counts=[[3, 0, 2], [1, 0, 4]], dups=[(0, 0, 2)]),
}
TEST_CASE = dict(seed=13, E=16, h=7, w=9, rows_all=12, rows=[5, 0, 5, 11])


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def make_case(seed, B, E, H, W, grids, counts, dups=(), integers=False):
    """Seeded inputs of one training-layout case as numpy arrays.  ``counts[l][b]`` rows for (level, image); ``dups`` lists (level, image,
    times): the first cell of that segment is named ``times`` times in a row (counts include the repeats).  ``integers``: feature and kernels
    integer-valued in [-15, 15], upstream gradient in [-7, 7] -- every partial sum of every product below stays an integer below 2^24 in any
    order (E <= 1024, H*W <= 2^14), so fp32 is exact."""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-15, 16, size=s).astype(np.float32)) if integers else (lambda *s: rng.standard_normal(s).astype(np.float32))
    feat = draw(B, E, H, W)
    maps = [draw(B, E, S, S) for S in grids]
    if not integers:
        feat *= 0.5
        maps = [m * (1.0 / np.sqrt(E)) for m in maps]
    order = []
    for l, S in enumerate(grids):
        row = []
        for b in range(B):
            n = int(counts[l][b])
            times = max([t for (dl, db, t) in dups if dl == l and db == b] + [1])
            fresh = n - (times - 1)
            assert 0 <= fresh <= S * S and (n == 0 or fresh >= 1), (l, b, n, times, S)
            cells = rng.permutation(S * S)[:fresh]
            cells = np.concatenate([np.repeat(cells[:1], times), cells[1:]]) if n else np.zeros(0, np.int64)
            row.append(cells.astype(np.int64))
        order.append(row)
    N = int(sum(sum(c) for c in counts))
    g = rng.integers(-7, 8, size=(N, H, W)).astype(np.float32) if integers else rng.standard_normal((N, H, W)).astype(np.float32)
    return dict(feat=feat, maps=[np.ascontiguousarray(m, dtype=np.float32) for m in maps], order=order, g=g, grids=list(grids), N=N)


def to_torch(case, dtype=torch.float64, device='cpu', requires_grad=False):
    feat = torch.from_numpy(case['feat']).to(device=device, dtype=dtype).requires_grad_(requires_grad)
    maps = [torch.from_numpy(m).to(device=device, dtype=dtype).requires_grad_(requires_grad) for m in case['maps']]
    order = [[torch.from_numpy(o).to(device) for o in row] for row in case['order']]
    g = torch.from_numpy(case['g']).to(device=device, dtype=dtype)
    return feat, maps, order, g


def cat_levels(masks):
    """The non-empty levels concatenated: the [N,H,W] buffer in row order (None when there is no row)."""
    live = [m for m in masks if m is not None]
    return torch.cat(live, 0) if live else None


def run_ref(case, dtype, sigmoid=True):
    """The restatement on the CPU in ``dtype`` with the case's upstream gradient: (masks [N,H,W], grad_feat, [grad_map per level]) as
    float64 numpy arrays; zero gradients and an empty mask array when the case has no row."""
    feat, maps, order, g = to_torch(case, dtype, requires_grad=True)
    masks, _ = dynamic_masks(maps, order, feat, sigmoid)
    out = cat_levels(masks)
    if out is None:
        return np.zeros((0,) + case['feat'].shape[-2:]), np.zeros(case['feat'].shape), [np.zeros(m.shape) for m in case['maps']]
    (out * g).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                                    # noqa: E731
    return out.detach().double().numpy(), zero(feat).double().numpy(), [zero(m).double().numpy() for m in maps]


def bound(q32, q64):
    """4 x the restatement's own fp32 error, relative to the largest fp64 value."""
    q32, q64 = np.asarray(q32, np.float64), np.asarray(q64, np.float64)
    top = float(np.abs(q64).max()) if q64.size else 0.0
    return 4.0 * float(np.abs(q32 - q64).max()) / top if top > 0 else 0.0


def assert_within(got, q64, tol, what):
    got, q64 = np.asarray(got, np.float64), np.asarray(q64, np.float64)
    assert got.shape == q64.shape, (what, got.shape, q64.shape)
    if q64.size == 0:
        return
    top = float(np.abs(q64).max())
    err = float(np.abs(got - q64).max())
    print(f'{what}: max error {err:.3e}, allowed {tol * top:.3e} (relative bound {tol:.3e}, largest value {top:.3e})')
    assert np.isfinite(got).all() and err <= tol * top, (what, err, tol * top)
