"""A literal restatement of ``Box2MaskHead.loss_single`` after its classification loss (mmdet/models/dense_heads/box2mask_head.py:260-335)
for the tests of boxinstseg_amd/box2mask_loss.py: per layer and per matched instance, WITH the reference's per-instance repeats of the
image, the level-set feature and both trees (:280-297), torch on the CPU, in float32 or float64.

It is deliberately not the shared-per-image form of the package: it is what proves the sharing equal.  The losses are the reference's
arithmetic restated (levelset_loss.py:13-45 LevelsetLoss / region_levelset, :64-126 LCM / LocalConsistencyModule,
box_projection_loss.py:11-42); the tree filter is a torch.autograd.Function over the fp64 oracle of oracle/tree_filter_oracle.py
(with tests/tree_filter_ref.embed_grad; instances whose copies of tree and embedding are byte-identical run as channels of one call).
No GPU, no library."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tree_filter_oracle as tfo
from tests import tree_filter_ref as tfr

W_IMG, W_FEAT, W_LCM = 0.05, 5.0, 0.2


def scale_target(t, scaled_size=(96, 96)):
    """mmdet/models/utils/misc.py:75-86"""
    if t.dim() == 3:
        t = t.unsqueeze(1)
    return F.interpolate(t, size=tuple(scaled_size), mode='bilinear', align_corners=False)


def mst_trees(fm):
    """MinimumSpanningTree(norm2_distance)(fm [B,C,H,W]) (tree_filter.py:10-63) -> int32 [B,V-1,2], edges in ascending edge order."""
    fm = fm.detach().cpu().numpy().astype(np.float32)
    B, _, H, W = fm.shape
    index = tfo.grid_edges(H, W)
    return np.stack([index[tfo.mst_edges(index, tfo.grid_weights(fm[b]), H * W)] for b in range(B)]).astype(np.int32)


def _groups(emb, trees):
    """Instances that carry byte-identical copies of one tree and one embedding (the reference's repeats of an image, :280-297), in order
    of first appearance.  The oracle treats channels independently, so such a group is evaluated as the channels of ONE oracle call: the
    same numbers as one call per instance at a fraction of the Python time.  The weight gradient of a group is then the sum over its
    instances, which is all autograd keeps of the per-instance embedding gradients once it adds them up through the repeat."""
    found = {}
    for n in range(emb.shape[0]):
        found.setdefault((np.ascontiguousarray(trees[n]).tobytes(), np.ascontiguousarray(emb[n]).tobytes()), []).append(n)
    return list(found.values())


class _TreeFilter(torch.autograd.Function):
    """TreeFilter2D()(feature_in [N,1,H,W], embed_in [N,Ce,H,W], tree [N,V-1,2], low_tree) (tree_filter.py:66-150), sigma 0.02, one group,
    in fp64 through oracle/tree_filter_oracle.py whatever the tensors' dtype.  ``info`` (a dict) collects 'gw_absmax': per group of the
    backward on the high-level tree (first instance, max |d loss / d w| of the group's summed weight gradient)."""

    @staticmethod
    def forward(ctx, feat, emb, trees, low_tree, info):
        f, e = feat.detach().numpy().astype(np.float64), emb.detach().numpy()
        N, _, H, W = f.shape
        V = H * W
        out = np.empty((N, 1, V))
        saved = []
        for rows in _groups(e, trees):
            si, sp, sc = tfo.bfs_order(np.ascontiguousarray(trees[rows[0]]), V)
            w = tfo.edge_weights(e[rows[0]].reshape(-1, V).astype(np.float64), si, sp, low_tree, 0.02)
            x = f[rows, 0].reshape(len(rows), V)
            y, keep = tfo.refine_forward(x, w, si, sp, sc)
            out[rows, 0] = y
            saved.append((rows, si, sp, sc, w, x, keep))
        ctx.saved = (saved, low_tree, info, feat.dtype, emb.dtype, tuple(feat.shape), tuple(emb.shape), e)
        return torch.from_numpy(out.reshape(N, 1, H, W)).to(feat.dtype)

    @staticmethod
    def backward(ctx, g):
        saved, low_tree, info, fdt, edt, fshape, eshape, e = ctx.saved
        N, _, H, W = fshape
        V = H * W
        go = g.detach().numpy().astype(np.float64).reshape(N, V)
        dfeat = np.empty((N, 1, V))
        demb = None if low_tree else np.zeros((N, eshape[1], V))
        for rows, si, sp, sc, w, x, keep in saved:
            dfeat[rows, 0] = tfo.refine_backward_feature(go[rows], w, si, sp, sc, keep)
            if not low_tree:
                gw = tfo.refine_backward_weight(x, go[rows], w, si, sp, sc, keep)
                demb[rows[0]] = tfr.embed_grad(e[rows[0]].reshape(-1, V), gw, si, sp, False, 0.02)
                if info is not None:
                    info.setdefault('gw_absmax', []).append((rows[0], float(np.abs(gw).max())))
        return (torch.from_numpy(dfeat.reshape(fshape)).to(fdt), None if demb is None else torch.from_numpy(demb.reshape(eshape)).to(edt),
                None, None, None)


def box_projection_loss(mask_scores, box_bitmask, loss_weight):
    def dice(x, target):
        n = x.size(0)
        x, target = x.reshape(n, -1), target.reshape(n, -1)
        inter = (x * target).sum(dim=1)
        union = (x ** 2.0).sum(dim=1) + (target ** 2.0).sum(dim=1) + 1e-5
        return 1. - (2 * inter / union)
    ly = dice(mask_scores.max(dim=2, keepdim=True)[0], box_bitmask.max(dim=2, keepdim=True)[0])
    lx = dice(mask_scores.max(dim=3, keepdim=True)[0], box_bitmask.max(dim=3, keepdim=True)[0])
    return loss_weight * (lx + ly)


def levelset_loss(mask_score, lst_target, pixel_num, loss_weight):
    f, b = mask_score[:, 0, :, :].unsqueeze(1), mask_score[:, 1, :, :].unsqueeze(1)
    interior = torch.sum(f * lst_target, (2, 3)) / torch.sum(f, (2, 3)).clamp(min=0.00001)
    exterior = torch.sum(b * lst_target, (2, 3)) / torch.sum(b, (2, 3)).clamp(min=0.00001)
    il = torch.pow(lst_target - interior.unsqueeze(-1).unsqueeze(-1), 2)
    el = torch.pow(lst_target - exterior.unsqueeze(-1).unsqueeze(-1), 2)
    return loss_weight * (torch.sum(il * f + el * b, (1, 2, 3)) / lst_target.shape[1] / pixel_num)


def _neighbours(x, d=2):
    b, c, h, w = x.shape
    kernel = torch.zeros(8, 1, 3, 3, dtype=x.dtype)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2))):
        kernel[k, 0, i, j] = 1
    pad = F.pad(x, [d] * 4, mode='replicate')
    pad = pad.reshape(b * c, -1, pad.shape[-2], pad.shape[-1])
    return F.conv2d(pad, kernel, dilation=d).view(b, c, -1, h, w)


def lcm(imgs, pred_phis, box_targets, iters=10, alpha=0.3):
    nb = _neighbours(imgs)
    rep = imgs.unsqueeze(2).repeat(1, 1, nb.shape[2], 1, 1)
    aff = -(torch.abs(nb - rep) / (torch.std(nb, dim=2, keepdim=True) + 1e-8) / alpha) ** 2
    aff = F.softmax(aff.mean(dim=1, keepdim=True), dim=2)
    refine = pred_phis
    for _ in range(iters):
        refine = (_neighbours(refine) * aff).sum(2)
    consist = (torch.abs(refine - pred_phis) * box_targets).sum()
    return consist / box_targets.sum().clamp(min=1)


def loss_single_masks(mask_preds, lst_feat, norm_img, gt_masks_list, pos_inds, pos_gt_inds, scaled_size=(96, 96), trees=None,
                      loss_box_weight=1.0, loss_mask_weight=1.0, info=None):
    """:230-233 and :260-335 for one layer.  ``mask_preds`` [B,Q,h,w], ``lst_feat`` [B,Cf,hf,wf], ``norm_img`` [B,3,H,W] of one dtype on
    the CPU; per image ``gt_masks`` [G_i,H,W], ``pos_inds`` (ascending queries) and ``pos_gt_inds`` as integer sequences.
    ``trees`` = (img_tree, lst_tree) numpy [B,V-1,2] replaces the two ``self.mst`` calls.  -> (loss_project, loss_levelset)."""
    dtype = mask_preds.dtype
    pred_shape = mask_preds.shape[-2:]
    norm_img = F.interpolate(norm_img, pred_shape, mode='bilinear', align_corners=False)
    lst_feat = F.interpolate(lst_feat, pred_shape, mode='bilinear', align_corners=False)
    num_imgs, Q = mask_preds.shape[:2]
    mask_weights = torch.zeros((num_imgs, Q), dtype=dtype)
    mask_targets_list = []
    for i in range(num_imgs):
        mask_weights[i, torch.as_tensor(list(pos_inds[i]), dtype=torch.long)] = 1.0
        gm = gt_masks_list[i] if gt_masks_list[i].dim() == 4 else gt_masks_list[i].unsqueeze(1)
        mask_targets_list.append(gm[torch.as_tensor(list(pos_gt_inds[i]), dtype=torch.long)])
    mask_targets = torch.cat(mask_targets_list, dim=0)
    mask_preds = mask_preds[mask_weights > 0]
    if mask_targets.shape[0] == 0:
        return mask_preds.sum(), mask_preds.sum()
    scale_img = scale_target(norm_img, scaled_size)
    scale_feat = scale_target(lst_feat, scaled_size)
    norm_img_tree, lst_feat_tree = (mst_trees(scale_img), mst_trees(scale_feat)) if trees is None else trees
    target_img_idx = mask_weights.sum(dim=1).numpy().tolist()
    img_l, lst_l, it_l, ft_l = [], [], [], []
    for i in range(num_imgs):
        repeat_num = int(target_img_idx[i])
        if repeat_num == 0:
            continue
        img_l.append(norm_img[i:i + 1].repeat(repeat_num, 1, 1, 1))
        lst_l.append(lst_feat[i:i + 1].repeat(repeat_num, 1, 1, 1))
        it_l.append(np.repeat(norm_img_tree[i:i + 1], repeat_num, 0))
        ft_l.append(np.repeat(lst_feat_tree[i:i + 1], repeat_num, 0))
    img_targets, lst_targets = torch.cat(img_l, dim=0), torch.cat(lst_l, dim=0)
    target_img_tree, target_feat_tree = np.concatenate(it_l), np.concatenate(ft_l)

    box_mask_targets = F.interpolate(mask_targets.to(dtype), pred_shape, mode='bilinear', align_corners=False)
    mask_preds = torch.sigmoid(mask_preds.unsqueeze(dim=1))
    loss_project = box_projection_loss(mask_preds, box_mask_targets, loss_box_weight).mean()
    back_scores = 1.0 - mask_preds
    mask_scores_concat = torch.cat((mask_preds, back_scores), dim=1)
    mask_scores_phi = mask_scores_concat * box_mask_targets
    img_target_wbox = img_targets * box_mask_targets
    pixel_num = torch.clamp(box_mask_targets.sum((1, 2, 3)), min=1)
    loss_img_lst = levelset_loss(mask_scores_phi, img_target_wbox, pixel_num, loss_mask_weight).mean() * W_IMG
    img_targets = scale_target(img_targets, scaled_size)
    lst_targets = scale_target(lst_targets, scaled_size)
    mask_preds = scale_target(mask_preds, scaled_size)
    stru_img_s = _TreeFilter.apply(mask_preds, img_targets, target_img_tree, True, info)
    stru_lst_s = _TreeFilter.apply(stru_img_s, lst_targets, target_feat_tree, False, info)
    stru_img = F.interpolate(stru_img_s, pred_shape, mode='bilinear', align_corners=False)
    stru_lst = F.interpolate(stru_lst_s, pred_shape, mode='bilinear', align_corners=False)
    deep_stru_feats = torch.cat((stru_img, stru_lst), dim=1) * box_mask_targets
    loss_feat_lst = levelset_loss(mask_scores_phi, deep_stru_feats, pixel_num, loss_mask_weight).mean() * W_FEAT
    box_mask_targets = scale_target(box_mask_targets, scaled_size)
    loss_lcm = W_LCM * lcm(img_targets, mask_preds, box_mask_targets)
    return loss_project, loss_img_lst + loss_feat_lst + loss_lcm


def all_layers(all_mask_preds, lst_feat, norm_img, gt_masks_list, pos_inds, pos_gt_inds, dtype, scaled_size=(96, 96), trees=None,
               loss_box_weight=1.0, loss_mask_weight=1.0, g_project=None, g_levelset=None):
    """``loss_single_masks`` for every layer (``pos_inds[l][i]`` / ``pos_gt_inds[l][i]``: layer l, image i) in ``dtype``, and the gradients
    of sum_l (g_project[l] * loss_project[l] + g_levelset[l] * loss_levelset[l]) -- ones by default.
    -> dict: loss_project [L], loss_levelset [L], grads (list of [B,Q,h,w]), lst_grad, gw_sum [B] (per image the sum over the
    layers of max |d loss / d w| of the high-level tree, the gradient summed over the image's instances of the layer: an upper bound of
    the magnitude of the weight gradient that one filter call over the rows of all layers returns)."""
    L = len(all_mask_preds)
    mps = [torch.as_tensor(m).to(dtype).clone().requires_grad_(True) for m in all_mask_preds]
    lf = torch.as_tensor(lst_feat).to(dtype).clone().requires_grad_(True)
    img = torch.as_tensor(norm_img).to(dtype)
    gts = [torch.as_tensor(g).to(dtype) for g in gt_masks_list]
    gp = [1.0] * L if g_project is None else list(g_project)
    gl = [1.0] * L if g_levelset is None else list(g_levelset)
    lp, ll = [], []
    B = img.shape[0]
    gw_sum = np.zeros(B)
    for l in range(L):
        info = {}
        a, b = loss_single_masks(mps[l], lf, img, gts, pos_inds[l], pos_gt_inds[l], scaled_size, trees, loss_box_weight, loss_mask_weight, info)
        lp.append(a)
        ll.append(b)
        layer_total = gp[l] * a + gl[l] * b
        if layer_total.requires_grad:
            layer_total.backward()
        if 'gw_absmax' in info:
            owner = np.concatenate([np.full(len(pos_inds[l][i]), i) for i in range(B)])
            for first, gmax in info['gw_absmax']:
                gw_sum[owner[first]] += gmax
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss_project=torch.stack([v.detach() for v in lp]).numpy().astype(np.float64),
                loss_levelset=torch.stack([v.detach() for v in ll]).numpy().astype(np.float64),
                grads=[zero(m).numpy().astype(np.float64) for m in mps], lst_grad=zero(lf).numpy().astype(np.float64), gw_sum=gw_sum)
