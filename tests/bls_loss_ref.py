"""A literal restatement of the mask part of ``BoxSOLOv2Head.loss`` (mmdet/models/dense_heads/box_solov2_head.py:334-367, with the resizes
of :412-416 and the per-row repeats of :300-314 in front) for the tests of boxinstseg_amd/boxlevelset_loss.py: per level and per set
cell, WITH the reference's per-row copies of the resized image and level-set feature and one tree per copy, torch on the CPU, in
float32 or float64.

It is deliberately not the shared-per-(size, image) form of the package: it is what proves the sharing equal.  The losses and the tree
filter are those of tests/b2m_loss_ref.py (box_projection_loss, levelset_loss, _TreeFilter over the fp64 oracle, mst_trees).  Rows whose
tgt_of / img_of is -1 are dropped before anything is computed: the reference never sees them.  No GPU, no library."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.b2m_loss_ref import _TreeFilter, box_projection_loss, levelset_loss, mst_trees

W_IMG, W_FEAT = 0.05, 5.0                              # :351, :360


def level_rows(ins_pred, box_mask, img_target, lst_target, trees, w_boxpro, w_levelset, info):
    """The body of the loop :338-364 for one level: ``ins_pred`` [N,h,w] logits, ``box_mask`` [N,h,w] uint8, ``img_target`` [N,3,h,w],
    ``lst_target`` [N,Cf,h,w] (the per-row copies), ``trees`` = (img_tree, lst_tree) numpy [N,V-1,2] or None for ``self.mst``.
    -> (loss_project [N], loss_levelset_term [N])."""
    mask_pred = torch.sigmoid(ins_pred.unsqueeze(dim=1))
    box_mask_target = box_mask.unsqueeze(dim=1).to(dtype=mask_pred.dtype)
    loss_project = box_projection_loss(mask_pred, box_mask_target, w_boxpro)
    back_scores = 1.0 - mask_pred
    mask_scores_concat = torch.cat((mask_pred, back_scores), dim=1)
    mask_scores_phi = mask_scores_concat * box_mask_target
    img_target_wbox = img_target * box_mask_target
    pixel_num = box_mask_target.sum((1, 2, 3))
    pixel_num = torch.clamp(pixel_num, min=1)
    loss_img_lst = levelset_loss(mask_scores_phi, img_target_wbox, pixel_num, w_levelset) * W_IMG
    img_mst_tree = mst_trees(img_target) if trees is None else trees[0]
    deep_stru_feature_img = _TreeFilter.apply(mask_pred, img_target, img_mst_tree, True, None)
    lst_mst_tree = mst_trees(lst_target) if trees is None else trees[1]
    deep_stru_feature_lst = _TreeFilter.apply(deep_stru_feature_img, lst_target, lst_mst_tree, False, info)
    high_feature = torch.cat((deep_stru_feature_img, deep_stru_feature_lst), dim=1) * box_mask_target
    loss_feat_lst = levelset_loss(mask_scores_phi, high_feature, pixel_num, w_levelset) * W_FEAT
    return loss_project, loss_img_lst + loss_feat_lst


def all_levels(ins_preds, masks, tgt_of, img_of, norm_img, lst_feat, level_sizes, dtype, trees=None, w_boxpro=1.0, w_levelset=1.0):
    """``ins_preds``: per level [N_l,h_l,w_l]; ``masks``: per level uint8 [G,h_l,w_l]; ``tgt_of`` / ``img_of``: per level integer arrays
    [N_l] (-1: the row is dropped); ``norm_img`` [B,3,H,W], ``lst_feat`` [B,Cf,hf,wf]; ``trees``: None, or per distinct size (in order
    of first appearance) a pair (img_tree, lst_tree) of numpy [B,V-1,2].  Runs :334-367 in ``dtype`` and backpropagates
    loss_boxpro + loss_levelset.
    -> dict: loss_boxpro, loss_levelset (floats), proj / levelset (per level [N_l] float64, zeros in dropped rows), grads (per level
    [N_l,h,w] float64), lst_grad, gw_sum [groups, B]: per (size, image) the sum over the size's levels of max |d loss / d w| of the
    high-level tree summed over the level's rows of that image -- an upper bound of the weight gradient that one filter call over the
    image's rows of all the size's levels returns."""
    sizes = list(dict.fromkeys(tuple(s) for s in level_sizes))
    # (a tensor that already carries a graph is taken as it is: the caller reads the gradients of its own leaves)
    own = lambda t: t if torch.is_tensor(t) and t.requires_grad else torch.as_tensor(t).to(dtype).clone().requires_grad_(True)
    preds = [own(p) for p in ins_preds]
    lf = own(lst_feat)
    img = torch.as_tensor(norm_img).to(dtype)
    B = img.shape[0]
    gw_sum = np.zeros((len(sizes), B))
    loss_project, loss_levelset = [], []
    proj = [np.zeros(len(p)) for p in ins_preds]
    levelset = [np.zeros(len(p)) for p in ins_preds]
    infos = []
    for l, size in enumerate(level_sizes):
        t_of, i_of = np.asarray(tgt_of[l]).astype(np.int64), np.asarray(img_of[l]).astype(np.int64)
        live = np.nonzero((t_of >= 0) & (t_of < len(masks[l])) & (i_of >= 0) & (i_of < B))[0]
        if len(live) == 0:                                   # :335-336
            continue
        g = sizes.index(tuple(size))
        # :412-416, per image; :300-314, the per-row copies
        scale_img = torch.cat([F.interpolate(img[i].unsqueeze(dim=0), size=tuple(size), mode='bilinear') for i in range(B)])
        scale_lst = torch.cat([F.interpolate(lf[i].unsqueeze(dim=0), size=tuple(size), mode='bilinear') for i in range(B)])
        sel = torch.from_numpy(i_of[live])
        img_target, lst_target = scale_img[sel], scale_lst[sel]
        row_trees = None if trees is None else (trees[g][0][i_of[live]], trees[g][1][i_of[live]])
        info = {}
        a, b = level_rows(preds[l][torch.from_numpy(live)], torch.as_tensor(masks[l])[torch.from_numpy(t_of[live])], img_target, lst_target,
                          row_trees, w_boxpro, w_levelset, info)
        loss_project.append(a)
        loss_levelset.append(b)
        proj[l][live], levelset[l][live] = a.detach().numpy(), b.detach().numpy()
        infos.append((g, i_of[live], info))
    zero = lambda t: np.zeros(t.shape) if not t.is_leaf or t.grad is None else t.grad.numpy().astype(np.float64)
    if not loss_project:
        return dict(loss_boxpro=0.0, loss_levelset=0.0, proj=proj, levelset=levelset, grads=[zero(p) for p in preds], lst_grad=zero(lf), gw_sum=gw_sum)
    loss_project = torch.cat(loss_project).mean()                # :366
    loss_levelset = torch.cat(loss_levelset).mean()              # :367
    (loss_project + loss_levelset).backward()
    for g, owner, info in infos:                                 # filled by the backward of the high-level filter
        for first, gmax in info.get('gw_absmax', []):
            gw_sum[g, owner[first]] += gmax
    return dict(loss_boxpro=float(loss_project.detach()), loss_levelset=float(loss_levelset.detach()), proj=proj, levelset=levelset,
                grads=[zero(p) for p in preds], lst_grad=zero(lf), gw_sum=gw_sum)
