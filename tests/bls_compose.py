"""``BoxSOLOv2Head.loss`` (box_solov2_head.py:259-388) composed from the package's modules as they existed before
boxinstseg_amd/boxlevelset_loss.py: box_solov2_targets, box_solov2_set_cells, box_solov2_ins_preds, BoxProjectionLoss, LevelsetLoss,
MinimumSpanningTree, TreeFilter2D, solo_cate_loss, with the reference's statements in between -- the level loop, the resize per (level,
image), the per-row repeats and one tree per row.  GPU only.  What tests/test_gpu_bls_whole.py compares ``box_solov2_loss`` with and
tools/box_solov2_loss_bench.py times it against; ``share=True`` is the same loop with the trees, the breadth-first orders and the edge
weights built once per (size, image) by hand and an image's rows filtered as channels -- the best a user could do with those modules.

``restate`` is the same computation in torch on the CPU (tests/bls_loss_ref.py) from the head's raw outputs, for a given assignment."""
import numpy as np
import torch
import torch.nn.functional as F

W_IMG, W_FEAT = 0.05, 5.0


def compose_loss(kernel_preds, cate_preds, feature_pred, levelset_feats, gt_bbox_list, gt_label_list, gt_mask_list, img, head_cfg, level_sizes,
                 share=False):
    import boxinstseg_amd as B
    from boxinstseg_amd.tree_filter import _bfs_levels, _Refine
    head = B.parse_solo_head_cfg(head_cfg)
    loss_boxpro = B.BoxProjectionLoss(head_cfg['loss_boxpro']['loss_weight'])
    loss_levelset = B.LevelsetLoss(head_cfg['loss_levelset']['loss_weight'])
    mst, tree_filter = B.MinimumSpanningTree(B.TreeFilter2D.norm2_distance), B.TreeFilter2D()
    targets = B.box_solov2_targets(gt_bbox_list, gt_label_list, gt_mask_list, level_sizes,
                                   **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')})
    cells = B.box_solov2_set_cells(targets)
    ins_preds = B.box_solov2_ins_preds(kernel_preds, feature_pred, cells, level_sizes)
    ins_labels = targets.ins_labels()
    nb = img.shape[0]
    shared = {}
    loss_project, loss_levelset_rows = [], []
    for l, size in enumerate(level_sizes):
        n = [int(targets.counts[l][b][1]) for b in range(nb)]
        if sum(n) == 0:
            continue
        size = tuple(size)
        if share and size in shared:
            scale_img, scale_lst, orders = shared[size]
        else:
            scale_img = [F.interpolate(img[i].unsqueeze(dim=0), size=size, mode='bilinear') for i in range(nb)]
            scale_lst = [F.interpolate(levelset_feats[i].unsqueeze(dim=0), size=size, mode='bilinear') for i in range(nb)]
            orders = None
            if share:
                orders = []
                for i in range(nb):
                    io, lo = _bfs_levels(mst(scale_img[i]), 4), _bfs_levels(mst(scale_lst[i]), 4)
                    orders.append((io, tree_filter.build_edge_weight(scale_img[i], io[0], io[1], True), lo,
                                   tree_filter.build_edge_weight(scale_lst[i], lo[0], lo[1], False)))
                shared[size] = (scale_img, scale_lst, orders)
        img_target = torch.cat([scale_img[i].repeat(n[i], 1, 1, 1) for i in range(nb)], 0)
        mask_pred = torch.sigmoid(ins_preds[l].unsqueeze(dim=1))
        box_mask_target = ins_labels[l].unsqueeze(dim=1).to(dtype=mask_pred.dtype)
        loss_project.append(loss_boxpro(mask_pred, box_mask_target))
        mask_scores_phi = torch.cat((mask_pred, 1.0 - mask_pred), dim=1) * box_mask_target
        pixel_num = torch.clamp(box_mask_target.sum((1, 2, 3)), min=1)
        loss_img_lst = loss_levelset(mask_scores_phi, img_target * box_mask_target, pixel_num) * W_IMG
        if share:
            ys, zs, at = [], [], 0
            for i in range(nb):
                if n[i] == 0:
                    continue
                io, w_img, lo, w_lst = orders[i]
                x = mask_pred[at:at + n[i], 0].reshape(1, n[i], -1)
                y = _Refine.apply(x, w_img, io[0], io[1], io[2], True, io[3])
                z = _Refine.apply(y, w_lst, lo[0], lo[1], lo[2], False, lo[3])
                ys.append(y.view(n[i], 1, *size))
                zs.append(z.view(n[i], 1, *size))
                at += n[i]
            deep_img, deep_lst = torch.cat(ys), torch.cat(zs)
        else:
            lst_target = torch.cat([scale_lst[i].expand(n[i], -1, -1, -1) for i in range(nb)], 0)
            deep_img = tree_filter(mask_pred, img_target, mst(img_target))
            deep_lst = tree_filter(deep_img, lst_target, mst(lst_target), low_tree=False)
        high_feature = torch.cat((deep_img, deep_lst), dim=1) * box_mask_target
        loss_levelset_rows.append(loss_img_lst + loss_levelset(mask_scores_phi, high_feature, pixel_num) * W_FEAT)
    loss_cate = B.solo_cate_loss(list(cate_preds), targets.flat_cate_labels, targets.num_ins, head['gamma'], head['alpha'], head['loss_weight_cate'])
    return dict(loss_boxpro=torch.cat(loss_project).mean(), loss_levelset=torch.cat(loss_levelset_rows).mean(), loss_cate=loss_cate), targets


def restate(kernel_preds, feature_pred, levelset_feats, img, cells, sel_inst, masks, level_sizes, dtype, w_boxpro, w_levelset):
    """From numpy inputs and a given assignment (``cells[l][b]`` and ``sel_inst[l]`` as integer arrays, ``masks[l]`` uint8 [G,h_l,w_l]):
    the set cells' dynamic convolution and resize (:205-216, :317-320) and tests/bls_loss_ref.all_levels on the CPU in ``dtype``.
    -> (result dict of all_levels, gradients of kernel_preds, feature_pred, levelset_feats as numpy float64)."""
    from tests import bls_loss_ref as R
    kern = [torch.from_numpy(k).to(dtype).requires_grad_(True) for k in kernel_preds]
    feat = torch.from_numpy(feature_pred).to(dtype).requires_grad_(True)
    lst = torch.from_numpy(levelset_feats).to(dtype).requires_grad_(True)
    nb, E = feat.shape[:2]
    ins_preds, img_of = [], []
    for l, size in enumerate(level_sizes):
        per, owner = [], []
        for b in range(nb):
            c = torch.as_tensor(np.asarray(cells[l][b]), dtype=torch.long)
            if len(c) == 0:
                continue
            k = kern[l][b].reshape(E, -1)[:, c].t()
            ins = torch.einsum('ne,ehw->nhw', k, feat[b])
            per.append(F.interpolate(ins.unsqueeze(0), size=tuple(size), mode='bilinear', align_corners=False)[0])
            owner += [b] * len(c)
        ins_preds.append(torch.cat(per) if per else feat.new_zeros((0,) + tuple(size)).requires_grad_(True))
        img_of.append(np.array(owner, np.int64))
    out = R.all_levels(ins_preds, masks, [np.asarray(s) for s in sel_inst], img_of, img, lst, level_sizes, dtype, None, w_boxpro, w_levelset)
    z = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy().astype(np.float64)
    return out, [z(k) for k in kern], z(feat), z(lst)
