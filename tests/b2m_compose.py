"""``Box2MaskHead.loss_single`` / ``loss`` (box2mask_head.py:192-335) composed per layer from the package's modules as they existed before
boxinstseg_amd/box2mask_loss.py: box2mask_get_targets, BoxProjectionLoss, LevelsetLoss, LCM, MinimumSpanningTree, TreeFilter2D, with the
reference's statements in between -- the per-instance repeats, the boolean index and the ``.cpu()`` of :274 included.  GPU only.
What tests/test_gpu_b2m_loss.py compares ``box2mask_loss`` with and tools/box2mask_loss_bench.py times it against."""
import torch
import torch.nn.functional as F


def _scale_target(t, scaled_size):
    if t.dim() == 3:
        t = t.unsqueeze(1)
    return F.interpolate(t, size=tuple(scaled_size), mode='bilinear', align_corners=False)


def loss_single(cls_scores, mask_preds, lst_feat, gt_labels_list, gt_masks_list, norm_img, *, assigner, class_weight, loss_cls_weight,
                loss_box, loss_mask, num_classes, scaled_size=(96, 96)):
    from boxinstseg_amd import LCM, BoxProjectionLoss, LevelsetLoss, MinimumSpanningTree, TreeFilter2D, box2mask_get_targets
    pred_shape = mask_preds.shape[-2:]
    norm_img = F.interpolate(norm_img, pred_shape, mode='bilinear', align_corners=False)
    lst_feat = F.interpolate(lst_feat, pred_shape, mode='bilinear', align_corners=False)
    num_imgs = cls_scores.size(0)
    labels_list, label_weights_list, mask_targets_list, mask_weights_list, _, _ = box2mask_get_targets(
        cls_scores, mask_preds, gt_labels_list, gt_masks_list, assigner, num_classes)
    labels = torch.stack(labels_list, dim=0).flatten(0, 1)
    label_weights = torch.stack(label_weights_list, dim=0).flatten(0, 1)
    mask_targets = torch.cat(mask_targets_list, dim=0)
    mask_weights = torch.stack(mask_weights_list, dim=0)
    cw = cls_scores.new_tensor(class_weight)
    ce = F.cross_entropy(cls_scores.flatten(0, 1), labels, weight=cw, reduction='none') * label_weights
    loss_cls = loss_cls_weight * ce.sum() / (cw[labels].sum() + torch.finfo(torch.float32).eps)
    mask_preds = mask_preds[mask_weights > 0]
    if mask_targets.shape[0] == 0:
        return loss_cls, mask_preds.sum(), mask_preds.sum()
    mst, tree_filter = MinimumSpanningTree(TreeFilter2D.norm2_distance), TreeFilter2D()
    scale_img, scale_feat = _scale_target(norm_img, scaled_size), _scale_target(lst_feat, scaled_size)
    norm_img_tree, lst_feat_tree = mst(scale_img), mst(scale_feat)
    target_img_idx = mask_weights.sum(dim=1).cpu().numpy().tolist()
    img_l, lst_l, it_l, ft_l = [], [], [], []
    for i in range(num_imgs):
        repeat_num = int(target_img_idx[i])
        if repeat_num == 0:
            continue
        img_l.append(norm_img[i:i + 1].repeat(repeat_num, 1, 1, 1))
        lst_l.append(lst_feat[i:i + 1].repeat(repeat_num, 1, 1, 1))
        it_l.append(norm_img_tree[i:i + 1].repeat(repeat_num, 1, 1))
        ft_l.append(lst_feat_tree[i:i + 1].repeat(repeat_num, 1, 1))
    img_targets, lst_targets = torch.cat(img_l, dim=0), torch.cat(lst_l, dim=0)
    target_img_tree, target_feat_tree = torch.cat(it_l, dim=0), torch.cat(ft_l, dim=0)
    box_mask_targets = F.interpolate(mask_targets.to(mask_preds.dtype), pred_shape, mode='bilinear', align_corners=False)
    mask_preds = torch.sigmoid(mask_preds.unsqueeze(dim=1))
    loss_project = BoxProjectionLoss(loss_box)(mask_preds, box_mask_targets).mean()
    mask_scores_phi = torch.cat((mask_preds, 1.0 - mask_preds), dim=1) * box_mask_targets
    img_target_wbox = img_targets * box_mask_targets
    pixel_num = torch.clamp(box_mask_targets.sum((1, 2, 3)), min=1)
    levelset = LevelsetLoss(loss_mask)
    loss_img_lst = levelset(mask_scores_phi, img_target_wbox, pixel_num).mean() * 0.05
    img_targets, lst_targets = _scale_target(img_targets, scaled_size), _scale_target(lst_targets, scaled_size)
    mask_preds = _scale_target(mask_preds, scaled_size)
    s_img = tree_filter(feature_in=mask_preds, embed_in=img_targets, tree=target_img_tree)
    s_lst = tree_filter(s_img, lst_targets, target_feat_tree, low_tree=False)
    deep = torch.cat((F.interpolate(s_img, pred_shape, mode='bilinear', align_corners=False),
                      F.interpolate(s_lst, pred_shape, mode='bilinear', align_corners=False)), dim=1) * box_mask_targets
    loss_feat_lst = levelset(mask_scores_phi, deep, pixel_num).mean() * 5.0
    loss_lcm = 0.2 * LCM(img_targets, mask_preds, _scale_target(box_mask_targets, scaled_size))
    return loss_cls, loss_project, loss_img_lst + loss_feat_lst + loss_lcm


def loss(all_cls_scores, all_mask_preds, lst_feat, gt_labels_list, gt_masks_list, norm_img, **kw):
    """:192-221: ``loss_single`` per layer, the dict keyed as the reference keys it."""
    per = [loss_single(c, m, lst_feat, gt_labels_list, gt_masks_list, norm_img, **kw) for c, m in zip(all_cls_scores, all_mask_preds)]
    out = dict(loss_cls=per[-1][0], loss_project=per[-1][1], loss_levelset=per[-1][2])
    for i, (a, b, c) in enumerate(per[:-1]):
        out[f'd{i}.loss_cls'], out[f'd{i}.loss_project'], out[f'd{i}.loss_levelset'] = a, b, c
    return out
