"""DiscoBoxSOLOv2Head.loss as a user had to write it before ``discobox_loss``: the reference's loops (discobox_head.py:1271-1339 and the
tail of corr_loss, :1127-1137) over the package's modules -- ``solov2_targets``, ``solo_dynamic_masks(_pair)``, ``MeanField``, ``mil_loss``,
``dice_loss``, ``corr_level``, ``solo_cate_loss``.  TEST INFRASTRUCTURE (tests/test_gpu_dbx_whole.py) and the competitor of
tools/discobox_loss_bench.py.  It synchronises where the reference does: one ``.sum()`` per level, one per (level, image), boolean indexing.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def compose_loss(cate_preds, s_kernel_preds_raw, t_kernel_preds_raw, s_ins_pred, t_ins_pred, gt_bbox_list, gt_label_list, gt_mask_list, img, *,
                 use_loss_ts, use_ind_teacher, use_corr, s_feat=None, t_feat=None, bank=None, solver=None, head_cfg, details=None):
    import boxinstseg_amd as B
    head, lcfg = B.parse_solo_head_cfg(head_cfg), B.parse_discobox_loss_cfg(head_cfg)
    H, W = int(s_ins_pred.shape[-2]), int(s_ins_pred.shape[-1])
    targets = B.solov2_targets(gt_bbox_list, gt_label_list, gt_mask_list, (H, W),
                               **{k: head[k] for k in ('scale_ranges', 'num_grids', 'strides', 'sigma', 'num_classes')})
    if use_ind_teacher:
        s_list, t_list, ind_list = B.solo_dynamic_masks_pair(s_kernel_preds_raw, t_kernel_preds_raw, targets, s_ins_pred, t_ins_pred, sigmoid=False)
    else:
        s_list, ind_list = B.solo_dynamic_masks(s_kernel_preds_raw, targets, s_ins_pred, sigmoid=False)
        t_list = s_list
    ins_labels, kernel_labels = targets.ins_labels(), targets.kernel_labels()
    color = F.interpolate(img.float(), (H, W), mode='bilinear', align_corners=True)
    mean_fields = [B.MeanField(c.unsqueeze(0), alpha0=lcfg['alpha0'], theta0=lcfg['theta0'], theta1=lcfg['theta1'], theta2=lcfg['theta2'],
                               iter=lcfg['max_iter'], kernel_size=lcfg['kernel'], base=lcfg['base']) for c in color]
    dev = s_ins_pred.device
    zero = torch.zeros((), device=dev)
    loss_ins, loss_ts, corr_ts, labels, labels_corr = [], [], [], [], []
    corr_sum, corr_num = zero.clone(), zero.clone()
    use_corr = bool(use_loss_ts and use_corr)
    ccfg = B.parse_corr_cfg(head_cfg) if use_corr else None
    at = 0
    for s_raw, t_raw, img_inds, target, klab in zip(s_list, t_list, ind_list, ins_labels, kernel_labels):
        if s_raw is None:
            continue
        first, at = at, at + int(s_raw.shape[0])                           # the level's rows in the level-major row order
        s_input = torch.sigmoid(s_raw)
        t_input = torch.sigmoid(t_raw) if use_ind_teacher else s_input
        iiu = None
        if use_corr:                                                       # the front of corr_loss for the level (:1018-1127), all rows
            ls, ni, iiu, _ = B.corr_level(s_raw, t_raw if use_ind_teacher else s_raw, target, img_inds, klab, s_feat[0], t_feat[0], bank, solver,
                                          ccfg['min_size'], ccfg['min_objs'], own_labels=False)
            corr_sum, corr_num = corr_sum + ls, corr_num + ni.float()
        mask = target.flatten(1).sum(1).bool()                             # remove all-zero target (:1281-1286)
        if int(mask.sum()) == 0:
            continue
        s_in, t_in, inds, tg = s_input[mask], t_input[mask], img_inds[mask], target[mask]
        loss_ins.append(B.mil_loss(B.dice_loss, s_in, s_in, tg))
        if not use_loss_ts:
            continue
        enlarged = F.max_pool2d(tg.float().unsqueeze(1), kernel_size=3, stride=1, padding=1).squeeze(1).byte()
        for b in range(len(mean_fields)):
            obj = inds == b
            if int(obj.sum()) > 0:
                x = (t_in[obj].unsqueeze(1) + s_in[obj].unsqueeze(1)) / 2
                pseudo, _ = mean_fields[b](x, tg[obj].unsqueeze(1))
                loss_ts.append(B.dice_loss(s_in[obj] * enlarged[obj], pseudo))
                labels.append((first + mask.nonzero().flatten()[obj], pseudo.squeeze(1)))
                if use_corr:
                    pseudo_c, _ = mean_fields[b](x, tg[obj].unsqueeze(1), iiu[mask][obj])
                    cropped = s_in[obj] * enlarged[obj]
                    cropped = cropped * mean_fields[b].gamma + cropped.detach() * (1 - mean_fields[b].gamma)
                    corr_ts.append(B.dice_loss(cropped, pseudo_c))
                    labels_corr.append(pseudo_c.squeeze(1))
    out = dict(loss_ins=torch.cat(loss_ins).mean() * lcfg['w_ins'] if loss_ins else zero.clone())
    corr_mean = torch.cat(corr_ts).mean() if corr_ts else zero.clone()
    out['loss_ts'] = (torch.cat(loss_ts).mean() + corr_mean) * lcfg['w_ts'] if use_loss_ts and loss_ts else zero.clone()
    out['loss_cate'] = B.solo_cate_loss(list(cate_preds), targets.flat_cate_labels, targets.num_ins, head['gamma'], head['alpha'], head['loss_weight_cate'])
    out['loss_corr'] = corr_sum / (corr_num + 1e-4) * lcfg['w_corr'] if use_corr else zero.clone()
    if details is not None:
        details.update(labels=labels, labels_corr=labels_corr, level_rows=[0 if m is None else int(m.shape[0]) for m in s_list])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def head_block(num_grids, strides, scale_ranges, num_classes=2):
    """A bbox_head block in the shape of configs/discobox, with the grids of the test."""
    return dict(type='DiscoBoxSOLOv2Head', num_classes=num_classes, in_channels=8, stacked_convs=2, seg_feat_channels=8, strides=list(strides),
                scale_ranges=tuple(scale_ranges), sigma=0.2, num_grids=list(num_grids), ins_out_channels=8,
                loss_ins=dict(type='DiceLoss', use_sigmoid=True, loss_weight=1.0),
                loss_ts=dict(type='DiceLoss', momentum=0.999, use_ind_teacher=True, loss_weight=1.0, kernel=3, max_iter=10, alpha0=2.0, theta0=0.5,
                             theta1=30.0, theta2=20.0, base=0.1, crf_height=28, crf_width=28),
                loss_cate=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_corr=dict(type='InfoNCE', loss_weight=1.0, corr_exp=1.0, corr_eps=0.05, gaussian_filter_size=3, low_score=0.3, corr_num_iter=10,
                               corr_num_smooth_iter=1, save_corr_img=False, dist_kernel=9,
                               obj_bank=dict(img_norm_cfg=None, len_object_queues=100, fg_iou_thresh=0.7, bg_iou_thresh=0.7, ratio_range=[0.9, 1.2],
                                             appear_thresh=0.7, min_retrieval_objs=2, max_retrieval_objs=5, feat_height=7, feat_width=7,
                                             mask_height=28, mask_width=28, img_height=200, img_width=200, min_size=4, num_gpu_bank=20)))


def make_inputs(num_grids, hw=(24, 40), E=8, B=2, C=8, num_classes=2, empty_image=None, seed=0, boxes_per_image=3, box_size=None, sharp=False):
    """Seeded tensors of one call (numpy -> the caller moves them): category maps, student / teacher kernel maps and mask features, the
    image, s_feat / t_feat, and per image rectangular gt boxes with their box masks on the 4x canvas.  ``empty_image``: that image has no box.
    ``box_size``: (w, h) of every box instead of drawn sizes, so that the objects of a class resemble each other for the object bank.
    ``sharp``: masks the object bank can match -- channel 0 of the mask feature is a +-1 pattern and every kernel weighs it by 8, so the
    sigmoid masks are nearly 0 / 1 with both values inside every box; the teacher's tensors are the student's and the RoI features are
    positive, so an object stored by one call passes all four retrieval thresholds for the same object of a later call."""
    rng = np.random.default_rng(1000 + seed)
    h, w = hw
    Hc, Wc = 4 * h, 4 * w
    d = dict(cate=[(0.5 * rng.standard_normal((B, num_classes, S, S)) - 2.0).astype(np.float32) for S in num_grids],
             s_kern=[(0.4 * rng.standard_normal((B, E, S, S))).astype(np.float32) for S in num_grids],
             t_kern=[(0.4 * rng.standard_normal((B, E, S, S))).astype(np.float32) for S in num_grids],
             s_ins=rng.standard_normal((B, E, h, w)).astype(np.float32), t_ins=rng.standard_normal((B, E, h, w)).astype(np.float32),
             img=rng.standard_normal((B, 3, Hc, Wc)).astype(np.float32),
             s_feat=rng.standard_normal((B, C, h, w)).astype(np.float32), t_feat=rng.standard_normal((B, C, h, w)).astype(np.float32),
             boxes=[], labels=[], masks=[])
    if sharp:
        yy, xx = np.mgrid[0:h, 0:w]
        d['s_ins'][:, 0] = np.sign(np.sin(xx / 3.0) + np.cos(yy / 2.5) + 0.01).astype(np.float32)
        d['s_ins'][:, 1:] *= 0.1
        for m in d['s_kern']:
            m[:, 0] = 8.0
        d['t_ins'], d['t_kern'] = d['s_ins'].copy(), [m.copy() for m in d['s_kern']]
        d['s_feat'] = (np.abs(d['s_feat']) + 0.1).astype(np.float32)
        d['t_feat'] = d['s_feat'].copy()
    for b in range(B):
        n = 0 if b == empty_image else boxes_per_image
        bx = np.zeros((n, 4), np.float32)
        mk = np.zeros((n, Hc, Wc), np.uint8)
        for i in range(n):
            bw, bh = (int(rng.integers(24, Wc // 2)), int(rng.integers(24, Hc // 2))) if box_size is None else box_size
            x0, y0 = int(rng.integers(0, Wc - bw)), int(rng.integers(0, Hc - bh))
            bx[i] = (x0, y0, x0 + bw, y0 + bh)
            mk[i, y0:y0 + bh, x0:x0 + bw] = 1
        d['boxes'].append(bx); d['masks'].append(mk); d['labels'].append(np.zeros(n, np.int64))
    return d
