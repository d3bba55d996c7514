"""RoIAlign and the front of one level of DiscoBox's corr_loss restated in plain torch (any device, any float dtype): what the tests of
boxinstseg_amd.roi_align lean on.  ``roi_align`` is the documented per-sample algorithm of mmcv.ops.roi_align (the one Detectron2 and
torchvision share), every sample with its own four taps and weights -- deliberately NOT the separable form the kernels use; autograd gives
its backward.  mmcv itself never ran here: the arithmetic is restated and unpinned, tests/test_host_roi.py holds it against a second
statement built from ``F.grid_sample`` and against rules checked by hand.  ``front`` restates discobox_head.py:1018-1057 of the reference
(tests/golden/make_golden_roi.py records what the reference's own statements give, with ``roi_align`` standing in for mmcv's module)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'roi_front.npz')
CASES = os.path.join(HERE, 'golden', 'roi_front_cases.json')
FEAT, MASK = 7, 28


def load_cases():
    with open(CASES) as fh:
        return json.load(fh)


def _axis(s, size):
    """One axis of the bilinear samples at coordinates ``s``: (inside, low index, high index, low weight l, high weight h)."""
    inside = ~((s < -1.0) | (s > size))
    s = torch.clamp(s, min=0.0)
    lo = s.floor().long()                                   # (int)y of a non-negative y
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    s = torch.where(edge, lo.to(s.dtype), s)
    lw = s - lo.to(s.dtype)
    return inside, lo, hi, lw, 1.0 - lw


def roi_align(feat, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    """``feat [B,C,H,W]``, ``rois [K,5]`` -> ``[K,C,PH,PW]`` in the dtype of ``feat``; the roi arithmetic runs in that dtype too.  A batch
    index outside ``[0,B)`` gives a zero row."""
    PH, PW = (output_size, output_size) if isinstance(output_size, int) else output_size
    B, C, H, W = feat.shape
    dt = feat.dtype
    rois = rois.detach().to(dt)
    out = []
    for r in rois:
        b = int(r[0])
        if not 0 <= b < B:
            out.append(feat.new_zeros(C, PH, PW))
            continue
        off = 0.5 if aligned else 0.0
        xs, ys, xe, ye = (r[i] * spatial_scale - off for i in (1, 2, 3, 4))
        rw, rh = xe - xs, ye - ys
        if not aligned:
            rw, rh = torch.clamp(rw, min=1.0), torch.clamp(rh, min=1.0)
        bin_h, bin_w = rh / PH, rw / PW
        gh = sampling_ratio if sampling_ratio > 0 else max(int(torch.ceil(rh / PH)), 0)
        gw = sampling_ratio if sampling_ratio > 0 else max(int(torch.ceil(rw / PW)), 0)
        count = max(gh * gw, 1)
        if gh == 0 or gw == 0:
            out.append(feat.new_zeros(C, PH, PW))
            continue
        ph, iy = torch.arange(PH, dtype=dt, device=feat.device)[:, None], torch.arange(gh, dtype=dt, device=feat.device)[None, :]
        pw, ix = torch.arange(PW, dtype=dt, device=feat.device)[:, None], torch.arange(gw, dtype=dt, device=feat.device)[None, :]
        y = (ys + ph * bin_h + (iy + 0.5) * bin_h / gh).reshape(-1)          # [PH * gh]
        x = (xs + pw * bin_w + (ix + 0.5) * bin_w / gw).reshape(-1)          # [PW * gw]
        in_y, yl, yh, ly, hy = _axis(y, H)
        in_x, xl, xh, lx, hx = _axis(x, W)
        f = feat[b]
        tap = lambda yy, xx: f[:, yy][:, :, xx]                             # noqa: E731  [C, PH * gh, PW * gw]
        val = (hy[:, None] * hx[None, :]) * tap(yl, xl) + (hy[:, None] * lx[None, :]) * tap(yl, xh) + \
              (ly[:, None] * hx[None, :]) * tap(yh, xl) + (ly[:, None] * lx[None, :]) * tap(yh, xh)
        val = val * (in_y[:, None] & in_x[None, :]).to(dt)
        out.append(val.reshape(C, PH, gh, PW, gw).sum((2, 4)) / count)
    return torch.stack(out) if out else feat.new_zeros(0, C, PH, PW)


def roi_align_grid_sample(feat, rois, output_size):
    """The second statement, for aligned boxes inside the canvas: the same sample points through ``F.grid_sample`` (bilinear, border padding,
    align_corners=True), then the mean over each bin's samples.  Built from torch ops mmcv has no part in."""
    PH, PW = (output_size, output_size) if isinstance(output_size, int) else output_size
    B, C, H, W = feat.shape
    out = []
    for r in rois:
        b = int(r[0])
        x1, y1, x2, y2 = (float(v) - 0.5 for v in r[1:])
        rw, rh = x2 - x1, y2 - y1
        gh, gw = math.ceil(rh / PH), math.ceil(rw / PW)
        ys = y1 + (torch.arange(PH * gh, dtype=feat.dtype) + 0.5) * rh / (PH * gh)
        xs = x1 + (torch.arange(PW * gw, dtype=feat.dtype) + 0.5) * rw / (PW * gw)
        gy, gx = ys / (H - 1) * 2 - 1, xs / (W - 1) * 2 - 1
        grid = torch.stack(torch.broadcast_tensors(gx[None, :], gy[:, None]), -1)[None]
        s = F.grid_sample(feat[b:b + 1], grid, mode='bilinear', padding_mode='border', align_corners=True)
        out.append(F.avg_pool2d(s, (gh, gw))[0])
    return torch.stack(out)


def relu_and_l2_norm_feat(feat, dim=1):
    feat = F.relu(feat)
    return feat / (((feat ** 2).sum(dim=dim, keepdim=True) + 1e-6) ** 0.5 + 1e-6)


def target_boxes(target, kernel_labels, own_labels=False):
    """``(boxes [N,4] float64, keep [N] bool, labels [N] int64)`` as boxinstseg_amd.target_boxes defines them."""
    N = target.shape[0]
    boxes, keep, labels = torch.zeros(N, 4, dtype=torch.float64), torch.zeros(N, dtype=torch.bool), -torch.ones(N, dtype=torch.int64)
    rank = 0
    for i in range(N):
        ys, xs = torch.where(target[i].cpu() != 0)
        if ys.numel():
            boxes[i] = torch.tensor([int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1], dtype=torch.float64)
            keep[i] = True
            labels[i] = int(kernel_labels[i if own_labels else rank])
            rank += 1
    return boxes, keep, labels


def front(s_input, t_input, target, img_inds, kernel_labels, s_feat, t_feat, own_labels=False):
    """:1018-1057 for one level, over ALL N objects (the reference drops the all-zero targets; here their rows are zero and ``keep`` says
    which).  ``s_input`` / ``t_input [N,H,W]`` raw predictions (``t_input`` may be ``s_input``), features ``[B,C,H,W]`` of the working dtype.
    Returns a dict: boxes, keep, labels, roi_s_feat (differentiable w.r.t. ``s_feat``), roi_t_feat, roi_s_mask, roi_t_mask."""
    dt = s_feat.dtype
    boxes, keep, labels = target_boxes(target, kernel_labels, own_labels)
    boxes = boxes.to(dt)
    N = boxes.shape[0]
    rois = torch.cat([img_inds.to(dt).view(N, 1), boxes], 1)
    roi_s_feat = relu_and_l2_norm_feat(roi_align(s_feat, rois, FEAT))
    with torch.no_grad():
        roi_t_feat = relu_and_l2_norm_feat(roi_align(t_feat.detach(), rois, FEAT))
        mrois = torch.cat([torch.arange(N).to(dt).view(N, 1), boxes], 1)
        s_sig = torch.sigmoid(s_input.detach().to(dt))
        roi_s_mask = roi_align(s_sig.unsqueeze(1), mrois, MASK).squeeze(1)
        roi_t_mask = roi_s_mask if t_input is s_input else roi_align(torch.sigmoid(t_input.detach().to(dt)).unsqueeze(1), mrois, MASK).squeeze(1)
    return dict(boxes=boxes, keep=keep, labels=labels, roi_s_feat=roi_s_feat, roi_t_feat=roi_t_feat, roi_s_mask=roi_s_mask, roi_t_mask=roi_t_mask)


def corr_level(inp, bank, cfg, own_labels=False):
    """``front`` and then tests/corr_ref.corr_objects over the kept objects: ``inp`` has s_input, target, img_inds, kernel_labels, s_feat,
    t_feat (``t_input is s_input``); ``bank`` has bank_feature, bank_mask, bank_box, bank_ptr (updated in place).  Returns the front's dict
    plus loss_sum, num_ins, iiu [N,2,H,W] (zero rows for the dropped), ret_slot / count [N, ...] (-1 / 0 for the dropped)."""
    from tests import corr_ref as R
    f = front(inp['s_input'], inp['s_input'], inp['target'], inp['img_inds'], inp['kernel_labels'], inp['s_feat'], inp['t_feat'], own_labels)
    keep = f['keep']
    N, (H, W) = keep.shape[0], inp['s_input'].shape[1:]
    sub = dict(s_feat=f['roi_s_feat'][keep], s_mask=f['roi_s_mask'][keep], t_feat=f['roi_t_feat'][keep], t_mask=f['roi_t_mask'][keep],
               boxes=f['boxes'][keep], labels=f['labels'][keep], **bank)
    out = R.corr_objects(sub, cfg, (H, W), record=True)
    K = cfg['max_retrieval_objs']
    iiu = torch.zeros(N, 2, H, W, dtype=f['boxes'].dtype)
    iiu[keep] = out['iiu']
    ret_slot, count = -torch.ones(N, K, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    ret_slot[keep], count[keep] = out['ret_slot'], out['count']
    f.update(loss_sum=out['loss_sum'], num_ins=out['num_ins'], iiu=iiu, ret_slot=ret_slot, count=count)
    return f


# ---- what the recorded case is made of (tests/golden/make_golden_roi.py) ---------------------------------------------------------------
def half(a):
    """Rounded to float16 (what the fixture stores), as float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def inputs_of(g, device='cpu', dtype=torch.float32):
    """The recorded inputs of the level case and its bank: floats as ``dtype``."""
    inp = dict(s_input=torch.from_numpy(g['s_input'].astype(np.float32)).to(dtype), target=torch.from_numpy(g['target']),
               img_inds=torch.from_numpy(g['img_inds']), kernel_labels=torch.from_numpy(g['kernel_labels']),
               s_feat=torch.from_numpy(g['s_feat'].astype(np.float32)).to(dtype), t_feat=torch.from_numpy(g['t_feat'].astype(np.float32)).to(dtype))
    bank = dict(bank_feature=torch.from_numpy(g['bank_feature'].astype(np.float32)).to(dtype), bank_mask=torch.from_numpy(g['bank_mask'].astype(np.float32)).to(dtype),
                bank_box=torch.from_numpy(g['bank_box'].astype(np.float32)).to(dtype), bank_ptr=torch.from_numpy(np.array(g['bank_ptr'], np.int32)))
    return {k: v.to(device) for k, v in inp.items()}, {k: v.to(device) for k, v in bank.items()}


# ---- the op-level cases: shared by the generator (which measures the tolerances on them) and the GPU tests ---------------------------------
def _rand(rng, shape, scale=1.0):
    return torch.from_numpy(half(scale * rng.standard_normal(shape)))


FEAT7_ROIS = [[0, 2, 3, 9, 10],        # the exact copy: 7 x 7 at unit bins, every sample on a pixel centre
              [0, 4, 1, 5, 2],         # 1 x 1
              [1, 0, 0, 20, 12],       # the whole canvas: every edge clamp
              [1, 3, 0, 18, 11],       # 15 x 11: a 2 x 3 grid
              [0, 1, 2, 12, 9], [0, 6, 4, 17, 12],      # two overlapping boxes in one image
              [1, 5, 2, 13, 10], [1, 5, 2, 13, 10],     # the same box twice
              [2, 1, 1, 9, 9]]         # batch index 2 of 2 images: a zero row
FLOAT_ROIS = [[0, 1.3, 2.2, 11.7, 9.1], [1, 0.4, 0.3, 19.2, 11.4], [1, 6.25, 3.5, 9.0, 5.1], [0, -1.5, -0.75, 6.3, 4.9], [0, 15.1, 7.2, 21.4, 13.6]]


def op_cases():
    """name -> dict(feat [B,C,H,W] float32, rois [K,5] float32, size, kw): the 7 x 7 op on a 2 x 5 x 12 x 20 map."""
    rng = np.random.RandomState(31)
    feat = _rand(rng, (2, 5, 12, 20))
    rois, frois = torch.tensor(FEAT7_ROIS, dtype=torch.float32), torch.tensor(FLOAT_ROIS, dtype=torch.float32)
    for r in FLOAT_ROIS:            # no fp32 ceil can flip: rh / PH and rw / PW stay away from the integers
        for v in ((r[4] - r[2]) / 7, (r[3] - r[1]) / 7):
            assert abs(v - round(v)) > 1e-3
    return {
        'plain': dict(feat=feat, rois=rois, size=7, kw=dict()),
        'ratio2': dict(feat=feat, rois=rois, size=7, kw=dict(sampling_ratio=2)),
        'unaligned': dict(feat=feat, rois=rois, size=7, kw=dict(aligned=False)),
        'image1_empty': dict(feat=feat, rois=rois[rois[:, 0] != 1], size=7, kw=dict()),
        'float': dict(feat=feat, rois=frois, size=7, kw=dict()),
        'float_ratio2_unaligned': dict(feat=feat, rois=frois, size=7, kw=dict(sampling_ratio=2, aligned=False)),
        'scale_half_5x3': dict(feat=feat, rois=frois * torch.tensor([1, 2, 2, 2, 2.]), size=(5, 3), kw=dict(spatial_scale=0.5)),
    }


def mask_cases():
    """name -> dict(logits [N,H,W], boxes [N,4]): the 28 x 28 mask path, the roi of object i reads plane i."""
    rng = np.random.RandomState(32)
    return {
        'small': dict(logits=_rand(rng, (3, 12, 20), 3.0), boxes=torch.tensor([[2, 1, 13, 9], [0, 0, 20, 12], [19, 11, 20, 12.]])),   # grid 1: up-sampling
        'large': dict(logits=_rand(rng, (1, 64, 96), 3.0), boxes=torch.tensor([[3, 2, 93, 62.]])),                                    # 60 x 90: grid 3 x 4
    }


def fused_cases():
    """name -> dict(feat [B,C,40,56], rois [K,5], dead=(roi, ph, pw)): the fused feature path; in bin `dead` every channel is <= 0."""
    out = {}
    for C, seed in ((256, 33), (5, 34), (70, 35)):
        rng = np.random.RandomState(seed)
        feat = _rand(rng, (2, C, 40, 56))
        rois = torch.tensor([[0, 4, 6, 32, 34], [1, 0, 0, 56, 40], [1, 10.5, 3.25, 24.0, 30.5], [0, 40, 20, 47, 27]], dtype=torch.float32)
        feat[0, :, 5:12, 3:10] = -feat[0, :, 5:12, 3:10].abs()      # roi 0, bin (0, 0): rows 5.5 .. 9.5, columns 3.5 .. 7.5 and their taps
        out[f'c{C}'] = dict(feat=feat, rois=rois, dead=(0, 0, 0))
    return out
