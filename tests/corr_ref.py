"""DiscoBox's cross-image correspondence restated in plain torch (any device, fp32 or fp64): what the GPU tests of boxinstseg_amd.corr
lean on, and the op sequence tools/corr_bench.py times.  It restates ``ObjectQueues`` (:132-227), ``SemanticCorrSolver.solve`` /
``pass_message`` (:349-411), ``superres_T`` (:851-865) and the object loop of ``corr_loss`` (:1056-1127) of the reference's
mmdet/models/dense_heads/discobox_head.py, with the bank as dense tensors.  tests/test_host_corr.py holds it against the fixture that
tests/golden/make_golden_corr.py records by executing the reference's own code.

The fixture (tests/golden/corr.npz, corr_cases.json): per case the inputs (stored as float16, so exactly representable), and what the
reference gave: retrieved slots and counts, fp64 Cu / C / loss / gradient / iiu, the bank afterwards; ``tol_*`` are the reference's own
fp32-against-fp64 differences, pooled over the cases."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'corr.npz')
CASES = os.path.join(HERE, 'golden', 'corr_cases.json')
FEAT, MASK = 7, 28
INPUT_KEYS = ('s_feat', 's_mask', 't_feat', 't_mask', 'boxes', 'labels', 'bank_feature', 'bank_mask', 'bank_box', 'bank_ptr')
TOLERANCED = ('Cu', 'C', 'loss_sum', 'grad', 'iiu')


def load_cases():
    with open(CASES) as fh:
        return json.load(fh)


def inputs_of(g, name, device='cpu', dtype=torch.float32):
    """The recorded inputs of one case: floats as ``dtype``, labels int64, bank_ptr int32."""
    out = {}
    for k in INPUT_KEYS:
        a = torch.from_numpy(np.asarray(g[f'{name}_{k}']))
        if k == 'labels':
            a = a.long()
        elif k == 'bank_ptr':
            a = a.int()
        else:
            a = a.to(dtype)
        out[k] = a.to(device)
    return out


def down7(m):
    """[n,28,28] -> [n,7,7], the bilinear rule (the mean of the middle 2 x 2 of each 4 x 4 block)."""
    return F.interpolate(m.unsqueeze(1), (FEAT, FEAT), mode='bilinear', align_corners=False).squeeze(1)


def slot_scores(qm, qf, qbox, km, kf, kbox):
    """fg IoU, bg IoU, appearance and box-ratio of a query (mask [28,28], feature [C,7,7], box [4]) against L entries."""
    A = qm[None]
    fg = (A * km).sum((1, 2)) / ((A + km) >= 1).to(A).sum((1, 2))
    bg = ((1 - A) * (1 - km)).sum((1, 2)) / ((2 - A - km) >= 1).to(A).sum((1, 2))
    m0, m1 = down7(A), down7(km)
    sim = (qf[None] * kf * m0[:, None] * m1[:, None]).sum((1, 2, 3)) / ((m0 * m1).sum((1, 2)) + 1e-6)
    r0 = (qbox[2] - qbox[0]) / (qbox[3] - qbox[1] + 1e-5)
    r1 = (kbox[:, 2] - kbox[:, 0]) / (kbox[:, 3] - kbox[:, 1] + 1e-5)
    return fg, bg, sim, r0 / r1


def passing(scores, cfg):
    fg, bg, sim, ratio = scores
    lo, hi = cfg['ratio_range']
    return (fg > cfg['fg_iou_thresh']) & (bg > cfg['bg_iou_thresh']) & (sim > cfg['appear_thresh']) & (ratio >= lo) & (ratio <= hi)


def dist_mask(dist_kernel, like):
    ys, xs = torch.meshgrid(torch.arange(FEAT), torch.arange(FEAT), indexing='ij')
    y, x = ys.reshape(-1), xs.reshape(-1)
    cheb = torch.maximum((y[:, None] - y[None]).abs(), (x[:, None] - x[None]).abs())
    return (cheb <= dist_kernel // 2).to(like)


def pass_message(T):
    """[K,49,49] -> the mean over the in-range shifts (dy, dx), the same shift on source and target."""
    S = FEAT
    T5 = T.view(-1, S, S, S, S)
    acc, cnt = torch.zeros_like(T5), torch.zeros_like(T5)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            dst_y, dst_x = slice(max(0, dy), min(S + dy, S)), slice(max(0, dx), min(S + dx, S))
            src_y, src_x = slice(max(0, -dy), min(S - dy, S)), slice(max(0, -dx), min(S - dx, S))
            cnt[:, dst_y, dst_x, dst_y, dst_x] += 1
            acc[:, dst_y, dst_x, dst_y, dst_x] += T5[:, src_y, src_x, src_y, src_x]
    return (acc / cnt).view(-1, S * S, S * S)


def solve(f0, f1, cfg):
    """f0 [C,7,7] (may require grad), f1 [K,C,7,7] -> (Cu [K,49,49] differentiable, C [K,49,49])."""
    K, C = f1.shape[0], f1.shape[1]
    a = f0.reshape(1, C, -1).transpose(2, 1)
    b = f1.reshape(K, C, -1)
    a = a / (torch.norm(a, p=2, dim=2, keepdim=True) + 1e-4)
    b = b / (torch.norm(b, p=2, dim=1, keepdim=True) + 1e-4)
    Cu = torch.matmul(a, b)
    with torch.no_grad():
        Cm = Cu.detach() * dist_mask(cfg['dist_kernel'], Cu)
        for _ in range(cfg['corr_num_iter']):
            votes = Cm
            for _ in range(cfg['corr_num_smooth_iter']):
                votes = pass_message(votes.clone())
                votes = votes / (votes.sum(2, keepdim=True) + 1e-4)
            Cm = Cu.detach() + votes
            Cm = Cm / (Cm.sum(2, keepdim=True) + 1e-4)
    return Cu, Cm


def up_matrix(like):
    """[784,49]: the 7 -> 28 bilinear matrix (align_corners=False) of both axes."""
    u = F.interpolate(torch.eye(FEAT).to(like)[None], size=MASK, mode='linear', align_corners=False)[0].t()      # [28,7]
    return torch.kron(u, u)


def superres(T):
    U = up_matrix(T)
    return torch.matmul(torch.matmul(U, T), U.t()) * (FEAT * FEAT / (MASK * MASK))


def class_maps(T, m0, m1):
    """T [K,49,49] (normalised), m0 [28,28], m1 [K,28,28] -> (bg_ci, fg_ci) [28,28]."""
    Tsr = superres(T)
    a, b = m0.reshape(1, -1, 1), m1.reshape(m1.shape[0], 1, -1)
    fgm, bgm = a * b, (1 - a) * (1 - b)
    v = m1.reshape(m1.shape[0], -1, 1)
    fg = torch.matmul(Tsr * (fgm > 0.5).to(T), torch.clamp(v, min=0.1, max=0.9)).mean(0).reshape(MASK, MASK)
    bg = torch.matmul(Tsr * (bgm > 0.5).to(T), torch.clamp(1 - v, min=0.1, max=0.9)).mean(0).reshape(MASK, MASK)
    return bg, fg


def corr_objects(inp, cfg, out_hw, record=False):
    """The loop of :1056-1127 over the N objects of ``inp`` (see INPUT_KEYS); the bank tensors of ``inp`` are updated in place.
    Returns a dict: loss_sum (differentiable w.r.t. inp['s_feat']), num_ins, iiu [N,2,H,W], and with ``record`` the per-object lists;
    among them ``scores`` [N,L,4] (fg, bg, appearance, ratio against the bank as it stood for that object) and ``ret_src`` [N,K], the
    earlier object of the call whose append put the retrieved entry there, else -1.  An object whose label is outside [0, num_class)
    is passed over, as the header says: it retrieves nothing (scores 0) and is not appended."""
    s_feat, s_mask, t_feat, t_mask, boxes, labels = (inp[k] for k in INPUT_KEYS[:6])
    bf, bm, bb, ptr = (inp[k] for k in INPUT_KEYS[6:])
    N, L, K = s_feat.shape[0], bf.shape[1], cfg['max_retrieval_objs']
    H, W = out_hw
    iiu = torch.zeros(N, 2, H, W).to(s_mask)
    loss_sum = torch.zeros(()).to(s_mask)
    num_ins = 0
    rec = dict(ret_slot=-torch.ones(N, K, dtype=torch.int64), count=torch.zeros(N, dtype=torch.int64), Cu=torch.zeros(N, K, 49, 49).to(s_mask),
               C=torch.zeros(N, K, 49, 49).to(s_mask), assign=-torch.ones(N, K, 49, dtype=torch.int64), scores=torch.zeros(N, L, 4).to(s_mask),
               ret_src=-torch.ones(N, K, dtype=torch.int64)) if record else {}
    writer = -torch.ones(bf.shape[0], L, dtype=torch.int64)          # who wrote this slot: an object of this call, or -1 (it was stored)
    for i in range(N):
        c = int(labels[i])
        if not 0 <= c < bf.shape[0]:
            continue
        with torch.no_grad():
            scores = slot_scores(s_mask[i], s_feat[i].detach(), boxes[i], bm[c], bf[c], bb[c])
            keep = torch.where(passing(scores, cfg))[0][:K]
        n = int(keep.numel())
        if record:
            rec['count'][i] = n
            rec['ret_slot'][i, :n] = keep.cpu()
            rec['scores'][i] = torch.stack(scores, 1)
            rec['ret_src'][i, :n] = writer[c][keep.cpu()]
        if n >= cfg['min_objs']:
            f1, m1 = bf[c][keep], bm[c][keep]
            Cu, Cm = solve(s_feat[i], f1, cfg)
            assignment = Cm.argmax(2).reshape(-1)
            p = F.softmax(Cu, 2).reshape(-1, 49)
            loss_sum = loss_sum + F.cross_entropy(p, assignment)
            num_ins += 1
            with torch.no_grad():
                T = Cm * p.detach().reshape(Cm.shape)
                T = T / (T.sum(2, keepdim=True) + 1e-5)
                bg, fg = class_maps(T, s_mask[i], m1)
                x1, y1, x2, y2 = (int(v) for v in boxes[i])
                h, w = int(boxes[i][3] - boxes[i][1]), int(boxes[i][2] - boxes[i][0])
                for ch, ci in ((0, bg), (1, fg)):
                    iiu[i, ch, y1:y2, x1:x2] = F.interpolate(ci[None, None], (h, w), mode='bilinear', align_corners=False)[0, 0]
            if record:
                rec['Cu'][i, :n], rec['C'][i, :n], rec['assign'][i, :n] = Cu.detach(), Cm, Cm.argmax(2).cpu()
        if (boxes[i][2] - boxes[i][0]) > cfg['min_size'] and (boxes[i][3] - boxes[i][1]) > cfg['min_size']:
            with torch.no_grad():
                s = int(ptr[c])
                bf[c, s], bm[c, s], bb[c, s] = t_feat[i], t_mask[i], boxes[i]
                ptr[c] = (s + 1) % L
                writer[c, s] = i
    out = dict(loss_sum=loss_sum, num_ins=num_ins, iiu=iiu)
    if record:
        out.update(rec)
    return out


# ---- what the cases are made of (tests/golden/make_golden_corr.py and tools/corr_bench.py) ---------------------------------------------------
def blob(cy=13.5, cx=13.5, radius=9.0, floor=0.0):
    """A soft disc on the 28 x 28 grid, sigmoid(1.5 (radius - distance)); ``floor`` lifts the background."""
    ys, xs = np.meshgrid(np.arange(MASK), np.arange(MASK), indexing='ij')
    d = np.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)
    m = 1.0 / (1.0 + np.exp(-1.5 * (radius - d)))
    return np.maximum(m, floor)


# Mask values of the fixture: the soft disc snapped to these eight levels.  With continuous values some of the 784 x 784 products m0 m1 of a
# pair always land within 1e-7 of 0.5; no two of these levels add up to 1, and no product of two of them or of their complements is 0.5,
# to within 4e-3.  0.02 and 0.97 lie outside clamp(., 0.1, 0.9), so the clamp works too.
LEVELS = np.array([0.02, 0.15, 0.29, 0.44, 0.61, 0.76, 0.88, 0.97])


def snap(m):
    return LEVELS[np.abs(np.asarray(m)[..., None] - LEVELS).argmin(-1)]


def feature(base, rng, noise=0.3):
    """relu_and_l2_norm_feat(base + noise * N(0,1)) of a [C,7,7] base."""
    f = np.maximum(base + noise * rng.standard_normal(base.shape), 0.0)
    n = np.sqrt((f ** 2).sum(0, keepdims=True) + 1e-6)
    return f / (n + 1e-6)


def half(a):
    """Rounded to float16 (what the fixture stores), as float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
