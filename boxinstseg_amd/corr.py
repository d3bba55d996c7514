"""DiscoBox's cross-image correspondence on the HIP kernels of ``csrc/corr.hip`` (include/boxinst/boxinst_hip_corr.h): the object bank,
the retrieval, the correspondence solver, ``loss_corr`` with its gradient and the inter-image mask ``iiu`` that ``MeanField.forward`` takes.

    ObjectBank          <-> ObjectQueues (discobox_head.py:132-227): ONE device-resident store for all classes
    SemanticCorrSolver  <-> SemanticCorrSolver (:230-411; ``solve`` and ``pass_message``, the rest is dead code there)
    superres_T          <-> DiscoBoxSOLOv2Head.superres_T (:851-865)
    corr_objects        <-> the object loop of DiscoBoxSOLOv2Head.corr_loss (:1056-1127) for one level: eight launches, no host sync
    parse_corr_cfg      : the loss_corr / obj_bank block of configs/discobox/* as the classes here take it

The RoI tensors (mmcv's RoIAlign of the mask features and masks, then relu_and_l2_norm_feat) are the caller's.  Thin marshalling only:
there is no CPU and no torch path.  Features are 7 x 7, masks 28 x 28, everything fp32.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import cfg_get, cfg_require, current_stream, need_cuda

FEAT, MASK = _lib.CORR_FEAT, _lib.CORR_MASK
_FF, _MM = FEAT * FEAT, MASK * MASK


def _f32(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    t = t.detach().to(torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'{name} must be {list(shape)}, got {list(t.shape)}')
    return t


class ObjectBank:
    """Drop-in for ``ObjectQueues``: ``feature [num_class, L, C, 7, 7]``, ``mask [num_class, L, 28, 28]``, ``box [num_class, L, 4]`` and
    ``ptr [num_class]`` (int32) on the device, allocated at the first use (the channel count and the device are known then).  A class that
    was never appended to is all zeros and retrieves nothing (the reference returns ``None`` for it; here ``get_similar_obj`` returns
    empty tensors).  At 80 classes, L = 100 and C = 256 the store is about 430 MB."""

    def __init__(self, num_class, len_queue, fg_iou_thresh, bg_iou_thresh, ratio_range, appear_thresh, max_retrieval_objs):
        self.num_class, self.len_queue = int(num_class), int(len_queue)
        self.fg_iou_thresh, self.bg_iou_thresh, self.appear_thresh = float(fg_iou_thresh), float(bg_iou_thresh), float(appear_thresh)
        self.ratio_range = (float(ratio_range[0]), float(ratio_range[1]))
        self.max_retrieval_objs = int(max_retrieval_objs)
        if self.num_class < 1:
            raise ValueError('num_class must be at least 1')
        if not 1 <= self.len_queue <= _lib.CORR_MAX_QUEUE:
            raise ValueError(f'len_queue must be in 1..{_lib.CORR_MAX_QUEUE}')
        if not 1 <= self.max_retrieval_objs <= _lib.CORR_MAX_OBJS:
            raise ValueError(f'max_retrieval_objs must be in 1..{_lib.CORR_MAX_OBJS} (a limit of this library)')
        self.feature = self.mask = self.box = self.ptr = None
        self._used = set()

    def ensure(self, channels: int, device: torch.device) -> None:
        """Allocate the zeroed store; a second call checks that it still fits."""
        if self.feature is None:
            n, L = self.num_class, self.len_queue
            self.feature = torch.zeros((n, L, int(channels), FEAT, FEAT), dtype=torch.float32, device=device)
            self.mask = torch.zeros((n, L, MASK, MASK), dtype=torch.float32, device=device)
            self.box = torch.zeros((n, L, 4), dtype=torch.float32, device=device)
            self.ptr = torch.zeros((n,), dtype=torch.int32, device=device)
        elif self.feature.shape[2] != int(channels) or self.feature.device != device:
            raise RuntimeError(f'the bank holds {self.feature.shape[2]} channels on {self.feature.device}, got {int(channels)} on {device}')

    def _thresholds(self):
        return (self.fg_iou_thresh, self.bg_iou_thresh, self.appear_thresh, self.ratio_range[0], self.ratio_range[1])

    def get_similar_obj(self, qobj):
        """``qobj`` has ``mask [1,28,28]``, ``feature [1,C,7,7]``, ``box [1,4]`` and ``category``.  Returns the reference's dict (``img`` is
        None) of the first ``max_retrieval_objs`` matching entries; its size depends on data, so this drop-in synchronises once."""
        need_cuda(mask=qobj.mask, feature=qobj.feature, box=qobj.box)
        dev = qobj.mask.device
        C = int(qobj.feature.shape[1])
        self.ensure(C, dev)
        f, m, b = _f32(qobj.feature, (1, C, FEAT, FEAT), 'feature'), _f32(qobj.mask, (1, MASK, MASK), 'mask'), _f32(qobj.box, (1, 4), 'box')
        labels = torch.full((1,), int(qobj.category), dtype=torch.int64, device=dev)
        none = torch.full((1,), -1, dtype=torch.int32, device=dev)
        ret_slot, _, count = _retrieve(self, f, m, f, m, b, labels, none)
        with torch.no_grad():
            c = int(qobj.category)
            keep = ret_slot[0, :int(count[0])].long()
            return dict(img=None, mask=self.mask[c][keep], feature=self.feature[c][keep], box=self.box[c][keep], category=c)

    def append(self, class_idx, idx, feature, mask, box, img=None, device=None):
        """Entry ``idx`` of the batched ``feature`` / ``mask`` / ``box`` goes to slot ``ptr`` of class ``class_idx``; ``img`` and ``device``
        are accepted and ignored (every bank lives on the device).  Returns whether this was the class's first entry."""
        need_cuda(feature=feature, mask=mask, box=box)
        class_idx, idx = int(class_idx), int(idx)
        if not 0 <= class_idx < self.num_class:
            raise ValueError(f'class_idx {class_idx} outside 0..{self.num_class - 1}')
        dev = feature.device
        C = int(feature.shape[1])
        self.ensure(C, dev)
        f, m, b = (_f32(feature[idx:idx + 1], (1, C, FEAT, FEAT), 'feature'), _f32(mask[idx:idx + 1], (1, MASK, MASK), 'mask'),
                   _f32(box[idx:idx + 1], (1, 4), 'box'))
        labels = torch.full((1,), class_idx, dtype=torch.int64, device=dev)
        slot, role = _plan(self, b, labels, float('-inf'))
        _append(self, f, m, b, labels, slot, role)
        first = class_idx not in self._used
        self._used.add(class_idx)
        return first


def _plan(bank: ObjectBank, boxes, labels, min_size: float):
    dev, N = boxes.device, boxes.shape[0]
    slot = torch.empty((N,), dtype=torch.int32, device=dev)
    role = torch.empty((N,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_corr_plan_f32', _lib.load().bxi_corr_plan_f32(
            boxes.data_ptr(), labels.data_ptr(), bank.ptr.data_ptr(), N, bank.num_class, bank.len_queue, float(min_size), slot.data_ptr(),
            role.data_ptr(), current_stream(dev)))
    return slot, role


def _retrieve(bank: ObjectBank, s_feat, s_mask, t_feat, t_mask, boxes, labels, obj_slot, scores=None):
    dev, N, C, K = s_feat.device, s_feat.shape[0], s_feat.shape[1], bank.max_retrieval_objs
    ret_slot = torch.empty((N, K), dtype=torch.int32, device=dev)
    ret_src = torch.empty((N, K), dtype=torch.int32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    slot_pass = torch.empty((N, bank.len_queue), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_corr_retrieve_f32', _lib.load().bxi_corr_retrieve_f32(
            s_feat.data_ptr(), s_mask.data_ptr(), t_feat.data_ptr(), t_mask.data_ptr(), boxes.data_ptr(), labels.data_ptr(), obj_slot.data_ptr(), N, C,
            bank.feature.data_ptr(), bank.mask.data_ptr(), bank.box.data_ptr(), bank.num_class, bank.len_queue, *bank._thresholds(), K,
            slot_pass.data_ptr(), ret_slot.data_ptr(), ret_src.data_ptr(), count.data_ptr(), None if scores is None else scores.data_ptr(), current_stream(dev)))
    return ret_slot, ret_src, count


def _append(bank: ObjectBank, t_feat, t_mask, boxes, labels, obj_slot, obj_role):
    dev, N, C = t_feat.device, t_feat.shape[0], t_feat.shape[1]
    with torch.cuda.device(dev):
        _lib.check('bxi_corr_append_f32', _lib.load().bxi_corr_append_f32(
            t_feat.data_ptr(), t_mask.data_ptr(), boxes.data_ptr(), labels.data_ptr(), obj_slot.data_ptr(), obj_role.data_ptr(), N, C,
            bank.feature.data_ptr(), bank.mask.data_ptr(), bank.box.data_ptr(), bank.ptr.data_ptr(), bank.num_class, bank.len_queue,
            current_stream(dev)))


def _workspace(N: int, C: int, K: int, dev) -> torch.Tensor:
    nbytes = _lib.load().bxi_corr_workspace_bytes(N, C, K)
    if nbytes == 0:
        raise RuntimeError(f'no correspondence workspace for N={N}, C={C}, max_retrieval_objs={K}')
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def _solve(s_feat, t_feat, labels, bank_feature, num_class, L, ret_slot, ret_src, count, K, min_objs, solver, ws):
    dev, N, C = s_feat.device, s_feat.shape[0], s_feat.shape[1]
    Cu = torch.empty((N, K, _FF, _FF), dtype=torch.float32, device=dev)
    Cm = torch.empty((N, K, _FF, _FF), dtype=torch.float32, device=dev)
    assign = torch.empty((N, K, _FF), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check('bxi_corr_solve_f32', _lib.load().bxi_corr_solve_f32(
            s_feat.data_ptr(), t_feat.data_ptr(), labels.data_ptr(), N, C, bank_feature.data_ptr(), num_class, L, ret_slot.data_ptr(),
            ret_src.data_ptr(), count.data_ptr(), K, int(min_objs), solver.dist_kernel, solver.num_iter, solver.num_smooth_iter, Cu.data_ptr(),
            Cm.data_ptr(), assign.data_ptr(), ws.data_ptr(), ws.numel(), current_stream(dev)))
    return Cu, Cm, assign


class _CuGrad(torch.autograd.Function):
    """Attaches d Cu / d f0 to the Cu that the solve kernel returned."""

    @staticmethod
    def forward(ctx, f0, f1, Cu):
        ctx.save_for_backward(f0.detach(), f1)
        return Cu.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f0, f1 = ctx.saved_tensors
        K, C = f1.shape[0], f1.shape[1]
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(f0)
        with torch.cuda.device(f0.device):
            _lib.check('bxi_corr_cu_backward_f32', _lib.load().bxi_corr_cu_backward_f32(
                f0.data_ptr(), f1.data_ptr(), g.data_ptr(), K, C, grad.data_ptr(), current_stream(f0.device)))
        return grad, None, None


class SemanticCorrSolver:
    """Drop-in for the reference's ``SemanticCorrSolver``: same constructor; ``exp``, ``eps``, ``gaussian_filter_size`` and ``low_score`` feed
    only code that nothing calls there (perform_sinkhorn, appearance_similarityOT, build_hspace, receptive_fields, hsfilter) and are kept
    as attributes."""

    def __init__(self, exp, eps, gaussian_filter_size, low_score, num_iter, num_smooth_iter, dist_kernel):
        self.exp, self.eps, self.gaussian_filter_size, self.low_score = exp, eps, gaussian_filter_size, low_score
        self.num_iter, self.num_smooth_iter, self.dist_kernel = int(num_iter), int(num_smooth_iter), int(dist_kernel)
        if self.num_iter < 0 or self.num_smooth_iter < 0:
            raise ValueError('num_iter and num_smooth_iter must not be negative')
        if self.dist_kernel < 1 or self.dist_kernel % 2 == 0:
            raise ValueError('dist_kernel must be odd and positive')

    def solve(self, qobjs, kobjs, f0):
        """``qobjs.mask [1,28,28]``, ``kobjs`` the dict of ``ObjectBank.get_similar_obj`` (K entries), ``f0 [1,C,7,7]`` ->
        ``(Cu, C, fg_mask, bg_mask)``: ``Cu [K,49,49]`` differentiable w.r.t. ``f0``, ``C`` the solved correspondence, the masks
        ``[K,784,784]`` by plain broadcasting."""
        need_cuda(f0=f0, feature=kobjs['feature'], mask=kobjs['mask'], qmask=qobjs.mask)
        dev = f0.device
        K, C = int(kobjs['feature'].shape[0]), int(f0.shape[1])
        if not 1 <= K <= _lib.CORR_MAX_OBJS:
            raise RuntimeError(f'solve takes 1..{_lib.CORR_MAX_OBJS} retrieved objects, got {K}')
        f0c = _f32(f0, (1, C, FEAT, FEAT), 'f0')
        f1 = _f32(kobjs['feature'], (K, C, FEAT, FEAT), "kobjs['feature']")
        m0, m1 = _f32(qobjs.mask, (1, MASK, MASK), 'qobjs.mask'), _f32(kobjs['mask'], (K, MASK, MASK), "kobjs['mask']")
        labels = torch.zeros((1,), dtype=torch.int64, device=dev)
        ret_slot = torch.arange(K, dtype=torch.int32, device=dev).view(1, K)
        ret_src = torch.full((1, K), -1, dtype=torch.int32, device=dev)
        count = torch.full((1,), K, dtype=torch.int32, device=dev)
        ws = _workspace(1, C, K, dev)
        Cu, Cm, _ = _solve(f0c, f0c, labels, f1, 1, K, ret_slot, ret_src, count, K, K, self, ws)     # the K entries as a bank of one class
        Cu = _CuGrad.apply(f0.view(1, C, FEAT, FEAT) if f0.dtype == torch.float32 else f0.float(), f1, Cu[0])
        fg_mask = m0.reshape(1, -1, 1) * m1.reshape(K, 1, -1)
        bg_mask = (1 - m0).reshape(1, -1, 1) * (1 - m1).reshape(K, 1, -1)
        return Cu, Cm[0], fg_mask, bg_mask


def superres_T(T: torch.Tensor, feat_hw=(FEAT, FEAT), mask_hw=(MASK, MASK)) -> torch.Tensor:
    """``T [K,49,49]`` -> ``[K,784,784]``: bilinear on the target cells, then on the source cells, times 49 / 784."""
    need_cuda(T=T)
    if tuple(feat_hw) != (FEAT, FEAT) or tuple(mask_hw) != (MASK, MASK):
        raise NotImplementedError(f'superres_T is built for {FEAT} x {FEAT} features and {MASK} x {MASK} masks')
    Tc = T.detach().to(torch.float32).contiguous().view(-1, _FF, _FF)
    K = Tc.shape[0]
    out = torch.empty((K, _MM, _MM), dtype=torch.float32, device=T.device)
    with torch.cuda.device(T.device):
        _lib.check('bxi_corr_superres_f32', _lib.load().bxi_corr_superres_f32(Tc.data_ptr(), K, out.data_ptr(), current_stream(T.device)))
    return out


class _CorrObjects(torch.autograd.Function):
    @staticmethod
    def forward(ctx, roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, kernel_labels, bank, solver, out_hw, min_size, min_objs, details):
        need_cuda(roi_s_feat=roi_s_feat, roi_s_mask=roi_s_mask, roi_t_feat=roi_t_feat, roi_t_mask=roi_t_mask, boxes=boxes, kernel_labels=kernel_labels)
        if roi_s_feat.dim() != 4:
            raise RuntimeError(f'roi_s_feat must be [N,C,{FEAT},{FEAT}]')
        dev, N, C = roi_s_feat.device, int(roi_s_feat.shape[0]), int(roi_s_feat.shape[1])
        H, W = int(out_hw[0]), int(out_hw[1])
        if H < 1 or W < 1 or int(min_objs) < 1 or int(min_objs) > bank.max_retrieval_objs:
            raise RuntimeError(f'out_hw must be positive and min_objs in 1..max_retrieval_objs ({bank.max_retrieval_objs})')
        bank.ensure(C, dev)
        sf, tf = _f32(roi_s_feat, (N, C, FEAT, FEAT), 'roi_s_feat'), _f32(roi_t_feat, (N, C, FEAT, FEAT), 'roi_t_feat')
        sm, tm = _f32(roi_s_mask, (N, MASK, MASK), 'roi_s_mask'), _f32(roi_t_mask, (N, MASK, MASK), 'roi_t_mask')
        bx = _f32(boxes, (N, 4), 'boxes')
        labels = kernel_labels.detach().to(torch.int64).contiguous()
        if tuple(labels.shape) != (N,):
            raise RuntimeError(f'kernel_labels must be [{N}]')
        K, L, lib = bank.max_retrieval_objs, bank.len_queue, _lib.load()
        loss_sum = torch.empty((1,), dtype=torch.float32, device=dev)
        num_ins = torch.empty((1,), dtype=torch.int32, device=dev)
        grad = torch.empty((N, C, FEAT, FEAT), dtype=torch.float32, device=dev)
        iiu = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
        ws = _workspace(N, C, K, dev)
        scores = None if details is None else torch.empty((N, L, 4), dtype=torch.float32, device=dev)
        obj_slot, obj_role = _plan(bank, bx, labels, float(min_size))
        ret_slot, ret_src, count = _retrieve(bank, sf, sm, tf, tm, bx, labels, obj_slot, scores)
        Cu, Cm, assign = _solve(sf, tf, labels, bank.feature, bank.num_class, L, ret_slot, ret_src, count, K, min_objs, solver, ws)
        stream = current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check('bxi_corr_loss_f32', lib.bxi_corr_loss_f32(count.data_ptr(), N, C, K, int(min_objs), loss_sum.data_ptr(), num_ins.data_ptr(),
                                                                  grad.data_ptr(), ws.data_ptr(), ws.numel(), stream))
            _lib.check('bxi_corr_iiu_f32', lib.bxi_corr_iiu_f32(
                sm.data_ptr(), tm.data_ptr(), bx.data_ptr(), labels.data_ptr(), N, C, bank.mask.data_ptr(), bank.num_class, L, ret_slot.data_ptr(),
                ret_src.data_ptr(), count.data_ptr(), K, int(min_objs), H, W, iiu.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        _append(bank, tf, tm, bx, labels, obj_slot, obj_role)
        if details is not None:
            details.update(obj_slot=obj_slot, obj_role=obj_role, ret_slot=ret_slot, ret_src=ret_src, count=count, Cu=Cu, C=Cm, assign=assign,
                           scores=scores, grad=grad)
        ctx.save_for_backward(grad)
        ctx.dtype = roi_s_feat.dtype
        loss_sum, num_ins = loss_sum.view(()), num_ins.view(())
        ctx.mark_non_differentiable(num_ins, iiu)
        return loss_sum, num_ins, iiu

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_num, _g_iiu):
        (unit,) = ctx.saved_tensors
        g = g_loss.to(torch.float32).contiguous().view(1)
        out = torch.empty_like(unit)
        with torch.cuda.device(unit.device):
            _lib.check('bxi_corr_grad_rescale_f32', _lib.load().bxi_corr_grad_rescale_f32(unit.data_ptr(), g.data_ptr(), unit.numel(), out.data_ptr(),
                                                                                          current_stream(unit.device)))
        return (out.to(ctx.dtype),) + (None,) * 11


def corr_objects(roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, kernel_labels, bank: ObjectBank, solver: SemanticCorrSolver, out_hw,
                 min_size, min_objs=5, details=None):
    """The object loop of ``corr_loss`` (discobox_head.py:1056-1127) for the N objects of one level, the loop's order kept: object i
    retrieves from the bank as the appends of the objects before it left it.  ``roi_s_feat`` / ``roi_t_feat [N,C,7,7]`` (student /
    teacher, after relu_and_l2_norm_feat), ``roi_s_mask`` / ``roi_t_mask [N,28,28]``, ``boxes [N,4]`` (the boxes of the target masks),
    ``kernel_labels [N]``; ``out_hw`` the size of the mask predictions, ``min_size`` the config's ``obj_bank.min_size``, ``min_objs`` the
    match count an object needs (the reference hard-codes 5 at :1075).

    Returns ``(loss_sum, num_ins, iiu)``: the sum of the objects' losses (0-dim, differentiable w.r.t. ``roi_s_feat``), how many objects ran
    (0-dim int32; ``loss_sum / (num_ins + 1e-4)`` is the caller's, :1139) and ``iiu [N,2,H,W]`` for ``MeanField.forward``.  Nothing is read
    back.  ``details``: a dict that receives the intermediate tensors (tests, debugging)."""
    return _CorrObjects.apply(roi_s_feat, roi_s_mask, roi_t_feat, roi_t_mask, boxes, kernel_labels, bank, solver, out_hw, min_size, min_objs, details)


def parse_corr_cfg(bbox_head_cfg):
    """``bbox_head=dict(type='DiscoBoxSOLOv2Head', loss_corr=dict(..., obj_bank=dict(...)))`` (dict or namespace) -> ``dict(bank=...,
    solver=..., min_size, loss_weight, min_objs)``: ``ObjectBank(**bank)``, ``SemanticCorrSolver(**solver)``.  ``min_objs`` is 5: the
    reference never reads ``min_retrieval_objs`` (:1075)."""
    lc = cfg_get(bbox_head_cfg, 'loss_corr')
    if lc is None:
        raise TypeError('bbox_head has no `loss_corr`')
    ob = cfg_require(lc, 'obj_bank')
    if cfg_get(lc, 'save_corr_img', False):
        raise NotImplementedError('loss_corr.save_corr_img=True is not supported')
    sizes = (cfg_require(ob, 'feat_height'), cfg_require(ob, 'feat_width'), cfg_require(ob, 'mask_height'), cfg_require(ob, 'mask_width'))
    if sizes != (FEAT, FEAT, MASK, MASK):
        raise NotImplementedError(f'obj_bank feature / mask size {sizes} is not supported: only {(FEAT, FEAT, MASK, MASK)}')
    bank = dict(num_class=int(cfg_require(bbox_head_cfg, 'num_classes')), len_queue=int(cfg_require(ob, 'len_object_queues')),
                fg_iou_thresh=float(cfg_require(ob, 'fg_iou_thresh')), bg_iou_thresh=float(cfg_require(ob, 'bg_iou_thresh')),
                ratio_range=[float(v) for v in cfg_require(ob, 'ratio_range')], appear_thresh=float(cfg_require(ob, 'appear_thresh')),
                max_retrieval_objs=int(cfg_require(ob, 'max_retrieval_objs')))
    solver = dict(exp=float(cfg_require(lc, 'corr_exp')), eps=float(cfg_require(lc, 'corr_eps')), gaussian_filter_size=int(cfg_require(lc, 'gaussian_filter_size')),
                  low_score=float(cfg_require(lc, 'low_score')), num_iter=int(cfg_require(lc, 'corr_num_iter')),
                  num_smooth_iter=int(cfg_require(lc, 'corr_num_smooth_iter')), dist_kernel=int(cfg_require(lc, 'dist_kernel')))
    return dict(bank=bank, solver=solver, min_size=float(cfg_require(ob, 'min_size')), loss_weight=float(cfg_get(lc, 'loss_weight', 1.0)), min_objs=5)
