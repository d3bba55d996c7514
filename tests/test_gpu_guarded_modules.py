"""The Python surface with guarded inputs and poisoned scratch (run on a real MI355X: -m gpu).

Entry points with long signatures are reached through their wrappers: every input is a contiguous view inside NaN / -1 bands at a
chosen misalignment (tests/guarded.py) -- the wrappers' `.detach().to(dtype).contiguous()` passes such a view through unchanged, which
every case asserts so that it does not test a copy -- and the call runs inside poisoned_empty(): every output, state and workspace the
wrapper allocates holds a NaN / 0xA5 / 0x5A5A5A5A pattern before the kernel sees it.  Results against the family's oracle at the
tolerance the family's existing test uses; inputs unchanged; bands intact.

Then the inputs as the reference's callers produce them -- slices, permuted and channels_last tensors, expanded gradients -- against
the call on .contiguous() copies, bit for bit; and a selection of the existing oracle checks once more under poisoned_empty().

A guard band cannot see a load whose value is selected away afterwards; a NaN band shows an out-of-bounds load only if it reaches an
output."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import mf_decided as M

pytestmark = pytest.mark.gpu
SOI = [64, 128, 256, 512, 1024]

# entry point -> the test of this module that runs it guarded (tests/test_abi_families.py checks the table against _lib.SIGNATURES)
GUARDED = {
    'bxi_dynamic_mask_forward_f32': 'test_dynamic_head_guarded',
    'bxi_dynamic_mask_backward_f32': 'test_dynamic_head_guarded',
    'bxi_dynamic_mask_generic_forward_f32': 'test_generic_dynamic_head_guarded',
    'bxi_dynamic_mask_generic_backward_f32': 'test_generic_dynamic_head_guarded',
    'bxi_boxinst_head_eval_f32': 'test_forward_loss_guarded',
    'bxi_meanfield_kernel_f32': 'test_meanfield_guarded',
    'bxi_meanfield_forward_f32': 'test_meanfield_guarded',
    'bxi_dice_loss_forward_f32': 'test_mil_and_dice_guarded',
    'bxi_dice_loss_backward_f32': 'test_mil_and_dice_guarded',
    'bxi_mil_loss_forward_f32': 'test_mil_and_dice_guarded',
    'bxi_mil_loss_backward_f32': 'test_mil_and_dice_guarded',
    'bxi_projection_loss_forward_f32': 'test_projection_and_levelset_guarded',
    'bxi_lcm_affinity_f32': 'test_lcm_guarded',
    'bxi_lcm_refine_f32': 'test_lcm_guarded',
    'bxi_mst_forward_i32': 'test_tree_filter_guarded',
    'bxi_bfs_forward_i32': 'test_tree_filter_guarded',
    'bxi_tree_refine_forward_f32': 'test_tree_filter_guarded',
    'bxi_tree_refine_backward_feature_f32': 'test_tree_filter_guarded',
    'bxi_tree_refine_backward_weight_f32': 'test_tree_filter_guarded',
}


class _Inputs:
    """The guarded inputs of one call: embed() + the assertion that the wrappers' own conversion does not copy the view."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def __call__(self, array, lead, band=1024, dtype=None):
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        if dtype is not None:
            t = t.to(dtype)
        g = G.embed(t.to(self.dev), lead, band)
        assert g.t.detach().to(g.t.dtype).contiguous().data_ptr() == g.ptr() and g.ptr() % 16 == (lead * g.t.element_size()) % 16
        self.all.append(g)
        return g

    def check(self):
        G.check_bands(*self.all)
        G.check_unchanged(*self.all)


def _leaf(g):
    x = g.t.detach().requires_grad_(True)
    assert x.data_ptr() == g.ptr()
    return x


class _Hook:
    def __init__(self):
        from boxinstseg_amd import _lib
        self.names, self._lib = [], _lib
        self._cb = _lib.LAUNCH_HOOK(lambda name, phase, st, user: self.names.append(name.decode()))

    def __enter__(self):
        self._lib.load().bxi_dev_set_launch_hook(C.cast(self._cb, C.c_void_p), None)
        return self

    def __exit__(self, *exc):
        self._lib.load().bxi_dev_set_launch_hook(None, None)
        return False


# ---------------------------------------------------------------------------------------------
# the dynamic mask head
# ---------------------------------------------------------------------------------------------
HEAD_LEADS = {'aligned': {}, 'feat': dict(feat=1), 'params': dict(params=3), 'g': dict(g=2),
              'all': dict(feat=3, params=1, coors=1, lvl=1, img=1, soi=3, g=1)}


@pytest.mark.parametrize('shape', [(2, 16, 12, 32, 5), (3, 8, 9, 18, 7)], ids=['C16', 'C8'])
def test_dynamic_head_guarded(dev, shape):
    """The tuned 3 x 8 kernels (bxi_dynamic_mask_forward_f32 / _backward_f32), forward and backward, against the fp64 torch oracle at the
    tolerances of test_dynamic_head_vs_oracle_large."""
    from boxinstseg_amd import dynamic_mask_forward
    from oracle import torch_oracle as to
    from tests.test_gpu_dynamic_head import _close
    B, Cc, H, W, N = shape
    rng = np.random.default_rng(sum(shape))
    feat = rng.standard_normal((B, Cc, H, W)).astype(np.float32)
    params = (rng.standard_normal((N, (Cc + 2) * 8 + 64 + 8 + 17)) * 0.3).astype(np.float32)
    coors = rng.uniform(0, 8 * W, size=(N, 2)).astype(np.float32)
    lvl, img = rng.integers(0, 5, size=N), rng.integers(0, B, size=N)
    g = rng.standard_normal((N, 1, 2 * H, 2 * W)).astype(np.float32)
    f64 = lambda a: torch.from_numpy(a.astype(np.float64))
    ft, pt = f64(feat).requires_grad_(True), f64(params).requires_grad_(True)
    yo = to.dynamic_mask_forward(ft, pt, f64(coors), torch.from_numpy(lvl), torch.from_numpy(img), torch.tensor(SOI))
    yo.backward(f64(g))
    for name, L in HEAD_LEADS.items():
        E = _Inputs(dev)
        gf, gp = E(feat, L.get('feat', 0), G.plane_band(H, W)), E(params, L.get('params', 0))
        gc, gl, gi = E(coors, L.get('coors', 0), 64), E(lvl, L.get('lvl', 0), 64), E(img, L.get('img', 0), 64)
        gs, gg = E(torch.tensor(SOI, dtype=torch.float32), L.get('soi', 0), 64), E(g, L.get('g', 0), G.plane_band(2 * H, 2 * W))
        f, p = _leaf(gf), _leaf(gp)
        with G.poisoned_empty(), _Hook() as hk:
            y = dynamic_mask_forward(f, p, gc.t, gl.t, gi.t, gs.t, in_stride=8, out_stride=4)
            y.backward(gg.t)
        torch.cuda.synchronize()
        assert {'dyn_fwd', 'dyn_bwd', 'dyn_reduce'} <= set(hk.names) and 'dyn_fwd_generic' not in hk.names, hk.names
        E.check()
        assert f.grad.shape == f.shape and p.grad.shape == p.shape
        assert _close(y.detach().cpu().numpy(), yo.detach().numpy(), 2e-5), name
        assert _close(f.grad.cpu().numpy(), ft.grad.numpy(), 5e-5), name
        assert _close(p.grad.cpu().numpy(), pt.grad.numpy(), 5e-5), name


@pytest.mark.parametrize('convs,ch,cin,no_rel,fac,shape', [(3, 8, 16, False, 2, (2, 11, 18, 5)), (4, 12, 3, False, 3, (2, 7, 20, 4)),
                                                           (1, 8, 8, False, 2, (2, 6, 10, 3)), (3, 5, 7, True, 1, (1, 9, 33, 3))])
def test_generic_dynamic_head_guarded(dev, convs, ch, cin, no_rel, fac, shape):
    """The general kernels (bxi_dynamic_mask_generic_forward_f32 / _backward_f32) against the fp64 CPU composition, at the tolerances of
    test_general_dynamic_head_shapes_in_hip."""
    from boxinstseg_amd import CondInstMaskHead
    from boxinstseg_amd import dynamic as dyn
    from tests.test_gpu_dynamic_head import _close, _close_except_kinks
    B, H, W, N = shape
    rng = np.random.default_rng(convs * 1000 + ch * 10 + cin)
    head = CondInstMaskHead(in_channels=cin, dynamic_convs=convs, dynamic_channels=ch, boxinst_enabled=True, disable_rel_coors=no_rel)
    head.in_stride, head.out_stride = (4 * fac, 4) if 8 % fac else (8, 8 // fac)
    feat = rng.standard_normal((B, cin, H, W))
    params = rng.standard_normal((N, head.num_gen_params)) * 0.4
    coors = rng.uniform(0, head.in_stride * W, size=(N, 2))
    lvl, img = rng.integers(0, 5, size=N), rng.integers(0, B, size=N)
    g = rng.standard_normal((N, 1, fac * H, fac * W))
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ft, pt = f64(feat).requires_grad_(True), f64(params).requires_grad_(True)
    want = head.double()._composed_forward(ft, pt, f64(coors), torch.from_numpy(lvl), torch.from_numpy(img))
    want.backward(f64(g))
    pix = np.broadcast_to(np.arange(B * H * W).reshape(B, 1, H, W), feat.shape)
    inst = np.broadcast_to(np.arange(N)[:, None], params.shape)
    soi = head.sizes_of_interest.detach().float()
    for name, L in HEAD_LEADS.items():
        E = _Inputs(dev)
        f32 = torch.float32
        gf, gp = E(feat, L.get('feat', 0), G.plane_band(H, W), f32), E(params, L.get('params', 0), 1024, f32)
        gc, gl, gi = E(coors, L.get('coors', 0), 64, f32), E(lvl, L.get('lvl', 0), 64), E(img, L.get('img', 0), 64)
        gs, gg = E(soi, L.get('soi', 0), 64), E(g, L.get('g', 0), G.plane_band(fac * H, fac * W), f32)
        f, p = _leaf(gf), _leaf(gp)
        with G.poisoned_empty(), _Hook() as hk:
            y = dyn.dynamic_mask_forward_generic(f, p, gc.t, gl.t, gi.t, gs.t, convs, ch, in_stride=head.in_stride, out_stride=head.out_stride,
                                                 disable_rel_coors=no_rel)
            y.backward(gg.t)
        torch.cuda.synchronize()
        assert {'dyn_fwd_generic', 'dyn_bwd_generic'} <= set(hk.names) and 'dyn_fwd' not in hk.names, hk.names
        E.check()
        assert _close(y.detach().cpu().numpy(), want.detach().numpy(), 3e-5), name
        assert _close_except_kinks(f.grad.cpu().numpy(), ft.grad.numpy(), 1e-4, pix), name
        assert _close_except_kinks(p.grad.cpu().numpy(), pt.grad.numpy(), 1e-4, inst), name


@pytest.mark.parametrize('Cc,no_rel', [(16, False), (8, True)])
def test_forward_loss_guarded(dev, Cc, no_rel):
    """CondInstMaskHead.forward_loss with the head inside the evaluation's first launch (bxi_boxinst_head_eval_f32): guarded features,
    parameters, coordinates, index vectors, images, boxes, under poisoned_empty().  The logits against the fp64 torch oracle (2e-5, as
    test_dynamic_head_vs_oracle_large), the losses against the C oracle evaluated on those logits (1e-4), the gradients against the two
    separate calls on plain tensors at the tolerances of test_head_fused_into_the_loss_evaluation.  Misaligned images leave the fused
    launch (it is built for the vector pooling path): the two calls then, same checks."""
    import copy
    from boxinstseg_amd import CondInstMaskHead, synthetic
    from oracle import torch_oracle as to
    from tests.helpers import oracle_path, rel
    d = synthetic.cfg1(1)
    B, H, W = d['B'], d['H'], d['W']
    N = d['N']
    rng = np.random.default_rng(40 + Cc)
    counts = np.cumsum([0] + [len(b) for b in d['gt_bboxes']])
    img_inds = np.array([int(np.searchsorted(counts, int(k), side='right') - 1) for k in d['gt_inds']], np.int64)
    torch.manual_seed(Cc)
    head = CondInstMaskHead(in_channels=Cc, boxinst_enabled=True, disable_rel_coors=no_rel, max_proposals=-1, topk_per_img=64).to(dev)
    head.set_iter(5000)
    feat = rng.standard_normal((B, Cc, H // 8, W // 8)).astype(np.float32)
    params = (0.3 * rng.standard_normal((N, head.num_gen_params))).astype(np.float32)
    coors = (rng.uniform(size=(N, 2)) * np.array([W, H])).astype(np.float32)
    lvl = rng.integers(0, 5, size=N)
    allb = np.concatenate(d['gt_bboxes'], 0)

    # the two calls on plain tensors
    h2 = copy.deepcopy(head)
    f0 = torch.from_numpy(feat).to(dev).requires_grad_(True)
    p0 = torch.from_numpy(params).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    logits0 = h2(f0, p0, t(coors), t(lvl), t(img_inds))
    losses0 = h2.loss(t(d['imgs']), d['img_metas'], logits0, t(d['gt_inds']), [t(b) for b in d['gt_bboxes']], None, None)
    (losses0['loss_prj'] + 2.0 * losses0['loss_pairwise']).backward()
    f64 = lambda a: torch.from_numpy(a.astype(np.float64))
    yo = to.dynamic_mask_forward(f64(feat), f64(params), f64(coors), torch.from_numpy(lvl), torch.from_numpy(img_inds), torch.tensor(SOI),
                                 disable_rel_coors=no_rel).numpy()

    for name, L in {'aligned': {}, 'feat': dict(feat=1), 'params': dict(params=3), 'boxes': dict(boxes=1), 'imgs': dict(imgs=1),
                    'all_but_imgs': dict(feat=3, params=1, coors=1, lvl=1, img=1, boxes=3, gt_inds=1)}.items():
        E = _Inputs(dev)
        gf, gp = E(feat, L.get('feat', 0), G.plane_band(H // 8, W // 8)), E(params, L.get('params', 0))
        gc, gl, gi = E(coors, L.get('coors', 0), 64), E(lvl, L.get('lvl', 0), 64), E(img_inds, L.get('img', 0), 64)
        gim = E(d['imgs'], L.get('imgs', 0), G.plane_band(H, W))
        gb, ggi = E(allb, L.get('boxes', 0), 64), E(d['gt_inds'], L.get('gt_inds', 0), 64)
        boxes = [gb.t[counts[i]:counts[i + 1]] for i in range(B)]
        f, p = _leaf(gf), _leaf(gp)
        h3 = copy.deepcopy(head)
        with G.poisoned_empty(), _Hook() as hk:
            logits, losses = h3.forward_loss(f, p, gc.t, gl.t, gi.t, gim.t, d['img_metas'], ggi.t, boxes, fuse_head=True)
            (losses['loss_prj'] + 2.0 * losses['loss_pairwise']).backward()
        torch.cuda.synchronize()
        assert ('head_prep' in hk.names) == (not L.get('imgs', 0)), (name, hk.names)
        E.check()
        y = logits.detach().cpu().numpy()
        assert np.abs(y - yo).max() <= 2e-5 * max(np.abs(yo).max(), 1e-30), name
        dd = dict(d, mask_logits=y)
        ref = oracle_path(dd, warmup=min(5001.0 / float(head._warmup_iters), 1.0), want_targets=False)
        assert rel(float(losses['loss_prj']), ref['loss_prj']) <= 1e-4 and rel(float(losses['loss_pairwise']), ref['loss_pairwise']) <= 1e-4, name
        assert float(h3._iter) == 5001.0
        for a, b in ((f.grad, f0.grad), (p.grad, p0.grad)):
            assert a.shape == b.shape and bool(torch.isfinite(a).all())
            assert (a - b).abs().max() <= 2e-4 * max(float(b.abs().max()), 1e-8), name


# ---------------------------------------------------------------------------------------------
# DiscoBox: MeanField, mil_loss, dice_loss
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,n,ks,iters,base', [(37, 65, 4, 3, 2, 0.10), (20, 128, 5, 5, 3, 0.45), (100, 136, 6, 3, 4, 0.10)])
def test_meanfield_guarded(dev, H, W, n, ks, iters, base):
    """bxi_meanfield_kernel_f32 + bxi_meanfield_forward_f32 (uint8 and float targets, img_inds, inter_img_mask) against the numpy oracle
    under the rules of test_meanfield_vs_oracle / test_meanfield_fuzz."""
    from boxinstseg_amd import MeanField, meanfield_forward, meanfield_kernel
    from oracle import discobox_oracle as do
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    feats = np.stack([np.stack([np.sin(xx / (7.0 + b)) + 0.3 * np.cos(yy / 5.0), np.cos(xx / 9.0 + yy / 11.0), 0.5 * np.sin(yy / (4.0 + b))])
                      for b in range(2)])
    feats = (feats + 0.05 * rng.standard_normal(feats.shape)).astype(np.float32)
    Ko = np.stack([do.meanfield_kernel(feats[b], ks, 2.0, 0.5, 30.0) for b in range(2)])
    x = rng.uniform(0, 1, size=(n, H, W)).astype(np.float32)
    tg = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        r0, c0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
        tg[i, r0:r0 + int(rng.integers(4, H // 2 + 1)), c0:c0 + int(rng.integers(4, W // 2 + 1))] = 1
    tg[0] = 1
    img = rng.integers(0, 2, size=n)
    inter = rng.uniform(0, 20, size=(n, 2, H, W)).astype(np.float32)
    same = M.recipe(n, H, W, ks, with_inter=True)         # the inputs tests/test_host_meanfield_decided.py counts undecided pixels on
    assert all(np.array_equal(same[k], v) for k, v in dict(feats=feats, Ko=Ko, x=x, t=tg, img=img, inter=inter).items())
    band = G.plane_band(H, W, ks // 2)
    wants, trajectories = {}, {}
    for use_inter in (False, True):
        want = np.zeros_like(x); wv = np.zeros(n, np.float32)
        for b in range(2):
            m = img == b
            if m.any():
                want[m], wv[m] = do.meanfield_forward(Ko[b], x[m], tg[m], iters, base, inter[m] if use_inter else None, 0.01)
        wants[use_inter] = (want, wv)
        trajectories[use_inter] = M.trajectory_by_image(Ko, img, x, tg, iters, base, inter if use_inter else None, 0.01)
        assert np.array_equal(trajectories[use_inter][0][-1].astype(np.float32), want)
    want_m, wv_m = do.meanfield_forward(Ko[0], x, tg, iters, base)
    trajectories['module'] = M.trajectory(Ko[0], x, tg, iters, base)

    def labels(got, valid, want, wv, key, run, tag):
        """Every label is the oracle's where the trajectory has no undecided pixel (tests/test_host_meanfield_decided.py prints that these
        inputs have none); otherwise the decided labels of every single step are."""
        states, undecided = trajectories[key]
        if any(u.any() for u in undecided):
            M.assert_steps(run, tg, states, undecided, tag)
            return
        bad = int((got != want).sum())
        assert bad == 0, f'{tag}: {bad} of {want.size} labels differ'
        assert np.array_equal(valid, wv), tag
    for name, L in {'aligned': {}, 'feat': dict(feat=1), 'kernel': dict(K=1), 'x': dict(x=3), 'targets': dict(t=5), 'inter': dict(inter=2),
                    'all': dict(feat=3, K=2, x=1, t=7, img=1, inter=3)}.items():
        for use_inter in (False, True):
            E = _Inputs(dev)
            gfe, gK, gx = E(feats, L.get('feat', 0), band), E(Ko, L.get('K', 0), band), E(x, L.get('x', 0), band)
            gt8, gtf = E(tg, L.get('t', 0), band), E(tg.astype(np.float32), L.get('t', 0) % 4, band)
            gimg, gin = E(img, L.get('img', 0), 64), E(inter, L.get('inter', 0), band)
            with G.poisoned_empty():
                K = meanfield_kernel(gfe.t, ks, 2.0, 0.5, 30.0)
                ret, valid = meanfield_forward(gK.t, gx.t, gt8.t, iters, base, img_inds=gimg.t, inter_img_mask=gin.t if use_inter else None, gamma=0.01)
                ret_f, valid_f = meanfield_forward(gK.t, gx.t, gtf.t, iters, base, img_inds=gimg.t, inter_img_mask=gin.t if use_inter else None,
                                                   gamma=0.01)
            torch.cuda.synchronize()
            E.check()
            assert (np.abs(K.cpu().numpy() - Ko) <= 4e-7 * np.abs(Ko) + 1e-37).all(), name
            want, wv = wants[use_inter]
            got = ret.cpu().numpy()
            assert set(np.unique(got).tolist()) <= {0.0, 1.0}, name
            def run(xs, its, K=gK.t, t8=gt8.t, im=gimg.t, it=gin.t if use_inter else None):
                r, v = meanfield_forward(K, torch.from_numpy(xs).to(dev), t8, its, base, img_inds=im, inter_img_mask=it, gamma=0.01)
                return r.cpu().numpy(), v.cpu().numpy()
            labels(got, valid.cpu().numpy(), want, wv, use_inter, run, name)
            assert torch.equal(ret_f, ret) and torch.equal(valid_f, valid), name
            if name in ('aligned', 'all') and not use_inter:
                # the module (one object per image, discobox_head.py:591-655) on image 0's feature map, the oracle's kernel values in it
                with G.poisoned_empty():
                    mf = MeanField(gfe.t[:1], alpha0=2.0, theta0=0.5, theta1=30.0, iter=iters, kernel_size=ks, base=base)
                    mf._kernel = gK.t[:1]
                    ret_m, valid_m = mf(gx.t[:, None], gt8.t[:, None])
                torch.cuda.synchronize()
                E.check()
                assert (np.abs(mf.kernel.reshape(Ko[:1].shape).cpu().numpy() - Ko[:1]) <= 4e-7 * np.abs(Ko[:1]) + 1e-37).all(), name
                assert ret_m.shape == (n, 1, H, W)

                def run_m(xs, its, K=gK.t[:1], t8=gt8.t):
                    r, v = meanfield_forward(K, torch.from_numpy(xs).to(dev), t8, its, base)
                    return r.cpu().numpy(), v.cpu().numpy()
                labels(ret_m[:, 0].cpu().numpy(), valid_m.cpu().numpy(), want_m, wv_m, 'module', run_m, f'{name}: MeanField module')


@pytest.mark.parametrize('n,H,W', [(5, 20, 36), (3, 33, 71), (6, 200, 304)])
def test_mil_and_dice_guarded(dev, n, H, W):
    """mil_loss / dice_loss forward and backward (uint8 and float targets) against the numpy oracle at 2e-6 (test_mil_and_dice_full_size_vs_oracle)."""
    from boxinstseg_amd import dice_loss, mil_loss
    from oracle import discobox_oracle as do
    rng = np.random.default_rng(n + W)
    x = rng.uniform(0, 1, size=(n, H, W)).astype(np.float32)
    tg = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        r0, c0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
        tg[i, r0:r0 + int(rng.integers(4, H - r0)), c0:c0 + int(rng.integers(4, W - c0))] = 1
    gl = np.ones(n, np.float32)                       # (the existing tolerance is absolute: unit upstream gradients, as there)
    lo_, go_ = do.mil_loss(x, tg)
    band = G.plane_band(H, W)
    for name, L in {'aligned': {}, 'x': dict(x=1), 'targets': dict(t=3), 'all': dict(x=3, t=9, gl=1)}.items():
        E = _Inputs(dev)
        gx, gt8, gtf, ggl = E(x, L.get('x', 0), band), E(tg, L.get('t', 0), band), E(tg.astype(np.float32), L.get('t', 0) % 4, band), E(gl, L.get('gl', 0), 64)
        for tgt in (gt8, gtf):
            xd = _leaf(gx)
            with G.poisoned_empty():
                l = mil_loss(dice_loss, xd, xd, tgt.t)
                l.backward(ggl.t)
            assert np.abs(l.detach().cpu().numpy() - lo_).max() < 2e-6, name
            assert xd.grad.shape == xd.shape and np.abs(xd.grad.cpu().numpy() - go_).max() < 2e-6, name
            xd2 = _leaf(gx)
            with G.poisoned_empty():
                dl = dice_loss(xd2, tgt.t)
                dl.backward(ggl.t)
            assert np.abs(dl.detach().cpu().numpy() - do.dice_loss(x, tg)).max() < 2e-6, name
            assert np.abs(xd2.grad.cpu().numpy() - do.dice_loss_grad(x, tg)).max() < 2e-6, name
        E.check()


# ---------------------------------------------------------------------------------------------
# Box2Mask: BoxProjectionLoss, LevelsetLoss, LocalConsistencyModule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,W,Cc', [(3, 12, 20, 3), (2, 9, 7, 2), (2, 24, 40, 9), (2, 31, 33, 16)])
def test_projection_and_levelset_guarded(dev, N, H, W, Cc):
    """BoxProjectionLoss and LevelsetLoss, forward and backward, against the numpy oracle at 1e-4 (test_projection_and_levelset_vs_oracle).
    levelset.hip's `vec` (H * W % 4 == 0 and mask_score | target 16-byte aligned) takes its other side with mask_score and target misaligned
    SEPARATELY at a plane size that would allow the vector kernel (12 x 20, 24 x 40), next to plane sizes that never do (9 x 7, 31 x 33)."""
    from boxinstseg_amd import BoxProjectionLoss, LevelsetLoss
    from oracle import levelset_oracle as lo
    from tests.test_gpu_levelset import _close
    rng = np.random.default_rng(N * 100 + W)
    s = rng.uniform(0, 1, (N, 1, H, W)).astype(np.float32)
    box = np.zeros((N, 1, H, W), np.float32)
    for i in range(N):
        r0, c0 = int(rng.integers(0, max(H // 2, 1))), int(rng.integers(0, max(W // 2, 1)))
        box[i, 0, r0:r0 + int(rng.integers(1, H // 2 + 2)), c0:c0 + int(rng.integers(1, W // 2 + 2))] = rng.uniform(0.3, 1.0)
    ms = (rng.uniform(0, 1, (N, 2, H, W)) * (box > 0)).astype(np.float32)
    T = rng.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32)
    pn = np.maximum((box > 0).sum((1, 2, 3)), 1).astype(np.float32)
    gl = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    lw, gw = lo.box_projection_loss(s[:, 0], box[:, 0])
    lw2, gm, gT = lo.levelset_loss(ms, T, pn, 5.0)
    band = G.plane_band(H, W)
    for name, L in {'aligned': {}, 'mask_score': dict(ms=1), 'target': dict(T=1), 'scores': dict(s=2), 'bitmask': dict(box=3),
                    'all': dict(s=1, box=2, ms=3, T=2, pn=1, gl=1)}.items():
        E = _Inputs(dev)
        gs, gb, gms, gT_, gpn, ggl = (E(s, L.get('s', 0), band), E(box, L.get('box', 0), band), E(ms, L.get('ms', 0), band), E(T, L.get('T', 0), band),
                                      E(pn, L.get('pn', 0), 64), E(gl, L.get('gl', 0), 64))
        sd, md, Td = _leaf(gs), _leaf(gms), _leaf(gT_)
        with G.poisoned_empty(), _Hook() as hk:
            l = BoxProjectionLoss()(sd, gb.t)
            l.backward(ggl.t)
            l2 = LevelsetLoss(loss_weight=5.0)(md, Td, gpn.t)
            l2.backward(ggl.t)
        torch.cuda.synchronize()
        assert {'levelset_partial', 'levelset_finish', 'levelset_bwd', 'mil_band', 'mil_finish', 'mil_bwd'} <= set(hk.names), hk.names
        E.check()
        g3 = gl[:, None, None]
        assert _close(l.detach().cpu().numpy(), lw) and _close(sd.grad.cpu().numpy()[:, 0], gw * g3), name
        g4 = gl[:, None, None, None]
        assert _close(l2.detach().cpu().numpy(), lw2), name
        assert md.grad.shape == md.shape and Td.grad.shape == Td.shape
        assert _close(md.grad.cpu().numpy(), gm * g4) and _close(Td.grad.cpu().numpy(), gT * g4), name


@pytest.mark.parametrize('N,h,w,iters,d,regime', [(2, 96, 96, 10, 2, 'padded planes, compile-time shape'), (2, 33, 70, 2, 1, 'padded planes, run-time shape'),
                                                  (2, 64, 150, 2, 4, 'two-plane LDS'), (1, 97, 97, 2, 2, 'run-time padded forward, two-plane LDS adjoint'),
                                                  (2, 200, 304, 3, 2, 'one launch per iteration')])
def test_lcm_guarded(dev, N, h, w, iters, d, regime):
    """LocalConsistencyModule in its four dispatch regimes (levelset.hip: launch_lcm_refine), forward and backward, against the numpy oracle at
    the tolerances of test_lcm_vs_oracle; the per-iteration regime uses the wrapper's ping-pong workspace, which holds the pattern here."""
    from boxinstseg_amd import LocalConsistencyModule
    from oracle import levelset_oracle as lo
    from tests.test_gpu_levelset import _close
    rng = np.random.default_rng(h * 31 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([np.stack([np.sin(xx / 5.0 + i), np.cos(yy / 4.0), 0.1 * rng.standard_normal((h, w))]) for i in range(N)])
    img = (img + 0.05 * rng.standard_normal(img.shape)).astype(np.float32)
    phi = rng.uniform(0, 1, (N, 1, h, w)).astype(np.float32)
    gout = rng.standard_normal((N, 1, h, w)).astype(np.float32)
    aw = lo.lcm_affinity(img, d)
    want, want_g = lo.lcm_refine(aw, phi[:, 0], iters, d), lo.lcm_refine_backward(aw, gout[:, 0], iters, d)
    lcm = LocalConsistencyModule(num_iter=iters, dilations=[d])
    band = G.plane_band(h, w, d)
    expect = {'lcm_step'} if 'per iteration' in regime else ({'lcm_refine', 'lcm_adjoint'})
    for name, L in {'aligned': {}, 'imgs': dict(img=1), 'phi': dict(phi=3), 'g': dict(g=2), 'all': dict(img=3, phi=1, g=1)}.items():
        E = _Inputs(dev)
        gi, gp, gg = E(img, L.get('img', 0), band), E(phi, L.get('phi', 0), band), E(gout, L.get('g', 0), band)
        pd = _leaf(gp)
        with G.poisoned_empty(), _Hook() as hk:
            aff = lcm.affinity(gi.t)
            ref = lcm(gi.t, pd)
            ref.backward(gg.t)
        torch.cuda.synchronize()
        assert expect <= set(hk.names) and 'lcm_affinity' in hk.names and (('lcm_step' in hk.names) == ('per iteration' in regime)), (regime, hk.names)
        E.check()
        assert np.abs(aff.cpu().numpy() - aw).max() < 2e-5, name
        assert _close(ref.detach().cpu().numpy()[:, 0], want, 5e-5), name
        assert pd.grad.shape == pd.shape and _close(pd.grad.cpu().numpy()[:, 0], want_g, 5e-5), name


# ---------------------------------------------------------------------------------------------
# tree_filter: mst / bfs / refine, LDS-resident and large
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,form', [(10, 13, 'lds'), (96, 96, 'lds'), (120, 136, 'large')])
@pytest.mark.parametrize('low', [True, False], ids=['low_tree', 'high_tree'])
def test_tree_filter_guarded(dev, H, W, form, low):
    """mst / bfs / refine with every input guarded: the edge list and the tree -- int32 [B, E, 2] / [B, V-1, 2] -- at lead 1, 4- but not
    8-byte aligned (tree_filter_large.hip copies edges as int2), the BFS tables at lead 1-3.  mst against the tree the oracle selects, bfs
    under the validity rules of _check_bfs (which runs it three times, both algorithms), refine against the fp64 oracle at the tolerances
    of test_refine_forward_backward_vs_oracle / test_large_refine_forward_backward_vs_oracle."""
    from boxinstseg_amd import bfs, mst, refine
    from oracle import tree_filter_oracle as tfo
    from tests.test_gpu_tree_filter import _check_bfs, _edge_set
    B, Cc = 2, 2
    V = H * W
    assert (V > 10200) == (form == 'large')
    rng = np.random.default_rng(H * 5 + W + low)
    idx = tfo.grid_edges(H, W)
    fm = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    wt = np.stack([tfo.grid_weights(fm[b]) for b in range(B)])
    E = _Inputs(dev)
    gidx, gwt = E(np.repeat(idx[None], B, 0), 1, 1024, torch.int32), E(wt, 3)
    with G.poisoned_empty(), _Hook() as hk:
        tree = mst(gidx.t, gwt.t, V)
    torch.cuda.synchronize()
    assert ('mst_large_emit' in hk.names) == (form == 'large') and ('mst' in hk.names) == (form == 'lds'), hk.names
    tn = tree.cpu().numpy()
    for b in range(B):
        want = tfo.ref_boruvka_mst(idx, wt[b], V) if tfo.ref_available() else idx[tfo.mst_edges(idx, wt[b], V)]
        assert _edge_set(tn[b]) == _edge_set(want), 'not the tree the reference Boruvka selects'
    gtree = E(tree, 1, 1024)
    assert gtree.ptr() % 8 == 4
    with G.poisoned_empty(), _Hook() as hk:
        _check_bfs(gtree.t, V)
        si, sp, sc = bfs(gtree.t, 4)
    assert ('bfs_large_index' in hk.names) == (form == 'large') and ('bfs' in hk.names) == (form == 'lds'), hk.names
    sin, spn, scn = si.cpu().numpy(), sp.cpu().numpy(), sc.cpu().numpy()
    x = rng.standard_normal((B, Cc, V)).astype(np.float32)
    g = rng.standard_normal((B, Cc, V)).astype(np.float32)
    emb = rng.standard_normal((B, 3, V)) * (0.05 if low else 0.4)
    w = np.stack([tfo.edge_weights(emb[b], sin[b], spn[b], low) for b in range(B)]).astype(np.float32)
    gx, gw, gg = E(x, 1, G.plane_band(H, W)), E(w, 3, G.plane_band(H, W)), E(g, 2, G.plane_band(H, W))
    gsi, gsp, gsc, glv = E(si, 1), E(sp, 3), E(sc, 2), E(si._bxi_levels, 1)
    gsi.t._bxi_levels = glv.t
    xd, wd = _leaf(gx), _leaf(gw)
    with G.poisoned_empty(), _Hook() as hk:
        out = refine(xd, wd, gsi.t, gsp.t, gsc.t, low)
        out.backward(gg.t)
    torch.cuda.synchronize()
    assert ('tree_refine_large_out' in hk.names) == (form == 'large') and ('tree_refine' in hk.names) == (form == 'lds'), hk.names
    E.check()
    for b in range(B):
        want, saved = tfo.refine_forward(x[b].astype(np.float64), w[b].astype(np.float64), sin[b], spn[b], scn[b])
        assert np.abs(out[b].detach().cpu().numpy() - want).max() <= 2e-5 * max(np.abs(want).max(), 1.0)
        gf = tfo.refine_backward_feature(g[b].astype(np.float64), w[b].astype(np.float64), sin[b], spn[b], scn[b], saved)
        assert np.abs(xd.grad[b].cpu().numpy() - gf).max() <= 2e-5 * max(np.abs(gf).max(), 1.0)
        if low:
            assert wd.grad is None
        else:
            gwt_ = tfo.refine_backward_weight(x[b].astype(np.float64), g[b].astype(np.float64), w[b].astype(np.float64), sin[b], spn[b], scn[b], saved)
            assert wd.grad.shape == wd.shape and np.abs(wd.grad[b].cpu().numpy() - gwt_).max() <= 1e-4 * max(np.abs(gwt_).max(), 1.0)


# ---------------------------------------------------------------------------------------------
# non-contiguous inputs, as the reference's callers produce them
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def test_noncontiguous_inputs_equal_their_contiguous_copies(dev):
    """`[:, 0:1]` of a two-channel tensor, a permuted tensor, channels_last images, gt_bboxes as row slices of one tensor, an expanded
    (stride-0) upstream gradient as `.sum().backward()` makes it: the result equals the call on .contiguous() copies bit for bit, .grad has the
    input's shape, the caller's tensor is not modified.  pairwise_nlog_forward refuses non-contiguous input by contract (the reference's
    CHECK_INPUT): the refusal is asserted."""
    from boxinstseg_amd import (BoxProjectionLoss, LevelsetLoss, LocalConsistencyModule, boxinst_mask_loss, dice_loss, mil_loss, pairwise_nlog,
                                pairwise_nlog_forward, synthetic)
    rng = np.random.default_rng(3)
    T = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)

    def both(fn, make_inputs, grads_of):
        """fn(*inputs) -> a tensor; run on the non-contiguous inputs and on contiguous copies, `.sum().backward()` (an expanded gradient)."""
        res = []
        for contiguous in (False, True):
            ins = make_inputs()
            keep = [i.detach().clone() for i in ins]
            assert any(not i.is_contiguous() for i in ins)
            if contiguous:
                ins = [i.detach().contiguous() for i in ins]
            ins = [i.detach().requires_grad_(k in grads_of) if i.is_floating_point() else i for k, i in enumerate(ins)]
            with G.poisoned_empty():
                out = fn(*ins)
                out.sum().backward()
            torch.cuda.synchronize()
            for i, k in zip(ins, keep):
                assert torch.equal(i.detach(), k), 'the caller\'s tensor was modified'
            for k in grads_of:
                assert ins[k].grad.shape == ins[k].shape
            res.append((out.detach(), [ins[k].grad for k in grads_of]))
        assert torch.equal(_bits(res[0][0]), _bits(res[1][0]))
        for a, b in zip(res[0][1], res[1][1]):
            assert torch.equal(_bits(a), _bits(b))

    N, H, W = 3, 12, 20
    two = T(rng.uniform(0, 1, (N, 2, H, W)))
    box = T((rng.uniform(0, 1, (N, 2, H, W)) > 0.5))
    both(lambda s, b: BoxProjectionLoss()(s, b), lambda: [two[:, 0:1], box[:, 1:2]], [0])
    ms_nhwc, t_nhwc = T(rng.uniform(0, 1, (N, H, W, 2))), T(rng.uniform(-1, 1, (N, H, W, 3)))
    pn = T(np.full(N, 17.0))
    both(lambda m, t: LevelsetLoss(loss_weight=2.0)(m, t, pn), lambda: [ms_nhwc.permute(0, 3, 1, 2), t_nhwc.permute(0, 3, 1, 2)], [0, 1])
    x3 = T(rng.uniform(0, 1, (N, 2, H, W)))
    tg = T(rng.uniform(0, 1, (N, H, W)) > 0.6)
    both(lambda x: mil_loss(dice_loss, x, x, tg), lambda: [x3[:, 1]], [0])
    both(lambda x: dice_loss(x, tg), lambda: [x3.permute(1, 0, 2, 3)[0]], [0])
    img_cl = T(rng.standard_normal((2, 3, 24, 30))).contiguous(memory_format=torch.channels_last)
    phi2 = T(rng.uniform(0, 1, (2, 2, 24, 30)))
    lcm = LocalConsistencyModule(num_iter=3, dilations=[2])
    both(lambda im, ph: lcm(im, ph), lambda: [img_cl, phi2[:, 0:1]], [1])
    # the fused loss: channels_last images, logits as channel 0 of a two-channel tensor, gt_bboxes as row slices of one tensor
    d = synthetic.make_batch(B=2, H=96, W=160, boxes_per_img=3, inst_per_box=2, seed=7, img_shapes=[(96, 131), (70, 160)],
                             ori_shapes=[(48, 66), (210, 480)], min_box=16, max_box=80)
    imgs_cl = T(d['imgs']).contiguous(memory_format=torch.channels_last)
    lg2 = torch.stack([T(d['mask_logits'][:, 0]), T(rng.standard_normal(d['mask_logits'][:, 0].shape))], 1)
    allb = T(np.concatenate([np.concatenate(d['gt_bboxes'], 0), np.zeros((6, 1), np.float32)], 1))     # [G, 5]: xyxy + a label column
    gt_inds = torch.from_numpy(d['gt_inds']).to(dev)

    def loss(logits, imgs, boxes5):
        boxes = [boxes5[0:3, :4], boxes5[3:6, :4]]
        assert not boxes[0].is_contiguous()
        o = boxinst_mask_loss(logits, gt_inds, boxes, imgs=imgs, img_metas=d['img_metas'], warmup_factor=0.37)
        return 0.5 * o['loss_prj'] + 3.0 * o['loss_pairwise']
    both(loss, lambda: [lg2[:, 0:1], imgs_cl, allb], [0])
    # the op-level entry refuses non-contiguous input, as the reference's CHECK_INPUT does; the autograd op takes what its callers hand it
    with pytest.raises(RuntimeError, match='contiguous'):
        pairwise_nlog_forward(3, 2, lg2[:, 0:1])
    both(lambda x: pairwise_nlog(x.contiguous(), 3, 2), lambda: [lg2[:, 0:1]], [0])


# ---------------------------------------------------------------------------------------------
# existing oracle checks once more, with every torch.empty of the wrappers poisoned
# ---------------------------------------------------------------------------------------------
def _existing_checks():
    import tests.test_gpu_discobox as td
    import tests.test_gpu_dynamic_head as th
    import tests.test_gpu_levelset as tl
    import tests.test_gpu_mask_paste as tm
    import tests.test_gpu_parity as tp
    import tests.test_gpu_tree_filter as tt

    def params_of(fn):
        out = [()]
        for mark in getattr(fn, 'pytestmark', []):
            if mark.name == 'parametrize':
                names = [s.strip() for s in mark.args[0].split(',')] if isinstance(mark.args[0], str) else list(mark.args[0])
                vals = [v if len(names) > 1 else (v,) for v in mark.args[1]]
                out = [dict(zip(names, v), **(o if o else {})) for v in vals for o in out]
        return [o if o else {} for o in out]

    cases = [('test_loss_cfg2_four_per_box', lambda dev: tp.test_loss_cfg2_four_per_box(dev))]
    for seed in (100, 101, 102, 103):
        cases.append((f'test_loss_fuzz_forms_and_targets_ahead-{seed}', lambda dev, seed=seed: tp.test_loss_fuzz_forms_and_targets_ahead(dev, seed)))
    for mod, name, needs_built in ((tl, 'test_projection_and_levelset_vs_oracle', True), (tl, 'test_lcm_vs_oracle', True), (td, 'test_meanfield_vs_oracle', True),
                                   (th, 'test_dynamic_head_vs_oracle_large', False), (tm, 'test_kernel_vs_fp64_and_torch', False)):
        fn = getattr(mod, name)
        for kw in params_of(fn):
            tag = '-'.join('x'.join(str(e) for e in v) if isinstance(v, tuple) else str(v) for v in kw.values())
            if needs_built:
                cases.append((f'{name}-{tag}', lambda dev, fn=fn, kw=kw: fn(True, dev, **kw)))
            else:
                cases.append((f'{name}-{tag}', lambda dev, fn=fn, kw=kw: fn(dev, **kw)))
    for low in (True, False):
        for form in (0, 16):
            def run(dev, low=low, form=form):
                from boxinstseg_amd import _lib
                lib = _lib.load()
                lib.bxi_dev_set_tree_level_walk(1 if form else 0)          # (what the large_form fixture does)
                try:
                    tt.test_large_refine_forward_backward_vs_oracle(True, dev, low, form)
                finally:
                    lib.bxi_dev_set_tree_level_walk(0)
            cases.append((f'test_large_refine_forward_backward_vs_oracle-{low}-{form}', run))
    return cases


_EXISTING = _existing_checks()


@pytest.mark.parametrize('case', range(len(_EXISTING)), ids=[c[0] for c in _EXISTING])
def test_existing_oracle_checks_with_poisoned_allocations(dev, case):
    """The existing oracle checks, called directly (as test_many_shapes_in_one_process_without_resets calls test_loss_fuzz), while torch.empty /
    empty_like / new_empty hand out pattern-filled memory: a form that skips a tile can no longer find the other form's bits in a recycled block,
    and a kernel that depends on what its 'contents undefined' scratch holds shows."""
    with G.poisoned_empty():
        _EXISTING[case][1](dev)
