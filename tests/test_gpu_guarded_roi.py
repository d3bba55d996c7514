"""GPU: the kernel-launching entry points of include/boxinst/boxinst_hip_roi.h on misaligned views inside poisoned bands (tests/guarded.py).

fp32 inputs start 4, 8 or 12 bytes past a 16-byte boundary, the uint8 target 1 to 3 bytes, int64 labels at 8, surrounded by NaN / 0xFF / -1
(a NaN that was read reaches a pooled value or a gradient, a 0xFF byte widens a box); outputs are pre-filled with the 'nobody wrote this'
pattern, and so is the workspace, which is exactly as large as the size query says.  Afterwards the bands are intact, every output element
is written, the inputs are unchanged, and the results are bit-identical to the same call on plain tensors."""
import pytest
import torch

from tests import guarded as G
from tests import roi_ref as R

pytestmark = pytest.mark.gpu

# entry point -> the test that runs it guarded (tests/test_abi_families.py checks the table against _lib.ROI_SIGNATURES)
GUARDED = {
    'bxi_roi_target_boxes_u8': 'test_target_boxes_guarded',
    'bxi_roi_align_forward_f32': 'test_forward_guarded',
    'bxi_roi_align_backward_f32': 'test_backward_guarded',
    'bxi_roi_feat_norm_forward_f32': 'test_feat_norm_guarded',
    'bxi_roi_feat_norm_backward_f32': 'test_feat_norm_guarded',
}
CASE = R.op_cases()['float_ratio2_unaligned']
PLAIN = R.op_cases()['plain']
B_, C_, H_, W_ = (int(s) for s in CASE['feat'].shape)
BAND = G.plane_band(H_, W_)


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('own', [0, 1])
def test_target_boxes_guarded(dev, lead, own):
    from boxinstseg_amd import _lib, target_boxes
    from tests.test_gpu_roi_align import _targets
    t = _targets(lead % 2).to(dev)
    labels = torch.tensor([3, 1, 4, 1, 5, 9], device=dev)
    want = target_boxes(t, labels, bool(own))
    gt, gl = G.embed(t, lead, 1024), G.embed(labels, 1, 1024)
    boxes, keep, lab = G.out((6, 4), torch.float32, dev, lead), G.out(6, torch.uint8, dev, lead), G.out(6, torch.int64, dev, 1)
    G.ok(_lib.load().bxi_roi_target_boxes_u8(gt.ptr(), gl.ptr(), 6, 13, 21, own, boxes.ptr(), keep.ptr(), lab.ptr(), G.stream(dev)))
    G.check_bands(gt, gl, boxes, keep, lab)
    G.check_written(boxes, keep, lab)
    G.check_unchanged(gt, gl)
    assert G.same(boxes.t, want[0]) and torch.equal(keep.t.bool(), want[1]) and torch.equal(lab.t, want[2])


@pytest.mark.parametrize('lead', [1, 2, 3])
@pytest.mark.parametrize('flags', [0, 1])
def test_forward_guarded(dev, lead, flags):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    for c, size, sr, aligned in ((CASE, (7, 7), 2, 0), (PLAIN, (28, 5), 0, 1)):
        feat, rois = c['feat'].to(dev), c['rois'].to(dev)
        K = int(rois.shape[0])

        def call(f, r, o):
            G.ok(lib.bxi_roi_align_forward_f32(f, r, B_, C_, H_, W_, K, size[0], size[1], 1.0, sr, aligned, flags, o, G.stream(dev)))

        want = torch.empty((K, C_) + size, device=dev)
        call(feat.data_ptr(), rois.data_ptr(), want.data_ptr())
        gf, gr = G.embed(feat, lead, BAND), G.embed(rois, 4 - lead, BAND)
        out = G.out((K, C_) + size, torch.float32, dev, 4 - lead, BAND)
        call(gf.ptr(), gr.ptr(), out.ptr())
        G.check_bands(gf, gr, out)
        G.check_written(out)
        G.check_unchanged(gf, gr)
        assert G.same(out.t, want) and bool(torch.isfinite(out.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_backward_guarded(dev, lead):
    from boxinstseg_amd import _lib
    lib = _lib.load()
    for c, size, sr, aligned in ((CASE, (7, 7), 2, 0), (PLAIN, (28, 5), 0, 1)):
        rois = c['rois'].to(dev)
        K = int(rois.shape[0])
        g = torch.sin(torch.arange(K * C_ * size[0] * size[1], device=dev, dtype=torch.float32)).view((K, C_) + size)

        def call(gp, r, o):
            G.ok(lib.bxi_roi_align_backward_f32(gp, r, B_, C_, H_, W_, K, size[0], size[1], 1.0, sr, aligned, o, G.stream(dev)))

        want = torch.empty((B_, C_, H_, W_), device=dev)
        call(g.data_ptr(), rois.data_ptr(), want.data_ptr())
        gg, gr = G.embed(g, lead, BAND), G.embed(rois, 4 - lead, BAND)
        out = G.out((B_, C_, H_, W_), torch.float32, dev, lead, BAND)
        call(gg.ptr(), gr.ptr(), out.ptr())
        G.check_bands(gg, gr, out)
        G.check_written(out)
        G.check_unchanged(gg, gr)
        assert G.same(out.t, want) and bool(torch.isfinite(out.t).all())


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_feat_norm_guarded(dev, lead):
    """bxi_roi_feat_norm_forward_f32, then bxi_roi_feat_norm_backward_f32 on the workspace it left, both guarded."""
    from boxinstseg_amd import _lib, roi_feat_norm
    lib = _lib.load()
    c = R.fused_cases()['c70']
    feat, rois = c['feat'].to(dev), c['rois'].to(dev)
    Bn, Cn, Hn, Wn = (int(s) for s in feat.shape)
    K, band = int(rois.shape[0]), G.plane_band(Hn, Wn)
    x = feat.clone().requires_grad_(True)
    want = roi_feat_norm(x, rois)
    g = torch.sin(torch.arange(want.numel(), device=dev, dtype=torch.float32)).view(want.shape)
    want.backward(g)
    nbytes = lib.bxi_roi_feat_norm_workspace_bytes(K, Cn)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = G.out(nbytes // 4, torch.float32, dev, 0, band)                     # 16-byte aligned, exactly the size asked for
    gf, gr = G.embed(feat, lead, band), G.embed(rois, 4 - lead, band)
    out = G.out((K, Cn, 7, 7), torch.float32, dev, lead, band)
    G.ok(lib.bxi_roi_feat_norm_forward_f32(gf.ptr(), gr.ptr(), Bn, Cn, Hn, Wn, K, 1.0, 0, 1, out.ptr(), ws.ptr(), nbytes, G.stream(dev)))
    G.check_bands(gf, gr, out, ws)
    G.check_written(out)
    G.check_unchanged(gf, gr)
    assert G.same(out.t, want.detach())
    go, gg = G.embed(out.t.clone(), 4 - lead, band), G.embed(g, lead, band)
    gin = G.out((Bn, Cn, Hn, Wn), torch.float32, dev, 4 - lead, band)
    G.ok(lib.bxi_roi_feat_norm_backward_f32(go.ptr(), gg.ptr(), gr.ptr(), Bn, Cn, Hn, Wn, K, 1.0, 0, 1, gin.ptr(), ws.ptr(), nbytes, G.stream(dev)))
    G.check_bands(go, gg, gr, gin, ws)
    G.check_written(gin, ws)                                                 # the norms and the pooled gradients fill the workspace
    G.check_unchanged(go, gg, gr)
    assert G.same(gin.t, x.grad) and bool(torch.isfinite(gin.t).all())
