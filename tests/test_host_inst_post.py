"""CPU: the host side of Box2Mask's test-time path (no kernel is launched here).

* the float64 restatement of tests/inst_post_ref.py equals the reference fixture (tests/golden/box2mask_test.npz, made by executing the
  reference's statements) under the stated rules, and the fixture's inputs obey the input conditions;
* the header's constants are those of _lib; _lib.INST_SIGNATURES holds the three entry points and the build lists the sources;
* the panoptic_fusion_head and test_cfg blocks of the six configs/box2mask files build MaskFormerFusionHead unchanged;
* the exports and the documents name the feature;
* the three entry points validate their arguments before anything touches a device, in the order the header states; n == 0 and B == 0
  touch nothing; CPU tensors raise."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import inst_post_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


@pytest.fixture(scope='module')
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_restatement_equals_the_fixture(golden, name):
    c = R.CASES[name]
    g = {k.split('/', 1)[1]: v for k, v in golden.items() if k.startswith(name + '/')}
    cls, pred = R.case_inputs(name)
    assert np.array_equal(cls, g['cls']) and np.array_equal(pred, g['pred'])   # the seeded inputs are the recorded ones
    C, out = c['things'] + c['stuff'], tuple(c['ori']) if c['rescale'] else tuple(c['crop'])
    # input conditions: the top-k band holds at most two indices, the mask band at most 0.1 % of the pixels
    s64 = R.softmax64(cls).reshape(-1)
    cut = np.sort(s64)[::-1][c['k'] - 1]
    assert int(((s64 >= cut * (1 - 2.0 ** -20)) & (s64 <= cut * (1 + 2.0 ** -20))).sum()) - 1 <= 2
    scores, labels, query, flat = R.topk_ref(cls, c['things'], c['k'])
    assert len(flat) == len(g['flat']) and sorted(flat.tolist()) == sorted(g['flat'].tolist())
    assert np.all(np.diff(scores) <= 0) and (len(flat) < c['k']) == (c['stuff'] > 0)
    order = np.array([flat.tolist().index(f) for f in g['flat']], np.int64)
    assert np.array_equal(labels[order], g['labels']) and np.allclose(scores[order], g['cls_scores'], rtol=1e-5, atol=0)
    p = R.p64(pred, query[order], c['up'], c['crop'], out)
    ref_masks = np.unpackbits(g['masks'], axis=1)[:, :out[0] * out[1]].reshape(-1, *out)
    R.check_masks(ref_masks, p, pred, query[order], name)
    m, stats, mask_scores, boxes = R.instance_ref(p, scores[order])
    same = (m == ref_masks).reshape(len(m), -1).all(1)
    assert same.mean() >= 0.75
    assert np.array_equal(boxes[same, :4], g['bboxes'][same, :4].astype(np.float64))
    assert np.allclose(mask_scores[same], g['mask_scores'][same], rtol=1e-5, atol=1e-7)
    assert np.allclose(boxes[same, 4], g['bboxes'][same, 4], rtol=1e-5, atol=1e-7)
    # the detector's loop, restated, on the reference's own results
    fb, fm = R.format_ref(g['labels'], g['bboxes'], ref_masks, c['things'])
    assert np.array_equal(np.concatenate(fb), g['fmt_boxes']) and [len(b) for b in fb] == g['fmt_box_counts'].tolist()
    assert [len(x) for x in fm] == g['fmt_mask_counts'].tolist() and [int(x.sum()) for per in fm for x in per] == g['fmt_mask_areas'].tolist()
    assert all(b.dtype == np.float32 for b in fb) and all(x.dtype == np.bool_ for per in fm for x in per)
    if name == 'zero_plane':
        z = np.nonzero(query[order] == 2)[0]
        assert len(z) >= 1 and not m[z].any() and not boxes[z].any() and stats[z[0]].tolist() == [0, -1, -1, -1, -1]


def test_restatement_by_hand():
    p = np.full((3, 4, 6), -1.0)
    p[1, 1:3, 2:5] = np.log(3.0)                                                # sigmoid = 0.75
    p[2] = 30.0
    m, stats, ms, boxes = R.instance_ref(p, [0.5, 0.5, 0.25])
    assert stats.tolist() == [[0, -1, -1, -1, -1], [6, 2, 1, 4, 2], [24, 0, 0, 5, 3]]
    assert boxes[0].tolist() == [0, 0, 0, 0, 0] and boxes[1, :4].tolist() == [2, 1, 5, 3] and boxes[2, :4].tolist() == [0, 0, 6, 4]
    assert abs(ms[1] - 0.75 * 6 / (6 + 1e-6)) < 1e-15 and abs(boxes[1, 4] - 0.5 * ms[1]) < 1e-16 and abs(ms[2] - 24 / (24 + 1e-6)) < 1e-12
    # the defined order: descending, ties by ascending index, NaN last
    assert R.defined_order([0.1, 0.5, np.nan, 0.5, 0.7]).tolist() == [4, 1, 3, 0, 2]
    cls = np.log(np.array([[1, 2, 3, 4.0], [1, 2, 3, 4.0]]))
    s, lab, q, flat = R.topk_ref(cls, 2, 3)
    assert flat.tolist() == [1] and lab.tolist() == [1] and q.tolist() == [0] and abs(s[0] - 0.2) < 1e-15     # [2, 5, 1] cut to labels < 2
    assert R.tie_band(np.array([[[4.0, -8.0]], [[0.0, 0.0]]]), [1, 0, 7]).tolist() == [0.0, 8 * 2.0 ** -20, 0.0]


def test_header_constants_exports_and_build_lists():
    from boxinstseg_amd import _lib, build
    with open(os.path.join(ROOT, 'include/boxinst/boxinst_hip_inst.h')) as fh:
        header = fh.read()
    assert int(re.search(r'#define BXI_INST_TOPK_MAX (\d+)', header).group(1)) == _lib.INST_TOPK_MAX >= 100 * 133
    assert sorted(_lib.INST_SIGNATURES) == ['bxi_inst_paste_u8', 'bxi_inst_paste_workspace_bytes', 'bxi_inst_topk_f32']
    assert 'inst_post.hip' in build.SOURCES and 'paste_device.hpp' in build.HEADERS
    assert any(h.endswith('boxinst_hip_inst.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS)
    with open(os.path.join(build.CSRC, 'inst_post.hip')) as fh:
        code = fh.read()
    assert 'paste_tile<false, true, true>' in code and 'atomicAdd' not in code        # the third user of the tile, no float atomics of its own


def test_the_six_configs_build_the_fusion_head():
    import boxinstseg_amd as B
    stored = R.load_cfg()
    assert len(stored) == 6 and all(f.startswith('box2mask_') and f.endswith('.py') for f in stored)
    configs = os.path.join(REFERENCE, 'configs/box2mask')
    if os.path.isdir(configs):
        assert sorted(stored) == sorted(os.listdir(configs))
        for f in stored:
            model = B.load_config(os.path.join(configs, f))['model']
            assert dict(panoptic_fusion_head=model['panoptic_fusion_head'], test_cfg=model['test_cfg']) == stored[f], f
    assert B.HEADS.get('MaskFormerFusionHead') is B.MaskFormerFusionHead
    for f, blocks in stored.items():
        cfg = dict(blocks['panoptic_fusion_head'])
        assert cfg['type'] == 'MaskFormerFusionHead'
        head = B.build_head(cfg, default_args=dict(test_cfg=blocks['test_cfg']))           # as the detector builds it
        assert isinstance(head, B.MaskFormerFusionHead) and head.test_cfg == blocks['test_cfg']
        things = 20 if f.endswith('_voc.py') else 80
        assert (head.num_things_classes, head.num_stuff_classes, head.num_classes) == (things, 0, things) and head.test_cfg['max_per_image'] == 100
        assert head.test_cfg['panoptic_on'] is False and head.test_cfg['instance_on'] is True and head.forward_train() == {}
    assert list(inspect.signature(B.MaskFormerFusionHead.simple_test).parameters) == \
        ['self', 'mask_cls_results', 'mask_pred_results', 'img_metas', 'rescale', 'kwargs']
    assert list(inspect.signature(B.MaskFormerFusionHead.__init__).parameters) == \
        ['self', 'num_things_classes', 'num_stuff_classes', 'test_cfg', 'loss_panoptic', 'init_cfg', 'kwargs']
    # the modes that are not built raise before anything else is looked at
    x = torch.zeros(1, 2, 3)
    with pytest.raises(NotImplementedError, match='panoptic_on'):
        B.MaskFormerFusionHead(2, 0, test_cfg=dict(instance_on=True)).simple_test(x, x, [{}])           # the reference's default is True
    with pytest.raises(NotImplementedError, match='semantic_on'):
        B.MaskFormerFusionHead(2, 0, test_cfg=dict(panoptic_on=False, semantic_on=True)).simple_test(x, x, [{}])
    with pytest.raises(NotImplementedError, match='loss_panoptic'):
        B.MaskFormerFusionHead(2, 0, loss_panoptic=dict(type='X'))
    assert B.MaskFormerFusionHead(2, 0, test_cfg=dict(panoptic_on=False)).simple_test(x, x, [{}]) == [{}]   # instance_on defaults to False


def test_exports_and_documents_name_the_feature():
    import boxinstseg_amd as B
    for name in ('instance_topk', 'box2mask_instances', 'MaskFormerFusionHead', 'box2mask_format_results'):
        assert name in B.__all__ and name in B.__doc__ and callable(getattr(B, name)), name
    for rel, words in (('README.md', ('inst_post', 'box2mask_instances')),
                       ('INTEGRATION.md', ('Level 3m', 'instance_topk', 'box2mask_instances', 'box2mask_format_results', 'MaskFormerFusionHead',
                                           'bxi_inst_topk_f32', 'bxi_inst_paste_u8', 'ascending flat index', '2^-20', 'BXI_INST_TOPK_MAX')),
                       ('profiles/NOTES.md', ('inst_post',))):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (rel, word)


def test_topk_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000
    d = dict(cls=X, B=2, Q=12, C=5, things=3, k=14, scores=X, labels=X, query=X, count=X)

    def call(**kw):
        a = {**d, **kw}
        return lib.bxi_inst_topk_f32(a['cls'], a['B'], a['Q'], a['C'], a['things'], a['k'], a['scores'], a['labels'], a['query'], a['count'], None)
    # BAD_SHAPE, in the header's order; each before the later checks (the pointers are never NULL-checked first)
    assert call(B=-1, cls=None) == -2 and call(Q=0, cls=None) == -2 and call(C=0, cls=None) == -2 and call(k=0, cls=None) == -2
    assert call(things=-1, cls=None) == -2 and call(things=6, cls=None) == -2 and call(things=5, cls=None) == -1 and call(things=0, cls=None) == -1
    assert call(B=1 << 20, Q=1 << 10, C=1, k=1) == -2                          # B * Q * (C + 1) >= 2^31
    assert call(k=0, Q=1 << 20) == -2                                          # BAD_SHAPE before UNSUPPORTED
    # UNSUPPORTED: k > Q * C, Q * C > BXI_INST_TOPK_MAX; before the B == 0 exit and the pointers
    assert call(k=61) == _lib.BXI_ERR_UNSUPPORTED and call(k=60, cls=None) == -1
    assert call(Q=128, C=129, things=3, cls=None) == _lib.BXI_ERR_UNSUPPORTED and call(Q=128, C=128, cls=None) == -1 and call(Q=100, C=133, cls=None) == -1
    assert call(k=61, B=0) == _lib.BXI_ERR_UNSUPPORTED
    assert call(B=0, cls=None, scores=None, labels=None, query=None, count=None) == 0
    for key in ('cls', 'scores', 'labels', 'query', 'count'):
        assert call(**{key: None}) == -1, key


def test_paste_validation_without_device():
    from boxinstseg_amd import _lib
    lib = _lib.load()
    X = 0x1000
    d = dict(logits=X, n_all=5, h=13, w=21, query=X, cls=X, n=4, up_h=52, up_w=84, crop_h=50, crop_w=81, out_h=37, out_w=61, masks=X, stats=X,
             ms=X, boxes=X, ws=X)
    need = lib.bxi_inst_paste_workspace_bytes(4, 37, 61)
    assert need == 16 * 4 * 37

    def call(**k):
        a = {**d, 'bytes': need, **k}
        return lib.bxi_inst_paste_u8(a['logits'], a['n_all'], a['h'], a['w'], a['query'], a['cls'], a['n'], a['up_h'], a['up_w'], a['crop_h'],
                                     a['crop_w'], a['out_h'], a['out_w'], a['masks'], a['stats'], a['ms'], a['boxes'], a['ws'], a['bytes'], None)
    for key in ('n_all', 'h', 'w', 'up_h', 'up_w', 'crop_h', 'crop_w', 'out_h', 'out_w'):
        assert call(**{key: 0}) == -2 and call(**{key: -3}) == -2, key
    assert call(crop_h=53) == -2 and call(crop_w=85) == -2 and call(n=-1) == -2
    assert call(crop_h=52, crop_w=84, ws=None) == -5                          # crop == up is fine: the next check answers
    assert call(h=52, w=84, ws=None) == -5                                    # so is an identity stage 1
    assert call(n=1 << 27, out_h=256, out_w=61) == -2 and call(n=1 << 20, out_h=1 << 14, out_w=2048) == -2
    assert call(n_all=1 << 23, h=16, w=16) == -2 and call(n_all=(1 << 23) - 1, h=16, w=16, ws=None) == -5
    assert call(out_h=1 << 16, out_w=1 << 15) == -2
    assert call(n=-1, logits=None) == -2                                      # the shape before the pointers
    # n == 0 touches nothing, whatever the pointers are
    assert call(n=0, logits=None, query=None, cls=None, masks=None, stats=None, ms=None, boxes=None, ws=None, bytes=0) == 0
    for key in ('logits', 'query', 'cls', 'masks', 'stats', 'ms', 'boxes'):
        assert call(**{key: None}) == -1 and call(**{key: None}, ws=None) == -1, key      # the pointers before the workspace
    assert call(ws=None) == -5 and call(bytes=need - 1) == -5 and call(ws=X + 8) == -5
    assert call(w=9000, up_w=36000, crop_w=81) == _lib.BXI_ERR_UNSUPPORTED    # source rows that do not fit the staging buffer
    assert call(w=9000, up_w=36000, crop_w=81, ws=None) == -5                 # ... which is looked at last


def test_workspace_size():
    from boxinstseg_amd import _lib
    q = _lib.load().bxi_inst_paste_workspace_bytes
    assert q(0, 37, 61) == 0 and q(1, 37, 61) == 16 * 37 and q(1, 37, 1024) == 16 * 37 and q(1, 37, 1025) == 2 * 16 * 37
    assert q(100, 480, 640) == 100 * 480 * 16 and q(100, 800, 1333) == 2 * 100 * 800 * 16
    assert q(-1, 37, 61) == 0 and q(4, 0, 61) == 0 and q(4, 37, 0) == 0 and q(1 << 27, 256, 61) == 0 and q(1, 1 << 16, 1 << 15) == 0


def test_cpu_tensors_raise_and_empty_batch():
    import types
    import boxinstseg_amd as B
    meta = dict(batch_input_shape=(28, 36), img_shape=(27, 33, 3), ori_shape=(40, 51, 3))
    cfg = dict(max_per_image=4)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.instance_topk(torch.rand(2, 5, 4), 3, 0, 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box2mask_instances(torch.rand(1, 5, 4), torch.rand(1, 5, 7, 9), [meta], cfg, 3, 0)
    res = types.SimpleNamespace(masks=torch.zeros(2, 40, 51, dtype=torch.bool), host_block=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='CUDA'):
        B.box2mask_format_results(res, 3)
