"""Regenerate tests/golden/det_nms.npz by EXECUTING the reference's own code on the CPU (developer tool; needs the upstream
checkout, BOXINST_REFERENCE_ROOT or /root/reference).  Nothing of the reference is copied: ``CondInstBoxHead._get_bboxes``,
``nms_with_others``, ``distance2bbox``, ``get_k_for_topk`` and ``MlvlPointGenerator`` are taken out of their files by AST and compiled
in memory; a stand-in module answers the inner ``from mmdet.core.export import get_k_for_topk``; ``batched_nms`` -- mmcv's, whose
source is not part of the reference -- is supplied by tests/box_nms_ref.py:batched_nms_mmcv_style (the class-offset trick), and
records the candidates it is handed.  The fixture holds arrays only.

Cases (tests/box_nms_ref.py:DET_CASES), all on one set of inputs: levels 12x20, 6x10, 3x5 at strides 8 / 16 / 32, C = 5, P = 9,
B = 3, nms_pre = 40 (it cuts the 240 and the 60 locations of the first two levels), image 1 without any candidate.
  lv3   rescale off            resc  rescale on, non-square scale factors
  cut   max_per_img = 7        agn   class_agnostic=True

Every case runs twice, in float32 and in float64; ``tol`` is the largest difference between the two runs' candidate scores.
A seed is rejected unless, relative to 100 * tol: every sigmoid(cls) is away from score_thr, every level's top-k boundary is
separated, neighbouring candidate scores are separated; and every pair of candidates NMS may compare has |IoU - thr| > 1e-4 in
float64 (about six fp32 roundings of 6e-8 each decide the fp32 test: 1e-4 is more than 100 times that, and it covers the division
form of the threshold test as well)."""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch.nn.modules.utils import _pair

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import box_nms_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD_FILE = os.path.join(REF, 'mmdet/models/dense_heads/condinst_head.py')
TRANSFORMS_FILE = os.path.join(REF, 'mmdet/core/bbox/transforms.py')
EXPORT_FILE = os.path.join(REF, 'mmdet/core/export/onnx_helper.py')
POINTS_FILE = os.path.join(REF, 'mmdet/core/anchor/point_generator.py')
SEED0 = 11
IOU_MARGIN = 1e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _take(path, name, env, cls=None):
    """Compile one function (of class ``cls``) or one class of the file into ``env``, decorators dropped."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = tree.body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name)
    node.decorator_list = []
    m = ast.Module(body=[node], type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, 'exec'), env)
    return env[name]


def load_reference(record):
    def batched_nms(bboxes, scores, labels, nms_cfg):
        record.append((bboxes.numpy().copy(), scores.numpy().copy(), labels.numpy().copy()))
        dtype = np.float32 if bboxes.dtype == torch.float32 else np.float64
        dets, keep = R.batched_nms_mmcv_style(bboxes.numpy(), scores.numpy(), labels.numpy(), dict(nms_cfg), dtype=dtype)
        return torch.from_numpy(dets), torch.from_numpy(keep)

    get_k = _take(EXPORT_FILE, 'get_k_for_topk', {'torch': torch, 'os': os})
    for name in ('mmdet', 'mmdet.core', 'mmdet.core.export'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['mmdet.core.export'].get_k_for_topk = get_k
    distance2bbox = _take(TRANSFORMS_FILE, 'distance2bbox', {'torch': torch, 'np': np})
    nwo = _take(HEAD_FILE, 'nms_with_others', {'torch': torch, 'batched_nms': batched_nms})
    get = _take(HEAD_FILE, '_get_bboxes', {'torch': torch, 'distance2bbox': distance2bbox, 'nms_with_others': nwo}, cls='CondInstBoxHead')
    gen = _take(POINTS_FILE, 'MlvlPointGenerator', {'torch': torch, 'np': np, '_pair': _pair})
    return get, gen


def run_reference(inp, name, dtype):
    """The reference's _get_bboxes on the case, in ``dtype``: (per image outputs, per image candidates handed to batched_nms)."""
    rescale, c = R.DET_CASES[name]
    record = []
    get, gen = load_reference(record)
    t = lambda maps: [torch.from_numpy(m).to(dtype) for m in maps]          # noqa: E731
    cls, bbox, ctr, params = t(inp['cls']), t(inp['bbox']), t(inp['ctr']), t(inp['params'])
    points = gen(list(R.DET_STRIDES)).grid_priors([m.shape[-2:] for m in cls], dtype, 'cpu')
    nms = dict(type='nms', iou_threshold=c['iou_threshold'])
    if c['class_agnostic']:
        nms['class_agnostic'] = True
    cfg = Cfg(nms_pre=c['nms_pre'], min_bbox_size=0, score_thr=c['score_thr'], nms=nms, max_per_img=c['max_per_img'])
    me = types.SimpleNamespace(cls_out_channels=R.DET_C, test_cfg=None)
    scale_factors = [np.array(s, np.float32) for s in R.DET_SCALES]
    res = get(me, cls, bbox, ctr, params, points, list(R.DET_IMG_SHAPES), scale_factors, cfg, rescale, True)
    cands, at = [], 0
    for b in range(R.DET_B):
        if res[b][0].shape[0] == 0 and (at >= len(record) or b == R.DET_EMPTY_IMAGE):
            cands.append((np.zeros((0, 4), np.float32), np.zeros(0), np.zeros(0, np.int64)))
        else:
            cands.append(record[at])
            at += 1
    assert at == len(record)
    return res, cands


def reference_case(name, inp):
    """name -> {fixture key: array} from two runs of the reference (float32 and float64)."""
    res32, cand32 = run_reference(inp, name, torch.float32)
    res64, cand64 = run_reference(inp, name, torch.float64)
    out, tol = {}, 0.0
    for b in range(R.DET_B):
        k = f'{name}{b}'
        assert np.array_equal(cand32[b][2], cand64[b][2]) and np.array_equal(cand32[b][0], cand64[b][0].astype(np.float32)), k
        assert np.array_equal(res32[b][1].numpy(), res64[b][1].numpy()) and np.array_equal(res32[b][3].numpy(), res64[b][3].numpy()), k
        if len(cand32[b][1]):
            tol = max(tol, float(np.abs(cand32[b][1].astype(np.float64) - cand64[b][1]).max()))
        out.update({f'{k}_cand_boxes': cand32[b][0].astype(np.float32), f'{k}_cand_scores32': cand32[b][1].astype(np.float32),
                    f'{k}_cand_scores64': cand64[b][1].astype(np.float64), f'{k}_cand_labels': cand32[b][2].astype(np.int64),
                    f'{k}_dets32': res32[b][0].numpy().astype(np.float32), f'{k}_scores64': res64[b][0][:, 4].numpy().astype(np.float64),
                    f'{k}_labels': res32[b][1].numpy().astype(np.int64), f'{k}_params': res32[b][2].numpy().astype(np.float32),
                    f'{k}_coors': res32[b][3].numpy().astype(np.float32), f'{k}_level_inds': res32[b][4].numpy().astype(np.int64)})
    out[f'{name}_tol'] = np.array(tol)
    return out


def _rel_gap(values, at=None):
    """Smallest relative distance between neighbours of the sorted values, or of every value from ``at``."""
    v = np.sort(np.asarray(values, np.float64).reshape(-1))
    if at is not None:
        return float((np.abs(v - at) / at).min()) if len(v) else np.inf
    return float((np.diff(v) / np.maximum(v[1:], 1e-30)).min()) if len(v) > 1 else np.inf


def margins_ok(inp, name, case):
    """The rejection rules of the module docstring; prints what it found."""
    rescale, c = R.DET_CASES[name]
    tol = float(case[f'{name}_tol'])
    need = 100 * tol
    sig = R.sigmoid(R.flatten_levels(inp['cls']), np.float64)
    g_thr = _rel_gap(sig, at=c['score_thr'])
    score = R.location_scores(inp, np.float64)
    off = R.level_offsets(R.DET_SIZES)
    g_topk = np.inf
    for i in range(len(R.DET_SIZES)):
        hw = int(off[i + 1] - off[i])
        if 0 < c['nms_pre'] < hw:
            for b in range(R.DET_B):
                s = np.sort(score[b, off[i]:off[i + 1]])[::-1]
                g_topk = min(g_topk, (s[c['nms_pre'] - 1] - s[c['nms_pre']]) / s[c['nms_pre'] - 1])
    g_score, g_iou = np.inf, np.inf
    for b in range(R.DET_B):
        g_score = min(g_score, _rel_gap(case[f'{name}{b}_cand_scores64']))
        g_iou = min(g_iou, R.iou_margin(case[f'{name}{b}_cand_boxes'], None if c['class_agnostic'] else case[f'{name}{b}_cand_labels'], c['iou_threshold']))
    print(f'{name}: tol {tol:.2e}; relative gaps: score_thr {g_thr:.1e}, top-k {g_topk:.1e}, scores {g_score:.1e} (need {need:.1e}); IoU margin {g_iou:.1e}')
    return tol > 0 and min(g_thr, g_topk, g_score) > need and g_iou > IOU_MARGIN


def restatement_agrees(inp, name, case):
    """tests/box_nms_ref.py:get_bboxes (label compare, the library's rules) gives what the reference executed gave."""
    rescale, c = R.DET_CASES[name]
    for T in (np.float32, np.float64):
        got = R.get_bboxes(inp, R.DET_STRIDES, R.det_img_dims(), c, rescale, T)
        for b, g in enumerate(got):
            k = f'{name}{b}'
            if not (np.array_equal(g['cand']['boxes'], case[f'{k}_cand_boxes']) and np.array_equal(g['cand']['labels'], case[f'{k}_cand_labels'])
                    and np.array_equal(g['dets'][:, :4].astype(np.float32), case[f'{k}_dets32'][:, :4]) and np.array_equal(g['labels'], case[f'{k}_labels'])
                    and np.array_equal(g['params'], case[f'{k}_params']) and np.array_equal(g['coors'], case[f'{k}_coors'])
                    and np.array_equal(g['level_inds'], case[f'{k}_level_inds'])):
                return False
    return True


def main():
    for seed in range(SEED0, SEED0 + 100):
        inp = R.det_inputs(seed)
        cases = {name: reference_case(name, inp) for name in R.DET_CASES}
        if all(margins_ok(inp, name, cases[name]) for name in R.DET_CASES) and all(restatement_agrees(inp, n, cases[n]) for n in R.DET_CASES):
            break
        print(f'seed {seed} rejected')
    else:
        raise SystemExit('no seed passed')
    out = {'seed': np.array(seed)}
    for k, maps in inp.items():
        for lv, m in enumerate(maps):
            out[f'in_{k}{lv}'] = m
    for name, case in cases.items():
        kept = [len(case[f'{name}{b}_labels']) for b in range(R.DET_B)]
        cand = [len(case[f'{name}{b}_cand_labels']) for b in range(R.DET_B)]
        print(f'{name}: candidates {cand}, kept {kept}')
        assert cand[R.DET_EMPTY_IMAGE] == 0 and min(c for b, c in enumerate(cand) if b != R.DET_EMPTY_IMAGE) > 20
        out.update(case)
    assert any(len(cases['lv3'][f'lv3{b}_labels']) > 7 for b in range(R.DET_B)), 'cut must cut'
    path = os.path.join(HERE, 'det_nms.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
