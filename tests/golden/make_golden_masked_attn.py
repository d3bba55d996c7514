"""Regenerate tests/golden/masked_attn.npz and masked_attn_cfg.json by EXECUTING the reference's own statements on the CPU (developer tool;
needs the upstream checkout, BOXINST_REFERENCE_ROOT).  Nothing of the reference is copied: the statements are taken out of
mmdet/models/dense_heads/box2mask_head.py by AST and compiled in memory --

    Box2MaskHead.forward_head   the four assignments to ``attn_mask`` (:346-355): F.interpolate, flatten / repeat over the heads,
                                ``sigmoid() < 0.5``, detach
    Box2MaskHead.forward        ``attn_mask[torch.where(attn_mask.sum(-1) == attn_mask.shape[-1])] = False`` (:397)

-- and run on the seeded logits and the planted integer logits of tests/masked_attn_ref.py for every size of MASK_CASES.  Recorded: the
logits and, per case, the reference's bool mask [B*heads, Q, S] packed to bits.  Checked before anything is written: the restatement
``box2mask_mask`` of tests/masked_attn_ref.py equals the reference's statements EXACTLY, in fp32 and fp64, and the heads' copies are equal.
The attn_cfgs block of the transformer decoder of every configs/box2mask file goes to masked_attn_cfg.json (they must all agree)."""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import masked_attn_ref as R  # noqa: E402

REF = os.environ.get('BOXINST_REFERENCE_ROOT', '/root/reference')
HEAD = 'mmdet/models/dense_heads/box2mask_head.py'


def _method(tree, cls, name):
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)


def _compile(nodes, path):
    m = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(m)
    return compile(m, path, 'exec')


def load_statements():
    path = os.path.join(REF, HEAD)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    head = _method(tree, 'Box2MaskHead', 'forward_head')
    block = [n for n in head.body if isinstance(n, ast.Assign) and [getattr(t, 'id', None) for t in n.targets] == ['attn_mask']]
    text = [ast.unparse(n) for n in block]
    assert len(block) == 4 and 'F.interpolate' in text[0] and 'repeat' in text[1] and 'sigmoid() < 0.5' in text[2] and 'detach' in text[3], text
    fwd = _method(tree, 'Box2MaskHead', 'forward')
    loop = next(n for n in fwd.body if isinstance(n, ast.For) and 'num_transformer_decoder_layers' in ast.unparse(n.iter))
    repair = [n for n in loop.body if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Subscript) and 'torch.where' in ast.unparse(n.targets[0])]
    assert len(repair) == 1 and 'attn_mask.sum(-1) == attn_mask.shape[-1]' in ast.unparse(repair[0]), [ast.unparse(n) for n in repair]
    return _compile(block, path), _compile(repair, path)


def reference_mask(code, mask_pred, size, heads):
    env = dict(torch=torch, F=F, mask_pred=mask_pred, attn_mask_target_size=size, self=types.SimpleNamespace(num_heads=heads))
    exec(code[0], env)
    exec(code[1], env)
    return env['attn_mask']


def main():
    import boxinstseg_amd as B
    code = load_statements()
    arrays = {'mask_pred': R.seeded_mask_pred().numpy(), 'planted': R.planted_mask_pred().numpy().astype(np.int8)}
    inputs = {'': torch.from_numpy(arrays['mask_pred']), 'planted_': R.planted_mask_pred()}
    for tag, pred in inputs.items():
        for name, (H, W, h, w) in R.MASK_CASES.items():
            if tag and name != 'f8':
                continue
            assert tuple(pred.shape) == (*R.MASK_SHAPE, H, W)
            for dtype in (torch.float32, torch.float64):
                ref = reference_mask(code, pred.to(dtype), (h, w), R.MASK_HEADS)
                mine = R.box2mask_mask(pred.to(dtype), (h, w), R.MASK_HEADS)
                assert ref.dtype == torch.bool and torch.equal(ref, mine), (tag, name, dtype)
                per_image = ref.view(R.MASK_SHAPE[0], R.MASK_HEADS, R.MASK_SHAPE[1], h * w)
                assert bool((per_image == per_image[:, :1]).all())               # the heads' copies are equal
                if dtype == torch.float32:
                    arrays[f'{tag}bits_{name}'] = R.pack_bits(ref).numpy()
                    assert torch.equal(R.unpack_bits(R.pack_bits(ref), h * w), ref)
    np.savez_compressed(R.GOLDEN, **arrays)
    print(f'wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes, {len(arrays)} arrays')
    blocks = {}
    for f in sorted(os.listdir(os.path.join(REF, 'configs/box2mask'))):
        cfg = B.load_config(os.path.join(REF, 'configs/box2mask', f))
        blocks[f] = cfg['model']['panoptic_head']['transformer_decoder']['transformerlayers']['attn_cfgs']
    first = next(iter(blocks))
    assert all(v == blocks[first] for v in blocks.values()), blocks
    with open(R.CFG_JSON, 'w') as fh:
        json.dump({'config': f'configs/box2mask/{first}', 'attn_cfgs': blocks[first]}, fh, indent=1)
        fh.write('\n')
    print(f'wrote {R.CFG_JSON}: {blocks[first]}')


if __name__ == '__main__':
    main()
