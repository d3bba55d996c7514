"""Writes tests/golden/msda.npz, msda_decoder.npz, msda_decoder_inputs.npz, msda_cases.json and (with the upstream checkout present) msda_cfg.json.

    python tests/golden/make_golden_msda.py [path of the upstream checkout]

Inputs are drawn in fp32; the expected results are msda_scalar (tests/msda_ref.py) in fp64 on those fp32 values.  The tolerances are
FACTOR x the largest difference, over all cases, between msda_scalar in fp32 and in fp64, relative to the largest fp64 magnitude of
the quantity in the case -- measured here, once per quantity, stored in the fixture.  Asserted here: no sample of a gradient case lies
within MARGIN of an integer pixel coordinate (the planted boundary samples of `edges` are listed and held to hand rules instead); the two
restatements agree within 1e-12 in fp64 on every gradient case; and n * Mx <= 2^16 * max|grad_value| for every case, the condition
under which the fixed-point accumulation of csrc/msda.hip stays below 2^-25 max|grad_value| (n <= Q * P contributions to a cell,
Mx = max|grad_out| * max|weight|)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import msda_ref as R  # noqa: E402

FACTOR = 4
CONFIG = 'configs/box2mask/box2mask_r50_lsj_8x2_50e_coco.py'
MODULE_CFG = dict(embed_dims=64, num_heads=4, num_levels=2, num_points=2, dropout=0.0, batch_first=False)
MODULE_SHAPES = [(3, 4), (2, 2)]


def _nudge(c):
    """Pixel coordinates (fp64) moved off the integers: anything within 4 * MARGIN of one goes a quarter pixel up."""
    near = (c - c.round()).abs() < 4 * R.MARGIN
    return torch.where(near, c.round() + 0.25, c)


def _locations(gen, B, Q, M, shapes, P, lo=-0.15, hi=1.15):
    L = len(shapes)
    xy = torch.rand(B, Q, M, L, P, 2, generator=gen, dtype=torch.float64) * (hi - lo) + lo
    for lvl, (H, W) in enumerate(shapes):
        xy[:, :, :, lvl, :, 0] = (_nudge(xy[:, :, :, lvl, :, 0] * W - 0.5) + 0.5) / W
        xy[:, :, :, lvl, :, 1] = (_nudge(xy[:, :, :, lvl, :, 1] * H - 0.5) + 0.5) / H
    return xy


def _grid_reference_points(shapes, B):
    """The centre of every position of every level, the same for all levels: what the pixel decoder's encoder passes (valid ratios of 1)."""
    pts = []
    for H, W in shapes:
        ys, xs = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H, (torch.arange(W, dtype=torch.float64) + 0.5) / W, indexing='ij')
        pts.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(pts, 0)
    return ref[None, :, None, :].repeat(B, 1, len(shapes), 1)


def make_case(name, B, M, D, shapes, Q, P, seed, fused, grid_ref=False):
    gen = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)
    t = {'value': torch.randn(B, S, M, D, generator=gen), 'grad_out': torch.randn(B, Q, M * D, generator=gen)}
    loc = _locations(gen, B, Q, M, shapes, P)
    if fused:
        ref = _grid_reference_points(shapes, B) if grid_ref else torch.rand(B, Q, L, 2, generator=gen, dtype=torch.float64) * 0.9 + 0.05
        t['ref'] = ref.float()
        norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
        t['off'] = ((loc - t['ref'].double()[:, :, None, :, None, :]) * norm[None, None, None, :, None, :]).float()
        t['logits'] = torch.randn(B, Q, M, L * P, generator=gen) * 2
    else:
        t['loc'] = loc.float()
        t['w'] = torch.randn(B, Q, M, L, P, generator=gen)
    return t, dict(name=name, B=B, M=M, D=D, shapes=[list(s) for s in shapes], Q=Q, P=P, fused=fused, seed=seed, extra=[])


def make_hot_cell():
    t, spec = make_case('hot_cell', 1, 1, 32, [(4, 4)], 300, 4, 41, False)
    gen = torch.Generator().manual_seed(42)
    hw = torch.rand(1, 300, 1, 1, 4, 2, generator=gen, dtype=torch.float64) * 0.9 + 0.05            # all inside the cell h in (1, 2), w in (2, 3)
    t['loc'] = torch.stack([(2 + hw[..., 0] + 0.5) / 4, (1 + hw[..., 1] + 0.5) / 4], -1).float()
    t['w'] = (torch.rand(1, 300, 1, 1, 4, generator=gen) * 100 - 50)
    mag = 10.0 ** (torch.rand(1, 300, 32, generator=gen, dtype=torch.float64) * 9 - 6)
    t['grad_out'] = (mag * torch.where(torch.rand(1, 300, 32, generator=gen) < 0.5, -1.0, 1.0)).float()
    return t, spec


def make_edges():
    t, spec = make_case('edges', 1, 2, 16, [(4, 8), (1, 1)], 6, 4, 51, False)
    loc = t['loc']
    boundary = torch.zeros(1, 6, 2, 2, 4, dtype=torch.bool)
    zero = torch.zeros_like(boundary)
    nan = float('nan')
    #        q  l  p   x            y                        boundary  zero
    plant = [(0, 0, 0, 5.0, -3.0, True, True),                                  # far outside
             (0, 0, 1, None, 0.0, False, False),                                 # h = -0.5: the upper row out of the map
             (0, 0, 2, 1.0, None, False, False),                                 # w = 7.5: the right column out of the map
             (0, 0, 3, -0.0625, None, True, True),                               # w = -1 exactly
             (1, 0, 0, 2.5 / 8, 1.5 / 4, True, False),                           # the centre of pixel (1, 2)
             (1, 0, 1, None, -0.125, True, True),                                # h = -1 exactly
             (1, 0, 2, None, (4 - 1 / 1024 + 0.5) / 4, True, False),             # just inside H
             (1, 0, 3, nan, None, True, True),                                   # a NaN location
             (2, 1, 0, 0.5, 0.5, True, False),                                   # the centre of the 1 x 1 level
             (2, 1, 1, 1.5, None, True, True)]                                   # w = 1 = W on the 1 x 1 level: not inside
    for q, lvl, p, x, y, b, z in plant:
        if x is not None:
            loc[0, q, :, lvl, p, 0] = x
        if y is not None:
            loc[0, q, :, lvl, p, 1] = y
        boundary[0, q, :, lvl, p], zero[0, q, :, lvl, p] = b, z
    t['boundary'], t['zero'] = boundary, zero
    spec['extra'] = ['boundary', 'zero']
    spec['plant'] = [[q, lvl, p] for q, lvl, p, *_ in plant]
    return t, spec


def all_cases():
    eight = [(1 + lvl % 3, 2 + lvl % 2) for lvl in range(8)]
    cases = [make_case('plain', 2, 2, 32, [(5, 7), (3, 4)], 11, 2, 11, False),
             make_case('decoder_small', 1, 8, 32, [(2, 3), (4, 6), (8, 12)], 126, 4, 21, True, grid_ref=True),
             make_edges(), make_hot_cell()]
    seed = 60
    for D, L, P, fused in ((8, 1, 1, False), (8, 8, 8, True), (16, 8, 1, True), (16, 1, 8, False), (64, 1, 8, True), (64, 8, 1, False)):
        seed += 1
        cases.append(make_case(f'heads_d{D}_l{L}_p{P}', 1, 4, D, eight if L == 8 else [(3, 4)], 5, P, seed, fused))
    return cases


def _rel(a, b, mask=None):
    d, m = (a.double() - b).abs(), b.abs()
    if mask is not None:
        d, m = d[mask], m[mask]
    return float(d.max() / m.max()) if d.numel() else 0.0


def module_case():
    """A small module with every parameter perturbed (mmcv's init leaves the offset and attention weights at zero), a padding mask and
    a query_pos; the first seed whose samples keep off the grid."""
    B, Q, C = 2, sum(h * w for h, w in MODULE_SHAPES), MODULE_CFG['embed_dims']
    for seed in range(100, 400):
        torch.manual_seed(seed)
        mod = R.RefMSDA(**MODULE_CFG)
        with torch.no_grad():
            for prm in mod.parameters():
                prm.add_(torch.randn_like(prm) * 0.3)
        t = dict(query=torch.randn(Q, B, C), query_pos=torch.randn(Q, B, C) * 0.1, ref=torch.rand(B, Q, 2, 2) * 0.9 + 0.05,
                 ref4=torch.cat([torch.rand(B, Q, 2, 2) * 0.6 + 0.2, torch.rand(B, Q, 2, 2) * 0.5 + 0.1], -1), mask=torch.rand(B, Q) < 0.15)
        m64 = R.RefMSDA(**MODULE_CFG).double()
        m64.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
        ok = True
        for ref in (t['ref'], t['ref4']):
            q = (t['query'] + t['query_pos']).double().permute(1, 0, 2)
            off = m64.sampling_offsets(q).view(B, Q, 4, 2, 2, 2)
            if ref.shape[-1] == 2:
                loc = R.fused_to_plain(MODULE_SHAPES, ref.double(), off, torch.zeros(B, Q, 4, 4, dtype=torch.float64))[0]
            else:
                loc = ref.double()[:, :, None, :, None, :2] + off / 2 * ref.double()[:, :, None, :, None, 2:] * 0.5
            h, w = R.sample_hw(MODULE_SHAPES, loc.detach())
            ok = ok and not bool((((h - h.round()).abs() < R.MARGIN) | ((w - w.round()).abs() < R.MARGIN)).any())
        if ok:
            return seed, mod, m64, t
    raise AssertionError('no seed keeps the module case off the grid')


def run_module(mod, t, key, dtype):
    kw = dict(query_pos=t['query_pos'].to(dtype), key_padding_mask=t['mask'], reference_points=t[key].to(dtype),
              spatial_shapes=torch.tensor(MODULE_SHAPES), level_start_index=torch.tensor(R.level_starts(MODULE_SHAPES)))
    q = t['query'].to(dtype).requires_grad_(True)
    out = mod(q, **kw)
    g = torch.sin(torch.arange(out.numel(), dtype=dtype)).view(out.shape)
    names = [n for n, _ in mod.named_parameters()]
    grads = torch.autograd.grad((out * g).sum(), [q] + [p for _, p in mod.named_parameters()])
    return out.detach(), dict(zip(['query'] + names, grads))


def main(reference=None):
    arrays, decoder, decoder_in, specs = {}, {}, {}, {}
    tols = {q: 0.0 for q in R.QUANTITIES}
    for t, spec in all_cases():
        name, skip = spec['name'], t.get('boundary')
        assert R.off_grid(t, spec, skip), name
        t64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in t.items()}
        want, got32 = R.run_case(t64, spec), R.run_case(t, spec)
        if skip is None:
            other = R.run_case(t64, spec, core=R.msda_grid_sample)
            for k in want:
                assert _rel(other[k], want[k]) < 1e-12, (name, k, _rel(other[k], want[k]))
        for k in want:
            mask = ~skip[..., None].expand_as(want[k]) if (k == 'grad_loc' and skip is not None) else None
            tols[k] = max(tols[k], _rel(got32[k], want[k], mask))
        w_max = 1.0 if spec['fused'] else float(t64['w'].abs().max())
        ratio = spec['Q'] * spec['P'] * float(t64['grad_out'].abs().max()) * w_max / float(want['grad_value'].abs().max())
        assert ratio <= 2 ** 16, (name, ratio)
        spec['fixed_point_ratio'] = ratio
        if 'zero' in t:
            assert float(want['grad_loc'][t['zero']].abs().max()) == 0.0 and float(want['grad_attn'][t['zero']].abs().max()) == 0.0
        for k, v in t.items():
            (decoder_in if name == 'decoder_small' else arrays)[f'{name}_{k}'] = v.numpy()
        for k, v in want.items():
            (decoder if name == 'decoder_small' else arrays)[f'{name}_want_{k}'] = v.numpy()
        specs[name] = spec
    seed, mod, m64, t = module_case()
    for k, v in mod.state_dict().items():
        arrays[f'module_param_{k}'] = v.numpy()
    for k, v in t.items():
        arrays[f'module_{k}'] = v.numpy()
    for key in ('ref', 'ref4'):
        out64, g64 = run_module(m64, t, key, torch.float64)
        out32, g32 = run_module(mod, t, key, torch.float32)
        tols['module_out'] = max(tols['module_out'], _rel(out32, out64))
        arrays[f'module_want_out_{key}'] = out64.numpy()
        for k in g64:
            tols['module_param_grad'] = max(tols['module_param_grad'], _rel(g32[k], g64[k]))
            arrays[f'module_want_grad_{key}_{k}'] = g64[k].numpy()
    for q, v in tols.items():
        assert 0 < v < 1e-4, (q, v)
        arrays[f'tol_{q}'] = np.float64(FACTOR * v)
    np.savez_compressed(R.GOLDEN, **arrays)
    np.savez_compressed(R.GOLDEN_DECODER, **decoder)
    np.savez_compressed(R.GOLDEN_DECODER_IN, **decoder_in)
    with open(R.CASES, 'w') as fh:
        json.dump(dict(factor=FACTOR, margin=R.MARGIN, cases=specs, module=dict(cfg=MODULE_CFG, shapes=[list(s) for s in MODULE_SHAPES], seed=seed)),
                  fh, indent=1)
    if reference and os.path.exists(os.path.join(reference, CONFIG)):
        from boxinstseg_amd import load_config
        layer = load_config(os.path.join(reference, CONFIG))['model']['panoptic_head']['pixel_decoder']['encoder']['transformerlayers']
        with open(R.CFG_JSON, 'w') as fh:
            json.dump(dict(config=CONFIG, attn_cfgs=layer['attn_cfgs']), fh, indent=1)
    for p in (R.GOLDEN, R.GOLDEN_DECODER, R.GOLDEN_DECODER_IN):
        print(p, os.path.getsize(p), 'bytes')
    print({q: FACTOR * v for q, v in tols.items()})


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('BOXINST_REFERENCE_ROOT'))
