"""Plain torch on the CPU: multi-scale deformable attention restated twice, and the module around it.  fp64-capable, autograd for all gradients.

mmcv's op never ran next to this library: its arithmetic is restated from its documented algorithm and is unpinned.

    msda_grid_sample   mmcv's torch fallback (multi_scale_deformable_attn_pytorch): F.grid_sample per level, then the weighted sum
    msda_scalar        the kernel's documented algorithm, independent of grid_sample: sample by sample (l, p), h = y H - 0.5, the strict
                       validity rule, floor, the four corners written out, a corner outside the map contributing nothing.  A sample that does
                       not count (outside, on h = -1 / w = -1, NaN, inf) gives zero AND takes a zero gradient.  Every sample (l, p) is
                       one step of the loop, taken for all (b, q, m) at once.
    fused_to_plain     reference points, raw offsets, raw logits -> locations (ref + off / (W, H)) and softmax weights
    RefMSDA            the module restated: the same four linear layers, offset normaliser, softmax, box form, residual
    dyadic_case        inputs that are small dyadic rationals: every intermediate of the forward and of the gradients is exact in fp32, so
                       msda_scalar gives the same bits in fp32 and in fp64 and the kernel has to give them too (no fixture file: seeded)
    cell_hits          how many corners of valid samples land on every cell of value: the count of the fixed-point quantisation bound

The fixture (tests/golden/msda.npz, msda_decoder.npz, msda_decoder_inputs.npz, msda_cases.json; make_golden_msda.py) holds the inputs of every case, the fp64
results of msda_scalar and the tolerances: 4 x the fp32-against-fp64 difference of msda_scalar itself."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = os.path.join(GOLDEN_DIR, 'msda.npz')
GOLDEN_DECODER = os.path.join(GOLDEN_DIR, 'msda_decoder.npz')      # the results of decoder_small and
GOLDEN_DECODER_IN = os.path.join(GOLDEN_DIR, 'msda_decoder_inputs.npz')      # its inputs: files of their own, each under the size limit
CASES = os.path.join(GOLDEN_DIR, 'msda_cases.json')
CFG_JSON = os.path.join(GOLDEN_DIR, 'msda_cfg.json')
MARGIN = 1e-3              # no sample of a gradient case has h or w this close to an integer (-1 and H / W are integers)
QUANTITIES = ('out', 'grad_value', 'grad_loc', 'grad_attn', 'grad_offsets', 'grad_logits', 'module_out', 'module_param_grad')


def level_starts(shapes):
    starts, at = [], 0
    for h, w in shapes:
        starts.append(at)
        at += h * w
    return starts


def msda_grid_sample(value, shapes, loc, w):
    """value [B,S,M,D], shapes [(H, W)], loc [B,Q,M,L,P,2], w [B,Q,M,L,P] -> [B,Q,M*D]."""
    B, _, M, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    value_list = value.split([h * ww for h, ww in shapes], dim=1)
    grids = 2 * loc - 1
    sampled = []
    for lvl, (h, ww) in enumerate(shapes):
        v = value_list[lvl].flatten(2).transpose(1, 2).reshape(B * M, D, h, ww)
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(v, g, mode='bilinear', padding_mode='zeros', align_corners=False))
    aw = w.transpose(1, 2).reshape(B * M, 1, Q, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, M * D, Q)
    return out.transpose(1, 2).contiguous()


def sample_hw(shapes, loc):
    """The pixel coordinates (h, w) [B,Q,M,L,P] of every sample."""
    H = torch.tensor([s[0] for s in shapes], dtype=loc.dtype).view(1, 1, 1, -1, 1)
    W = torch.tensor([s[1] for s in shapes], dtype=loc.dtype).view(1, 1, 1, -1, 1)
    return loc[..., 1] * H - 0.5, loc[..., 0] * W - 0.5


def msda_scalar(value, shapes, loc, w):
    B, _, M, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    starts = level_starts(shapes)
    bi = torch.arange(B).view(B, 1, 1).expand(B, Q, M)
    mi = torch.arange(M).view(1, 1, M).expand(B, Q, M)
    out = torch.zeros(B, Q, M, D, dtype=value.dtype)
    for lvl, (H, W) in enumerate(shapes):
        for p in range(P):
            xy = loc[:, :, :, lvl, p]
            with torch.no_grad():
                h0, w0 = xy[..., 1] * H - 0.5, xy[..., 0] * W - 0.5
                valid = (h0 > -1) & (w0 > -1) & (h0 < H) & (w0 < W)            # strict; NaN fails
            xy = torch.where(valid[..., None], xy, torch.full_like(xy, 0.5))   # a sample that does not count takes no gradient
            h, ww = xy[..., 1] * H - 0.5, xy[..., 0] * W - 0.5
            hl, wl = h.detach().floor(), ww.detach().floor()
            lh, lw = h - hl, ww - wl
            hh, hw = 1 - lh, 1 - lw
            hl, wl = hl.long(), wl.long()
            val = torch.zeros(B, Q, M, D, dtype=value.dtype)
            for dy, dx, wt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
                y, x = hl + dy, wl + dx
                inside = valid & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
                cell = starts[lvl] + y.clamp(0, H - 1) * W + x.clamp(0, W - 1)
                val = val + torch.where(inside, wt, torch.zeros_like(wt))[..., None] * value[bi, cell, mi]
            out = out + w[:, :, :, lvl, p, None] * val
    return out.reshape(B, Q, M * D)


def fused_to_plain(shapes, ref, off, logits):
    """ref [B,Q,L,2], off [B,Q,M,L,P,2], logits [B,Q,M,L*P] -> loc [B,Q,M,L,P,2], weights [B,Q,M,L,P]."""
    B, Q, M, L, P, _ = off.shape
    norm = torch.tensor([[s[1], s[0]] for s in shapes], dtype=off.dtype)           # (W, H)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return loc, logits.softmax(-1).view(B, Q, M, L, P)


class RefMSDA(nn.Module):
    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False, norm_cfg=None,
                 init_cfg=None, core=msda_scalar):
        super().__init__()
        self.embed_dims, self.num_heads, self.num_levels, self.num_points, self.batch_first, self.core = embed_dims, num_heads, num_levels, num_points, batch_first, core
        self.dropout = nn.Dropout(dropout)
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.init_weights()

    def init_weights(self):
        M, L, P = self.num_heads, self.num_levels, self.num_points
        with torch.no_grad():
            self.sampling_offsets.weight.fill_(0.)
            bias = torch.zeros(M, L, P, 2)
            for m in range(M):
                theta = torch.tensor(m, dtype=torch.float32) * (2.0 * math.pi / M)
                c, s = theta.cos(), theta.sin()
                top = torch.maximum(c.abs(), s.abs())
                for p in range(P):
                    bias[m, :, p, 0] = c / top * (p + 1)
                    bias[m, :, p, 1] = s / top * (p + 1)
            self.sampling_offsets.bias.copy_(bias.view(-1))
            self.attention_weights.weight.fill_(0.)
            self.attention_weights.bias.fill_(0.)
            for proj in (self.value_proj, self.output_proj):
                bound = math.sqrt(6.0 / (proj.in_features + proj.out_features))            # xavier, uniform, gain 1
                proj.weight.uniform_(-bound, bound)
                proj.bias.fill_(0.)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None, reference_points=None, spatial_shapes=None,
                level_start_index=None, **kwargs):
        value = query if value is None else value
        identity = query if identity is None else identity
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        B, Q, _ = query.shape
        S = value.shape[1]
        shapes = [(int(h), int(w)) for h, w in torch.as_tensor(spatial_shapes).tolist()]
        assert sum(h * w for h, w in shapes) == S
        M, L, P = self.num_heads, self.num_levels, self.num_points
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        value = value.view(B, S, M, -1)
        off = self.sampling_offsets(query).view(B, Q, M, L, P, 2)
        logits = self.attention_weights(query).view(B, Q, M, L * P)
        if reference_points.shape[-1] == 2:
            loc, w = fused_to_plain(shapes, reference_points, off, logits)
        else:
            w = logits.softmax(-1).view(B, Q, M, L, P)
            loc = reference_points[:, :, None, :, None, :2] + off / P * reference_points[:, :, None, :, None, 2:] * 0.5
        out = self.output_proj(self.core(value, shapes, loc, w))
        if not self.batch_first:
            out = out.permute(1, 0, 2)
        return self.dropout(out) + identity


# ---- the fixture --------------------------------------------------------------------------------------------------------------
def load_cases():
    with open(CASES) as fh:
        return json.load(fh)


_CACHE = {}


def golden():
    """Both files as one dict of arrays, read once."""
    if 'g' not in _CACHE:
        g = dict(np.load(GOLDEN))
        g.update(np.load(GOLDEN_DECODER))
        g.update(np.load(GOLDEN_DECODER_IN))
        _CACHE['g'] = g
    return _CACHE['g']


def case_tensors(name, dtype=torch.float32):
    """The inputs of one case as CPU tensors (floats as `dtype`) and its spec."""
    spec, g = load_cases()['cases'][name], golden()
    keys = ('value', 'grad_out', 'ref', 'off', 'logits') if spec['fused'] else ('value', 'grad_out', 'loc', 'w')
    t = {k: torch.from_numpy(g[f'{name}_{k}']).to(dtype) for k in keys}
    for k in spec.get('extra', []):
        t[k] = torch.from_numpy(g[f'{name}_{k}'])
    return t, spec


def expected(name):
    spec, g = load_cases()['cases'][name], golden()
    keys = ('out', 'grad_value', 'grad_offsets', 'grad_logits') if spec['fused'] else ('out', 'grad_value', 'grad_loc', 'grad_attn')
    return {k: torch.from_numpy(g[f'{name}_want_{k}']) for k in keys}


def tol(quantity):
    return float(golden()[f'tol_{quantity}'])


def run_case(t, spec, core=msda_scalar):
    """The case in the dtype of its tensors: out and the gradients of (out * grad_out).sum() w.r.t. every input that takes one."""
    shapes = [tuple(s) for s in spec['shapes']]
    value = t['value'].clone().requires_grad_(True)
    if spec['fused']:
        leaves = {'grad_offsets': t['off'].clone().requires_grad_(True), 'grad_logits': t['logits'].clone().requires_grad_(True)}
        loc, w = fused_to_plain(shapes, t['ref'], leaves['grad_offsets'], leaves['grad_logits'])
    else:
        leaves = {'grad_loc': t['loc'].clone().requires_grad_(True), 'grad_attn': t['w'].clone().requires_grad_(True)}
        loc, w = leaves['grad_loc'], leaves['grad_attn']
    out = core(value, shapes, loc, w)
    names = ['grad_value'] + list(leaves)
    grads = torch.autograd.grad((out * t['grad_out']).sum(), [value] + list(leaves.values()))
    res = {'out': out.detach()}
    res.update({n: gr for n, gr in zip(names, grads)})
    return res


def case_hw(t, spec):
    """fp64 pixel coordinates of every sample of a case."""
    shapes = [tuple(s) for s in spec['shapes']]
    d = {k: v.double() for k, v in t.items() if v.dtype.is_floating_point}
    loc = fused_to_plain(shapes, d['ref'], d['off'], d['logits'])[0] if spec['fused'] else d['loc']
    return sample_hw(shapes, loc)


def off_grid(t, spec, skip=None):
    """The condition on the inputs of a gradient case: no h or w within MARGIN of an integer (samples under `skip` excepted)."""
    h, w = case_hw(t, spec)
    bad = ((h - h.round()).abs() < MARGIN) | ((w - w.round()).abs() < MARGIN)
    bad = bad & torch.isfinite(h) & torch.isfinite(w)
    if skip is not None:
        bad = bad & ~skip
    return not bool(bad.any())


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def dyadic_case(seed, B, Q, M, D, shapes, P, fused, gmax=8, scale_b1=0):
    """Inputs on which fp32 arithmetic is exact (every level side a power of two), as fp32 CPU tensors, and the spec run_case takes.

    value and grad_out are integers in [-8, 8] and [-gmax, gmax], one grad_out of batch 0 planted at gmax: max|grad_out| = gmax.
    plain: locations are multiples of 1/32 in [-6/32, 38/32] (inside, outside, on pixel centres, on h = -1), weights multiples of 1/16 in
           [-1, 1] with one planted 1: Mx = gmax, a power of two for gmax = 8 and not for gmax = 7.
    fused: reference points multiples of 1/8 in [0, 1], offsets multiples of 1/8 in [-2, 2], logits 0 at exactly four of the L * P
           positions of every (b, q, m) and -inf elsewhere: the softmax is 1/4 four times and 0 elsewhere, exactly.
    scale_b1 = k multiplies grad_out[1] by 2^-k (exact): a batch item whose gradients are small against Mx."""
    assert all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes)
    assert not fused or len(shapes) * P >= 4
    gen = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)

    def ints(lo, hi, *size):
        return torch.randint(lo, hi + 1, size, generator=gen).float()

    t = {'value': ints(-8, 8, B, S, M, D), 'grad_out': ints(-gmax, gmax, B, Q, M * D)}
    t['grad_out'][0, 0, 0] = gmax
    if fused:
        t['ref'] = ints(0, 8, B, Q, L, 2) / 8
        t['off'] = ints(-16, 16, B, Q, M, L, P, 2) / 8
        logits = torch.full((B * Q * M, L * P), float('-inf'))
        for row in logits:
            row[torch.randperm(L * P, generator=gen)[:4]] = 0.0
        t['logits'] = logits.view(B, Q, M, L * P)
    else:
        t['loc'] = ints(-6, 38, B, Q, M, L, P, 2) / 32
        t['w'] = ints(-16, 16, B, Q, M, L, P) / 16
        t['w'][0, 0, 0, 0, 0] = 1.0
    if scale_b1:
        t['grad_out'][1] = torch.ldexp(t['grad_out'][1], torch.tensor(-scale_b1))
    return t, dict(B=B, Q=Q, M=M, D=D, P=P, shapes=[list(s) for s in shapes], fused=fused)


def fixed_point_mx(t, spec):
    """Mx of include/boxinst/boxinst_hip_msda.h in fp64: max|grad_out| * max|weight|, the weight maximum 1 in the fused form."""
    mx = float(t['grad_out'].double().abs().max())
    return mx if spec['fused'] else mx * float(t['w'].double().abs().max())


def cell_hits(shapes, loc, B, S, M):
    """n [B,S,M] int64: over all samples of loc [B,Q,M,L,P,2] that count (h > -1, w > -1, h < H, w < W, strict; a NaN fails), the corners
    that land inside the map, per cell.  An upper bound on the contributions a cell of grad_value receives: a corner of weight 0 adds
    nothing to the sum and no error."""
    n = torch.zeros(B, S, M, dtype=torch.int64)
    bi = torch.arange(B).view(B, 1, 1, 1).expand(loc.shape[:3] + loc.shape[4:5])
    mi = torch.arange(M).view(1, 1, M, 1).expand_as(bi)
    for lvl, ((H, W), start) in enumerate(zip(shapes, level_starts(shapes))):
        h, w = loc[:, :, :, lvl, :, 1] * H - 0.5, loc[:, :, :, lvl, :, 0] * W - 0.5
        valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        h0 = torch.where(valid, h, torch.zeros_like(h)).floor().long()
        w0 = torch.where(valid, w, torch.zeros_like(w)).floor().long()
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = h0 + dy, w0 + dx
                inside = valid & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
                cell = start + y.clamp(0, H - 1) * W + x.clamp(0, W - 1)
                n.index_put_((bi[inside], cell[inside], mi[inside]), torch.ones((), dtype=torch.int64), accumulate=True)
    return n


# the dyadic cases of tests/test_gpu_msda_fixed_point.py: name -> the arguments of dyadic_case without gmax / scale_b1
DYADIC = {
    'plain_d8_tail': dict(seed=1, B=2, Q=7, M=3, D=8, shapes=[(4, 8), (2, 2)], P=8, fused=False),      # L * P = 16 > D; 42 items: a tail group
    'plain_d64': dict(seed=3, B=1, Q=9, M=1, D=64, shapes=[(2, 4)], P=2, fused=False),
    'fused_d16': dict(seed=2, B=2, Q=5, M=3, D=16, shapes=[(4, 4), (8, 2)], P=4, fused=True),
    'fused_d32': dict(seed=4, B=2, Q=3, M=5, D=32, shapes=[(8, 8), (4, 4), (2, 2), (1, 1)], P=2, fused=True),
}
# (case, gmax, scale_b1): Mx a power of two, every result exact; Mx = 7 and a batch item 2^-32 below the rest, the quantisation bound
DYADIC_EXACT = [(n, 8, 0) for n in DYADIC]
DYADIC_BOUND = [(n, 7, 0) for n in DYADIC] + [('plain_d8_tail', 7, 32), ('plain_d8_tail', 8, 32)]


def dyadic(name, gmax=8, scale_b1=0):
    return dyadic_case(gmax=gmax, scale_b1=scale_b1, **DYADIC[name])


def plain_locations(t, spec):
    """The fp64 locations [B,Q,M,L,P,2] of a case of either form."""
    shapes = [tuple(s) for s in spec['shapes']]
    return fused_to_plain(shapes, t['ref'].double(), t['off'].double(), t['logits'].double())[0] if spec['fused'] else t['loc'].double()
