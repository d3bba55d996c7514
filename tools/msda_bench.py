#!/usr/bin/env python3
"""Developer measurement of multi-scale deformable attention on the GPU box at the shape Box2Mask's pixel decoder runs: B = 2, levels
32 x 32, 64 x 64, 128 x 128 (low to high resolution, as the decoder orders them), Q = S = 21504, M = 8 heads of D = 32, P = 4 points.

  kernel     boxinstseg_amd.multi_scale_deformable_attn_fused (csrc/msda.hip): reference points, raw offsets, raw logits in, one launch
             forward, three backward
  composed   mmcv's documented torch fallback on the same box with the same inputs: the offset normaliser and the softmax as torch ops,
             F.grid_sample per level, the weighted sum; autograd backward

  forward, forward_backward   one call; wall clock between two device synchronisations over the alternated repetitions after warm-up
                              (ms, p25, p75, min, max); event_ms: the kernel path between two device events
  six_layers                  six MultiScaleDeformableAttention modules in sequence (each layer's output is the next one's query, the
                              encoder's self-attention without its FFN and norms), forward + backward, against the same modules with the
                              composed core
  launches, host_syncs        device kernels of one call (torch.profiler), synchronising calls torch reports
  backward_alone              the kernel path's backward between two device events; contributions = samples x 4 corners (an upper bound:
                              corners outside the map add nothing), int64_atomic_bytes = contributions x D x 8, and those bytes over the time
  max_*_diff_rel              how far the two paths are apart (fp32 both), relative to the largest element
There is no pass / fail ratio.  Writes one JSON object to --out (default profiles/r16_msda_bench.json) and prints it.
GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from corr_bench import count_launches, count_syncs, stats

B, SHAPES, M, D, P, LAYERS = 2, [(32, 32), (64, 64), (128, 128)], 8, 32, 4, 6
L, S = len(SHAPES), sum(h * w for h, w in SHAPES)
Q = S


def make_inputs(seed, dev):
    gen = torch.Generator().manual_seed(seed)
    pts = []
    for H, W in SHAPES:
        ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H, (torch.arange(W) + 0.5) / W, indexing='ij')
        pts.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(pts, 0)[None, :, None, :].repeat(B, 1, L, 1)
    t = dict(value=torch.randn(B, S, M, D, generator=gen), ref=ref, off=torch.randn(B, Q, M, L, P, 2, generator=gen) * 2.0,
             logits=torch.randn(B, Q, M, L * P, generator=gen), grad_out=torch.randn(B, Q, M * D, generator=gen))
    t = {k: v.to(dev) for k, v in t.items()}
    t['ss'] = torch.tensor(SHAPES, device=dev)
    t['ls'] = torch.tensor([0] + [sum(h * w for h, w in SHAPES[:i]) for i in range(1, L)], device=dev)
    t['norm'] = torch.tensor([[w, h] for h, w in SHAPES], dtype=torch.float32, device=dev)
    return t


def torch_core(value, loc, w):
    """multi_scale_deformable_attn_pytorch of mmcv, as documented."""
    value_list = value.split([h * ww for h, ww in SHAPES], dim=1)
    grids = 2 * loc - 1
    sampled = []
    for lvl, (h, ww) in enumerate(SHAPES):
        v = value_list[lvl].flatten(2).transpose(1, 2).reshape(B * M, D, h, ww)
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(v, g, mode='bilinear', padding_mode='zeros', align_corners=False))
    aw = w.transpose(1, 2).reshape(B * M, 1, Q, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, M * D, Q)
    return out.transpose(1, 2).contiguous()


def composed(t, value, off, logits):
    loc = t['ref'][:, :, None, :, None, :] + off / t['norm'][None, None, None, :, None, :]
    return torch_core(value, loc, logits.softmax(-1).view(B, Q, M, L, P))


def kernel(t, value, off, logits):
    from boxinstseg_amd import multi_scale_deformable_attn_fused
    return multi_scale_deformable_attn_fused(value, t['ss'], t['ls'], t['ref'], off, logits)


def one_call(t, path, backward):
    leaves = [t[k].clone().requires_grad_(backward) for k in ('value', 'off', 'logits')]
    out = path(t, *leaves)
    if not backward:
        return (out,)
    return (out,) + torch.autograd.grad(out, leaves, t['grad_out'])


class ComposedLayer(torch.nn.Module):
    """The module's own linear layers around the composed core."""

    def __init__(self, mod, t):
        super().__init__()
        self.mod, self.t = mod, t

    def forward(self, query, reference_points):
        m = self.mod
        q = query.permute(1, 0, 2)
        value = m.value_proj(q).view(B, S, M, D)
        off = m.sampling_offsets(q).view(B, Q, M, L, P, 2)
        logits = m.attention_weights(q).view(B, Q, M, L * P)
        return m.output_proj(composed(self.t, value, off, logits)).permute(1, 0, 2) + query


def six_layers(t, layers, query, use_kernel):
    x = query.clone().requires_grad_(True)
    y = x
    for m in layers:
        y = m(y, reference_points=t['ref'], spatial_shapes=t['ss'], level_start_index=t['ls']) if use_kernel else ComposedLayer(m, t)(y, t['ref'])
    params = [p for m in layers for p in m.parameters()]
    return (y,) + torch.autograd.grad(y, [x] + params, torch.ones_like(y))


def timed(paths, reps):
    for f in paths.values():
        for _ in range(2):
            f()
    ts, ev = {k: [] for k in paths}, []
    for _ in range(reps):                                                # alternated: the paths see the same neighbours on the box
        for name, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        paths['kernel']()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    out = {}
    for name, f in paths.items():
        out[name] = stats(ts[name])
        out[name]['host_syncs'] = count_syncs(f)
        out[name]['launches'] = count_launches(f)
    out['kernel']['event_ms'] = stats(ev)
    return out


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_msda_bench.json'))
    ap.add_argument('--reps', type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('msda_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    t = make_inputs(1600, dev)
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps, 'shape': dict(B=B, levels=SHAPES, Q=Q, S=S, M=M, D=D, P=P, layers=LAYERS)}
    a, b = one_call(t, kernel, True), one_call(t, composed, True)
    for name, x, y in zip(('out', 'grad_value', 'grad_offsets', 'grad_logits'), a, b):
        out[f'max_{name}_diff_rel'] = rel(x, y)
    again = one_call(t, kernel, True)
    out['backward_bit_identical_twice'] = all(torch.equal(x, y) for x, y in zip(a, again))
    out['forward'] = timed({'kernel': lambda: one_call(t, kernel, False), 'composed': lambda: one_call(t, composed, False)}, args.reps)
    out['forward_backward'] = timed({'kernel': lambda: one_call(t, kernel, True), 'composed': lambda: one_call(t, composed, True)}, args.reps)
    bw = []
    for r in range(args.reps + 2):
        leaves = [t[k].clone().requires_grad_(True) for k in ('value', 'off', 'logits')]
        y = kernel(t, *leaves)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        torch.autograd.grad(y, leaves, t['grad_out'])
        e1.record()
        e1.synchronize()
        if r >= 2:
            bw.append(e0.elapsed_time(e1))
    contributions = B * Q * M * L * P * 4
    out['backward_alone'] = dict(stats(bw), contributions_upper_bound=contributions, int64_atomic_bytes=contributions * D * 8)
    out['backward_alone']['atomic_bytes_per_second'] = round(contributions * D * 8 / (out['backward_alone']['ms'] * 1e-3), 1)
    torch.manual_seed(1601)
    layers = [bx.MultiScaleDeformableAttention(embed_dims=M * D, num_heads=M, num_levels=L, num_points=P, dropout=0.0).to(dev) for _ in range(LAYERS)]
    for m in layers:                                                     # off mmcv's all-zero start: every query would sample the same pattern
        with torch.no_grad():
            m.sampling_offsets.weight.normal_(0, 0.02)
            m.attention_weights.weight.normal_(0, 0.02)
    query = torch.randn(Q, B, M * D, device=dev)
    ka, kb = six_layers(t, layers, query, True), six_layers(t, layers, query, False)
    out['six_layers_max_out_diff_rel'] = rel(ka[0], kb[0])
    out['six_layers'] = timed({'kernel': lambda: six_layers(t, layers, query, True), 'composed': lambda: six_layers(t, layers, query, False)},
                              max(args.reps // 2, 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
