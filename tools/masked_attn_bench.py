#!/usr/bin/env python3
"""Developer measurement of Box2Mask's masked cross-attention on the GPU box, at the configs' shape: B = 2, Q = 100, M = 8, D = 32,
S in {32^2, 64^2, 128^2} (the three memory levels at the 1024^2 LSJ input), mask_pred [2, 100, 256, 256].

  mask        box2mask_attn_mask (one launch, bits [B, Q, S / 32]) against the reference's statements as torch ops: interpolate, repeat over
              the heads, sigmoid, compare, the ``where`` repair (tests/masked_attn_ref.py: box2mask_mask)
  forward     boxinstseg_amd.MultiheadAttention against torch.nn.MultiheadAttention (need_weights at its default, the bool mask
              [B * M, Q, S]) on the same projected inputs, under no_grad
  train       the same, forward + backward of ``(out * g).sum()`` with gradients to the inputs and the parameters
  nine_layers the nine decoder layers' cross-attention in the reference's level order (i % 3): mask, then attention, forward + backward;
              the mask of a layer comes from the same mask_pred (the einsum that makes it is out of scope)
  --trace-only  ten forward + backward C-ABI calls at S = 128^2, for a rocprofv3 --kernel-trace --stats run of their own
  core        one C-ABI call of the forward, and of forward + backward, between device events in a back-to-back window: the share of the
              achievable HBM rate for the bytes that must move (forward: K, V, q, out, bits; train: those twice plus dout, dq, dk, dv)

Both paths warmed, then timed interleaved in one process between device events (median, p25, p75 over the samples); launches: kernels in
torch's profiler trace of one call; host_syncs: the synchronising calls torch's sync debug mode reports; peak_bytes: the allocator's peak
above what was allocated before the call.  There is no pass / fail ratio.  Writes one JSON object to --out (default
profiles/r20_masked_attn_bench.json) and prints it.  GPU only; reads nothing but this repository."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
from torch import nn

import __graft_entry__ as entry
from corr_bench import count_launches, count_syncs
from seg_paste_bench import peak_bytes, timed
from tests import masked_attn_ref as R

B, Q, M, D, SIZES, PRED = 2, 100, 8, 32, [(32, 32), (64, 64), (128, 128)], (256, 256)
E = M * D
HBM_ACHIEVABLE = 6.29e12            # bytes / s, a float4 copy on this part (8.0e12 is the data sheet's figure)


def event_us(fn, reps=100):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    v = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        v.append(e0.elapsed_time(e1) * 1e3 / reps)
    return round(float(np.median(v)), 2)


def counted(paths, row):
    for k, f in paths.items():
        row[k]['launches'], row[k]['host_syncs'], row[k]['peak_bytes'] = count_launches(f), count_syncs(f), peak_bytes(f)
    spread = (row['hip']['ms_p75'] - row['hip']['ms_p25']) + (row['torch']['ms_p75'] - row['torch']['ms_p25'])
    row['torch_minus_hip_ms'] = round(row['torch']['ms'] - row['hip']['ms'], 4)
    row['sum_of_p25_p75_spreads_ms'] = round(spread, 4)
    row['hip_is_slower'] = bool(row['hip']['ms'] > row['torch']['ms'])
    return row


def rel(x, y):
    return float((x - y).abs().max() / y.abs().max())


def core_calls(q, k, v, g, mask, trace_only=False):
    """One forward call and one forward + backward pair of the C ABI on preallocated tensors: nothing but the library's launches is timed."""
    from boxinstseg_amd import _lib
    from boxinstseg_amd._common import current_stream
    lib, dev = _lib.load(), q.device
    S = int(k.shape[0])
    out, lse = torch.empty_like(q), torch.empty((B, M, Q), device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    fb, bb = lib.bxi_masked_attn_forward_workspace_bytes(B, M, Q, S, D), lib.bxi_masked_attn_backward_workspace_bytes(B, M, Q, S, D)
    ws = torch.empty(max(fb, bb), dtype=torch.uint8, device=dev)
    st, scale = current_stream(dev), (1.0 / D) ** 0.5
    fwd = lambda: _lib.check('fwd', lib.bxi_masked_attn_forward_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.bits.data_ptr(), 0, B, M, Q, S, D,  # noqa: E731
                                                                    scale, out.data_ptr(), lse.data_ptr(), ws.data_ptr(), fb, st))
    bwd = lambda: _lib.check('bwd', lib.bxi_masked_attn_backward_f32(g.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.bits.data_ptr(), 0,  # noqa: E731
                                                                     out.data_ptr(), lse.data_ptr(), B, M, Q, S, D, scale, dq.data_ptr(), dk.data_ptr(),
                                                                     dv.data_ptr(), ws.data_ptr(), bb, st))

    def both():
        fwd()
        bwd()
    kv, qo, bits = 2 * 4 * S * B * E, 2 * 4 * Q * B * E, 4 * mask.bits.numel()
    need_f, need_t = kv + qo + bits, 2 * (kv + qo + bits) + 4 * Q * B * E + 2 * 4 * S * B * E + 4 * Q * B * E
    if trace_only:
        for _ in range(10):
            both()
        torch.cuda.synchronize()
        return None
    f_us, t_us = event_us(fwd), event_us(both)
    return dict(forward=dict(event_us=f_us, needed_bytes=need_f, share_of_achievable_hbm=round(need_f / HBM_ACHIEVABLE / (f_us * 1e-6), 4),
                             workspace_bytes=fb),
                train=dict(event_us=t_us, needed_bytes=need_t, share_of_achievable_hbm=round(need_t / HBM_ACHIEVABLE / (t_us * 1e-6), 4),
                           workspace_bytes=bb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20_masked_attn_bench.json'))
    ap.add_argument('--trace-only', action='store_true', help='ten forward + backward C-ABI calls at S = 128^2 and nothing else (for rocprofv3 --kernel-trace --stats)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('masked_attn_bench needs a GPU: nothing is measured on the CPU')
    entry.build()
    import boxinstseg_amd as bx
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(20)
    pred = (3.0 * torch.randn(B, Q, *PRED, generator=gen)).to(dev)
    mine = bx.MultiheadAttention(E, M, dropout_layer=None).to(dev)
    ref = nn.MultiheadAttention(E, M).to(dev)
    ref.load_state_dict({k[len('attn.'):]: v for k, v in mine.state_dict().items()})
    query, qpos, g = (torch.randn(Q, B, E, generator=gen).to(dev) for _ in range(3))
    mem = [torch.randn(h * w, B, E, generator=gen).to(dev) for h, w in SIZES]
    mpos = [torch.randn(h * w, B, E, generator=gen).to(dev) for h, w in SIZES]
    params = list(mine.parameters()) + list(ref.parameters())

    def hip_layer(l, mask=None):
        mask = bx.box2mask_attn_mask(pred, SIZES[l]) if mask is None else mask
        return mine(query, mem[l], mem[l], query_pos=qpos, key_pos=mpos[l], attn_mask=mask)

    def torch_layer(l, mask=None):
        mask = R.box2mask_mask(pred, SIZES[l], M) if mask is None else mask
        return query + ref(query + qpos, mem[l] + mpos[l], mem[l], attn_mask=mask)[0]

    def train(layer, *a):
        for p in params:
            p.grad = None
        (layer(*a) * g).sum().backward()

    out = {'gpu': torch.cuda.get_device_name(0), 'shape': dict(B=B, Q=Q, M=M, D=D, S=[h * w for h, w in SIZES], mask_pred=[B, Q, *PRED]),
           'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'levels': {}}
    if args.trace_only:
        with torch.no_grad():
            w_, b_ = mine.attn.in_proj_weight, mine.attn.in_proj_bias
            core_calls(nn.functional.linear(query + qpos, w_[:E], b_[:E]), nn.functional.linear(mem[2] + mpos[2], w_[E:2 * E], b_[E:2 * E]),
                       nn.functional.linear(mem[2], w_[2 * E:], b_[2 * E:]), g, bx.box2mask_attn_mask(pred, SIZES[2]), trace_only=True)
        return
    for l, (h, w) in enumerate(SIZES):
        S = h * w
        hm, tm = bx.box2mask_attn_mask(pred, (h, w)), R.box2mask_mask(pred, (h, w), M)
        differ = int((R.unpack_bits(hm.bits.cpu(), S) != tm.view(B, M, Q, S)[:, 0].cpu()).sum())
        with torch.no_grad():
            agree = rel(hip_layer(l, hm), torch_layer(l, tm))
        row = {'mask_bits_that_differ_from_the_torch_mask': differ, 'of_bits': B * Q * S, 'max_relative_difference_hip_vs_torch_forward': agree}
        paths = {'hip': lambda: bx.box2mask_attn_mask(pred, (h, w)), 'torch': lambda: R.box2mask_mask(pred, (h, w), M)}
        row['mask'] = counted(paths, timed(paths))

        def no_grad(f, *a):
            with torch.no_grad():
                return f(*a)
        paths = {'hip': lambda: no_grad(hip_layer, l, hm), 'torch': lambda: no_grad(torch_layer, l, tm)}
        row['forward'] = counted(paths, timed(paths))
        paths = {'hip': lambda: train(hip_layer, l, hm), 'torch': lambda: train(torch_layer, l, tm)}
        row['train'] = counted(paths, timed(paths))
        with torch.no_grad():
            w_, b_ = mine.attn.in_proj_weight, mine.attn.in_proj_bias
            q = nn.functional.linear(query + qpos, w_[:E], b_[:E])
            k = nn.functional.linear(mem[l] + mpos[l], w_[E:2 * E], b_[E:2 * E])
            v = nn.functional.linear(mem[l], w_[2 * E:], b_[2 * E:])
        row['core'] = core_calls(q, k, v, g, hm)
        out['levels'][f'S_{S}'] = row

    def nine(layer):
        for p in params:
            p.grad = None
        total = 0
        for i in range(9):
            total = total + (layer(i % 3) * g).sum()
        total.backward()
    paths = {'hip': lambda: nine(hip_layer), 'torch': lambda: nine(torch_layer)}
    out['nine_layers'] = counted(paths, timed(paths, window_s=0.7, samples=9))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
