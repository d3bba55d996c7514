"""Exactly representable cases for the dynamic mask head (a plain module, no fixtures; in the manner of tests/msda_ref.py).

The head is three (in general `layers`) per-instance 1x1 convolutions -- sums of products --, relative coordinates that are
`(integer - integer) / power of two`, and `aligned_bilinear`, whose weights at factors 1, 2, 4 and 8 are multiples of 1/f.  On
inputs that are small multiples of 1/2 every intermediate is a multiple of a known power of two (its QUANTUM) and small enough
to be held exactly in fp32.  Then every summation order and every FMA grouping gives the same bits as fp64, forward and
backward: a kernel with its own summation order, tiles, slots and partial sums owes the fp64 result bit for bit.

  dyadic_case(...)          seeded inputs of that kind (numpy), for the tuned 3 x 8 head and for any head shape
  expected(case)            logits, d feat, d params of the reference evaluation in fp64 (or fp32): oracle.torch_oracle for the 3 x 8
                            head, CondInstMaskHead._composed_forward for the others
  restate(case, ...)        the same arithmetic layer by layer with every intermediate kept: pre-activations, y, d y; optionally with
                            every input replaced by its absolute value and every ReLU gate open, or with the first hidden layer zeroed
                            at one pixel (what fmaxf makes of a NaN feature)
  order_free_ratio(case)    the premise: per quantity the largest sum|terms| / (quantum * 2^24); below 1 every partial sum in any
                            order is exact
  slots_for(...)            the number of workgroups per (image, tile) the backward launches (csrc/dynamic_head.hip)
  first_difference(...)     index, both values, tile and slot of the first element that differs
"""
from __future__ import annotations

import numpy as np
import torch

SOI = (64, 128, 256, 512, 1024)
IN_STRIDE = 8
TILE_FWD = {1: (14, 32), 2: (14, 32)}        # forward y tile (rows, columns); other factors 8 x 32
TILE_BWD = (8, 32)                            # backward y tile
MAX_SLOTS = 8


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def param_sizes(cin: int, layers: int, channels: int):
    """(weights, biases) of parse_dynamic_params: all weights first, layer by layer, rows = output channels; then all biases."""
    w, b = [], []
    for i in range(layers):
        ci = cin if i == 0 else channels
        co = 1 if i == layers - 1 else channels
        w.append(co * ci)
        b.append(co)
    return w, b


def dyadic_case(seed, B, C, H, W, N, factor, rel, *, layers=3, channels=8, feat_density=1.0, param_density=0.5, grad_density=0.25,
                empty_image=None):
    """Seeded inputs on which the head is exact in fp32.

    Features in {-1, -1/2, 0, 1/2, 1} (`feat_density` = share of the drawn values kept, the rest 0), parameters in {-1, -1/2, 1/2, 1}
    at `param_density` and 0 elsewhere (the first layer's weights of the two relative coordinates in {-1, 0, 1}), coors = 64 k + 4
    inside the image (so coors - location is a multiple of 8 and the relative coordinate a multiple of 8 / 1024), level indices
    over all five sizes of interest, an upstream gradient in {-1, 1} at `grad_density` and 0 elsewhere.  The instances are dealt
    unevenly over the images in a shuffled order and, with more than one image, image `empty_image` (default: seed % B) receives
    none."""
    rng = np.random.default_rng(seed)
    cin = C + (2 if rel else 0)
    wsz, bsz = param_sizes(cin, layers, channels)
    P = sum(wsz) + sum(bsz)
    feat = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), size=(B, C, H, W))
    feat = feat * (rng.random((B, C, H, W)) < feat_density)
    params = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0]), size=(N, P)) * (rng.random((N, P)) < param_density)
    if rel:                                                # the weights of the relative coordinates: whole numbers (see order_free_ratio)
        w0 = params[:, :wsz[0]].reshape(N, bsz[0], cin)
        w0[:, :, :2] = np.sign(w0[:, :, :2])
    kx = rng.integers(0, max(1, (IN_STRIDE * W + 59) // 64), size=N)
    ky = rng.integers(0, max(1, (IN_STRIDE * H + 59) // 64), size=N)
    coors = np.stack([64.0 * kx + 4.0, 64.0 * ky + 4.0], axis=1)
    lvl = rng.permutation(np.arange(N) % len(SOI))
    if B > 1:
        empty = seed % B if empty_image is None else empty_image
        live = [b for b in range(B) if b != empty]
        share = np.array([2.0 ** -i for i in range(len(live))])      # uneven: each image about half of the one before
        img = np.array(live)[np.minimum(np.searchsorted(np.cumsum(share / share.sum()), (np.arange(N) + 0.5) / max(N, 1)), len(live) - 1)]
        img = rng.permutation(img)
    else:
        img = np.zeros(N, np.int64)
    g = rng.choice(np.array([-1.0, 1.0]), size=(N, 1, factor * H, factor * W)) * (rng.random((N, 1, factor * H, factor * W)) < grad_density)
    return dict(seed=seed, B=B, C=C, H=H, W=W, N=N, factor=factor, rel=bool(rel), layers=layers, channels=channels,
                feat=(feat + 0.0).astype(np.float32), params=(params + 0.0).astype(np.float32),          # + 0.0: no -0 among the inputs
                coors=coors.astype(np.float32), lvl=lvl.astype(np.int64), img=np.asarray(img, np.int64), g=(g + 0.0).astype(np.float32))


def name_of(c) -> str:
    head = '' if (c['layers'], c['channels']) == (3, 8) else f" {c['layers']}x{c['channels']}"
    return f"B{c['B']} C{c['C']} {c['H']}x{c['W']} N{c['N']} f{c['factor']} rel{int(c['rel'])}{head} s{c['seed']}"


def spec_name(args, kw) -> str:
    """name_of(dyadic_case(*args, **kw)) without drawing the case (test ids)."""
    seed, B, C, H, W, N, factor, rel = args
    return name_of(dict(seed=seed, B=B, C=C, H=H, W=W, N=N, factor=factor, rel=rel, layers=kw.get('layers', 3), channels=kw.get('channels', 8)))


def is_tuned(c) -> bool:
    return (c['layers'], c['channels']) == (3, 8) and c['C'] in (8, 16)


# ------------------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def expected(c, dtype=torch.float64, general=None):
    """(logits, d feat, d params) of the reference evaluation in `dtype` on the CPU, as numpy arrays of that dtype."""
    feat, params = _t(c['feat'], dtype).requires_grad_(True), _t(c['params'], dtype).requires_grad_(True)
    coors, lvl, img = _t(c['coors'], dtype), torch.from_numpy(c['lvl']), torch.from_numpy(c['img'])
    if is_tuned(c) if general is None else not general:
        from oracle import torch_oracle as to
        y = to.dynamic_mask_forward(feat, params, coors, lvl, img, torch.tensor(SOI), in_stride=IN_STRIDE, out_stride=IN_STRIDE // c['factor'],
                                    disable_rel_coors=not c['rel'])
    else:
        from boxinstseg_amd import CondInstMaskHead
        head = CondInstMaskHead(in_channels=c['C'], dynamic_convs=c['layers'], dynamic_channels=c['channels'], boxinst_enabled=True,
                                disable_rel_coors=not c['rel'], in_stride=IN_STRIDE, out_stride=IN_STRIDE // c['factor']).to(dtype)
        y = head._composed_forward(feat, params, coors, lvl, img)
    y.backward(_t(c['g'], dtype))
    return y.detach().numpy(), feat.grad.numpy(), params.grad.numpy()


def restate(c, dtype=torch.float64, *, absolute=False, open_gates=False, zero_h1_at=None):
    """The head layer by layer with everything kept.  Returns a dict: 'pre' (list of pre-activations [N, co, H, W], one per hidden
    layer), 'y' [N,1,H,W], 'logits', and the gradients 'd_y', 'd_feat', 'd_params', 'd_pre' (list).  `absolute` replaces every input
    (features, relative coordinates, parameters, upstream gradient) by its absolute value; `open_gates` makes every ReLU the
    identity; `zero_h1_at` = (image, row, column): the first hidden layer of that pixel is 0 for every instance of that image."""
    from oracle import torch_oracle as to
    ab = (lambda a: a.abs()) if absolute else (lambda a: a)
    N, H, W, f = c['N'], c['H'], c['W'], c['factor']
    feat, params = ab(_t(c['feat'], dtype)).requires_grad_(True), ab(_t(c['params'], dtype)).requires_grad_(True)
    img = torch.from_numpy(c['img'])
    x = feat[img]
    if c['rel']:
        xs = torch.arange(W, dtype=dtype) * IN_STRIDE + IN_STRIDE // 2
        ys = torch.arange(H, dtype=dtype) * IN_STRIDE + IN_STRIDE // 2
        soi = torch.tensor(SOI, dtype=dtype)[torch.from_numpy(c['lvl'])].view(N, 1, 1)
        coors = _t(c['coors'], dtype)
        rx = ab((coors[:, 0].view(N, 1, 1) - xs.view(1, 1, W)) / soi).expand(N, H, W)
        ry = ab((coors[:, 1].view(N, 1, 1) - ys.view(1, H, 1)) / soi).expand(N, H, W)
        x = torch.cat([rx[:, None], ry[:, None], x], dim=1)
    cin = x.size(1)
    wsz, bsz = param_sizes(cin, c['layers'], c['channels'])
    pre, w_off, b_off = [], 0, sum(wsz)
    for i, (nw, nb) in enumerate(zip(wsz, bsz)):
        w = params[:, w_off:w_off + nw].reshape(N, nb, nw // nb)
        b = params[:, b_off:b_off + nb].reshape(N, nb, 1, 1)
        x = torch.einsum('noi,nihw->nohw', w, x) + b
        if i < c['layers'] - 1:
            x.retain_grad()
            pre.append(x)
            if not open_gates:
                x = torch.relu(x)
            if i == 0 and zero_h1_at is not None:
                keep = torch.ones(N, 1, H, W, dtype=dtype)
                keep[img == zero_h1_at[0], :, zero_h1_at[1], zero_h1_at[2]] = 0
                x = x * keep
        w_off += nw
        b_off += nb
    y = x
    y.retain_grad()
    logits = to.aligned_upsample(y, f)
    logits.backward(ab(_t(c['g'], dtype)))
    return dict(pre=[p.detach() for p in pre], y=y.detach(), logits=logits.detach(), d_y=y.grad, d_feat=feat.grad, d_params=params.grad,
                d_pre=[p.grad for p in pre])


# ------------------------------------------------------------------------------------------------------------------------------
# the premise
# ------------------------------------------------------------------------------------------------------------------------------
def order_free_ratio(c):
    """Per quantity the largest  sum|terms| / (quantum * 2^24).

    sum|terms| comes from restate(absolute=True, open_gates=True): with every input non-negative and no gate closed each value IS
    the sum of the absolute values of the terms that any evaluation order adds up for it (and bounds each product among them).
    The quantum -- the power of two every term of the reduction is a multiple of -- follows from the construction:
        features, parameters 1/2;  relative coordinates 8 / soi of the instance;  upstream gradient 1;  up-sampling weights 1/f per axis
        input of layer 1: q_0 = min(1/2, 8 / soi)           pre-activation of layer 1: q_1 = min(1/4, 8 / soi) -- the weights of the
        relative coordinates are whole numbers --           of layer k > 1: q_k = q_{k-1} / 2   (a bias is a multiple of it)
        logits: q_y / f^2          d y: 1 / f^2          d pre of layer k: d q_{k+1} / 2
        weight gradient of layer k: d q_k * q_{k-1}         bias gradient: d q_k         d feat: d q_1 / 2
    A sum of multiples of q whose absolute values add up to less than q * 2^24 has every partial sum, in any order and under any
    grouping into FMAs, tiles, slots and partial buffers, a multiple of q below q * 2^24 in magnitude: exactly representable."""
    r = restate(c, torch.float64, absolute=True, open_gates=True)
    N, L, f = c['N'], c['layers'], c['factor']
    cap = 2.0 ** 24
    per_inst = lambda t: t.reshape(N, -1).max(dim=1).values if N else torch.zeros(0, dtype=torch.float64)
    soi = torch.tensor(SOI, dtype=torch.float64)[torch.from_numpy(c['lvl'])]
    q_in = torch.minimum(torch.full_like(soi, 0.5), IN_STRIDE / soi) if c['rel'] else torch.full((N,), 0.5, dtype=torch.float64)
    q = [q_in]                                            # q[k] = quantum of the input of layer k + 1
    q.append(torch.minimum(torch.full_like(soi, 0.25), IN_STRIDE / soi) if c['rel'] else q_in / 2)
    for _ in range(L - 1):
        q.append(q[-1] / 2)
    out = {}
    for k, p in enumerate(r['pre']):
        out[f'h{k + 1}'] = float((per_inst(p) / (q[k + 1] * cap)).max()) if N else 0.0
    out['y'] = float((per_inst(r['y']) / (q[L] * cap)).max()) if N else 0.0
    out['logits'] = float((per_inst(r['logits']) / (q[L] / f ** 2 * cap)).max()) if N else 0.0
    dq = [None] * (L + 1)                                 # dq[k] = quantum of d (output of layer k), k = 1 .. L
    dq[L] = 1.0 / f ** 2
    for k in range(L - 1, 0, -1):
        dq[k] = dq[k + 1] / 2
    out['dy'] = float(r['d_y'].max() / (dq[L] * cap)) if N else 0.0
    for k, d in enumerate(r['d_pre']):
        out[f'dh{k + 1}'] = float(d.max() / (dq[k + 1] * cap)) if N else 0.0
    cin = c['C'] + (2 if c['rel'] else 0)
    wsz, bsz = param_sizes(cin, L, c['channels'])
    gp, w_off, b_off = r['d_params'], 0, sum(wsz)
    for k, (nw, nb) in enumerate(zip(wsz, bsz)):
        out[f'dW{k}'] = float((per_inst(gp[:, w_off:w_off + nw]) / (dq[k + 1] * q[k] * cap)).max()) if N else 0.0
        out[f'db{k}'] = float(gp[:, b_off:b_off + nb].max() / (dq[k + 1] * cap)) if N else 0.0
        w_off += nw
        b_off += nb
    out['d_feat'] = float(r['d_feat'].max() / (dq[1] / 2 * cap))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# where an element belongs
# ------------------------------------------------------------------------------------------------------------------------------
def slots_for(cus: int, B: int, H: int, W: int, N: int, factor: int) -> int:
    """Workgroups per (image, tile) of the tuned backward (csrc/dynamic_head.hip, bxi_dynamic_mask_backward_f32)."""
    T = -(-H // TILE_BWD[0]) * -(-W // TILE_BWD[1])
    if factor in (1, 2):
        cap = 4 * cus // (B * T)
        return MAX_SLOTS if N > 16 * B or cap >= MAX_SLOTS else max(cap, 1)
    return 4 if N <= 16 * B else MAX_SLOTS


def slot_of(c, n: int, slots: int) -> int:
    """The slot that walks instance n: its ordinal among the instances of its image, modulo the slot count."""
    return int((c['img'][:n] == c['img'][n]).sum()) % slots


def first_difference(c, what: str, got: np.ndarray, want: np.ndarray, slots=None) -> str:
    """'' when the arrays are equal element by element, as torch.equal has it except that a NaN equals a NaN: the sign of a zero
    is NOT order-free ((-0) + (+0) = +0: it depends on what an accumulator starts with), so +0 and -0 compare equal.  Otherwise a
    description of the first differing element and their number."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return ''
    idx = tuple(int(v) for v in bad[0])
    f = c['factor']
    where = ''
    if what == 'logits':
        fr, fc = TILE_FWD.get(f, (8, 32))
        where = f'instance {idx[0]} (image {int(c["img"][idx[0]])}), forward tile ({idx[2] // (fr * f)}, {idx[3] // (fc * f)})'
    elif what == 'd_feat':
        where = f'image {idx[0]}, backward tile ({idx[2] // TILE_BWD[0]}, {idx[3] // TILE_BWD[1]}), summed over {slots} slots'
    elif what == 'd_params':
        where = f'instance {idx[0]} (image {int(c["img"][idx[0]])}' + (f', slot {slot_of(c, idx[0], slots)} of {slots}' if slots else '') + '), summed over the tiles'
    return (f'{name_of(c)}: {what}{list(idx)} = {got[idx]!r}, expected {want[idx]!r}; {where}; {len(bad)} of {got.size} elements differ')


_CACHE: dict = {}


def case_and_expected(*args, **kw):
    """dyadic_case(*args, **kw) and expected() of it in fp64 rounded to fp32 -- computed once per distinct case and shared."""
    key = (args, tuple(sorted(kw.items())))
    if key not in _CACHE:
        c = dyadic_case(*args, **kw)
        want = tuple(np.ascontiguousarray(a.astype(np.float32)) for a in expected(c, torch.float64)) if c['N'] else None
        for a in (want or ()):
            a.setflags(write=False)
        _CACHE[key] = (c, want)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_host_dyn_exact.py and tests/test_gpu_dynamic_head_exact.py: (args, kwargs) of dyadic_case
# ------------------------------------------------------------------------------------------------------------------------------
def _case(seed, B, C, H, W, N, factor, rel, grad_budget=2400, **kw):
    """Densities lowered until the premise holds (tests/test_host_dyn_exact.py asserts it): the weight gradients sum
    d y * hidden over the map, d y is a multiple of 1 / f^2 and the last hidden layer of 8 / 1024 / 2, so the number of non-zero
    upstream gradients per instance is held to grad_budget / f^2 (never above a quarter of the map) and, with relative coordinates,
    three parameters in ten are non-zero instead of five."""
    kw.setdefault('param_density', 0.3 if rel else 0.5)
    kw.setdefault('grad_density', min(0.25, grad_budget / float(factor ** 4 * H * W)))
    return (seed, B, C, H, W, N, factor, bool(rel)), kw


TUNED = [_case(100 + 8 * (C // 16) + 4 * rel + i, 2, C, 17, 37, 6, f, rel) for C in (8, 16) for rel in (1, 0) for i, f in enumerate((1, 2, 4, 8))]
# (B, C, H, W, N, factor): see test_slot_counts for the slot counts these give
SLOTS = [TUNED[1],
         _case(201, 3, 8, 57, 200, 9, 2, 1),
         _case(202, 4, 16, 80, 256, 8, 2, 1),
         _case(203, 4, 8, 104, 320, 4, 2, 1),
         _case(204, 2, 16, 17, 37, 40, 2, 1),
         TUNED[2], _case(205, 2, 8, 17, 37, 40, 4, 1),
         TUNED[3], _case(206, 2, 16, 17, 37, 40, 8, 0)]
EDGE_SHAPES = [(1, 1), (1, 33), (33, 1), (2, 32), (32, 2), (8, 32), (9, 33), (8, 64), (15, 64), (16, 9)]
EDGES = [_case(300 + 10 * k + f, 2, (8, 16)[(k + f) % 2], H, W, 5, f, (k + f // 2) % 2) for k, (H, W) in enumerate(EDGE_SHAPES) for f in (1, 2, 4)]
# (layers, channels, in_channels, rel, factor, (B, H, W, N)); the fourth is the shipped shape through the general entry
GENERIC = [_case(400 + i, B, cin, H, W, N, f, rel, layers=L, channels=ch)
           for i, (L, ch, cin, rel, f, (B, H, W, N)) in enumerate([
               (1, 8, 8, 1, 2, (2, 12, 20, 5)), (2, 4, 6, 1, 2, (2, 12, 20, 5)), (3, 5, 7, 0, 1, (2, 9, 33, 5)),
               (3, 8, 16, 1, 2, (2, 23, 37, 9)), (4, 16, 32, 1, 4, (2, 10, 35, 6)), (4, 12, 3, 1, 8, (3, 17, 40, 7))])]
# four layers: one more factor of (channels x density) in every hidden magnitude -- fewer parameters, and half the gradient budget at 16 channels
GENERIC[4] = (GENERIC[4][0], dict(GENERIC[4][1], param_density=0.15, grad_density=GENERIC[4][1]['grad_density'] / 2))
GENERIC[5] = (GENERIC[5][0], dict(GENERIC[5][1], param_density=0.2))
# non-finite inputs: two images with instances (six and three), a third without
NAN = _case(600, 3, 8, 17, 37, 9, 2, 1, empty_image=2)
# the shapes of test_head_fused_into_the_loss_evaluation: (C, rel, B, H, W, N) -- the instance -> image map comes from the batch
FUSED = [(16, 1, 2, 100, 128, 32), (8, 1, 1, 32, 32, 4), (8, 0, 1, 32, 32, 3)]


def fused_case(C, rel, B, H, W, N, img):
    c = dyadic_case(500 + C + rel, B, C, H, W, N, 2, rel, param_density=0.3 if rel else 0.5, grad_density=min(0.25, 600.0 / (4 * H * W)))
    c['img'] = np.asarray(img, np.int64)
    return c


def all_cases():
    """Every distinct case the GPU file runs through dyadic_case (the head-fused ones are built in the tests: they need a batch)."""
    seen, out = set(), []
    for args, kw in TUNED + SLOTS + EDGES + GENERIC + [NAN]:
        key = (args, tuple(sorted(kw.items())))
        if key not in seen:
            seen.add(key)
            out.append((args, kw))
    return out


def fused_batch(C, rel, B, H, W, N):
    """The synthetic batch of test_head_fused_into_the_loss_evaluation for one of FUSED and the dyadic case on its instance -> image map."""
    from boxinstseg_amd import synthetic
    d = synthetic.cfg2(3) if B == 2 else synthetic.cfg1(1)
    assert d['imgs'].shape[0] == B and d['imgs'].shape[2] == IN_STRIDE * H and d['imgs'].shape[3] == IN_STRIDE * W
    gt_inds = np.asarray(d['gt_inds'])[:N]
    counts = np.cumsum([0] + [b.shape[0] for b in d['gt_bboxes']])
    img = [int(np.searchsorted(counts, int(g), side='right') - 1) for g in gt_inds]
    assert len(img) == N
    return d, gt_inds, fused_case(C, rel, B, H, W, N, img)
