"""Reference statements of the masked-attention tests, all on the CPU in the dtype of their inputs.

    mha_torch          (i)   torch's own ``nn.MultiheadAttention(E, M)(q, k, v, attn_mask=bool)[0]`` -- THE yardstick
    attention_heads    (ii)  the same per head, restated: in-projection, scale q, ``masked_fill(-inf)``, softmax, bmm, out-projection
    box2mask_mask      (iii) Box2MaskHead.forward_head, box2mask_head.py:346-355, and the repair of forward, :397, restated statement by
                             statement; tests/golden/make_golden_masked_attn.py executes the reference's own statements (taken out by AST)
                             and checks that this restatement equals them exactly before it writes tests/golden/masked_attn.npz
    RefMultiheadAttention    mmcv's wrapper restated from its documented behaviour over torch's nn.MultiheadAttention (unpinned: mmcv never
                             ran here)

plus the seeded cases, the bit packing and the tolerance rule of the project: 4 x the fp32-against-fp64 difference of statement (i),
relative to the largest fp64 value."""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'masked_attn.npz')
CFG_JSON = os.path.join(HERE, 'golden', 'masked_attn_cfg.json')
FACTOR = 4

# the mask-bit cases of the fixture: name -> (input H, W, target h, w); mask_pred is [2, 5, H, W]
MASK_SHAPE = (2, 5)
MASK_CASES = {'f8': (64, 64, 8, 8), 'f4': (64, 64, 16, 16), 'f2': (64, 64, 32, 32), 'odd': (64, 64, 5, 7), 'up': (64, 64, 96, 80)}
MASK_SEED, MASK_HEADS = 0, 8


# ---- (i) and (ii) --------------------------------------------------------------------------------------------------------------------
def identity_params(E, dtype=torch.float64):
    """Projections that leave q, k, v and the result as they are (exact in any dtype): statement (i) is then the attention core alone."""
    eye = torch.eye(E, dtype=dtype)
    return {'in_proj_weight': torch.cat([eye, eye, eye]), 'in_proj_bias': torch.zeros(3 * E, dtype=dtype), 'out_proj.weight': eye.clone(),
            'out_proj.bias': torch.zeros(E, dtype=dtype)}


def random_params(E, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return {'in_proj_weight': (torch.randn(3 * E, E, generator=g) / E ** 0.5).to(dtype), 'in_proj_bias': (0.1 * torch.randn(3 * E, generator=g)).to(dtype),
            'out_proj.weight': (torch.randn(E, E, generator=g) / E ** 0.5).to(dtype), 'out_proj.bias': (0.1 * torch.randn(E, generator=g)).to(dtype)}


def mha_torch(q, k, v, mask, M, params):
    """(i): q [Q,B,E], k and v [S,B,E], mask bool [B*M,Q,S] / [Q,S] / None (True = masked)."""
    E = q.shape[-1]
    mha = nn.MultiheadAttention(E, M).to(q.dtype)
    mha.load_state_dict({n: p.to(q.dtype) for n, p in params.items()})
    return mha(q, k, v, attn_mask=mask)[0]


def attention_heads(q, k, v, mask, M, params):
    """(ii)"""
    Q, B, E = q.shape
    S, D = k.shape[0], E // M
    w, b = params['in_proj_weight'].to(q.dtype), params['in_proj_bias'].to(q.dtype)
    qp, kp, vp = F.linear(q, w[:E], b[:E]), F.linear(k, w[E:2 * E], b[E:2 * E]), F.linear(v, w[2 * E:], b[2 * E:])
    qh = qp.reshape(Q, B * M, D).transpose(0, 1) * (1.0 / D) ** 0.5
    kh, vh = kp.reshape(S, B * M, D).transpose(0, 1), vp.reshape(S, B * M, D).transpose(0, 1)
    scores = torch.bmm(qh, kh.transpose(1, 2))
    if mask is not None:
        scores = scores.masked_fill(mask if mask.dim() == 3 else mask[None], float('-inf'))
    out = torch.bmm(torch.softmax(scores, -1), vh).transpose(0, 1).reshape(Q, B, E)
    return F.linear(out, params['out_proj.weight'].to(q.dtype), params['out_proj.bias'].to(q.dtype))


def core_with_grads(t, M, dtype, statement=mha_torch):
    """Statement (i) with identity projections on the case ``t`` (q, k, v, g, mask): out and the gradients of ``(out * g).sum()``."""
    q, k, v = (t[n].to(dtype).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    out = statement(q, k, v, t.get('mask'), M, identity_params(q.shape[-1], dtype))
    (out * t['g'].to(dtype)).sum().backward()
    return {'out': out.detach(), 'dq': q.grad, 'dk': k.grad, 'dv': v.grad}


def bound(q32, q64):
    """4 x statement (i)'s own fp32 error, relative to the largest fp64 value."""
    top = float(q64.abs().max())
    return FACTOR * float((q32.double() - q64).abs().max()) / top if top > 0 else 0.0


def make_case(seed, Q, S, D, B=2, M=2, keep=0.4, mask=True, spread=1.0):
    """Seeded q, k, v, upstream gradient and a bool mask [B*M,Q,S] in which every row keeps at least one key."""
    g = torch.Generator().manual_seed(seed)
    E = M * D
    t = {'q': spread * torch.randn(Q, B, E, generator=g), 'k': spread * torch.randn(S, B, E, generator=g), 'v': torch.randn(S, B, E, generator=g),
         'g': torch.randn(Q, B, E, generator=g)}
    if mask:
        m = torch.rand(B * M, Q, S, generator=g) >= keep
        m[..., 0] &= ~m.all(-1)                                       # a row with nothing kept keeps key 0
        t['mask'] = m
    return t


# ---- bits ----------------------------------------------------------------------------------------------------------------------------
def pack_bits(mask):
    """bool [..., S] (True = masked) -> int32 [..., ceil(S / 32)], bit s & 31 of word s >> 5, tail bits clear."""
    S = mask.shape[-1]
    words = (S + 31) // 32
    m = F.pad(mask.to(torch.int64), (0, words * 32 - S)).reshape(*mask.shape[:-1], words, 32)
    w = (m << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(bits, S):
    b = (bits.to(torch.int64)[..., None] >> torch.arange(32, dtype=torch.int64)) & 1
    return b.reshape(*bits.shape[:-1], -1)[..., :S].bool()


# ---- (iii) ---------------------------------------------------------------------------------------------------------------------------
def box2mask_mask(mask_pred, attn_mask_target_size, num_heads):
    """box2mask_head.py:346-355 and :397: the bool mask [B*num_heads, Q, S] the reference hands to its cross-attention."""
    attn_mask = F.interpolate(mask_pred, attn_mask_target_size, mode='bilinear', align_corners=False)
    attn_mask = attn_mask.flatten(2).unsqueeze(1).repeat((1, num_heads, 1, 1)).flatten(0, 1)
    attn_mask = attn_mask.sigmoid() < 0.5
    attn_mask = attn_mask.detach()
    attn_mask[torch.where(attn_mask.sum(-1) == attn_mask.shape[-1])] = False
    return attn_mask


def resized(mask_pred, size):
    return F.interpolate(mask_pred, size, mode='bilinear', align_corners=False).flatten(2)


def seeded_mask_pred():
    """The N(0, 3^2) logits of the mask cases, fp32 [2, 5, 64, 64] (the fixture stores them: the tests read them from there)."""
    g = torch.Generator().manual_seed(MASK_SEED)
    return 3.0 * torch.randn(*MASK_SHAPE, 64, 64, generator=g)


def planted_mask_pred():
    """Integer logits [2, 5, 64, 64] for the factor-8 case (weights 1/2 * 1/2: every resized value is exact in fp32): row (0, 1) all negative
    (repaired to all clear), row (0, 2) resized values exactly 0 in places (not masked), row (1, 3) all zero."""
    g = torch.Generator().manual_seed(77)
    p = torch.randint(-6, 7, (2, 5, 64, 64), generator=g).float()
    p[0, 1] = -1.0 - torch.randint(0, 5, (64, 64), generator=g).float()
    p[0, 2, 3:5, 3:5] = torch.tensor([[1.0, -1.0], [-1.0, 1.0]])     # the taps of target (0, 0): their mean is exactly 0
    p[0, 2, 11:13, 3:5] = 0.0
    p[1, 3] = 0.0
    return p


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- mmcv's wrapper ------------------------------------------------------------------------------------------------------------------
class RefMultiheadAttention(nn.Module):
    """mmcv.cnn.bricks.transformer.MultiheadAttention, restated: positions added to query and key only, torch's module in [L,B,C] order,
    ``identity + dropout_layer(proj_drop(out))``."""

    def __init__(self, embed_dims, num_heads, attn_drop=0., proj_drop=0., dropout_layer=dict(type='Dropout', drop_prob=0.), init_cfg=None,
                 batch_first=False, **kwargs):
        super().__init__()
        self.embed_dims, self.num_heads, self.batch_first = embed_dims, num_heads, batch_first
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
        self.proj_drop = nn.Dropout(proj_drop)
        self.dropout_layer = nn.Dropout(dropout_layer.get('drop_prob', 0.5)) if dropout_layer else nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None, key_padding_mask=None, **kwargs):
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None:
            if query_pos is not None and query_pos.shape == key.shape:
                key_pos = query_pos
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
        out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))
