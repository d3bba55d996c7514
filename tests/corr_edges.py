"""Case builders for the edge tests of DiscoBox's cross-image correspondence (tests/test_host_corr_edges.py checks on the CPU that every
case is what it claims to be; tests/test_gpu_corr_edges.py runs the kernels of csrc/corr.hip on them).

The referee is tests/corr_ref.py in fp64 on the same inputs.  Inputs are rounded to float16 (``R.half``), 'good' entries are built as in
tests/test_gpu_corr.py::test_odd_sizes_and_other_settings_against_the_restatement (snapped blobs, ``R.feature``), every case is
deterministic from the fixed seeds below, and everything is built once per process (functools.lru_cache) and must not be modified.

A fused case is ``dict(inp, cfg, hw)``: ``inp`` the numpy arrays of ``R.INPUT_KEYS``, ``cfg`` the fixture's settings with the case's own
(``max_retrieval_objs``, ``min_objs``, ``min_size``, the solver's three), ``hw`` the canvas.  The student entry of object i is drawn from
seed ``1000 case + 300 + 20 i + RETRY[name][i]``: the retry is the first for which the restatement alone leaves no near tie among the
arg-maxes of that object's rows of C (``GAP``); tests/test_host_corr_edges.py asserts that it does."""
import functools

import numpy as np
import torch

from tests import corr_ref as R

SPEC = R.load_cases()
CFG = SPEC['cfg']
GAP = 1e-3                       # relative gap between the largest and the second largest entry of every row of every running plane of C
AWAY = 1e-2                      # relative distance of every non-exact score of a generic case from its threshold
MARGIN = 4.0                     # the project's margin over the reference's own fp32-against-fp64 difference
STORED_BOX = (0, 0, 20, 19)
BOXES3 = ((3, 2, 24, 21), (20, 9, 47, 33), (0, 5, 17, 20))
BANK_KEYS = ('bank_feature', 'bank_mask', 'bank_box', 'bank_ptr')


def base_of(seed, C):
    return np.abs(np.random.RandomState(seed).standard_normal((C, 7, 7)))


def good(base, seed):
    """(feature, mask) of a 'good' entry: every score of two of them is far from its threshold."""
    rng = np.random.RandomState(seed)
    f = R.half(R.feature(base, rng))
    return f, R.half(R.snap(R.blob(13.5 + rng.uniform(-0.4, 0.4), 13.5, 9.0 + rng.uniform(-0.3, 0.3))))


def blank(C, L, num_class, ptr, boxes, labels):
    N = len(labels)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    return dict(s_feat=z(N, C, 7, 7), s_mask=z(N, 28, 28), t_feat=z(N, C, 7, 7), t_mask=z(N, 28, 28), boxes=np.asarray(boxes, np.float32).reshape(N, 4),
                labels=np.asarray(labels, np.int64), bank_feature=z(num_class, L, C, 7, 7), bank_mask=z(num_class, L, 28, 28), bank_box=z(num_class, L, 4),
                bank_ptr=np.asarray(ptr, np.int32))


def _fill(inp, cid, base, retry, objects, stored):
    """Good entries: ``stored`` (class, slot, box) into the bank, ``objects`` (indices, in order) as student and teacher entries."""
    for n, (c, s, box) in enumerate(stored):
        inp['bank_feature'][c, s], inp['bank_mask'][c, s] = good(base, 1000 * cid + 100 + n)
        inp['bank_box'][c, s] = box
    for n, i in enumerate(objects):
        inp['t_feat'][i], inp['t_mask'][i] = good(base, 1000 * cid + 200 + n)
        inp['s_feat'][i], inp['s_mask'][i] = good(base, 1000 * cid + 300 + 20 * n + (retry[n] if n < len(retry) else 0))
    return inp


def _cfg(**kw):
    return dict(CFG, **kw)


# ---- 1: many objects, a short queue ------------------------------------------------------------------------------------------------------
MANY_N, MANY_GOOD, MANY_WIDTHS, MANY_PTR = 300, (0, 63, 64, 65, 255, 256, 299), (9, 13, 16, 11, 8), (2, 0, 1)


def many(retry=(), reduced=False):
    """N = 300 over three classes, L = 3, K = 3, min_objs = 2, C = 17, canvas 24 x 40, min_size = 8.  Class 0: two good stored entries
    (slots 0 and 1, ptr 2) and the good objects ``MANY_GOOD``.  Every other object j is of class 1 + j % 2 with zero masks (its fg score
    is 0 / 0: it neither retrieves nor is retrieved), a t_feat whose first element is j / 512, height 10 and width ``MANY_WIDTHS[j % 5]``:
    every fifth is exactly min_size wide and must not be appended.  ``reduced``: the good objects alone (class 0 sees nothing else)."""
    N, C, L = MANY_N, 17, 3
    base = base_of(1000, C)
    rng = np.random.RandomState(1001)
    boxes, labels = np.zeros((N, 4), np.float32), np.zeros(N, np.int64)
    for j in range(N):
        if j in MANY_GOOD:
            g = MANY_GOOD.index(j)
            boxes[j] = [3 * g, g % 5, 3 * g + 21, g % 5 + 19]
        else:
            labels[j] = 1 + j % 2
            boxes[j] = [j % 7, j % 11, j % 7 + MANY_WIDTHS[j % 5], j % 11 + 10]
    inp = blank(C, L, 3, MANY_PTR, boxes, labels)
    for j in range(N):
        if j not in MANY_GOOD:
            inp['t_feat'][j] = R.half(rng.random_sample((C, 7, 7)))
            inp['t_feat'][j, 0, 0, 0] = j / 512.0
            inp['s_feat'][j] = R.half(rng.random_sample((C, 7, 7)))
    _fill(inp, 1, base, retry, MANY_GOOD, [(0, 0, STORED_BOX), (0, 1, STORED_BOX)])
    if reduced:
        sel = list(MANY_GOOD)
        inp = {k: (v[sel] if k in R.INPUT_KEYS[:6] else v) for k, v in inp.items()}
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=3, min_objs=2, min_size=8), hw=(24, 40))


# ---- 2: the configs' queue ---------------------------------------------------------------------------------------------------------------
QUEUE_SLOTS = (0, 3, 4, 5, 62, 63, 64, 65, 98, 99)


def queue(L, one_class=False, retry=()):
    """Three objects, K = 8, min_objs = 1, C = 32.  Class 0 holds good entries at those of ``QUEUE_SLOTS`` that exist, class 1 a single
    one (slot 7 of 100, else the last slot), class 2 none; the labels are 0, 1, 2.  ``one_class``: the same three objects, all of class
    0 with one stored entry at slot 0, so that each object retrieves what the objects before it appended."""
    C = 32
    base = base_of(2000, C)
    if one_class:
        stored, labels, ptr = [(0, 0, STORED_BOX)], [0, 0, 0], [1 % L, 0, 0]
    else:
        stored = [(0, s, STORED_BOX) for s in QUEUE_SLOTS if s < L] + [(1, 7 if L == 100 else L - 1, STORED_BOX)]
        labels, ptr = [0, 1, 2], ([6, 99, 0] if L == 100 else [1 % L, 0, 0])
    inp = _fill(blank(C, L, 3, ptr, BOXES3, labels), 2, base, retry, range(3), stored)
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=8, min_objs=1, min_size=6), hw=(40, 56))


# ---- 3: solver edges ---------------------------------------------------------------------------------------------------------------------
ZERO_S, ZERO_BANK = (1, 3, 3), (1, 2, 5)        # (object, y, x) of the zeroed cell of s_feat; (slot, y, x) of the zeroed cell of the bank


def solver_case(C, retry=(), zero=False, **settings):
    """Two objects of one class, K = 3, min_objs = 2, L = 5, stored entries at slots 1 and 3, ptr 4: object 0 runs with two retrieved
    objects, object 1 with three, the third being object 0's append.  ``zero``: one cell of object 1's s_feat and one of slot 1's feature
    are zero in every channel."""
    inp = _fill(blank(C, 5, 1, [4], BOXES3[:2], [0, 0]), 3, base_of(3000 + C, C), retry, range(2), [(0, 1, STORED_BOX), (0, 3, STORED_BOX)])
    if zero:
        inp['s_feat'][ZERO_S[0], :, ZERO_S[1], ZERO_S[2]] = 0
        inp['bank_feature'][0, ZERO_BANK[0], :, ZERO_BANK[1], ZERO_BANK[2]] = 0
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=3, min_objs=2, min_size=6, **settings), hw=(33, 47))


# ---- 4: paste geometry -------------------------------------------------------------------------------------------------------------------
PASTE_HW = (72, 88)
PASTE_BOXES = ((10, 5, 80, 65), (3.75, 2.5, 24.75, 21.5), (40, 30, 41, 55), (67, 53, 88, 72))
THIN_BOX = (0, 0, 1, 25)
CLIP_BOXES = ((-8, 10, 13, 29), (30, -7, 51, 12), (75, 20, 96, 39), (40, 60, 61, 79), (95, 10, 116, 29))
PAD = 32


def paste(retry=()):
    """72 x 88 (two tiles of 4096; element 4096 is row 46, column 48): a 70 x 60 box over the tile edge, fractional corners, a box one
    pixel wide (class 1, whose two stored entries have a box of the same shape), a box touching the last row and column."""
    stored = [(0, 1, STORED_BOX), (0, 3, STORED_BOX), (1, 0, THIN_BOX), (1, 1, THIN_BOX)]
    inp = _fill(blank(32, 5, 2, [4, 2], PASTE_BOXES, [0, 0, 1, 0]), 4, base_of(4000, 32), retry, range(4), stored)
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=3, min_objs=2, min_size=6), hw=PASTE_HW)


def clip(padded, retry=()):
    """Integer boxes leaving the 72 x 88 canvas on the left, top, right and bottom, and one wholly outside.  ``padded``: the same call on a
    canvas padded by ``PAD`` on every side with the boxes moved by +PAD, which the restatement can run; cropped, it is the referee."""
    boxes = np.asarray(CLIP_BOXES, np.float32) + (PAD if padded else 0)
    inp = _fill(blank(32, 8, 1, [4], boxes, [0] * 5), 5, base_of(5000, 32), retry, range(5), [(0, 1, STORED_BOX), (0, 3, STORED_BOX)])
    hw = (PASTE_HW[0] + 2 * PAD, PASTE_HW[1] + 2 * PAD) if padded else PASTE_HW
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=3, min_objs=2, min_size=6), hw=hw)


# ---- 5: labels outside the range ---------------------------------------------------------------------------------------------------------
BAD_LABELS = {1: -1, 3: 2}                      # object -> label, in the fixture's 'plain' case (two classes)


def labels_case(removed):
    g, c = np.load(R.GOLDEN), SPEC['cases']['plain']
    inp = {k: v.numpy().copy() for k, v in R.inputs_of(g, 'plain').items()}
    for i, lab in BAD_LABELS.items():
        inp['labels'][i] = lab
    if removed:
        keep = [i for i in range(len(inp['labels'])) if i not in BAD_LABELS]
        inp = {k: (v[keep] if k in R.INPUT_KEYS[:6] else v) for k, v in inp.items()}
    return dict(inp=inp, cfg=_cfg(min_size=c['min_size']), hw=tuple(c['out_hw']))


SOLVER_SETTINGS = dict(iter0=dict(corr_num_iter=0), smooth0=dict(corr_num_iter=2, corr_num_smooth_iter=0), dist1=dict(dist_kernel=1),
                       dist13=dict(dist_kernel=13), it1sm3d3=dict(corr_num_iter=1, corr_num_smooth_iter=3, dist_kernel=3),
                       # after ten rounds C no longer depends on dist_kernel beyond 1e-11 (the host test shows it): one round does
                       dist1_it1=dict(dist_kernel=1, corr_num_iter=1), dist13_it1=dict(dist_kernel=13, corr_num_iter=1))
BUILDERS = dict(many=many, many_reduced=lambda retry=(): many(retry, True), queue100=lambda retry=(): queue(100, False, retry),
                paste=paste, clip_padded=lambda retry=(): clip(True, retry), labels=lambda retry=(): labels_case(False),
                labels_removed=lambda retry=(): labels_case(True), zero_cells=lambda retry=(): solver_case(17, retry, True))
for _L in (1, 2, 3):
    BUILDERS[f'queue{_L}'] = lambda retry=(), L=_L: queue(L, False, retry)
    BUILDERS[f'queue{_L}_one_class'] = lambda retry=(), L=_L: queue(L, True, retry)
for _C in (15, 16, 17):
    BUILDERS[f'c{_C}'] = lambda retry=(), C=_C: solver_case(C, retry)
for _k, _v in SOLVER_SETTINGS.items():
    BUILDERS[_k] = lambda retry=(), kw=_v: solver_case(17, retry, **kw)

# the retries found for the rule of the module docstring (all zero where a name is absent)
RETRY = dict(many=(1, 0, 0, 0, 1, 0, 0), c15=(1, 5), c16=(0, 1), iter0=(1, 1), smooth0=(1, 1))
RETRY['many_reduced'] = RETRY['many']
# the calls that the restatement runs as they are: the generic fused cases of the GPU test ('clip' is compared through 'clip_padded')
FUSED = tuple(n for n in BUILDERS if n not in ('many_reduced', 'labels', 'labels_removed'))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'clip':
        return clip(False, RETRY.get('clip_padded', ()))
    return BUILDERS[name](RETRY.get(name, ()))


def as_torch(inp, dtype=torch.float64):
    out = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
    return {k: (v.to(dtype) if v.dtype == torch.float32 else v) for k, v in out.items()}


def restate(c, dtype=torch.float64):
    """The restatement on a case: its record, the gradient, the bank afterwards (``after_*``)."""
    t = as_torch(c['inp'], dtype)
    t['s_feat'].requires_grad_(True)
    out = R.corr_objects(t, c['cfg'], c['hw'], record=True)
    out['grad'] = torch.autograd.grad(out['loss_sum'], t['s_feat'])[0] if out['num_ins'] else torch.zeros_like(t['s_feat']).detach()
    out['loss_sum'] = out['loss_sum'].detach()
    for k in BANK_KEYS:
        out['after_' + k[5:]] = t[k]
    return out


@functools.lru_cache(maxsize=None)
def want(name, dtype='float64'):
    if name == 'clip':
        w = dict(want('clip_padded', dtype))
        w['iiu'] = w['iiu'][:, :, PAD:PAD + PASTE_HW[0], PAD:PAD + PASTE_HW[1]]
        box = w['after_box'].clone()
        box[(box != torch.from_numpy(case('clip_padded')['inp']['bank_box']).to(box)).any(-1)] -= PAD      # the rows that the call wrote
        w['after_box'] = box
        return w
    return restate(case(name), getattr(torch, dtype))


def object_gaps(w, min_objs):
    """Per object that ran: the smallest relative gap between the two largest entries of a row of its planes of C."""
    out = {}
    for i, n in enumerate(w['count'].tolist()):
        if n >= min_objs:
            top = w['C'][i, :n].topk(2, dim=2).values
            out[i] = float(((top[..., 0] - top[..., 1]) / top[..., 0]).min())
    return out


def min_gap(name):
    g = object_gaps(want(name), case(name)['cfg']['min_objs'])
    return min(g.values()) if g else float('inf')


def score_distance(name):
    """The smallest relative distance of a finite fp64 score of the case from its threshold."""
    cfg, s = case(name)['cfg'], want(name)['scores']
    th = (cfg['fg_iou_thresh'], cfg['bg_iou_thresh'], cfg['appear_thresh'])
    d = [((s[..., k] - th[k]).abs() / abs(th[k])) for k in range(3)] + [((s[..., 3] - t).abs() / abs(t)) for t in cfg['ratio_range']]
    d = torch.stack(d)
    fin = torch.isfinite(d)
    return float(d[fin].min()) if bool(fin.any()) else float('inf')


def assert_conditions(name):
    """The conditions under which the exact parts of a fused case are decided by the restatement alone."""
    gap, dist = min_gap(name), score_distance(name)
    print(f'{name}: smallest arg-max gap {gap:.3e}, smallest distance of a score from its threshold {dist:.3e}')
    assert gap >= GAP, f'{name}: a row of C is a near tie ({gap:.3e})'
    assert dist >= AWAY, f'{name}: a score lies {dist:.3e} from its threshold'


def rel(a32, a64):
    """max |fp32 - fp64| over the largest fp64 magnitude, over the finite entries of the fp64 array: the policy behind the fixture's tol_*."""
    a32, a64 = a32.double(), a64.double()
    fin = torch.isfinite(a64)
    if not bool(fin.any()):
        return 0.0
    top = float(a64[fin].abs().max())
    return float((a32[fin] - a64[fin]).abs().max()) / top if top > 0 else 0.0


@functools.lru_cache(maxsize=None)
def score_tols():
    """Per score (fg, bg, appearance, ratio): the fp32 restatement against the fp64 one, pooled over the generic fused cases as tol_* are."""
    return tuple(max(rel(want(n, 'float32')['scores'][..., k], want(n)['scores'][..., k]) for n in FUSED) for k in range(4))


# ---- exact scores --------------------------------------------------------------------------------------------------------------------------
WIDE = dict(fg_iou_thresh=float('-inf'), bg_iou_thresh=float('-inf'), appear_thresh=float('-inf'), ratio_range=[float('-inf'), float('inf')])
EXACT_L, EXACT_C, EXACT_EMPTY = 6, 4, 2
# slot -> (rows, columns) of the 7 x 7 blocks that are set, and the stored box; the query has rows 1..5, columns 1..5 and a 16 x 16 box
EXACT_SLOTS = {0: ((1, 6), (2, 7), (0, 0, 16, 16)), 1: ((1, 6), (1, 6), (0, 0, 16, 16)), 3: ((2, 7), (2, 7), (0, 0, 16, 16)),
               4: ((1, 6), (1, 6), (0, 0, 8, 16)), 5: ((1, 4), (1, 6), (0, 0, 32, 16))}


def block_mask(rows, cols):
    p = np.zeros((7, 7), np.float32)
    p[rows[0]:rows[1], cols[0]:cols[1]] = 1
    return np.kron(p, np.ones((4, 4), np.float32))


@functools.lru_cache(maxsize=None)
def exact_case(zero_query=False):
    """One object against six slots: binary masks constant on 4 x 4 blocks, features in multiples of 1/8, boxes whose ratios are powers
    of two apart.  Slot ``EXACT_EMPTY`` was never written.  min_size is out of reach: nothing is appended, the bank stays as it is.
    ``zero_query``: the object's mask is all zero, so its fg score against the empty slot is 0 / 0."""
    inp = blank(EXACT_C, EXACT_L, 1, [0], [(4, 4, 20, 20)], [0])
    c, y, x = np.meshgrid(np.arange(EXACT_C), np.arange(7), np.arange(7), indexing='ij')
    inp['s_feat'][0], inp['s_mask'][0] = ((3 * c + 5 * y + 7 * x) % 9) / 8.0, block_mask((1, 6), (1, 6)) * (0 if zero_query else 1)
    inp['t_feat'][0], inp['t_mask'][0] = inp['s_feat'][0], inp['s_mask'][0]
    for s, (rows, cols, box) in EXACT_SLOTS.items():
        inp['bank_feature'][0, s], inp['bank_mask'][0, s], inp['bank_box'][0, s] = ((5 * c + 3 * y + 2 * x + s) % 9) / 8.0, block_mask(rows, cols), box
    return dict(inp=inp, cfg=_cfg(max_retrieval_objs=8, min_objs=8, min_size=1e9, **WIDE), hw=(24, 40))


def exact_scores(dtype=torch.float32, zero_query=False):
    """[L, 4] by ``R.slot_scores`` in ``dtype`` on the CPU."""
    t = as_torch(exact_case(zero_query)['inp'], dtype)
    return torch.stack(R.slot_scores(t['s_mask'][0], t['s_feat'][0], t['boxes'][0], t['bank_mask'][0], t['bank_feature'][0], t['bank_box'][0]), 1)


def _step(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


@functools.lru_cache(maxsize=None)
def threshold_settings():
    """name -> (thresholds, slot, whether the slot passes): per predicate, everything else wide open, the threshold on the fp32 score of
    one slot and one ulp inside or outside of it."""
    s = exact_scores().numpy()
    out = {'wide': (dict(WIDE), None, None)}
    for key, col, slot in (('fg_iou_thresh', 0, 0), ('bg_iou_thresh', 1, 3), ('appear_thresh', 2, 5)):
        v = float(s[slot, col])
        out[f'{key}_equal'] = (dict(WIDE, **{key: v}), slot, False)
        out[f'{key}_ulp_below'] = (dict(WIDE, **{key: _step(v, False)}), slot, True)
    for slot in (0, 4):
        v = float(s[slot, 3])
        out[f'ratio{slot}_equal'] = (dict(WIDE, ratio_range=[v, v]), slot, True)
        out[f'ratio{slot}_lo_inward'] = (dict(WIDE, ratio_range=[_step(v, True), float('inf')]), slot, False)
        out[f'ratio{slot}_hi_inward'] = (dict(WIDE, ratio_range=[float('-inf'), _step(v, False)]), slot, False)
    return out


def exact_passing(th, zero_query=False):
    """The slots that pass under thresholds ``th``: the restatement's predicate on its fp32 scores."""
    s = exact_scores(zero_query=zero_query)
    return torch.where(R.passing(tuple(s[:, k] for k in range(4)), th))[0].tolist()


# ---- stand-alone entry points ----------------------------------------------------------------------------------------------------------------
SUPERRES_KS = (1, 8)
ONEHOT = ((0, 48), (24, 10), (6, 0), (48, 48))      # (source cell, target cell) of the one-hot planes
SOLVE_KS, SOLVE_CS = (1, 8), (1, 4, 15, 16, 17)
SOLVE_RUNS = tuple((K, C, False) for K in SOLVE_KS for C in SOLVE_CS) + ((3, 17, True),)
SOLVE_ZERO = (2, 4)


@functools.lru_cache(maxsize=None)
def superres_T(K):
    return R.half(np.random.RandomState(6000 + K).random_sample((K, 49, 49)))


@functools.lru_cache(maxsize=None)
def superres_want(K, dtype='float64'):
    return R.superres(torch.from_numpy(superres_T(K)).to(getattr(torch, dtype)))


def onehot_T():
    T = np.zeros((len(ONEHOT), 49, 49), np.float32)
    for k, (p, q) in enumerate(ONEHOT):
        T[k, p, q] = 1
    return T


@functools.lru_cache(maxsize=None)
def solve_inputs(K, C, zero):
    """(f0 [1,C,7,7], f1 [K,C,7,7], upstream dCu [K,49,49]): strictly positive features (no cell is zero unless ``zero`` plants one)."""
    rng = np.random.RandomState(7000 + 100 * K + C + (50 if zero else 0))
    f0, f1 = R.half(0.05 + rng.random_sample((1, C, 7, 7))), R.half(0.05 + rng.random_sample((K, C, 7, 7)))
    if zero:
        f0[0, :, SOLVE_ZERO[0], SOLVE_ZERO[1]] = 0
    return f0, f1, R.half(rng.standard_normal((K, 49, 49)))


@functools.lru_cache(maxsize=None)
def solve_want(K, C, zero, dtype='float64'):
    """(Cu, d sum(Cu dCu) / d f0) by autograd through ``R.solve`` at the fixture's settings."""
    dt = getattr(torch, dtype)
    f0, f1, g = (torch.from_numpy(a).to(dt) for a in solve_inputs(K, C, zero))
    f0.requires_grad_(True)
    Cu, _ = R.solve(f0[0], f1, CFG)
    return Cu.detach(), torch.autograd.grad((Cu * g).sum(), f0)[0]


def superres_tol(K):
    """The fp32 restatement against the fp64 one on the same T."""
    return rel(superres_want(K, 'float32'), superres_want(K))


def solve_tol(run):
    """The same for the gradient of one run.  Not pooled: at C = 1 the gradient is what is left of 1 / d - f^2 / (n d^2) with d = n + 1e-4
    rounded to fp32, and fp32 loses a hundred times more there than in any other run."""
    return rel(solve_want(*run, 'float32')[1], solve_want(*run)[1])
