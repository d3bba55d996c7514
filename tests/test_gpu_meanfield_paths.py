"""GPU: every instantiation of MeanField's per-item kernels (csrc/meanfield.hip), every decided label exact.

bxi_meanfield_forward_f32 runs four (instance, row, segment) items per wave when there are more than _lib.MF_MANY_ITEMS of them and one
otherwise.  The inputs of tests/mf_decided.py::CASES lie on the many-item side (33000 items with one segment per row and a 5x5 kernel;
32970 with three segments, 471 per instance -- no multiple of 16, so waves straddle rows and the last workgroup is partly filled; 33150
with W exactly one word), one stays small, and one sits on the threshold: 128 instances of 256x64 are exactly MF_MANY_ITEMS items, 129
are 256 more.  The kernel values are the oracle's on both sides (as in tests/test_gpu_discobox.py), the instances are spread over two
kernel planes by img_inds, targets are given as uint8 and as float.

Expected labels: oracle/discobox_oracle.py along tests/mf_decided.py::trajectory.  No allowance: a label may differ from the oracle's only
where one of the two corner evaluations differs (tests/test_host_meanfield_decided.py prints the counts: none on these inputs)."""
import numpy as np
import pytest
import torch

from oracle import discobox_oracle as do
from tests import mf_decided as M

pytestmark = pytest.mark.gpu
f32 = np.float32
MANY = [k for k in M.CASES if k != 'k5_small']


def _runner(dev, d, float_targets=False, sel=slice(None)):
    """run(x, iters) -> (ret, valid) as numpy arrays: meanfield_forward on the instances `sel` of case d; everything but x uploaded once."""
    from boxinstseg_amd import meanfield_forward
    Kd = torch.tensor(d['Ko']).to(dev)                 # torch.tensor: the shared arrays are read-only
    t = torch.tensor(d['t'][sel]).to(dev)
    t = t.float() if float_targets else t
    img = torch.tensor(d['img'][sel]).to(dev)
    inter = None if d['inter'] is None else torch.tensor(d['inter'][sel]).to(dev)

    def run(x, iters):
        ret, valid = meanfield_forward(Kd, torch.tensor(x).to(dev), t, iters, d['base'], img_inds=img,
                                       inter_img_mask=inter, gamma=d['gamma'])
        return ret.cpu().numpy(), valid.cpu().numpy()
    return run


def _items(d, n=None):
    return (d['n'] if n is None else n) * d['H'] * ((d['W'] + 63) // 64)


@pytest.fixture(scope='module')
def many_items(built):
    """The threshold the library was built with is the one the tests count against."""
    from boxinstseg_amd import _lib
    assert M.hip_many_items() == _lib.MF_MANY_ITEMS
    return _lib.MF_MANY_ITEMS


@pytest.mark.parametrize('targets', ['u8', 'f32'])
@pytest.mark.parametrize('name', list(M.CASES))
def test_every_step_and_the_whole_call(dev, many_items, name, targets):
    d = M.case(name)
    assert (_items(d) > many_items) == (name in MANY), f'{name}: {_items(d)} items are on the wrong side of {many_items}'
    run = _runner(dev, d, float_targets=targets == 'f32')
    M.assert_steps(run, d['t'], d['states'], d['undecided'], name)
    assert not any(u.any() for u in d['undecided'])              # so the whole call is pinned on every pixel
    M.assert_labels(run, d['x'], d['t'], d['states'], d['undecided'], name)


@pytest.mark.parametrize('name', MANY)
def test_many_items_equal_two_small_halves(dev, many_items, name):
    """Four items per wave against one: the same instances in two calls that each stay at or below the threshold."""
    d = M.case(name)
    half = d['n'] // 2
    assert _items(d) > many_items >= _items(d, d['n'] - half) >= _items(d, half)
    ret, valid = _runner(dev, d)(d['x'], d['iters'])
    for sel in (slice(0, half), slice(half, d['n'])):
        r, v = _runner(dev, d, sel=sel)(d['x'][sel], d['iters'])
        assert np.array_equal(r, ret[sel]) and np.array_equal(v, valid[sel]), (name, sel)


@pytest.mark.parametrize('name', M.FULL)
def test_every_item_is_written(dev, many_items, name):
    """x = 1 under a target that covers every map stays all-set (tests/mf_decided.py::full_case): an item that a four-per-wave launch leaves
    out -- the tail of a wave, of the last workgroup, a row that a wave straddles -- is a word of zeros in ret."""
    d = M.full_case(name)
    assert _items(d) > many_items and all(s.all() for s in d['states'])
    run = _runner(dev, d)
    for iters in (1, 2):
        ret, valid = run(d['x'], iters)
        assert ret.dtype == np.float32 and (ret == 1).all(), f'{name}: {int((ret != 1).sum())} labels not set after {iters} step(s)'
        assert not valid.any()
    M.assert_steps(run, d['t'], d['states'], d['undecided'], name)


def test_both_sides_of_the_threshold(dev, many_items):
    """128 instances of 256x64 are exactly MF_MANY_ITEMS items (one per wave); one more instance and the call runs four per wave."""
    d = M.case('k3_threshold')
    assert (d['n'], d['H'], d['W']) == (129, 256, 64)
    assert _items(d, 128) == many_items and _items(d) == many_items + 256 == 33024
    few, few_valid = _runner(dev, d, sel=slice(0, 128))(d['x'][:128], d['iters'])
    many, many_valid = _runner(dev, d)(d['x'], d['iters'])
    assert few.tobytes() == many[:128].tobytes() and few_valid.tobytes() == many_valid[:128].tobytes()
    assert np.array_equal(many, d['states'][-1].astype(f32)) and np.array_equal(many_valid, d['valid'])


def _planted(H, W, counts, order):
    """x [len(counts),H,W] with the first counts[i] pixels of `order` (flat indices) set to 1."""
    x = np.zeros((len(counts), H * W), f32)
    for i, c in enumerate(counts):
        x[i, order[:c]] = 1.0
    return x.reshape(len(counts), H, W)


@pytest.mark.parametrize('targets', ['u8', 'f32'])
def test_valid_at_its_edges(dev, targets):
    """valid = 0.05 * HW <= count <= 0.95 * HW with iters = 0, where the state is exactly the planted x * t > 0.5."""
    from boxinstseg_amd import meanfield_forward

    def run(x, t):
        H, W = x.shape[1:]
        K = torch.zeros(1, 9, H, W, device=dev)
        td = torch.from_numpy(t).to(dev)
        ret, valid = meanfield_forward(K, torch.from_numpy(x).to(dev), td.float() if targets == 'f32' else td, 0, 0.1)
        want, wv = do.meanfield_forward(np.zeros((9, H, W), f32), x, t, 0, 0.1)
        assert np.array_equal(ret.cpu().numpy(), want) and np.array_equal(want, ((x * t) > 0.5).astype(f32))
        assert np.array_equal(valid.cpu().numpy(), wv)
        assert want.sum((1, 2)).tolist() == [float(c) for c in counts]
        return valid.cpu().numpy().tolist()

    # 20 x 20: the bounds are exactly 20 and 380
    counts = [19, 20, 21, 379, 380, 381, 380, 381, 0, 400]
    x = _planted(20, 20, counts[:6], np.arange(400)[::-1])              # from the last pixel backwards
    x = np.concatenate([x, np.ones((2, 20, 20), f32), np.full((1, 20, 20), 0.5, f32), np.ones((1, 20, 20), f32)])
    t = np.ones((10, 20, 20), np.uint8)
    t[6].reshape(-1)[:20] = 0; t[7].reshape(-1)[:19] = 0                # x = 1 everywhere: the target decides the count
    assert run(x, t) == [0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    # 37 x 65: the bounds are 120.25 and 2284.75; two words per row, the second holds column 64 alone.  Column 64 is filled first.
    idx = np.arange(37 * 65).reshape(37, 65)
    order = np.concatenate([idx[:, 64], idx[:, :64].reshape(-1)])
    counts = [120, 121, 2284, 2285, 37]
    x = _planted(37, 65, counts, order)
    assert x[:, :, 64].all() and x[4, :, :64].sum() == 0
    assert run(x, np.ones((5, 37, 65), np.uint8)) == [0.0, 1.0, 1.0, 0.0, 0.0]
