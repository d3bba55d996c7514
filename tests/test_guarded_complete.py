"""Host side of the guarded tests: the helper itself (tests/guarded.py) does what it says.  Which entry point is run guarded by
which test, or exempt for which reason, is checked in tests/test_abi_families.py.  No GPU needed."""
import pytest
import torch

from tests import guarded as G


@pytest.mark.parametrize('dtype,lead', [(torch.float32, 0), (torch.float32, 3), (torch.float64, 1), (torch.int32, 1), (torch.int64, 1), (torch.uint8, 15)])
def test_embed_places_the_view_and_the_poison(dtype, lead):
    t = (torch.arange(24) % 7).to(dtype).view(2, 3, 4)
    g = G.embed(t, lead, 128)
    assert g.t.is_contiguous() and g.t.shape == t.shape and g.t.storage_offset() == 128 + lead and torch.equal(g.t, t)
    assert g.backing.numel() == 128 + lead + 24 + 128
    assert (g.ptr() - g.backing.data_ptr()) == (128 + lead) * t.element_size()
    lo, hi = g.backing[:128 + lead], g.backing[128 + lead + 24:]
    if dtype.is_floating_point:
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    elif dtype == torch.uint8:
        assert bool((lo == 255).all()) and bool((hi == 255).all())
    else:
        assert bool((lo == -1).all()) and bool((hi == -1).all())           # -1: range checks reject it, as an offset it stays in the band
    G.check_bands(g)
    G.check_unchanged(g)
    g.t.view(-1)[5] += 1
    with pytest.raises(AssertionError, match='modified'):
        G.check_unchanged(g)
    g.backing[128 + lead - 1] = 0
    with pytest.raises(AssertionError, match='outside'):
        G.check_bands(g)
    with pytest.raises(AssertionError):
        G.embed(t, 16 // t.element_size(), 128)                           # below 16 bytes only
    with pytest.raises(AssertionError):
        G.embed(t, 0, 100)                                                # bands are multiples of 64 elements


def test_outputs_carry_the_pattern_until_written():
    for dtype, bits in ((torch.float32, 0x7FC5A5A5), (torch.int32, 0x5A5A5A5A), (torch.uint8, 0xA5)):
        g = G.out((3, 5), dtype, 'cpu', 1, 64)
        iv = g.backing if dtype != torch.float32 else g.backing.view(torch.int32)
        assert bool((iv == bits).all())
        G.check_bands(g)
        with pytest.raises(AssertionError):
            G.check_written(g)
        g.t.fill_(1)
        G.check_written(g)
        g.t[1, 2] = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32) if dtype == torch.float32 else bits
        with pytest.raises(AssertionError):
            G.check_written(g)                                             # one element left (a 0xA5 byte is not a 0 / 1 mask value)
        g.t.fill_(0)
        g.backing[g.start + g.numel] = 0
        with pytest.raises(AssertionError, match='band after'):
            G.check_bands(g)
    assert G.plane_band(24, 40, 4) == 1216 and G.plane_band(4, 4) == 1024 and G.plane_band(336, 304, 2) % 64 == 0


def test_poisoned_empty_patches_and_restores():
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    base = torch.zeros(4)
    with G.poisoned_empty():
        a, b, c = torch.empty(5), torch.empty_like(base), base.new_empty((2, 2), dtype=torch.int32)
        d, e = torch.empty((3,), dtype=torch.uint8), torch.empty(0)
        assert bool((a.view(torch.int32) == G.PATTERN_F32).all()) and bool((b.view(torch.int32) == G.PATTERN_F32).all())
        assert bool((c == 0x5A5A5A5A).all()) and bool((d == 0xA5).all()) and e.numel() == 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    with pytest.raises(ZeroDivisionError):
        with G.poisoned_empty():
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real


def test_same_ptr_ok_and_stream(monkeypatch):
    for dtype, ibits in ((torch.float32, torch.int32), (torch.float64, torch.int64)):
        quiet = torch.tensor([1.0, float('nan'), 0.0], dtype=dtype)
        payload = quiet.clone()
        payload.view(ibits)[1] += 1                                        # still a NaN, another payload
        assert bool(torch.isnan(payload[1])) and G.same(quiet, quiet.clone()) and not G.same(quiet, payload)
        assert not torch.equal(quiet, quiet.clone())                       # by value a NaN equals nothing: same() is the stricter and the usable one
        zero, minus = torch.tensor([0.0], dtype=dtype), torch.tensor([-0.0], dtype=dtype)
        assert torch.equal(zero, minus) and not G.same(zero, minus) and G.same(minus, minus.clone())
    half = torch.tensor([0.0, 1.5], dtype=torch.float16)
    assert G.same(half, half.clone()) and not G.same(half, -half) and not G.same(half, half.float()) and not G.same(half.float(), half.double())
    wide = torch.arange(12, dtype=torch.float32).view(3, 4)
    assert G.same(wide.t(), wide.t().contiguous()) and not G.same(wide, wide[:, :3])                 # views count by their elements
    ints = torch.tensor([3, -1, 7])
    assert G.same(ints, ints.clone()) and not G.same(ints, ints + 1) and G.same(ints > 0, torch.tensor([True, False, True]))
    t = torch.zeros(5)
    g = G.embed(t, 1, 64)
    assert G.ptr(None) is None and G.ptr(t) == t.data_ptr() and G.ptr(g) == g.ptr() == g.backing.data_ptr() + 65 * 4
    G.ok(0)
    with pytest.raises(AssertionError, match='BXI_ERR_WORKSPACE'):
        G.ok(-5)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev: type('S', (), {'cuda_stream': (dev, 77)}))
    assert G.stream('cuda:1') == ('cuda:1', 77)
