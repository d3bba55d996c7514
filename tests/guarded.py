"""Guard bands, poisoned scratch and misaligned views for the GPU tests (a plain module, no fixtures).

Every tensor the other tests hand to a kernel is a fresh block of torch's caching allocator: 512-byte aligned, rounded up, with slack
behind it, often still holding the previous call's (right) answer.  The helpers here take that comfort away:

  embed(t, lead, band)           an input as a contiguous view that starts `band + lead` elements into ONE flat backing tensor whose
                                 every other element is poison: quiet NaN for floats, -1 for integers (range checks reject it; used
                                 as a raw offset it stays inside the band).  `band` is a multiple of 64 elements, so `lead` alone sets
                                 the misalignment of the data pointer -- never below the element's natural alignment.
  out(shape, dtype, dev, ...)    an output / "contents undefined" scratch the same way, bands AND interior filled with a recognisable
                                 bit pattern (a NaN with a fixed payload, 0xA5 bytes, 0x5A5A5A5A words).
  check_bands(g)                 both bands still hold the poison, bit for bit: nothing was stored outside the tensor.
  check_written(g)               no float / int32 element of the interior still carries the pattern; a uint8 mask is 0 / 1 only.
  check_unchanged(g)             an input's interior is bit-identical to what went in.
  stream(dev), ptr(x), ok(rc)    what a direct library call needs: the current stream's handle, the address of None / a Guarded / a
                                 tensor, and `rc == 0` with the status' name.
  same(got, want)                bit-for-bit equality: NaN payloads and signed zeros count, for every float width.
  poisoned_empty()               torch.empty / torch.empty_like / Tensor.new_empty hand out pattern-filled memory for the duration:
                                 a kernel that leaves an element of its output unwritten, or that depends on what it finds in its
                                 scratch, cannot hide behind a block the allocator recycled.

`band` is sized (plane_band) so that an over-run of up to one plane, or of one (D+1)-row tap offset, lands in the band -- inside the
test's own allocation.  That is what keeps these tests harmless even when a kernel is wrong.

What a guard band CANNOT see: a load outside the tensor whose value is selected away afterwards (it reads poison and drops it), and a
store beyond the band.  A NaN band catches an out-of-bounds load only if the value reaches an output.
"""
from __future__ import annotations

import contextlib

import torch

# bit patterns (as the integer type of the same width)
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NAN_BITS = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000, torch.float64: 0x7FF8000000000000}
_PATTERN_NAN = {torch.float16: 0x7EA5, torch.bfloat16: 0x7FA5, torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5}
_PATTERN_INT = {torch.uint8: 0xA5, torch.int8: 0x5A, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
PATTERN_F32 = 0x7FC5A5A5


def pattern_bits(dtype: torch.dtype) -> int:
    """The 'nobody wrote this' bit pattern of outputs and scratch."""
    if dtype in _PATTERN_NAN:
        return _PATTERN_NAN[dtype]
    if dtype in _PATTERN_INT:
        return _PATTERN_INT[dtype]
    raise TypeError(f'no pattern for {dtype}')


def input_poison_bits(dtype: torch.dtype) -> int:
    """What surrounds an input: quiet NaN for floats, -1 for integers (0xFF for uint8)."""
    if dtype in _NAN_BITS:
        return _NAN_BITS[dtype]
    if dtype == torch.uint8:
        return 0xFF
    if dtype in _PATTERN_INT:
        return -1
    raise TypeError(f'no poison for {dtype}')


def _as_int(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) else t.view(_INT_VIEW[t.element_size()])


def fill_bits(t: torch.Tensor, bits: int) -> torch.Tensor:
    if t.numel():
        if t.dtype == torch.bool:
            t.fill_(True)
        else:
            v = _as_int(t)
            if v.dtype != torch.uint8 and bits >= 1 << (8 * v.element_size() - 1):
                bits -= 1 << (8 * v.element_size())              # two's complement of the same bits
            v.fill_(bits)
    return t


def plane_band(H: int, W: int, D: int = 0, floor: int = 1024) -> int:
    """Band (elements, a multiple of 64) that holds an over-run of one H x W plane or of one (D+1)-row tap offset."""
    n = max(floor, H * W + (D + 1) * (W + 1))
    return (n + 63) // 64 * 64


class Guarded:
    """A tensor inside its guard bands.  `.t` is the view the kernel gets."""

    def __init__(self, backing: torch.Tensor, shape, lead: int, band: int, bits: int, is_input: bool):
        numel = 1
        for s in shape:
            numel *= int(s)
        self.backing, self.lead, self.band, self.bits, self.is_input = backing, lead, band, bits, is_input
        self.start, self.numel = band + lead, numel
        self.t = backing[self.start:self.start + numel].view(tuple(shape))
        self.before = None

    def ptr(self) -> int:
        return self.t.data_ptr()

    def interior(self) -> torch.Tensor:
        return self.backing[self.start:self.start + self.numel]


def _check_args(dtype: torch.dtype, lead: int, band: int) -> None:
    size = torch.empty((), dtype=dtype).element_size()
    assert band % 64 == 0 and band > 0, 'band must be a positive multiple of 64 elements'
    assert 0 <= lead and lead * size < 16, f'lead {lead} of {dtype}: offsets of 0..15 bytes only'


def embed(t: torch.Tensor, lead: int = 0, band: int = 1024, poison: int | None = None) -> Guarded:
    """`t` (any device tensor) as a contiguous view at element `band + lead` of a poisoned backing tensor of its dtype."""
    _check_args(t.dtype, lead, band)
    bits = input_poison_bits(t.dtype) if poison is None else poison
    backing = torch.zeros(band + lead + t.numel() + band, dtype=t.dtype, device=t.device)
    fill_bits(backing, bits)
    g = Guarded(backing, t.shape, lead, band, bits, True)
    g.t.copy_(t)
    g.before = g.interior().clone()
    assert g.t.is_contiguous() and g.t.storage_offset() == band + lead
    assert g.ptr() % backing.element_size() == 0 and (g.ptr() - backing.data_ptr()) == (band + lead) * backing.element_size()
    return g


def out(shape, dtype: torch.dtype, device, lead: int = 0, band: int = 1024) -> Guarded:
    """An output or a scratch buffer: bands and interior hold pattern_bits(dtype)."""
    _check_args(dtype, lead, band)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    numel = 1
    for s in shape:
        numel *= int(s)
    backing = torch.zeros(band + lead + numel + band, dtype=dtype, device=device)
    bits = pattern_bits(dtype)
    fill_bits(backing, bits)
    return Guarded(backing, shape, lead, band, bits, False)


def _sync() -> None:
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _same_bits(t: torch.Tensor, bits: int) -> torch.Tensor:
    v = _as_int(t)
    if v.dtype != torch.uint8 and bits >= 1 << (8 * v.element_size() - 1):
        bits -= 1 << (8 * v.element_size())
    return v == bits


def check_bands(*gs: Guarded) -> None:
    _sync()
    for g in gs:
        lo, hi = g.backing[:g.start], g.backing[g.start + g.numel:]
        bad_lo, bad_hi = int((~_same_bits(lo, g.bits)).sum()), int((~_same_bits(hi, g.bits)).sum())
        assert bad_lo == 0 and bad_hi == 0, \
            f'stores outside the tensor: {bad_lo} elements of the band before, {bad_hi} of the band after (shape {tuple(g.t.shape)}, lead {g.lead})'


def check_written(*gs: Guarded) -> None:
    _sync()
    for g in gs:
        assert not g.is_input
        body = g.interior()
        if body.dtype == torch.uint8:
            left = int((body > 1).sum())
            assert left == 0, f'{left} bytes of a 0/1 mask of shape {tuple(g.t.shape)} are neither 0 nor 1 (unwritten?)'
        else:
            left = int(_same_bits(body, g.bits).sum())
            assert left == 0, f'{left} of {g.numel} elements of an output of shape {tuple(g.t.shape)} were never written'


def check_unchanged(*gs: Guarded) -> None:
    _sync()
    for g in gs:
        assert g.is_input and g.before is not None
        assert torch.equal(_as_int(g.interior()), _as_int(g.before)), f'an input of shape {tuple(g.t.shape)} was modified'


def stream(dev) -> int:
    """The handle of the current stream of `dev`, as the entry points take it."""
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(x):
    """The address a library call gets for None, a Guarded or a tensor."""
    return None if x is None else x.ptr() if isinstance(x, Guarded) else x.data_ptr()


def ok(rc: int) -> None:
    from boxinstseg_amd import _lib
    assert rc == 0, _lib.STATUS.get(rc, rc)


def same(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit: floats of any width through their integer view, so that NaN payloads and signed zeros count; the rest by torch.equal."""
    if got.is_floating_point() or want.is_floating_point():
        return got.dtype == want.dtype and torch.equal(_as_int(got.contiguous()), _as_int(want.contiguous()))
    return torch.equal(got, want)


@contextlib.contextmanager
def poisoned_empty():
    """torch.empty / torch.empty_like / Tensor.new_empty return pattern-filled tensors inside the block (restored on exit, also on error)."""
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def _poison(t):
        if isinstance(t, torch.Tensor) and t.numel() and (t.dtype in _PATTERN_NAN or t.dtype in _PATTERN_INT):
            with torch.no_grad():
                fill_bits(t.detach(), pattern_bits(t.dtype))
        return t

    def empty(*a, **k):
        return _poison(real_empty(*a, **k))

    def empty_like(*a, **k):
        return _poison(real_like(*a, **k))

    def new_empty(self, *a, **k):
        return _poison(real_new(self, *a, **k))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_like, real_new
