"""Guard bands around test buffers: does a kernel touch only the memory it was given?

`guarded(shape, dtype, device, fill)` allocates ONE flat buffer laid out as

    [front guard | interior | back guard]

and returns `(view, checker)`.  `view` is the interior as a contiguous tensor of `shape` / `dtype` (it shares the buffer's
storage, so the guards live as long as it does); `checker()` synchronises and asserts that both guards still hold the bits
they were filled with, naming the first and last offending byte relative to the interior's first byte.

The whole buffer -- guards AND interior -- starts out holding `fill`.  An input is then copied into the interior
(`view.copy_(data)`); an output whose every element the contract says is written keeps the fill in its interior too, so a
fill value left in a result is an element that was never written (`poisoned()`).

Fills (`POISON`): NaNs with the sign bit and a non-canonical payload, so that even an atomic "+0" past the end changes the
bits; 0xA5 bytes for integers.  A number as `fill` fills with that value instead (index guards that are safe to dereference,
+-3e38 around min / max inputs, where a NaN would be lost in the comparisons).
"""
import torch

GUARD_BYTES = 4096   # per side: >= 4 KiB and a multiple of 256 bytes
ALIGN = 256          # the interior starts where the caching allocator would start a block

POISON_BITS = {
    torch.float32: 0xFFA5A5A5,
    torch.float64: 0xFFF5A5A5A5A5A5A5,
    torch.bfloat16: 0xFFA5,
    torch.float16: 0xFDA5,
}
_SAME_WIDTH_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(bits: int, nbytes: int) -> int:
    return bits - (1 << (8 * nbytes)) if bits >= 1 << (8 * nbytes - 1) else bits


def poison_bits(dtype: torch.dtype) -> int:
    """The poison of `dtype` as an unsigned bit pattern of its width."""
    size = torch.empty((), dtype=dtype).element_size()
    if dtype in POISON_BITS:
        return POISON_BITS[dtype]
    return int.from_bytes(b'\xa5' * size, 'little')


def big_value(dtype: torch.dtype, sign: int = 1):
    """A value that wins a max (sign = +1) / min (sign = -1) against any test data: +-3e38, the largest finite value of a
    16-bit float, the extreme of an integer type."""
    if dtype in (torch.float16, torch.bfloat16):
        return sign * torch.finfo(dtype).max
    if dtype.is_floating_point:
        return sign * 3e38
    return torch.iinfo(dtype).max if sign > 0 else torch.iinfo(dtype).min


def _fill_(flat: torch.Tensor, dtype: torch.dtype, fill) -> None:
    """Fill the byte tensor `flat` (a whole number of `dtype` elements) with the poison (fill None) or the value `fill`."""
    size = torch.empty((), dtype=dtype).element_size()
    if fill is None:
        flat.view(_SAME_WIDTH_INT[size]).fill_(_signed(poison_bits(dtype), size) if size > 1 else poison_bits(dtype))
    else:
        flat.view(dtype).fill_(fill)


def guarded(shape, dtype: torch.dtype, device, fill=None, guard: int = GUARD_BYTES):
    """Returns (interior view, checker).  `fill` None = the dtype's poison, else a value (see the module docstring)."""
    assert guard >= 4096 and guard % ALIGN == 0
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    size = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    nbytes = n * size
    raw = torch.empty(guard + ALIGN + nbytes + guard, dtype=torch.uint8, device=device)
    # the caching allocator hands out 512-byte aligned blocks (pad 0); the CPU allocator may not
    pad = (-raw.data_ptr()) % ALIGN
    front = guard + pad
    buf = raw[:front + nbytes + guard]
    # front guard, interior and back guard in dtype units (the pad is a multiple of the allocator's alignment, hence of `size`)
    _fill_(buf, dtype, fill)
    view = buf[front:front + nbytes].view(dtype).view(shape)
    want_front = buf[:front].clone()
    want_back = buf[front + nbytes:].clone()
    assert view.data_ptr() % ALIGN == 0

    def checker(what: str = 'buffer') -> None:
        if buf.is_cuda:
            torch.cuda.synchronize(buf.device)
        bad = []
        diff = torch.nonzero(buf[:front] != want_front).flatten()
        if diff.numel():
            bad += [int(diff[0]) - front, int(diff[-1]) - front]
        diff = torch.nonzero(buf[front + nbytes:] != want_back).flatten()
        if diff.numel():
            bad += [nbytes + int(diff[0]), nbytes + int(diff[-1])]
        assert not bad, (f'{what}: guard band changed -- offending bytes {min(bad)} ... {max(bad)} relative to the interior '
                         f'({nbytes} bytes, {shape} {dtype})')

    checker.raw = buf
    checker.nbytes = nbytes
    return view, checker


def guarded_copy(data: torch.Tensor, device, fill=None):
    """An input in a guarded buffer: `data` copied into the interior; guards hold `fill`."""
    view, check = guarded(tuple(data.shape), data.dtype, device, fill)
    view.copy_(data)
    return view, check


def poisoned(t: torch.Tensor) -> torch.Tensor:
    """Mask of the elements of `t` that still hold their dtype's poison bit pattern (= never written)."""
    size = t.element_size()
    bits = t.detach().contiguous().view(_SAME_WIDTH_INT[size])
    if size == 1:
        return bits == poison_bits(t.dtype)
    return bits == _signed(poison_bits(t.dtype), size)


def assert_no_poison(t: torch.Tensor, what: str = 'output') -> None:
    m = poisoned(t)
    if bool(m.any()):
        idx = torch.nonzero(m.flatten()).flatten()
        raise AssertionError(f'{what}: {idx.numel()} of {t.numel()} elements never written (first flat index {int(idx[0])}, '
                             f'last {int(idx[-1])})')
