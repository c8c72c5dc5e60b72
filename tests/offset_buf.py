"""Tensors at a chosen 4-byte offset inside guard bands (tests/test_offset_launches_host.py, tests/test_offset_launches.py).

Every tensor the other launch suites hand a kernel is a fresh allocation: its start is a multiple of 256 bytes and behind it
lies allocator slack that nobody inspects.  Training hands the kernels views that start anywhere (ops.SplitBatch: x[n:]).
The helpers here put a tensor `off` elements past a 16-byte boundary in the middle of ONE larger buffer:

    [ guard | off | payload (t.numel()) | guard ]        buffer start % 16 == 0, payload start % 16 == 4 * off

Inputs (`embed`): everything around the payload is NaN (fp32) or -1 (int32 mask words), so a kernel that stages a whole
16-byte group or a whole row or plane past either end of the tensor poisons its result.  Outputs (`out_like`): guards AND
payload hold a sentinel bit pattern, a NaN with a payload (0x7FC0BEEF), compared as int32: `guards_intact` finds a store one
element outside the tensor, `unwritten` a payload element the launch never stored.  The guards lie inside the allocation the
test made, so no such error can fault.  Plain torch; nothing here needs a GPU."""
import torch

# quiet NaN with a payload: no kernel of the library produces these bits (arithmetic NaNs are 0x7FC00000 / 0xFFC00000)
SENTINEL = 0x7FC0BEEF
NAN_BITS = 0x7FC00000
OFFSETS = (0, 1, 2, 3)          # elements: every residue data_ptr() % 16 a 4-byte tensor can have
_ITEM = {torch.float32: 4, torch.int32: 4}


def guard_for(shape):
    """Guard elements per side for a tensor of `shape` (..., H, W): two planes, so a whole-row or whole-plane overrun lands
    in it, and never fewer than 64."""
    hw = int(shape[-1]) * (int(shape[-2]) if len(shape) > 1 else 1)
    return _up4(max(64, 2 * hw + 8))


def _up4(guard):
    """Guards are whole 16-byte groups, so that the payload's residue is exactly 4 * off."""
    return (int(guard) + 3) // 4 * 4


def _buffer(n, dtype, device, bits):
    assert dtype in _ITEM, dtype
    buf = torch.empty(n, dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0, "allocation at %#x is not 16-byte aligned" % buf.data_ptr()
    buf.view(torch.int32).fill_(bits)
    return buf


def _place(buf, shape, off, guard, numel, fill_bits):
    start = guard + off
    view = buf[start:start + numel].view(tuple(shape))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * start
    view._offset_buf = (buf, start, numel, fill_bits)   # keeps the buffer alive and tells guards_intact where the guards are
    return view


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def embed(t, off, guard=None, device=None):
    """The contiguous view of t's shape that starts guard + off elements into a fresh 16-byte aligned buffer of
    guard + off + t.numel() + guard elements (guard rounded up to a multiple of 4) and holds t's values; everything else is
    NaN (fp32) or -1 (int32)."""
    assert 0 <= off <= 3
    guard = guard_for(t.shape) if guard is None else _up4(guard)
    device = t.device if device is None else device
    n = t.numel()
    bits = NAN_BITS if t.dtype == torch.float32 else -1
    buf = _buffer(guard + off + n + guard, t.dtype, device, bits)
    view = _place(buf, t.shape, off, guard, n, bits)
    view.copy_(t.detach())
    assert view.data_ptr() % 16 == 4 * off
    return view


def out_like(shape, dtype, off, guard=None, device="cpu"):
    """embed's layout for an output: guards and payload filled with SENTINEL."""
    assert 0 <= off <= 3
    shape = tuple(int(v) for v in shape)
    guard = guard_for(shape) if guard is None else _up4(guard)
    n = _numel(shape)
    buf = _buffer(guard + off + n + guard, dtype, device, SENTINEL)
    view = _place(buf, shape, off, guard, n, SENTINEL)
    assert view.data_ptr() % 16 == 4 * off
    return view


def residue(t):
    return t.data_ptr() % 16


def guards_intact(view):
    """Both guards of a view made by embed / out_like still hold their fill, bit for bit."""
    buf, start, n, bits = view._offset_buf
    words = buf.view(torch.int32)
    return bool((words[:start] == bits).all()) and bool((words[start + n:] == bits).all())


def unwritten(view):
    """Number of payload elements of an out_like view that still hold the sentinel bits."""
    return int((view.reshape(-1).view(torch.int32) == SENTINEL).sum())


def assert_written(view, what):
    """After a launch: guards bit-intact, no payload element NaN or still the sentinel."""
    assert guards_intact(view), what + ": a guard band around the output was written"
    assert unwritten(view) == 0, what + ": %d output elements were never stored" % unwritten(view)
    if view.dtype == torch.float32:
        assert not bool(torch.isnan(view).any()), what + ": NaN in the output (a guard value of an input was read)"
