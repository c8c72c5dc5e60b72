"""Tensors at a chosen 4-byte offset inside guard bands (tests/test_offset_launches_host.py, tests/test_offset_launches.py).

Every tensor the other launch suites hand a kernel is a fresh allocation: its start is a multiple of 256 bytes and behind it
lies allocator slack that nobody inspects.  Training hands the kernels views that start anywhere (ops.SplitBatch: x[n:]).
The helpers here put a tensor `off` elements past a 16-byte boundary in the middle of ONE larger buffer:

    [ guard | off | payload (t.numel()) | guard ]        buffer start % 16 == 0, payload start % 16 == 4 * off

Inputs (`embed`): everything around the payload is NaN (fp32) or -1 (int32 mask words), so a kernel that stages a whole
16-byte group or a whole row or plane past either end of the tensor poisons its result.  Outputs (`out_like`): guards AND
payload hold a sentinel bit pattern, a NaN with a payload (0x7FC0BEEF), compared as int32: `guards_intact` finds a store one
element outside the tensor, `unwritten` a payload element the launch never stored.  The guards lie inside the allocation the
test made, so no such error can fault.  Plain torch; nothing here needs a GPU.

Byte tensors (uint8 volumes and masks, int8 directions; tests/test_byte_offset_launches.py) have the same layout in bytes:

    [ guard | off | payload (t.numel() bytes) | guard ]   buffer start % 16 == 0, payload start % 16 == off % 16

with off in BYTE_OFFSETS - every residue mod 4 and two starts that are odd mod 8 and mod 16 - and a guard of at least two
planes (2 * H * W * 3 bytes) and never fewer than 64 bytes per side.  A byte has no NaN, so the rule is a pair of runs:
  inputs  (`embed_u8`): every launch runs once with the guards 0x00 and once with 0xFF (BYTE_FILLS) and BOTH results must equal
          the exact reference - a byte read outside [p, p + n) that reaches a result cannot pass both;
  outputs (`out_like_u8`): guards and payload hold a sentinel byte, the launch runs with both of BYTE_SENTINELS, the guards must
          be bit-intact after each (`guards_intact`) and BOTH payloads must equal the reference - a byte never stored holds 0x5A in
          one run and 0xA5 in the other.
`byte_rule` is that pair of runs as one function, for kernels and for the numpy stand-ins of the host test alike."""
import torch

# quiet NaN with a payload: no kernel of the library produces these bits (arithmetic NaNs are 0x7FC00000 / 0xFFC00000)
SENTINEL = 0x7FC0BEEF
NAN_BITS = 0x7FC00000
OFFSETS = (0, 1, 2, 3)          # elements: every residue data_ptr() % 16 a 4-byte tensor can have
BYTE_OFFSETS = (0, 1, 2, 3, 7, 13)   # bytes: every residue mod 4, and two that are odd mod 8 and mod 16
BYTE_FILLS = (0x00, 0xFF)       # what surrounds a byte input, one run each
BYTE_SENTINELS = (0x5A, 0xA5)   # what a byte output (guards and payload) holds before the launch, one run each
_BYTE = (torch.uint8, torch.int8)
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
    """Both guards of a view made by embed / out_like (or embed_u8 / out_like_u8) still hold their fill, bit for bit."""
    buf, start, n, bits = view._offset_buf
    if buf.dtype == torch.uint8:
        return bool((buf[:start] == bits).all()) and bool((buf[start + n:] == bits).all())
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


# ------------------------------------------------------------------------------------------------ byte tensors
def byte_guard_for(shape):
    """Guard bytes per side for a byte tensor of `shape`: two planes - (..., H, W, C) -> 2 * H * W * C, and the whole tensor
    twice where it has no plane axis (an image [H, W, 3], a mask [T, H, W], directions [P, D]) -, never fewer than 64, in whole
    16-byte groups."""
    shape = tuple(int(v) for v in shape)
    plane = _numel(shape[-3:]) if len(shape) >= 4 else _numel(shape)
    return (max(64, 2 * plane) + 15) // 16 * 16


def _byte_buffer(n, device, fill):
    buf = torch.empty(n, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0, "allocation at %#x is not 16-byte aligned" % buf.data_ptr()
    buf.fill_(fill)
    return buf


def _byte_place(buf, shape, dtype, off, guard, n, fill):
    start = guard + off
    view = buf[start:start + n].view(dtype).view(tuple(shape))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + start and view.data_ptr() % 16 == off % 16
    view._offset_buf = (buf, start, n, fill)
    return view


def embed_u8(t, off, fill, guard=None, device=None):
    """The contiguous view of t's shape and dtype (uint8 or int8) that starts guard + off BYTES into a fresh 16-byte aligned
    buffer of guard + off + t.numel() + guard bytes (guard a multiple of 16) and holds t's values; every other byte is `fill`."""
    assert t.dtype in _BYTE and 0 <= off <= 15 and 0 <= fill <= 255
    guard = byte_guard_for(t.shape) if guard is None else (int(guard) + 15) // 16 * 16
    device = t.device if device is None else device
    n = t.numel()
    view = _byte_place(_byte_buffer(guard + off + n + guard, device, fill), t.shape, t.dtype, off, guard, n, fill)
    view.copy_(t.detach())
    return view


def out_like_u8(shape, off, sentinel, guard=None, device="cpu", dtype=torch.uint8):
    """embed_u8's layout for an output: guards and payload filled with the byte `sentinel`."""
    assert dtype in _BYTE and 0 <= off <= 15 and 0 <= sentinel <= 255
    shape = tuple(int(v) for v in shape)
    guard = byte_guard_for(shape) if guard is None else (int(guard) + 15) // 16 * 16
    n = _numel(shape)
    return _byte_place(_byte_buffer(guard + off + n + guard, device, sentinel), shape, dtype, off, guard, n, sentinel)


def byte_rule(launch, inputs, out_shapes, want, offs=None, device="cpu", what="launch"):
    """The pair of runs.  launch(ins, outs) reads the placed byte inputs `ins` ({name: view}) and stores into the placed byte
    outputs `outs` ({name: view}); it may return further results ({name: tensor}).  inputs: {name: byte tensor}; out_shapes:
    {name: shape}; want: {name: tensor} for every output and returned result; offs: {name: byte offset} (default 0).  Run k
    uses BYTE_FILLS[k] around every input and BYTE_SENTINELS[k] in every output.  After each run every guard is bit-intact and
    every output and result equals `want`.  Returns the results of the first run."""
    offs = offs or {}
    first = None
    for fill, sentinel in zip(BYTE_FILLS, BYTE_SENTINELS):
        ins = {n: embed_u8(t, offs.get(n, 0), fill, device=device) for n, t in inputs.items()}
        outs = {n: out_like_u8(sh, offs.get(n, 0), sentinel, device=device) for n, sh in out_shapes.items()}
        extra = launch(ins, outs) or {}
        tag = "%s (guards %#04x, sentinel %#04x)" % (what, fill, sentinel)
        for n, v in list(ins.items()) + list(outs.items()):
            assert guards_intact(v), "%s: a guard band around %s was written" % (tag, n)
        res = dict(outs, **extra)
        for n, w in want.items():
            assert res[n].shape == w.shape and torch.equal(res[n].to(w.dtype).cpu(), w.cpu()), \
                "%s: %s differs from the reference (a byte outside the tensor was read, or a byte was never stored)" % (tag, n)
        first = res if first is None else first
    return first
