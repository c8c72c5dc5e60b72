"""Host checks (no GPU) behind tests/test_offset_launches.py: the guard-band helper of tests/offset_buf.py on CPU tensors -
including the proof that its guard check CAN fail -, the pointer half of the vector-width rules the per-channel reductions
pick their kernel by (hpvg_vec_width_at, hpvg_bn_vec_width_at), and the table of pyramid levels at which the critic's input
`fake = x[B:]` (ops.SplitBatch in modules/_nets.py forward_pair) starts off a 16-byte boundary."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
import ew_ref as E
import offset_buf as OB


@pytest.fixture(scope="module")
def lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("off", OB.OFFSETS)
def test_embed_residue_values_and_guards(off, dtype):
    g = torch.Generator().manual_seed(7 + off)
    shape = (2, 3, 3, 5, 7)
    t = torch.randn(*shape, generator=g) if dtype == torch.float32 else \
        torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    v = OB.embed(t, off)
    buf, start, n, bits = v._offset_buf
    guard = OB.guard_for(shape)
    assert guard >= max(64, 2 * 5 * 7 + 8) and guard % 4 == 0
    assert buf.data_ptr() % 16 == 0 and buf.numel() == guard + off + t.numel() + guard and start == guard + off
    assert OB.residue(v) == 4 * off and v.is_contiguous() and tuple(v.shape) == shape and v.dtype == dtype
    assert torch.equal(v, t)
    assert OB.guards_intact(v)
    outside = torch.cat([buf[:start], buf[start + n:]])
    if dtype == torch.float32:
        assert bool(torch.isnan(outside).all())
    else:
        assert bool((outside == -1).all())


def test_guard_size_follows_the_plane():
    assert OB.guard_for((2, 64, 2, 3, 2)) == 64                       # never fewer than 64
    assert OB.guard_for((1, 64, 3, 57, 102)) == 2 * 57 * 102 + 8      # two planes + 8
    assert OB.guard_for((2, 64, 9, 10)) == 188                        # 2-D: the plane is the image
    assert OB.guard_for((7,)) == 64
    assert OB.embed(torch.zeros(5), 1, guard=9)._offset_buf[1] == 12 + 1   # a guard given by hand is rounded up to 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("off", OB.OFFSETS)
def test_out_like_sentinel_and_guard_check_can_fail(off, dtype):
    """guards_intact holds after any write inside the payload and fails after a one-element write just before and just
    after it; unwritten counts the payload elements that still hold the sentinel."""
    shape = (3, 5, 7)
    v = OB.out_like(shape, dtype, off)
    buf, start, n, bits = v._offset_buf
    assert bits == OB.SENTINEL and OB.residue(v) == 4 * off and n == 105
    assert bool((buf.view(torch.int32) == OB.SENTINEL).all())
    if dtype == torch.float32:
        assert bool(torch.isnan(buf).all())          # the sentinel is a NaN: a payload element left alone is also caught as one
    assert OB.guards_intact(v) and OB.unwritten(v) == n
    with pytest.raises(AssertionError, match="never stored"):
        OB.assert_written(v, "fresh")
    flat = v.view(-1)
    flat[0] = 1
    flat[n - 1] = 2
    assert OB.guards_intact(v) and OB.unwritten(v) == n - 2
    v.fill_(3)
    assert OB.guards_intact(v) and OB.unwritten(v) == 0
    OB.assert_written(v, "filled")
    for pos in (start - 1, start + n):               # one element before the payload, one element after it
        keep = buf[pos].clone()
        buf[pos] = 0
        assert not OB.guards_intact(v)
        with pytest.raises(AssertionError, match="guard band"):
            OB.assert_written(v, "overrun")
        buf[pos] = keep
        assert OB.guards_intact(v)
    # the same bits as a different NaN do not pass: the comparison is on the int32 view
    if dtype == torch.float32:
        buf[start - 1] = float("nan")
        assert not OB.guards_intact(v)
        v2 = OB.out_like(shape, dtype, off)
        v2.fill_(0.0)
        v2.view(-1)[4] = float("nan")
        with pytest.raises(AssertionError, match="NaN in the output"):
            OB.assert_written(v2, "poisoned")


# ------------------------------------------------------------------------------------------------ the byte helper
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int8])
@pytest.mark.parametrize("off", OB.BYTE_OFFSETS)
def test_embed_u8_placement_residue_and_guards(off, dtype):
    g = torch.Generator().manual_seed(70 + off)
    shape = (3, 5, 7, 3)                                  # 315 bytes: not a multiple of 4
    t = torch.randint(0, 256, shape, generator=g, dtype=torch.int16).to(torch.uint8).view(dtype)
    for fill in OB.BYTE_FILLS:
        v = OB.embed_u8(t, off, fill)
        buf, start, n, bits = v._offset_buf
        guard = OB.byte_guard_for(shape)
        assert guard >= 2 * 5 * 7 * 3 and guard >= 64 and guard % 16 == 0
        assert buf.dtype == torch.uint8 and buf.data_ptr() % 16 == 0 and buf.numel() == guard + off + n + guard
        assert start == guard + off and n == 315 and bits == fill
        assert v.data_ptr() == buf.data_ptr() + start and v.data_ptr() % 16 == off % 16
        assert v.is_contiguous() and tuple(v.shape) == shape and v.dtype == dtype and torch.equal(v, t)
        assert bool((buf[:start] == fill).all()) and bool((buf[start + n:] == fill).all())
        assert OB.guards_intact(v)


def test_byte_offsets_cover_every_residue():
    assert OB.BYTE_OFFSETS == (0, 1, 2, 3, 7, 13)
    assert {o % 4 for o in OB.BYTE_OFFSETS} == {0, 1, 2, 3}
    assert sum(1 for o in OB.BYTE_OFFSETS if o % 8 in (1, 3, 5, 7) and o % 16 in (1, 3, 5, 7, 9, 11, 13, 15)) >= 2
    assert {7 % 8, 13 % 8} == {7, 5} and OB.BYTE_FILLS == (0x00, 0xFF) and OB.BYTE_SENTINELS == (0x5A, 0xA5)


def test_byte_guard_size_follows_the_plane():
    assert OB.byte_guard_for((3, 5, 7, 3)) == 224                 # two planes of 105 bytes = 210, in 16-byte groups
    assert OB.byte_guard_for((4, 9, 11, 3)) == 608                # 2 * 9 * 11 * 3 = 594
    assert OB.byte_guard_for((2, 3, 5, 7, 3)) == 224              # [B, T, H, W, C]: the plane is H * W * C
    assert OB.byte_guard_for((1, 2, 2, 3)) == 64                  # never fewer than 64
    assert OB.byte_guard_for((9, 10, 3)) == 544                   # an image: the whole of it, twice (540)
    assert OB.byte_guard_for((4, 9, 11)) == 800                   # a mask [T, H, W]: no smaller than two planes (198)
    assert OB.byte_guard_for((7, 54)) == 768
    assert OB.embed_u8(torch.zeros(5, dtype=torch.uint8), 3, 0, guard=9)._offset_buf[1] == 16 + 3


@pytest.mark.parametrize("off", OB.BYTE_OFFSETS)
def test_out_like_u8_sentinel_and_guard_check_can_fail(off):
    shape = (3, 5, 7, 3)
    for sentinel in OB.BYTE_SENTINELS:
        v = OB.out_like_u8(shape, off, sentinel)
        buf, start, n, bits = v._offset_buf
        assert bits == sentinel and v.data_ptr() % 16 == off % 16 and n == 315 and bool((buf == sentinel).all())
        v.fill_(3)
        assert OB.guards_intact(v)
        for pos in (start - 1, start + n):                        # one byte before the payload, one byte after it
            buf[pos] = sentinel ^ 0xFF
            assert not OB.guards_intact(v)
            buf[pos] = sentinel
            assert OB.guards_intact(v)


# numpy stand-ins of byte kernels on the raw buffer: p = the payload's start, n its length.  The sound one touches [p, p + n)
# alone; each defect is one of the four mistakes a byte kernel makes at its ends.
def _np_kernel(defect):
    def launch(ins, outs):
        src, p, n, _ = ins["x"]._offset_buf
        dst, q, m, _ = outs["y"]._offset_buf
        s, d = src.numpy(), dst.numpy()
        assert n == m
        # y[i] = x[i] + 1 (mod 256); total = the sum of the bytes the kernel read
        lo, hi = p, p + n
        if defect == "reads one byte before the start":
            lo = p - 1
        elif defect == "reads a whole 4-byte word at the end":
            hi = p + (n + 3) // 4 * 4
            assert hi > p + n
        total = int(s[lo:hi].astype(np.int64).sum())
        stores = n
        if defect == "stores one byte past the end":
            stores = n + 1
        elif defect == "skips the last byte":
            stores = n - 1
        d[q:q + min(stores, n)] = s[p:p + min(stores, n)] + np.uint8(1)
        if stores > n:
            d[q + n] = 0
        return {"total": torch.tensor([total])}
    return launch


BYTE_DEFECTS = ["reads one byte before the start", "reads a whole 4-byte word at the end", "stores one byte past the end",
                "skips the last byte"]


def _byte_case():
    g = torch.Generator().manual_seed(99)
    x = torch.randint(0, 256, (3, 5, 7, 3), generator=g, dtype=torch.int16).to(torch.uint8)     # 315 bytes
    want = {"y": x + 1, "total": torch.tensor([int(x.to(torch.int64).sum())])}
    assert int(want["y"].min()) == 0                              # the wrap-around occurs
    return x, want


@pytest.mark.parametrize("off", OB.BYTE_OFFSETS)
def test_byte_rule_passes_a_sound_kernel(off):
    x, want = _byte_case()
    res = OB.byte_rule(_np_kernel(None), {"x": x}, {"y": x.shape}, want, offs={"x": off, "y": (off * 5) % 16})
    assert torch.equal(res["y"], want["y"])


@pytest.mark.parametrize("off", OB.BYTE_OFFSETS)
@pytest.mark.parametrize("defect", BYTE_DEFECTS)
def test_byte_rule_catches_every_seeded_defect(defect, off):
    """Each defect fails the pair of runs at every offset: the 0x00 run alone would pass the two over-reads (a sum does not see
    a zero), the 0xFF run catches them; the store past the end breaks a guard; the skipped byte holds the sentinel, which equals
    the wanted byte in at most one of the two runs."""
    x, want = _byte_case()
    with pytest.raises(AssertionError, match="guard band|differs from the reference"):
        OB.byte_rule(_np_kernel(defect), {"x": x}, {"y": x.shape}, want, offs={"x": off, "y": off})
    if defect.startswith("reads"):
        # the run with zero guards does pass: it is the SECOND run that makes the rule
        keep = OB.BYTE_FILLS
        OB.BYTE_FILLS = (0x00, 0x00)
        try:
            OB.byte_rule(_np_kernel(defect), {"x": x}, {"y": x.shape}, want, offs={"x": off, "y": off})
        finally:
            OB.BYTE_FILLS = keep


# ------------------------------------------------------------------------------------------------ the size rules' pointer half
def _expected_width(addr, S):
    if addr % 16 == 0 and S % 4 == 0:
        return 4
    if addr % 8 == 0 and S % 2 == 0:
        return 2
    return 1


def test_vec_width_table(lib):
    """hpvg_vec_width_at over addr % 16 in {0, 4, 8, 12} x S % 4 in {0, 1, 2, 3}: 16 bytes and S % 4 == 0 -> 4, 8 bytes and even
    S -> 2, else 1.  The full table, written out."""
    table = {   # rows: addr % 16; columns: S % 4 = 0, 1, 2, 3
        0: (4, 1, 2, 1),
        4: (1, 1, 1, 1),
        8: (2, 1, 2, 1),
        12: (1, 1, 1, 1),
    }
    for base in (256, 0x7F0000001000):
        for res, row in table.items():
            for smod, want in enumerate(row):
                for S in (smod + 4, smod + 96, smod + 4 * 1000003):
                    got = lib.hpvg_vec_width_at(ctypes.c_void_p(base + res), ctypes.c_long(S))
                    assert got == want == _expected_width(base + res, S), (hex(base + res), S, got, want)
    assert lib.hpvg_vec_width_at(ctypes.c_void_p(256), ctypes.c_long(0)) < 0


@pytest.mark.parametrize("groups", [1, 2])
def test_bn_vec_width_table(lib, groups):
    """hpvg_bn_vec_width_at = the narrowest hpvg_vec_width_at over the starts of the groups: group g starts
    g * (B / groups) * C * S floats in.  A group start is a whole number of rows of S floats past the tensor's start, so it
    keeps whatever alignment the width of the first group needs (S % 4 == 0: a multiple of 16 bytes, S even: of 8): the table
    is the one-group table, for C = 64 and for the odd channel counts below alike."""
    C = E.BN_C
    for B in (groups, 2 * groups):
        for res in (0, 4, 8, 12):
            for smod in range(4):
                for S in (smod + 4, smod + 104):
                    got = lib.hpvg_bn_vec_width_at(ctypes.c_void_p(4096 + res), B, C, ctypes.c_long(S), groups)
                    want = min(_expected_width(4096 + res + 4 * g * (B // groups) * C * S, S) for g in range(groups))
                    assert got == want == _expected_width(4096 + res, S), (res, S, B, groups, got, want)
    # the plan query is the aligned row of this table
    for B, g in E.BN_BATCHES:
        for S in (96, 90, 105):
            assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), B, C, ctypes.c_long(S), g) == E.bn_plan_of(lib, B, S, g)[2]
    # group starts that move the residue without narrowing the width: C = 1, S = 6, one sample per group: group 1 starts 24
    # bytes in
    if groups == 2:
        assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), 2, 1, ctypes.c_long(6), 2) == 2
        assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256 + 8), 2, 1, ctypes.c_long(6), 2) == 2
        assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), 2, 1, ctypes.c_long(6), 1) == 2      # S % 4 != 0
        assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), 2, 3, ctypes.c_long(4), 2) == 4      # 48 bytes: stays aligned
        assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), 2, 1, ctypes.c_long(4), 2) == 4
    assert lib.hpvg_bn_vec_width_at(ctypes.c_void_p(256), 3, C, ctypes.c_long(8), 2) < 0           # B not divisible by groups


# ------------------------------------------------------------------------------------------------ where training is offset
# (config, level, B): residue in bytes of fake = x[B:] for x of shape (2B, 3, level shape) whose start is 16-byte aligned -
# B * 3 * S floats in.  Every (config, level, B) that is not listed has residue 0.  video level 4 is (5, 45, 81); video8
# levels 3 and 5 are (5, 55, 99) and (7, 89, 159): S odd, so B = 1 leaves 12 and B = 2 leaves 8; S = 2 (mod 4) leaves 8 at
# B = 1 alone.  A change of the pyramid geometry (bench.py's stage shapes) shows up here.
FAKE_RESIDUES = {
    ("video", 4, 1): 12, ("video", 4, 2): 8, ("video", 5, 1): 8, ("video", 7, 1): 8,
    ("video8", 3, 1): 12, ("video8", 3, 2): 8, ("video8", 4, 1): 8, ("video8", 5, 1): 12, ("video8", 5, 2): 8,
    ("video8", 6, 1): 8,
    ("image", 1, 1): 8, ("image", 2, 1): 8, ("image", 7, 1): 8,
}


def test_fake_residue_of_every_level():
    shapes = R.level_shapes()
    assert sum(len(s) for s in shapes.values()) == 28
    got = {}
    for cfg, sps in shapes.items():
        for lvl, sp in enumerate(sps):
            for B in (1, 2):
                res = (4 * B * 3 * E.spatial(sp)) % 16
                if B == 1 and lvl in (0, 4) or len(sp) == 2 and lvl == 1:
                    # the arithmetic above is what torch does: a real slice of a real (tiny-channel) tensor agrees
                    x = OB.embed(torch.zeros(2 * B, 3, *sp), 0, guard=64)
                    assert (x[B:].data_ptr() - x.data_ptr()) % 16 == res and x[B:].is_contiguous()
                if res:
                    got[(cfg, lvl, B)] = res
    assert got == FAKE_RESIDUES
    assert shapes["video"][4] == (5, 45, 81)
    assert sorted(k[:2] for k in got if k[2] == 2) == [("video", 4), ("video8", 3), ("video8", 5)]
    # a B = 1 slice real[b:b+1] of a 3-channel batch (multigpu.py, the pipelines) starts b * 3 * S floats in: over b = 1, 2, 3
    # every residue 4, 8, 12 occurs at the levels with odd S
    odd = [(cfg, lvl) for cfg, sps in shapes.items() for lvl, sp in enumerate(sps) if E.spatial(sp) % 2]
    assert odd == [("video", 4), ("video8", 3), ("video8", 5)]
    for cfg, lvl in odd:
        S = E.spatial(shapes[cfg][lvl])
        assert sorted((4 * b * 3 * S) % 16 for b in (1, 2, 3)) == [4, 8, 12]
