"""Host answers of hpvg_conv_w2_split (no GPU): how a launch of the two-axis Winograd conv is cut into a whole-tile launch over
the full rounds of 256 tiles and a launch of half or quarter tiles for a last round that is at most half full.  The rule is
restated here from the tile count alone and checked over the pyramid shapes of conv_ref.KINDS and over its boundaries."""
import ctypes

import pytest

import conv_ref
from hp_vae_gan_amd import lib as hplib

NUM_CU = 256
UNSUPPORTED = -3


def tiles(B, Cout, T, H, W):
    """Tiles of a two-axis launch: 64 quads (2 x 2 outputs) x 64 output channels each, planes never share a tile."""
    quads = ((H + 1) // 2) * ((W + 1) // 2)
    return B * T * ((quads + 63) // 64) * (((Cout + 31) // 32 + 1) // 2)


def rule(ntl):
    """[tiles of the whole-tile launch, leftover tiles, parts per leftover tile, workgroups of the part launch]"""
    r = ntl % NUM_CU
    if ntl <= NUM_CU or r == 0 or r > NUM_CU // 2:
        return [ntl, 0, 1, 0]
    parts = 4 if r <= NUM_CU // 4 else 2
    return [ntl - r, r, parts, r * parts]


def split(lib, B, Cin, Cout, T, H, W, KT=3):
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = lib.hpvg_conv_w2_split(B, Cin, Cout, T, H, W, KT, out)
    return rc, list(out)


@pytest.fixture
def forced_two_axis():
    """The two-axis kernel wherever it can run (the shapes of the boundary cases are below the size rule)."""
    lib = hplib.load()
    prev = lib.hpvg_conv_wino_config(-1, -1)
    assert lib.hpvg_conv_wino_config(5, -1) == 5
    yield lib
    lib.hpvg_conv_wino_config(prev, -1)


def test_rule_over_the_pyramid_shapes():
    lib = hplib.load()
    seen = 0
    for sp in conv_ref.KINDS:
        if len(sp) != 3:
            continue
        T, H, W = sp
        for B in conv_ref.BATCHES:
            for (Ci, Co) in conv_ref.KIND_LAYERS:
                for (cin, cout) in ((Ci, Co), (Co, Ci)):       # forward and backward-data
                    rc, out = split(lib, B, cin, cout, T, H, W)
                    if lib.hpvg_conv_fwd_kernel_kind(B, cin, cout, T, H, W, 3) != 2:
                        assert rc == UNSUPPORTED, (B, cin, cout, sp)
                        continue
                    ntl = tiles(B, cout, T, H, W)
                    assert rc == 0 and out == rule(ntl), (B, cin, cout, sp, ntl, out)
                    assert out[0] + out[1] == ntl and out[3] <= NUM_CU and (out[1] == 0 or out[0] % NUM_CU == 0)
                    seen += 1
    assert seen > 50


@pytest.mark.parametrize("lvl_shape,B,leftover,parts", [
    ((7, 72, 129), 2, 6, 4), ((7, 72, 129), 4, 12, 4), ((7, 91, 162), 2, 58, 4), ((7, 91, 162), 4, 116, 2),
    ((13, 144, 256), 4, 64, 4),
])
def test_the_launches_of_the_benchmark_that_are_cut(lvl_shape, B, leftover, parts):
    lib = hplib.load()
    T, H, W = lvl_shape
    rc, out = split(lib, B, 64, 64, T, H, W)
    assert rc == 0 and out[1] == leftover and out[2] == parts and out[3] == leftover * parts <= NUM_CU, out
    assert out[0] + out[1] == tiles(B, 64, T, H, W)


def test_full_enough_last_rounds_stay_whole():
    lib = hplib.load()
    for B, sp in ((2, (7, 114, 204)), (2, (13, 144, 256)), (4, (7, 114, 204))):
        rc, out = split(lib, B, 64, 64, *sp)
        assert rc == 0 and out == [tiles(B, 64, *sp), 0, 1, 0], (B, sp, out)


@pytest.mark.parametrize("B,T,H,W,r", [
    (1, 512, 16, 16, 0), (1, 257, 16, 16, 1), (2, 160, 16, 16, 64), (1, 321, 16, 16, 65), (2, 192, 16, 16, 128),
    (1, 385, 16, 16, 129), (1, 256, 16, 16, 0), (1, 100, 16, 16, 100), (1, 64, 16, 16, 64), (2, 259, 16, 16, 6),
    (2, 13, 36, 65, 4), (2, 13, 35, 66, 4), (2, 20, 36, 64, 104), (1, 511, 16, 16, 255),
])
def test_boundaries(forced_two_axis, B, T, H, W, r):
    lib = forced_two_axis
    ntl = tiles(B, 64, T, H, W)
    assert ntl % NUM_CU == r
    rc, out = split(lib, B, 64, 64, T, H, W)
    assert rc == 0 and out == rule(ntl), (ntl, out)
    assert out[0] + out[1] == ntl and out[3] <= NUM_CU
    if ntl <= NUM_CU or r == 0 or r > 128:
        assert out == [ntl, 0, 1, 0]
    else:
        assert out == [ntl - r, r, 4 if r <= 64 else 2, r * (4 if r <= 64 else 2)]
    # both m-tile pairs of a 128-channel output are tiles of their own
    rc, out = split(lib, B, 64, 128, T, H, W)
    assert rc == 0 and out == rule(2 * ntl)


def test_what_is_not_a_two_axis_launch(forced_two_axis):
    lib = forced_two_axis
    out = (ctypes.c_int * 4)()
    assert lib.hpvg_conv_w2_split(2, 64, 64, 1, 144, 256, 1, out) == UNSUPPORTED     # 3 x 3
    assert lib.hpvg_conv_w2_split(2, 3, 64, 7, 72, 129, 3, out) == UNSUPPORTED       # Cin < 8
    assert lib.hpvg_conv_w2_split(2, 64, 3, 7, 72, 129, 3, out) == UNSUPPORTED       # narrow output
    assert lib.hpvg_conv_w2_split(0, 64, 64, 7, 72, 129, 3, out) == -1
    assert lib.hpvg_conv_w2_split(2, 64, 64, 7, 72, 129, 3, None) == -1
    assert lib.hpvg_conv_wino_config(6, -1) == 6                                     # one-axis kernel only
    assert lib.hpvg_conv_w2_split(2, 64, 64, 7, 72, 129, 3, out) == UNSUPPORTED
