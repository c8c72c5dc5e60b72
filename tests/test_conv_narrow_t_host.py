"""Host answers of the narrow-output kernel with the time taps in N (conv_narrowt_kernel; no GPU).

The kernel streams its input with 16-byte loads from column WINDOWS of (Th + 2) rows that must lie inside the image - nothing
zeroes a halo column and no address outside the tensor may be formed - one thread owns at most four outputs of a tile, and
the P image of a tile (27 columns whatever Cout is) must leave room for two workgroups per CU.  Checked over every width the
pyramids can produce; and whichever narrow kernel the size rule or the knob picks, the launch stays kernel kind 3 (bench.py
prices the roofline's executed flops with it) and the second generation's plan stays what it was."""
import ctypes

import pytest

from hp_vae_gan_amd import lib as hplib

LDS_MAX = 76 * 1024          # NARROWT_LDS_MAX of csrc/conv_mfma.hip
OUTPUTS_PER_THREAD = 4       # NARROWT_PPT
HS = (1, 2, 9, 144)
TS = (1, 4, 13)
COUTS = (1, 3, 4)


def _plan(lib, B, Cin, Cout, T, H, W, KT=3):
    out = (ctypes.c_int * 57)()
    rc = lib.hpvg_conv_narrowt_plan(B, Cin, Cout, T, H, W, KT, out)
    return rc, list(out)


@pytest.fixture()
def lib():
    lib = hplib.load()
    prev = lib.hpvg_conv_narrowt_config(-1)
    yield lib
    lib.hpvg_conv_narrowt_config(prev)


@pytest.mark.parametrize("Cout", COUTS)
def test_plan_windows_cover_and_lds(lib, Cout):
    for W in range(4, 301):
        for H in HS:
            for T in TS:
                rc, out = _plan(lib, 2, 64, Cout, T, H, W)
                assert rc == 0, (Cout, W, H, T, rc)
                RS, Th, nth, nb, npos, G, pitch, lds = out[:8]
                what = (Cout, W, H, T, out[:9])
                assert RS % 4 == 0 and 4 <= RS <= W and npos == (Th + 2) * RS and npos % 4 == 0, what
                assert G * 128 >= npos and pitch >= G * 128, what
                assert nth * Th >= H and (nth - 1) * Th < H and 1 <= nb <= 16, what
                assert lds == 27 * pitch * 4 and lds <= LDS_MAX, what
                covered = [0] * W
                for k in range(nb):
                    ws, ob, on = out[9 + 3 * k: 12 + 3 * k]
                    assert 0 <= ws and ws + RS <= W, what                      # every 16-byte window inside [0, W)
                    assert on >= 1 and Th * on <= 256 * OUTPUTS_PER_THREAD, what
                    assert max(ob - 1, 0) >= ws and min(ob + on, W - 1) <= ws + RS - 1, what   # in-image neighbours in the window
                    for c in range(ob, ob + on):
                        covered[c] += 1
                assert covered == [1] * W, what                                   # every output column exactly once


def test_kind_stays_3_whatever_the_knob_says(lib):
    out55 = (ctypes.c_int * 55)()
    for mode in (0, 1, 2):
        assert lib.hpvg_conv_narrowt_config(mode) == mode
        for Cout in COUTS:
            for (T, H, W) in [(4, 18, 33), (5, 57, 102), (13, 144, 256), (1, 9, 16)]:
                assert lib.hpvg_conv_fwd_kernel_kind(2, 64, Cout, T, H, W, 3) == 3
                rc, out = _plan(lib, 2, 64, Cout, T, H, W)
                assert rc == 0 and out[8] == {0: out[8], 1: 0, 2: 1}[mode]
                before = None
                if lib.hpvg_conv_narrow_plan(2, 64, Cout, T, H, W, 3, out55) == 0:
                    before = list(out55)
                lib.hpvg_conv_narrowt_config(1)
                after = list(out55) if lib.hpvg_conv_narrow_plan(2, 64, Cout, T, H, W, 3, out55) == 0 else None
                lib.hpvg_conv_narrowt_config(mode)
                assert before == after
    assert lib.hpvg_conv_narrowt_config(3) == -1 and lib.hpvg_conv_narrowt_config(-1) == 2


def test_size_rule_takes_the_finest_levels_only(lib):
    """By size: the critic's 64 -> 1 tail of the benchmark's finest level runs on it; the smaller levels (too few workgroups
    to fill the chip), short clips and the 64 -> 3 layers (three passes per plane) stay on the second generation."""
    assert lib.hpvg_conv_narrowt_config(0) == 0
    assert _plan(lib, 2, 64, 1, 13, 144, 256)[1][8] == 1
    assert _plan(lib, 4, 64, 1, 7, 114, 204)[1][8] == 1
    assert _plan(lib, 2, 64, 1, 7, 114, 204)[1][8] == 0
    assert _plan(lib, 2, 64, 1, 4, 18, 33)[1][8] == 0
    assert _plan(lib, 2, 64, 1, 2, 144, 256)[1][8] == 0
    assert _plan(lib, 2, 64, 3, 13, 144, 256)[1][8] == 0


def test_where_the_kernel_cannot_run(lib):
    U = -3
    assert _plan(lib, 2, 64, 3, 1, 30, 41, KT=1)[0] == U      # 3 x 3: no time taps
    assert _plan(lib, 2, 5, 3, 5, 9, 16)[0] == U              # odd Cin
    assert _plan(lib, 2, 64, 3, 5, 9, 3)[0] == U              # narrower than one 16-byte group
    assert _plan(lib, 2, 64, 64, 5, 9, 16)[0] == U            # not a narrow layer
    assert _plan(lib, 2, 2, 3, 5, 9, 16)[0] == U              # Cin <= 4: the direct kernel's layer
    assert _plan(lib, 0, 64, 3, 5, 9, 16)[0] == -1
    assert lib.hpvg_conv_narrowt_plan(2, 64, 3, 5, 9, 16, 3, None) == -1
