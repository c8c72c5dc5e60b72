"""The narrow-output conv with the time taps in N (conv_narrowt_kernel) against float64, element by element.

The kernel is forced with hpvg_conv_narrowt_config(2) (the run-time form of HPVG_NARROWT) and every launch is compared with
conv_ref.conv_fwd64 / conv_bwd_data64 under the launch suites' criterion |got - ref| <= TAU * A.  Shapes, the smallest at
which each of its paths can go wrong:
  B = 2; Cin 2 (not a narrow layer: the knob must change nothing), 6 (three k-steps: a partly filled register set), 64;
  Cout 1, 3, 4 (one to four passes over the plane);
  T 1, 2, 3, 5: both time neighbours outside the tensor, a plane that is first and last, the ring's rotation;
  (H, W) (1, 4) one 16-byte group, (3, 5) W no multiple of 4, (9, 16), (10, 67) several bands, the last pulled back, and a
  ragged last row block, (7, 130) W above one window.
Forward with bias and LeakyReLU, and backward-data (the flipped pack).  Every case runs with all tensors at offsets 0, 1, 2 and
3 floats inside guard bands (offset_buf): guards intact, every output element written, no NaN read; and once more with
the knob forcing the second-generation kernel, under the same bound."""
import ctypes
import zlib

import pytest
import torch

import conv_ref as R
import launch_common as LC
import offset_buf as OB
from conv_ref import TAU

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2
CINS = (2, 6, 64)
COUTS = (1, 3, 4)
TS = (1, 2, 3, 5)
HWS = ((1, 4), (3, 5), (9, 16), (10, 67), (7, 130))
_STATS = {}


@pytest.fixture(scope="module")
def env():
    from hp_vae_gan_amd import lib as hplib
    from hp_vae_gan_amd import ops
    lib = hplib.load()
    prev = lib.hpvg_conv_narrowt_config(-1)
    yield ops, hplib, lib
    lib.hpvg_conv_narrowt_config(prev)
    LC.print_stats(_STATS, "conv_narrowt launches: worst |got - ref| / A per (pass, kernel), tau %.0e:" % TAU)


def _launch(ops, hplib, T, geom, Ci_l, Co_l, flip, out_lrelu):
    Bn, Tt, H, W = geom
    cin_k, cout_k = (Co_l, Ci_l) if flip else (Ci_l, Co_l)
    wp = ops.pack_weight(T["w"], flip, geom)
    nws = hplib.call("hpvg_conv_fwd_ws_bytes", Bn, cin_k, cout_k, Tt, H, W, 3)
    ws = ops._scratch(nws, T["x"].device) if nws else (None, 0)
    p = hplib.ptr
    hplib.call("hpvg_conv_fwd_f32", p(T["x"]), p(wp), p(T.get("bias")), None, None, 0, p(T["y"]), 1 if out_lrelu else 0, None, *ws,
               Bn, cin_k, cout_k, Tt, H, W, 3, hplib.stream())


def _at_offset(ops, hplib, ins, yshape, off, geom, Ci_l, Co_l, flip, out_lrelu, what):
    T = {n: OB.embed(t, off) for n, t in ins.items()}
    T["y"] = OB.out_like(yshape, torch.float32, off, device=DEV)
    _launch(ops, hplib, T, geom, Ci_l, Co_l, flip, out_lrelu)
    torch.cuda.synchronize()
    OB.assert_written(T["y"], what + " output")
    for n in ins:
        assert OB.guards_intact(T[n]), what + ": the guard band of input %s was written" % n
    ops.weights_changed()
    return T["y"]


def _runs_new(lib, Cin_k, Cout_k, T, H, W):
    out = (ctypes.c_int * 57)()
    return lib.hpvg_conv_narrowt_plan(B, Cin_k, Cout_k, T, H, W, 3, out) == 0 and out[8] == 1


@pytest.mark.parametrize("H,W", HWS, ids=["%dx%d" % hw for hw in HWS])
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
def test_every_launch_against_float64(env, Cin, Cout, H, W):
    ops, hplib, lib = env
    for T in TS:
        g = torch.Generator().manual_seed(zlib.crc32(repr(("narrowt", Cin, Cout, T, H, W)).encode()))
        sp = (T, H, W)
        geom = (B, T, H, W)
        # forward: a Cin -> Cout layer; backward-data: the flipped pack of a Cout -> Cin layer (kernel view Cin -> Cout again)
        x = torch.randn(B, Cin, *sp, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
        b = torch.randn(Cout, generator=g)
        wl = torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
        y64, yA = R.conv_fwd64(x, w, b)
        d64, dA = R.conv_bwd_data64(x, wl)
        fwd_in = {"x": x.to(DEV), "w": w.to(DEV), "bias": b.to(DEV)}
        bwd_in = {"x": x.to(DEV), "w": wl.to(DEV)}
        yshape = (B, Cout, *sp)
        for mode, kname in ((2, "time-in-N"), (1, "second-gen")):
            assert lib.hpvg_conv_narrowt_config(mode) == mode
            assert lib.hpvg_conv_fwd_kernel_kind(B, Cin, Cout, T, H, W, 3) == (3 if Cin > 4 else 0)
            if Cin > 4:
                assert _runs_new(lib, Cin, Cout, T, H, W) == (mode == 2), (mode, Cin, Cout, T, H, W)
            for off in (OB.OFFSETS if mode == 2 else (0,)):
                tag = "%d->%d T=%d %dx%d %s offset %d: " % (Cin, Cout, T, H, W, kname, off)
                y = _at_offset(ops, hplib, fwd_in, yshape, off, geom, Cin, Cout, False, True, tag + "forward")
                LC.checked(_STATS, y, R.lrelu(y64), yA, tag + "forward+bias+lrelu", "fwd", kname, tau=TAU)
                dx = _at_offset(ops, hplib, bwd_in, yshape, off, geom, Cout, Cin, True, False, tag + "backward-data")
                LC.checked(_STATS, dx, d64, dA, tag + "backward-data", "bwd", kname, tau=TAU)
