"""The two-axis Winograd conv with a thinly filled last round cut into half or quarter tiles (conv_wino2r_kernel's SUB
instances, hpvg_conv_w2_split) on the GPU: every output element against the float64 reference of conv_ref, every mask word
against the sign of the output it was made from, and everything bit for bit against the same launches in whole-tile rounds.

The whole-tile results come from ONE child process started with HPVG_W2_SPLIT=0 (the knob is read once per process), which
runs every case below on the same seeded inputs and leaves one file per case.

Mask words.  Bit c % 32 of a word is "activation of channel c > 0".  The float64 reference cannot say what that bit must be
where the output is within rounding of zero, so each word is compared with the sign of the fp32 output the same launch wrote
(every word, every bit of a channel the layer has), that output with the float64 reference, and the whole words with the
whole-tile launch's."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (ROOT, os.path.join(ROOT, "tests")):
    if _d not in sys.path:
        sys.path.insert(0, _d)

pytestmark = pytest.mark.gpu

DEV = "cuda"

# name: (B, layer Cin, layer Cout, T, H, W, forced two-axis kernel?, forward launch: (leftover tiles, parts per tile))
# Tiles of a launch: B * T * ceil(ceil(H/2) * ceil(W/2) / 64) per pair of 32-channel output tiles.  The backward-data launch of
# a layer runs Cout -> Cin on the same volume: the same cut for the square layers, its own for the others.
CASES = {
    # odd W, quarter tiles; 594 quads per plane: the tenth tile of a plane holds 18 quads, and the last plane's is a leftover
    "oddw_quarter": (2, 64, 64, 13, 36, 65, True, (4, 4)),
    # H * W % 4 = 2: the plane-end patch (TAIL instance)
    "tail_quarter": (2, 64, 64, 13, 35, 66, True, (4, 4)),
    # W % 4 = 0, half tiles
    "even_half": (2, 64, 64, 20, 36, 64, True, (104, 2)),
    # one tile per plane: the rule's boundaries
    "r64_quarter": (2, 64, 64, 160, 16, 16, True, (64, 4)),
    "r128_half": (2, 64, 64, 192, 16, 16, True, (128, 2)),
    "r129_whole": (1, 64, 64, 385, 16, 16, True, (0, 1)),
    # two full rounds before the leftover, as at level 6
    "two_rounds_r6": (2, 64, 64, 259, 16, 16, True, (6, 4)),
    # the decoder head 128 -> 64 (32 sub-chunks; its backward-data launch 64 -> 128 has two tiles per position: 520, r = 8)
    "head_128_64": (1, 128, 64, 260, 16, 16, True, (4, 4)),
    # ragged channels: 6 sub-chunks, 8 channels in the second output tile (backward-data 40 -> 24: the direct kernel)
    "ragged_24_40_half": (1, 24, 40, 330, 16, 16, True, (74, 2)),
    # the benchmark's level 6 at B = 2 under the default size rule
    "level6": (2, 64, 64, 7, 72, 129, False, (6, 4)),
}


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _inputs(case):
    B, Ci, Co, T, H, W = CASES[case][:6]
    x = _rand(B, Ci, T, H, W, seed=71)
    w = _rand(Co, Ci, 3, 3, 3, seed=72, scale=0.05)
    b = _rand(Co, seed=73)
    gy = _rand(B, Co, T, H, W, seed=74)
    g = torch.Generator().manual_seed(75)
    words = torch.randint(-2 ** 31, 2 ** 31, (B * ((Ci + 31) // 32) * T * H * W,), generator=g, dtype=torch.int64).to(torch.int32)
    return x, w, b, gy, words


def _run(case, ops, lib):
    """The three launches of a case on the library as this process has it -> dict of device tensors."""
    forced = CASES[case][6]
    prev = lib.hpvg_conv_wino_config(-1, -1)
    try:
        if forced:
            assert lib.hpvg_conv_wino_config(5, -1) == 5
        ops.weights_changed()
        x, w, b, gy, words = (t.to(DEV) for t in _inputs(case))
        y = ops.conv_fwd_raw(x, w, b)
        ya, bits = ops.conv_fwd_raw(x, w, b, out_lrelu=True, want_bits=True)
        dxm = ops.conv_fwd_raw(gy, w, None, flip=True, mask_bits=words)
        torch.cuda.synchronize()
    finally:
        lib.hpvg_conv_wino_config(prev, -1)
        ops.weights_changed()
    return dict(y=y, ya=ya, bits=bits, dxm=dxm)


def _child(outdir):
    import hp_vae_gan_amd as hp  # noqa: F401
    from hp_vae_gan_amd import lib as hplib, ops
    lib = hplib.load()
    out = (ctypes.c_int * 4)()
    for case, (B, Ci, Co, T, H, W, forced, _) in CASES.items():
        if forced:
            lib.hpvg_conv_wino_config(5, -1)
        rc = lib.hpvg_conv_w2_split(B, Ci, Co, T, H, W, 3, out)
        lib.hpvg_conv_wino_config(1, -1)
        assert rc == 0 and list(out)[1:] == [0, 1, 0], (case, rc, list(out))     # the knob is off in this process
        res = _run(case, ops, lib)
        torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, case + ".pt"))
    print("w2-split-child-done")


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd as hp  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


@pytest.fixture(scope="module")
def whole_tile_dir(tmp_path_factory):
    """Every case in whole-tile rounds: a fresh child process with HPVG_W2_SPLIT=0, one file per case."""
    d = str(tmp_path_factory.mktemp("w2_whole"))
    env = dict(os.environ, PYTHONPATH=ROOT, HPVG_W2_SPLIT="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), d], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "w2-split-child-done" in p.stdout, "child failed (%s):\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return d


def _unpack(words, B, C, sp):
    """[B][ceil(C/32)][positions] words -> bool [B, C, *sp]: bit c % 32 of word c / 32"""
    mt = (C + 31) // 32
    wv = words.view(B, mt, 1, -1)
    sh = torch.arange(32, device=words.device, dtype=torch.int32).view(1, 1, 32, 1)
    bit = ((wv >> sh) & 1).bool().reshape(B, mt * 32, -1)[:, :C]
    return bit.reshape((B, C) + tuple(sp))


@pytest.mark.parametrize("case", [c for c in CASES if c != "level6"])
def test_cut_last_round_against_float64_and_whole_tile_rounds(ops, lib, whole_tile_dir, case):
    import conv_ref
    B, Ci, Co, T, H, W, forced, (leftover, parts) = CASES[case]
    sp = (T, H, W)
    out = (ctypes.c_int * 4)()
    prev = lib.hpvg_conv_wino_config(-1, -1)
    try:
        assert lib.hpvg_conv_wino_config(5, -1) == 5
        assert lib.hpvg_conv_fwd_kernel_kind(B, Ci, Co, T, H, W, 3) == 2
        assert lib.hpvg_conv_w2_split(B, Ci, Co, T, H, W, 3, out) == 0
    finally:
        lib.hpvg_conv_wino_config(prev, -1)
    assert (out[1], out[2], out[3]) == (leftover, parts, leftover * parts if parts > 1 else 0), list(out)
    if case == "oddw_quarter":   # the last tile of the last plane (18 of 64 quads, none in its second quad half) is a leftover
        assert ((H + 1) // 2) * ((W + 1) // 2) == 594 and out[0] + out[1] == 2 * 13 * 10
    got = _run(case, ops, lib)
    x, w, b, gy, words = (t.to(DEV) for t in _inputs(case))
    # (i) every element against float64 (the same comparison and tolerance as the two-axis test of test_hip_ops.py, and the
    # per-element bound of conv_ref beside it)
    y64, A = conv_ref.conv_fwd64_taps(x, w, b)
    conv_ref.check(got["y"], y64, A, case + ".y")
    conv_ref.check(got["ya"], conv_ref.lrelu(y64), A, case + ".lrelu")
    # (the bits of a word past the layer's last channel are not specified: compared with the whole-tile launch's below)
    assert torch.equal(_unpack(got["bits"], B, Co, sp), got["ya"] > 0), case + ".bits: a mask bit differs from its output's sign"
    d64, Ad = conv_ref.conv_bwd_data64_taps(gy, w)
    m = torch.where(_unpack(words, B, Ci, sp), 1.0, 0.2).double()
    conv_ref.check(got["dxm"], d64 * m, Ad, case + ".dx.mask_bits")
    del y64, A, d64, Ad, m
    # (ii) bit for bit against whole-tile rounds
    whole = torch.load(os.path.join(whole_tile_dir, case + ".pt"), weights_only=True)
    for k in ("y", "ya", "bits", "dxm"):
        assert torch.equal(got[k].cpu(), whole[k]), "%s.%s differs from the whole-tile launch" % (case, k)
        if got[k].dtype == torch.float32:
            assert torch.equal(got[k].cpu().view(torch.int32), whole[k].view(torch.int32)), "%s.%s (bits of the floats)" % (case, k)


def test_level6_bench_shape_crops_and_whole_tile_rounds(ops, lib, whole_tile_dir):
    """The benchmark's level 6 at B = 2 (64 -> 64, 7 x 72 x 129: 518 tiles, the last 6 as 24 quarter tiles) under the default
    size rule: three crops of every launch against the oracle's conv of the matching input crop (+1 voxel of context), among
    them the far corner, which the quarter tiles write; everything bit for bit against whole-tile rounds."""
    from helpers import RTOL, assert_close
    from oracle import hpvg_oracle as O
    case = "level6"
    B, C, _, T, H, W, _, (leftover, parts) = CASES[case]
    out = (ctypes.c_int * 4)()
    assert lib.hpvg_conv_fwd_kernel_kind(B, C, C, T, H, W, 3) == 2
    assert lib.hpvg_conv_w2_split(B, C, C, T, H, W, 3, out) == 0 and list(out) == [512, leftover, parts, leftover * parts]
    got = _run(case, ops, lib)
    x, w, b, gy, words = _inputs(case)
    mask = torch.where(_unpack(words, B, C, (T, H, W)), 1.0, 0.2)
    for (t0, t1, h0, h1, w0, w1) in [(0, 3, 0, 6, 0, 9), (2, 5, 33, 40, 60, 71), (4, 7, 66, 72, 120, 129)]:
        ts, hs, ws_ = max(t0 - 1, 0), max(h0 - 1, 0), max(w0 - 1, 0)
        te, he, we = min(t1 + 1, T), min(h1 + 1, H), min(w1 + 1, W)
        crop = (slice(1, 2), slice(None), slice(t0, t1), slice(h0, h1), slice(w0, w1))
        inner = (slice(None), slice(None), slice(t0 - ts, t1 - ts), slice(h0 - hs, h1 - hs), slice(w0 - ws_, w1 - ws_))
        tag = "level6.crop(%d,%d,%d)" % (t0, h0, w0)
        want = O.conv(x[1:2, :, ts:te, hs:he, ws_:we], w, b)[inner]
        assert_close(got["y"][crop], want, RTOL, tag + ".y")
        assert_close(got["ya"][crop], O.leaky_relu(want), RTOL, tag + ".lrelu")
        gc = gy[1:2, :, ts:te, hs:he, ws_:we].clone()
        xr = torch.zeros(1, C, te - ts, he - hs, we - ws_, requires_grad=True)
        # backward-data of the crop: the dy outside the crop's context does not reach the compared voxels
        (dx,) = torch.autograd.grad(O.conv(xr, w, None), xr, gc)
        assert_close(got["dxm"][crop], dx[inner] * mask[crop], RTOL, tag + ".dx.mask_bits")
    assert torch.equal(_unpack(got["bits"], B, C, (T, H, W)), got["ya"] > 0), "level6.bits"
    whole = torch.load(os.path.join(whole_tile_dir, case + ".pt"), weights_only=True)
    for k in ("y", "ya", "bits", "dxm"):
        assert torch.equal(got[k].cpu(), whole[k]), "level6.%s differs from the whole-tile launch" % k
