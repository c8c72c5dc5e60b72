"""The exact antialiased volume resize (hpvg_volume_resize_u8 / ops.volume_resize_u8) on the host: the numpy restatement of the
contract (tests/volresize_ref.py) against itself, the hand case and the properties the generator relies on; the host-only
check and the refusals of the launch entry; and the host side of `generate_patchnn --antialias / --t-ratio / --min-frames` and
`evaluate --scales`.  Nothing here needs a GPU; every comparison is exact."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import evaluate, generate_patchnn, ops  # noqa: E402
import volresize_ref as VR  # noqa: E402
from test_patchinpaint import _conn  # noqa: E402

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
SIDES = range(1, 24)


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("src,out", [((3, 4, 5), (2, 3, 3)), ((2, 3, 4), (3, 5, 6)), ((3, 5, 2), (3, 2, 5)), ((3, 4, 5), (1, 1, 1)),
                                     ((1, 1, 1), (2, 3, 2)), ((2, 3, 2), (1, 5, 1))])
def test_the_two_reference_forms_agree(src, out):
    for seed, binary in ((1, False), (2, True)):
        v = _rand(src, seed)
        if binary:
            v = ((v & 1) * 255).astype(np.uint8)
        a, b = VR.resize(v, out), VR.resize_loops(v, out)
        assert a.shape == tuple(out) + (3,) and a.dtype == np.uint8 and np.array_equal(a, b)


def test_hand_case():
    assert VR.weights(7, 4)[1].tolist() == [0, 3, 6, 3, 0, 0, 0]
    row = np.array([0, 60, 120, 180, 240, 255, 255], np.uint8)
    for axis in range(3):
        shape = [1, 1, 1, 3]
        shape[axis] = 7
        v = np.repeat(row.reshape([7 if a == axis else 1 for a in range(3)] + [1]), 3, axis=3).reshape(shape)
        size = [1, 1, 1]
        size[axis] = 4
        for f in (VR.resize, VR.resize_loops):
            assert f(v, size).reshape(4, 3)[:, 1].tolist() == [20, 120, 229, 255]
    # the tie: 127.5 rounds up
    v = np.array([0, 255], np.uint8).reshape(1, 1, 2, 1).repeat(3, 3)
    assert VR.resize(v, (1, 1, 3))[0, 0, :, 0].tolist() == [0, 128, 255]


def test_the_footprint_is_the_mask_resize_rule():
    """w > 0 exactly where patchnn_mask_resize connects, so a level's mask covers exactly the voxels the resize reads."""
    for S in SIDES:
        for O in SIDES:
            w = VR.weights(S, O)
            if S == O:
                assert np.array_equal(w > 0, np.eye(S, dtype=bool))    # the mask resize returns an equal size unchanged
            else:
                assert np.array_equal(w > 0, _conn(S, O)), (S, O)
            assert (w >= 0).all() and (w.sum(1) > 0).all()
            if O < S:
                assert (w > 0).any(0).all(), (S, O)                     # every source reaches some output


def test_upsizing_is_exact_linear_interpolation():
    for S in SIDES:
        for O in range(S + 1, 24):
            w = VR.weights(S, O)
            for o in range(O):
                tot = int(w[o].sum())
                if S == 1:
                    assert w[o].tolist() == [tot] and tot > 0
                    continue
                x = Fraction(o * (S - 1), O - 1)
                i0 = int(x)
                f = x - i0
                want = [Fraction(0)] * S
                want[i0] += 1 - f
                if f:
                    want[i0 + 1] += f
                assert [Fraction(int(e), tot) for e in w[o]] == want, (S, O, o)


def test_constants_are_preserved_at_every_size():
    for c in (0, 1, 254, 255):
        for S in SIDES:
            for O in SIDES:
                w = VR.weights(S, O).sum(1)
                assert ((2 * w * c + w) // (2 * w) == c).all()
        for src, out in (((3, 4, 5), (2, 3, 7)), ((2, 9, 3), (5, 1, 4))):
            assert (VR.resize(np.full(src + (3,), c, np.uint8), out) == c).all()


# ------------------------------------------------------------------------------------------------------------ the library
def _check(src, out):
    o2 = (ctypes.c_long * 2)(-7, -7)
    rc = hplib.load().hpvg_volume_resize_check(*src, *out, o2)
    return rc, o2[0], o2[1]


def test_the_exports_are_declared_and_bound():
    names = hplib.check_symbols()
    assert "hpvg_volume_resize_check" in names and "hpvg_volume_resize_u8" in names
    lib = hplib.load()
    assert lib.hpvg_volume_resize_u8.argtypes == [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p]
    assert lib.hpvg_volume_resize_check.argtypes == [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert callable(ops.volume_resize_u8) and callable(ops.volume_resize_check)


def test_check_returns_the_reference_maxima():
    rng = np.random.default_rng(3)
    cases = [((7, 1, 1), (4, 1, 1)), ((1, 1, 4096), (1, 1, 1)), ((13, 144, 256), (13, 19, 34)), ((13, 144, 256), (4, 19, 34)),
             ((13, 108, 192), (13, 144, 256)), ((5, 5, 5), (5, 5, 5)), ((1, 1, 1), (1, 1, 1))]
    cases += [(tuple(int(e) for e in rng.integers(1, 24, 3)), tuple(int(e) for e in rng.integers(1, 24, 3))) for _ in range(200)]
    for src, out in cases:
        assert _check(src, out) == (OK,) + VR.dmax_and_reads(src, out), (src, out)
        assert ops.volume_resize_check(src, out) == VR.dmax_and_reads(src, out)
    assert hplib.load().hpvg_volume_resize_check(5, 9, 11, 3, 4, 5, None) == OK      # out2 is optional


def test_refusals_of_the_check_and_of_the_launch_entry():
    """The launch entry refuses the same cases before any launch: its buffers are two host bytes that stay as they were (no
    device exists here; were anything enqueued it would not be an error code that came back)."""
    unsupported = [((2000, 3000, 3000), (1, 1, 1)),     # 1.8e10 voxels
                   ((1, 1, 1), (2000, 3000, 3000)),
                   ((1000, 1000, 1000), (1, 1, 1)),     # below 2^31 voxels, D = (999 * 1000)^3 ~ 1e18: 511 D >= 2^63
                   ((1290, 1290, 1290), (2, 2, 2))]
    assert 511 * VR.dmax_and_reads((1000,) * 3, (1,) * 3)[0] >= 2 ** 63 and 1000 ** 3 < 2 ** 31
    # the largest cube -> 1 x 1 x 1 that passes, and the first that does not
    S = next(s for s in range(2, 2000) if 511 * (s * (s - 1)) ** 3 >= 2 ** 63)       # D of s^3 -> 1 is (s (s - 1))^3
    ok, bad = (S - 1,) * 3, (S,) * 3
    assert 511 * VR.dmax_and_reads(ok, (1, 1, 1))[0] < 2 ** 63 <= 511 * VR.dmax_and_reads(bad, (1, 1, 1))[0]
    assert _check(ok, (1, 1, 1))[0] == OK
    unsupported.append((bad, (1, 1, 1)))
    arg = [((0, 4, 4), (2, 2, 2)), ((4, 4, 4), (2, 0, 2)), ((4, 4, -1), (2, 2, 2)), ((4, 4, 4), (2, 2, -3))]
    dummy = (ctypes.c_ubyte * 2)(17, 34)
    src, out = ctypes.addressof(dummy), ctypes.addressof(dummy) + 1
    for cases, want in ((unsupported, ERR_UNSUPPORTED), (arg, ERR_ARG)):
        for s, o in cases:
            assert _check(s, o) == (want, -7, -7), (s, o)
            assert hplib.load().hpvg_volume_resize_u8(src, *s, out, *o, None) == want, (s, o)
            with pytest.raises(RuntimeError, match="HPVG_ERR_UNSUPPORTED" if want == ERR_UNSUPPORTED else "HPVG_ERR_ARG"):
                ops.volume_resize_check(s, o)
    # null pointers and overlap are refused before any launch as well
    assert hplib.load().hpvg_volume_resize_u8(None, 2, 2, 2, out, 1, 1, 1, None) == ERR_ARG
    assert hplib.load().hpvg_volume_resize_u8(src, 2, 2, 2, None, 1, 1, 1, None) == ERR_ARG
    assert hplib.load().hpvg_volume_resize_u8(src, 1, 1, 2, out, 1, 1, 1, None) == ERR_ARG       # out inside src
    assert list(dummy) == [17, 34]


def test_the_op_refuses_bad_tensors_by_name():
    import torch
    f = ops.volume_resize_u8
    with pytest.raises(RuntimeError, match="uint8"):
        f(torch.zeros(2, 3, 4, 3), (1, 2, 2))
    with pytest.raises(RuntimeError, match="uint8"):
        f(torch.zeros(2, 3, 4, 2, dtype=torch.uint8), (1, 2, 2))
    with pytest.raises(RuntimeError, match="size must be"):
        f(torch.zeros(2, 3, 4, 3, dtype=torch.uint8), (2, 2))
    with pytest.raises(RuntimeError, match="size must be"):
        f(torch.zeros(3, 4, 3, dtype=torch.uint8), (2, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(torch.zeros(2, 3, 4, 3, dtype=torch.uint8), (1, 2, 2))


# ------------------------------------------------------------------------------------------------------------ the programs
def test_parser_defaults_and_flags():
    p = generate_patchnn.generate_patchnn_parser()
    a = p.parse_args(["--video-path", "c.npy", "--out", "o"])
    assert (a.antialias, a.t_ratio, a.min_frames) == (False, 1.0, None)
    a = p.parse_args(["--video-path", "c.npy", "--out", "o", "--antialias", "--t-ratio", "0.85", "--min-frames", "5"])
    assert (a.antialias, a.t_ratio, a.min_frames) == (True, 0.85, 5)
    e = evaluate.evaluate_parser()
    a = e.parse_args(["--samples", "s.npy", "--real", "r.npy"])
    assert (a.scales, a.scale_ratio) == (0, None)
    a = e.parse_args(["--samples", "s.npy", "--real", "r.npy", "--scales", "2", "--scale-ratio", "0.6"])
    assert (a.scales, a.scale_ratio) == (2, 0.6)
    for bad in (["--scales", "-1"], ["--scales", "1", "--scale-ratio", "1.0"], ["--scales", "1", "--scale-ratio", "0"]):
        with pytest.raises(SystemExit):
            e.parse_args(["--samples", "s.npy", "--real", "r.npy"] + bad)


def test_refusals_in_process_before_any_file_or_device(tmp_path):
    clip, out = str(tmp_path / "clip.npy"), str(tmp_path / "o")
    f = generate_patchnn.generate_patchnn
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(SystemExit, match=r"--t-ratio must lie in \(0, 1\]"):
            f(video_path=clip, out=out, t_ratio=bad)
    with pytest.raises(SystemExit, match="--t-ratio needs a clip"):
        f(image_path=str(tmp_path / "i.png"), out=out, t_ratio=0.8)
    with pytest.raises(SystemExit, match="--t-ratio does not combine with --mask.*patchnn_mask_resize.*keeps T"):
        f(video_path=clip, out=out, t_ratio=0.8, mask=str(tmp_path / "hole.npy"))
    with pytest.raises(SystemExit, match="--min-frames needs --t-ratio below 1"):
        f(video_path=clip, out=out, min_frames=4)
    with pytest.raises(SystemExit, match="--min-frames needs --t-ratio below 1"):
        f(video_path=clip, out=out, t_ratio=1.0, min_frames=4)
    with pytest.raises(SystemExit, match="--min-frames must be at least the patch's T = 3, got 2"):
        f(video_path=clip, out=out, t_ratio=0.8, min_frames=2)
    with pytest.raises(SystemExit, match="--min-frames must be at least the patch's T = 5, got 4"):
        f(video_path=clip, out=out, t_ratio=0.8, min_frames=4, patch=(5, 7, 7))
    e = evaluate.evaluate
    with pytest.raises(SystemExit, match="--scale-ratio needs --scales"):
        e(samples=clip, real=clip, out=out, scale_ratio=0.5)
    with pytest.raises(SystemExit, match=r"--scale-ratio must lie in \(0, 1\)"):
        e(samples=clip, real=clip, out=out, scales=2, scale_ratio=1.0)
    with pytest.raises(SystemExit, match="--scales K must be >= 0"):
        e(samples=clip, real=clip, out=out, scales=-1)
    assert not os.path.exists(out)


def test_scales_sizes_and_the_largest_k_that_fits():
    assert evaluate.scale_sizes((6, 40, 48), 3) == [(6, 20, 24), (6, 10, 12), (6, 5, 6)]
    assert evaluate.scale_sizes((1, 45, 31), 2, 0.6) == [(1, 27, 19), (1, 16, 11)]
    assert evaluate.scales_check(2, None, [(6, 40, 48), (6, 40, 48)], (3, 7, 7)) == 0.5
    with pytest.raises(SystemExit, match="--scales 3: .*smaller than the patch.*largest K that fits is 2"):
        evaluate.scales_check(3, None, [(6, 40, 48), (6, 40, 48)], (3, 7, 7))
    with pytest.raises(SystemExit, match="largest K that fits is 1"):       # the smaller of the two volumes decides
        evaluate.scales_check(2, None, [(6, 40, 48), (6, 20, 48)], (3, 7, 7))
    assert evaluate.scales_check(0) is None


def test_pyramid_hand_cases():
    f = generate_patchnn.patchnn_pyramid_sizes
    s = f((13, 144, 256), 0.75, 16, t_ratio=0.85)
    assert [v[0] for v in s] == [4, 5, 6, 7, 8, 9, 11, 13]
    assert [v[1:] for v in s] == [v[1:] for v in f((13, 144, 256), 0.75, 16)]       # L and the spatial sides are unchanged
    assert f((6, 40, 48), 0.75, 30, t_ratio=0.6) == [(4, 30, 36), (6, 40, 48)]
    assert f((6, 40, 48), 0.75, 23, t_ratio=0.8) == [(4, 23, 27), (5, 30, 36), (6, 40, 48)]
    assert f((3, 40, 48), 0.75, 30, t_ratio=0.5) == [(3, 30, 36), (3, 40, 48)]
    assert f((13, 40, 48), 0.75, 23, t_ratio=0.5, min_frames=3) == [(3, 23, 27), (7, 30, 36), (13, 40, 48)]
    assert f((13, 40, 48), 0.75, 23, t_ratio=0.5, min_frames=9) == [(9, 23, 27), (9, 30, 36), (13, 40, 48)]
    assert f((9, 40, 48), 0.75, 23, (5, 7, 7), t_ratio=0.5) == [(6, 23, 27), (6, 30, 36), (9, 40, 48)]     # F = patch T + 1
    for kw in (dict(t_ratio=0.0), dict(t_ratio=1.01), dict(t_ratio=0.8, min_frames=2), dict(min_frames=4),
               dict(t_ratio=1.0, min_frames=4)):
        with pytest.raises(ValueError):
            f((6, 40, 48), 0.75, 30, **kw)


def test_t_ratio_one_is_the_old_call():
    f = generate_patchnn.patchnn_pyramid_sizes
    n = 0
    for T in (1, 3, 6, 13):
        for H, W in ((40, 48), (144, 256), (33, 77), (16, 16), (7, 9)):
            for ratio in (0.5, 0.75, 0.8):
                for min_size in (8, 16, 30):
                    patch = (min(T, 3), 7, 7)
                    try:
                        want = f((T, H, W), ratio, min_size, patch)
                    except ValueError as e:
                        with pytest.raises(ValueError, match="smaller than the patch"):
                            f((T, H, W), ratio, min_size, patch, t_ratio=1.0)
                        assert "smaller than the patch" in str(e)
                        continue
                    assert f((T, H, W), ratio, min_size, patch, t_ratio=1.0) == want
                    assert f((T, H, W), ratio, min_size, patch, 1.0, None) == want
                    n += 1
    assert n > 100
