"""generate --size / --wrap without a GPU: the level-size rule, the float64 references of tests/ring_ref.py against hand-worked
cases, their roll property, seeded defects that the cases of the GPU tests must tell from the clean references, and every
refusal of the program's flags (before the device is asked for, nothing written)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from hp_vae_gan_amd import generate, programs  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from make_golden import make_opt  # noqa: E402
from ring_ref import (level_sizes_ref, ring_conv_ref, ring_conv_route_ref, ring_pad_ref,  # noqa: E402
                      ring_resize_ref)

# the cases of tests/test_generate_ring_gpu.py
PAD_CASES = [(3, (1, 1, 1), (1, 1, 1)), (2, (2, 5, 7), (1, 0, 1)), (3, (4, 6, 33), (3, 3, 3)), (2, (1, 5, 9), (0, 1, 1))]
RESIZE_CASES = [((4, 5, 6), (7, 5, 11)), ((6, 5, 8), (4, 5, 3)), ((1, 4, 4), (3, 4, 8))]
FLAGS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]


# ---------------------------------------------------------------------------------------------------------- level sizes
TRAINED = [[4, 12, 16], [5, 15, 20], [7, 18, 25], [13, 30, 40]]


def test_level_sizes_identity_returns_trained_itself():
    assert generate.level_sizes(TRAINED, [13, 30, 40]) is TRAINED
    assert level_sizes_ref(TRAINED, [13, 30, 40]) == TRAINED


def test_level_sizes_finest_is_the_request_and_matches_the_reference():
    for size in ([26, 30, 60], [13, 31, 40], [1, 1, 1], [5, 144, 256], [27, 29, 41]):
        got = generate.level_sizes(TRAINED, size)
        assert got[-1] == size
        assert got == level_sizes_ref(TRAINED, size)
        assert all(min(q) >= 1 for q in got)


def test_level_sizes_hand_worked_rounding():
    # T 13 -> 26: 4 * 26 / 13 = 8, 5 * 2 = 10, 14, 26.  H kept (equal to the trained side): the trained sides themselves.
    # W 40 -> 60: 16 * 1.5 = 24, 20 * 1.5 = 30, 25 * 1.5 = 37.5 -> 38 (halves up), 60.
    assert generate.level_sizes(TRAINED, [26, 30, 60]) == [[8, 12, 24], [10, 15, 30], [14, 18, 38], [26, 30, 60]]
    # W 40 -> 3: 16 * 3 / 40 = 1.2 -> 1, 1.5 -> 2 (half up), 1.875 -> 2, 3.  T 13 -> 1: 4 / 13 = 0.31 -> 0 -> the floor of 1.
    assert generate.level_sizes(TRAINED, [1, 30, 3]) == [[1, 12, 1], [1, 15, 2], [1, 18, 2], [1, 30, 3]]


def test_level_sizes_refuses_bad_requests():
    with pytest.raises(ValueError):
        generate.level_sizes(TRAINED, [13, 30])
    with pytest.raises(ValueError):
        generate.level_sizes(TRAINED, [13, 0, 40])


def test_level_size_hook_of_the_generator_defaults_to_off():
    from hp_vae_gan_amd.modules import _nets, networks_3d
    assert _nets.Conv.ring is None and _nets.GeneratorHPVAEGAN.ring is None and _nets.GeneratorHPVAEGAN.level_sizes is None
    opt = make_opt(dims=3)
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    g = networks_3d.GeneratorHPVAEGAN(opt)
    assert g._level_size(2) == hu.images.level_shape_3d(2, opt)
    g.level_sizes = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert g._level_size(2) == [7, 8, 9]


# ------------------------------------------------------------------------------------------- references vs hand-worked cases
def _axis(v):
    return np.asarray(v, dtype=np.float64).reshape(1, 1, 1, -1)


def test_ring_resize_hand_worked_axis():
    x = _axis([0, 3, 6])
    ring = ring_resize_ref(x, (1, 1, 6), (0, 0, 1))
    assert np.array_equal(ring.ravel(), [0, 1.5, 3, 4.5, 6, 3])          # the last output is halfway from 6 back to 0
    plain = ring_resize_ref(x, (1, 1, 6), (0, 0, 0))
    assert np.allclose(plain.ravel(), [0, 1.2, 2.4, 3.6, 4.8, 6], atol=1e-15)   # align corners: o * 2 / 5 * 3
    # the other two axes follow the same rule
    for ax in (0, 1):
        sh = [1, 1, 1, 1]
        sh[1 + ax] = 3
        size, wrap = [1, 1, 1], [0, 0, 0]
        size[ax], wrap[ax] = 6, 1
        assert np.array_equal(ring_resize_ref(x.reshape(sh), size, wrap).ravel(), [0, 1.5, 3, 4.5, 6, 3])


def test_ring_resize_identity_and_scale():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 4, 5, 6))
    assert np.array_equal(ring_resize_ref(x, (4, 5, 6), (1, 1, 1)), x)
    y, A = ring_resize_ref(x, (7, 5, 11), (1, 0, 1), with_scale=True)
    assert y.shape == A.shape == (2, 7, 5, 11) and np.all(np.abs(y) <= A + 1e-15)


def test_ring_pad_hand_worked():
    x = np.arange(6, dtype=np.float64).reshape(1, 1, 2, 3)
    got = ring_pad_ref(x, (0, 1, 2))
    want = np.array([[4, 5, 3, 4, 5, 3, 4], [1, 2, 0, 1, 2, 0, 1], [4, 5, 3, 4, 5, 3, 4], [1, 2, 0, 1, 2, 0, 1]], dtype=np.float64)
    assert np.array_equal(got[0, 0], want)
    # a pad beyond the side: a side of 1 repeats, a side of 2 with a pad of 3 starts at mod(-3, 2) = 1
    assert np.array_equal(ring_pad_ref(np.full((1, 1, 1, 1), 7.0), (3, 3, 3)), np.full((1, 7, 7, 7), 7.0))
    assert np.array_equal(ring_pad_ref(_axis([10, 20]), (0, 0, 3)).ravel(), [20, 10, 20, 10, 20, 10, 20, 10])
    for nc, sp, pad in PAD_CASES:
        x = np.random.default_rng(1).standard_normal((nc,) + sp)
        assert np.array_equal(ring_pad_ref(x, pad), np.pad(x, [(0, 0)] + [(p, p) for p in pad], mode="wrap"))


# -------------------------------------------------------------------------------------------------------- roll property
@pytest.mark.parametrize("k", [2, 3])
def test_ring_resize_roll_property(k):
    rng = np.random.default_rng(k)
    x = rng.standard_normal((2, 4, 5, 6))
    for ax, flags in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        size = list(x.shape[1:])
        size[ax] *= k
        y = ring_resize_ref(x, size, flags)
        for r in (1, 3):
            rolled = ring_resize_ref(np.roll(x, r, axis=1 + ax), size, flags)
            assert np.array_equal(rolled, np.roll(y, k * r, axis=1 + ax))
            # ... which the align-corners rule does not have
            assert not np.array_equal(ring_resize_ref(np.roll(x, r, axis=1 + ax), size, (0, 0, 0)),
                                      np.roll(ring_resize_ref(x, size, (0, 0, 0)), k * r, axis=1 + ax))


# -------------------------------------------------------------------------------------------------------- seeded defects
def _far(a, b, scale):
    """further apart than the GPU tests' bound of 1e-5 x scale, by a wide margin"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) > 1e-2 * scale


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
@pytest.mark.parametrize("flags", FLAGS)
def test_resize_defects_are_rejected(src, dst, flags):
    x = np.random.default_rng(5).standard_normal((3,) + src)
    clean = ring_resize_ref(x, dst, flags)
    changing = [a for a in range(3) if flags[a] and src[a] != dst[a]]
    # i1 not wrapped: told apart wherever a ring axis has an output beyond its last source sample
    seam = [a for a in changing if src[a] > 1 and
            any((o * src[a]) // dst[a] == src[a] - 1 and (o * src[a]) % dst[a] for o in range(dst[a]))]
    if seam:
        assert _far(ring_resize_ref(x, dst, flags, defect="i1_unwrapped"), clean, 1.0)
    # a ring axis computed by the non-ring rule (a source of one slice is constant along its axis under either rule)
    if any(src[a] > 1 for a in changing):
        assert _far(ring_resize_ref(x, dst, flags, defect="ac_rule"), clean, 1.0)
    assert np.array_equal(ring_resize_ref(x, dst, (0, 0, 0), defect="ac_rule"), ring_resize_ref(x, dst, (0, 0, 0)))


def test_an_unchanged_ring_axis_is_the_identity():
    """h never changes in the GPU cases (5 -> 5, 4 -> 4): there the ring rule is the identity, as the align-corners rule is"""
    x = np.random.default_rng(2).standard_normal((2, 4, 5, 6))
    assert np.array_equal(ring_resize_ref(x, (7, 5, 11), (0, 1, 0)), ring_resize_ref(x, (7, 5, 11), (0, 0, 0)))


@pytest.mark.parametrize("nc,sp,pad", PAD_CASES)
def test_pad_sign_defect_is_rejected(nc, sp, pad):
    x = np.random.default_rng(3).standard_normal((nc,) + sp)
    clean, bad = ring_pad_ref(x, pad), ring_pad_ref(x, pad, defect="sign")
    # a wrong sign shifts by 2 p: the same volume exactly where 2 p is a multiple of the side on every padded axis
    same = all((2 * p) % s == 0 for p, s in zip(pad, sp))
    assert np.array_equal(clean, bad) == same
    assert same == (sp == (1, 1, 1))


CONV_CASES = [(3, (1, 0, 1), k, (3, 6, 9)) for k in (3, 5, 7)] + [(3, (1, 1, 1), k, (3, 6, 9)) for k in (3, 5, 7)] + \
             [(3, (1, 0, 0), k, (1, 6, 9)) for k in (3, 5, 7)] + [(2, (1, 1), 3, (6, 9))]


@pytest.mark.parametrize("dims,ring,k,sp", CONV_CASES)
def test_conv_route_equals_the_definition_and_defects_are_rejected(dims, ring, k, sp):
    g = torch.Generator().manual_seed(k * 10 + dims)
    x = torch.randn((2, 5) + sp, generator=g)
    w = torch.randn((6, 5) + (k,) * dims, generator=g) / k ** dims
    b = torch.randn(6, generator=g)
    ref, A = ring_conv_ref(x, w, b, ring)
    route = ring_conv_route_ref(x, w, b, ring)
    assert route.shape == ref.shape == (2, 6) + sp
    assert float((route - ref).abs().max()) <= 1e-13 * float(A.max())       # the same sums in float64
    for defect in ("sign", "crop"):
        bad = ring_conv_route_ref(x, w, b, ring, defect=defect)
        if defect == "sign" and all(s == 1 for s, f in zip(sp, ring) if f):
            assert torch.equal(bad, route)          # a ring of one slice: every shift is the identity
            continue
        assert float((bad - ref).abs().max()) > 1e-2 * float(A.max()), defect
    # and the ring conv is not the zero-padded one
    zero, _ = ring_conv_ref(x, w, b, [0] * dims)
    assert float((zero - ref).abs().max()) > 1e-2 * float(A.max())


# -------------------------------------------------------------------------------------------------------------- the flags
def _write_exp(path, kind, program=None):
    opt = make_opt(dims=3 if kind == "video" else 2, generator="GeneratorHPVAEGAN")
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    if program:
        opt.program = program
    os.makedirs(path)
    with open(os.path.join(path, "opt.json"), "w") as f:
        json.dump(programs.json_settings(opt), f)
    return path


def _tree(path):
    return sorted(os.path.join(d, n) for d, _, names in os.walk(path) for n in names)


REFUSALS = [
    ("video", None, ["--wrap", "x"], "--wrap"),
    ("video", None, ["--wrap", "tt"], "--wrap"),
    ("video", None, ["--wrap", ""], "--wrap"),
    ("video", None, ["--size", "13", "30"], "T H W"),
    ("video", None, ["--size", "13", "30", "40", "2"], "T H W"),
    ("video", None, ["--size", "13", "0", "40"], ">= 1"),
    ("video", None, ["--size", "-1", "30", "40"], ">= 1"),
    ("image", None, ["--wrap", "t"], "time axis"),
    ("image", None, ["--wrap", "th"], "time axis"),
    ("image", None, ["--size", "13", "30", "40"], "H W"),
    ("image", None, ["--size", "0", "40"], ">= 1"),
    ("video", "train_video_baselines", ["--size", "13", "30", "40"], "train_video_baselines"),
    ("video", "train_video_baselines", ["--wrap", "t"], "train_video_baselines"),
]


@pytest.mark.parametrize("kind,program,flags,word", REFUSALS)
def test_refusals_come_before_the_device_and_write_nothing(tmp_path, monkeypatch, kind, program, flags, word):
    exp = _write_exp(str(tmp_path / "exp"), kind, program)
    before = _tree(str(tmp_path))

    def no_device():
        raise AssertionError("the device was asked for before the flags were refused")
    monkeypatch.setattr(generate, "gpu_device", no_device)
    with pytest.raises(SystemExit) as e:
        generate.main(["--exp-dir", exp, "--num-samples", "1"] + flags)
    assert e.value.code not in (0, None) and word in str(e.value.code), e.value.code
    assert _tree(str(tmp_path)) == before


def test_good_flags_pass_the_host_checks():
    import types
    video = types.SimpleNamespace(dims=3)
    image = types.SimpleNamespace(dims=2)
    assert generate.check_request(video, None, None) is None
    assert generate.check_request(video, [26, 30, 60], "t") == (1, 0, 0)
    assert generate.check_request(video, None, "wh") == (0, 1, 1)
    assert generate.check_request(image, [30, 60], "hw") == (1, 1)
    assert generate.check_request(image, None, "w") == (0, 1)
    assert generate.check_request(types.SimpleNamespace(dims=3, program="train_video_baselines"), None, None) is None
    a = generate.generate_parser().parse_args(["--exp-dir", "e"])
    assert a.size is None and a.wrap is None and a.out is None
