"""Rings (generate_patchnn --wrap) without a GPU: the numpy restatement of the contract (tests/patchwrap_ref.py) against hand-worked
cases and against the plain references it must reduce to, the roll-equivariance a ring gives a refine step, the seeded
defects, the header / bindings / host refusals of hpvg_patch_vote_wrap_u8 and hpvg_patchmatch_wrap_u8, and the programs' flags."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import evaluate, generate_patchnn  # noqa: E402
from patchmatch_ref import patch_match_ref  # noqa: E402
from patchwrap_ref import (patch_match_wrap_ref, periodic_grid, refine_wrap_ref, seam_ref, vote_wrap_ref,  # noqa: E402
                           wrap_pad)
from test_patchgen import vote_ref  # noqa: E402
from test_patchnn import BAD, _rand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_WORKSPACE = -1, -2
I3 = ctypes.c_int * 3
FLAGS = {"t": (1, 0, 0), "hw": (0, 1, 1), "thw": (1, 1, 1), "w": (0, 0, 1), "tw": (1, 0, 1)}


# -------------------------------------------------------------------------------------------------------- pad and vote
def test_pad_appends_the_first_slices_in_the_order_t_y_x():
    v = _rand((4, 5, 6), 0)
    p = wrap_pad(v, (3, 2, 4), (1, 1, 1))
    assert p.shape == (6, 6, 9, 3)
    assert np.array_equal(p[:4, :5, :6], v) and np.array_equal(p[4:, :5, :6], v[:2]) and np.array_equal(p[:4, 5:, :6], v[:, :1])
    assert np.array_equal(p[4:, 5:, 6:], v[:2, :1, :3])                     # the corner: pads of pads
    assert np.array_equal(wrap_pad(v, (3, 2, 4), (0, 0, 0)), v)
    assert wrap_pad(v, (1, 2, 1), (1, 0, 1)).shape == v.shape              # p = 1: nothing to append
    got = generate_patchnn.patchnn_wrap_pad(torch.from_numpy(v), (3, 2, 4), (1, 1, 1))
    assert np.array_equal(got.numpy(), p) and got.is_contiguous()
    img = generate_patchnn.patchnn_wrap_pad(torch.from_numpy(v[0]), (1, 2, 4), (0, 1, 1))
    assert np.array_equal(img.numpy(), wrap_pad(v[:1], (1, 2, 4), (0, 1, 1))[0])
    assert generate_patchnn.patchnn_wrap_pad(torch.from_numpy(v), (3, 2, 4), None) is not None
    assert generate_patchnn.patchnn_wrap_grid((4, 5, 6), (3, 2, 4), (1, 0, 1)) == (4, 4, 6) == periodic_grid((4, 5, 6), (3, 2, 4), (1, 0, 1))


def test_vote_on_a_ring_of_four_by_hand():
    """1 x 1 x 4 ring along x, pw = 3, values 1 x 1 x 5 (three patches), nn = 0, 1, 2, 0 for the ring's four patches.  Patch g puts
    byte nn[g] + d of the values on voxel (g + d) mod 4: voxel 0 gets v[0] (g 0), v[1] (g 3, d 1), v[4] (g 2, d 2); voxel 1 gets
    v[1], v[1], v[2]; voxel 2 gets v[2] three times; voxel 3 gets v[0] (g 3), v[3] (g 2), v[3] (g 1)."""
    v = np.array([0, 30, 61, 90, 200])
    values = (v[:, None] + np.arange(3)[None, :]).astype(np.uint8).reshape(1, 1, 5, 3)
    fallback = np.full((1, 1, 4, 3), 7, np.uint8)
    out, cnt = vote_wrap_ref(values, np.array([0, 1, 2, 0]), (1, 1, 3), fallback, (0, 0, 1))
    assert cnt.tolist() == [[[3, 3, 3, 3]]]
    sums = [0 + 30 + 200, 30 + 30 + 61, 61 * 3, 0 + 90 + 90]
    want = [(2 * s + 3) // 6 for s in sums]
    assert want == [77, 40, 61, 60]
    assert out[0, 0, :, 0].tolist() == want and out[0, 0, :, 2].tolist() == [w + 2 for w in want]
    # skipped entries: only patch 1 votes, on voxels 1, 2, 3; voxel 0 takes the fallback
    out, cnt = vote_wrap_ref(values, np.array([-1, 1, 5, 3]), (1, 1, 3), fallback, (0, 0, 1))
    assert cnt.tolist() == [[[0, 1, 1, 1]]] and out[0, 0, :, 0].tolist() == [7, 30, 61, 90]
    # without the fold the seam patches' votes never reach voxels 0 and 1
    bad, cnt = vote_wrap_ref(values, np.array([0, 1, 2, 0]), (1, 1, 3), fallback, (0, 0, 1), defect="no_seam_votes")
    assert cnt.tolist() == [[[1, 2, 3, 3]]] and bad[0, 0, :, 0].tolist() == [0, 30, 61, 60]


def test_a_ring_as_long_as_the_patch_is_covered_by_every_patch():
    values, fallback = _rand((4, 9, 10), 1), _rand((3, 5, 6), 2)
    nn = np.random.default_rng(3).integers(0, 2 * 7 * 8, size=3 * 3 * 4)          # ring t: grid 3 x 3 x 4, S == p == 3 on t
    out, cnt = vote_wrap_ref(values, nn, (3, 3, 3), fallback, (1, 0, 0))
    assert (cnt == cnt[:1]).all() and cnt[0, 2, 2] == 3 * 3 * 3 and cnt[0, 0, 0] == 3
    nn = np.random.default_rng(4).integers(0, 2 * 7 * 8, size=3 * 5 * 6)          # every axis a ring, S == p on t
    out, cnt = vote_wrap_ref(values, nn, (3, 3, 3), fallback, (1, 1, 1))
    assert (cnt == 27).all()


def test_flags_all_zero_are_the_plain_references():
    values, fallback = _rand((4, 12, 14), 5), _rand((5, 9, 11), 6)
    nn = np.random.default_rng(7).integers(-2, 2 * 6 * 8 + 3, size=3 * 3 * 5)
    a, b = vote_wrap_ref(values, nn, (3, 7, 7), fallback, (0, 0, 0)), vote_ref(values, nn, (3, 7, 7), fallback)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    q, r = _rand((4, 12, 15), 8), _rand((4, 11, 13), 9)
    w = (0.25 + np.random.default_rng(10).random(2 * 5 * 7)).astype(np.float32)
    for rw in (None, w):
        want = patch_match_ref(q, r, (3, 7, 7), 2, 5, rw)
        got = patch_match_wrap_ref(q, r, (3, 7, 7), 2, 5, rw, qwrap=(0, 0, 0), rwrap=None)
        assert all(x is None and y is None or np.array_equal(x, y) for x, y in zip(want, got))


# -------------------------------------------------------------------------------------------------- roll-equivariance
def _drift(shape, seed):
    """Random 3 x 3 blocks whose brightness drifts along t: patches resemble each other, and the clip does not loop."""
    rng = np.random.default_rng(seed)
    T, H, W = shape
    base = np.kron(rng.standard_normal((T, H // 3 + 1, W // 3 + 1, 3)), np.ones((1, 3, 3, 1)))[:, :H, :W]
    return np.clip(base * 40 + 90 + 12 * np.arange(T)[:, None, None, None], 0, 255).astype(np.uint8)


@pytest.mark.parametrize("alpha", [0.005, float("inf")])
@pytest.mark.parametrize("axes", ["t", "thw"])
def test_a_step_on_a_ring_commutes_with_a_roll_and_a_plain_step_does_not(alpha, axes):
    patch, wrap = (3, 5, 5), FLAGS[axes]
    q, real = _rand((6, 10, 12), 11), _drift((5, 11, 13), 12)
    alpha_abs = alpha * 225 * 255 * 255
    shift = tuple(s * w for s, w in zip((2, 3, 5), wrap))
    roll = lambda v: np.roll(v, shift, axis=(0, 1, 2))   # noqa: E731
    step = lambda v, w: refine_wrap_ref(v, real, real, patch, alpha_abs, w)[0]   # noqa: E731
    assert np.array_equal(step(roll(q), wrap), roll(step(q, wrap)))
    assert not np.array_equal(step(roll(q), (0, 0, 0)), roll(step(q, (0, 0, 0))))
    assert not np.array_equal(step(q, wrap), step(q, (0, 0, 0)))


# ------------------------------------------------------------------------------------------------------------- defects
def _ring_pair():
    """A periodic smooth volume and a rolled copy, both padded: matches continue across every seam."""
    rng = np.random.default_rng(13)
    base = np.kron(rng.integers(0, 256, size=(3, 4, 5, 3)), np.ones((2, 4, 4, 1))).astype(np.uint8)       # 6 x 16 x 20
    patch = (3, 5, 5)
    return wrap_pad(np.roll(base, (2, 5, 7), (0, 1, 2)), patch, (1, 1, 1)), wrap_pad(base, patch, (1, 1, 1)), patch


@pytest.mark.parametrize("defect", ["prop_no_wrap", "clamp_not_mod"])
def test_seeded_search_defects_change_the_field(defect):
    q, r, patch = _ring_pair()
    good = patch_match_wrap_ref(q, r, patch, 3, 1, qwrap=(1, 1, 1), rwrap=(1, 1, 1))
    bad = patch_match_wrap_ref(q, r, patch, 3, 1, qwrap=(1, 1, 1), rwrap=(1, 1, 1), defect=defect)
    assert not np.array_equal(good[1], bad[1])
    plain = patch_match_ref(q, r, patch, 3, 1)
    assert not np.array_equal(good[1], plain[1])                # the flags matter at all
    assert good[0].mean() < plain[0].mean()                     # and the ring's neighbours help on a ring


def test_seeded_vote_defect_changes_a_step():
    q, real = _rand((6, 10, 12), 14), _drift((5, 11, 13), 15)
    a = refine_wrap_ref(q, real, real, (3, 5, 5), float("inf"), (1, 0, 0))[0]
    b = refine_wrap_ref(q, real, real, (3, 5, 5), float("inf"), (1, 0, 0), defect="no_seam_votes")[0]
    assert not np.array_equal(a[:2], b[:2]) and np.array_equal(a[2:], b[2:])     # only the first p - 1 frames lose votes


def test_seam_patches_and_seam_coherence_by_hand():
    idx, grid = evaluate.seam_patches((4, 5, 6), (3, 3, 3), (1, 2, 1), (1, 0, 1))
    assert grid == (4, 2, 6)
    cross = np.zeros(grid, bool)
    cross[2:], cross[:, :, 4:] = True, True
    assert np.array_equal(idx, np.flatnonzero(cross)) and (np.diff(idx) > 0).all()
    assert len(evaluate.seam_patches((4, 5, 6), (1, 3, 3), (1, 1, 1), (1, 0, 0))[0]) == 0       # p = 1: no patch crosses
    with pytest.raises(ValueError):
        evaluate.seam_patches((4, 5, 6), (3, 3, 3), (1, 2, 1), (0, 1, 0))
    smp, real = _rand((4, 6, 7), 16), _rand((4, 6, 7), 17)
    n, coh = seam_ref(smp, real, (3, 3, 3), (1, 0, 0))
    assert n == 2 * 4 * 5 and 0 < coh < 1
    assert seam_ref(real, real, (3, 3, 3), (0, 0, 0)) == (0, None)
    # a volume that is periodic along t scores 0 against itself on the seam
    loop = np.concatenate([real, real], 0)
    assert seam_ref(loop[:4], loop, (3, 3, 3), (1, 0, 0)) == (40, 0.0)


# ------------------------------------------------------------------------------------------- header, bindings, refusals
def test_exports_are_declared_and_bound():
    declared = hplib.check_symbols()
    assert "hpvg_patch_vote_wrap_u8" in declared and "hpvg_patchmatch_wrap_u8" in declared
    with open(hplib.HEADER_PATH) as f:
        text = f.read()
    for word in ("Periodic grid", "Circular pad", "(g + d) mod S", "non-negative modulus", "never skipped"):
        assert word in text


def _p():
    dummy = ctypes.create_string_buffer(64)       # never touched: every call below is refused before a launch
    return dummy, ctypes.cast(dummy, ctypes.c_void_p)


def _vote(lib, p, vs=(5, 17, 31), qs=(4, 20, 23), patch=(3, 7, 7), rstride=(1, 1, 1), wrap=(1, 0, 1), v=True, nn=True, fb=True,
          out=True, out_ptr=None):
    g = lambda on: p if on else None   # noqa: E731
    return lib.hpvg_patch_vote_wrap_u8(g(v), *vs, g(nn), *qs, None if patch is None else I3(*patch),
                                       None if rstride is None else I3(*rstride), None if wrap is None else I3(*wrap), g(fb),
                                       out_ptr if out and out_ptr is not None else g(out), None)


def _pm(lib, p, qs=(4, 20, 23), rs=(5, 17, 31), patch=(3, 7, 7), qwrap=(1, 0, 0), rwrap=(0, 1, 1), q=True, r=True, rw=False,
        init=False, iters=2, d2=True, nn=True, score=False, ws=True, ws_bytes=1 << 40):
    g = lambda on: p if on else None   # noqa: E731
    f3 = lambda t: None if t is None else I3(*t)   # noqa: E731
    return lib.hpvg_patchmatch_wrap_u8(g(q), *qs, g(r), *rs, f3(patch), f3(qwrap), f3(rwrap), g(rw), g(init), iters, 0, g(d2), g(nn),
                                       g(score), g(ws), ws_bytes, None)


@pytest.mark.parametrize("why", sorted(BAD))
def test_the_geometry_refusals_of_the_exact_search(why):
    qs, rs, patch, qstride, rstride = BAD[why]
    lib = hplib.load()
    keep, p = _p()
    one = I3(1, 1, 1)
    if lib.hpvg_patchnn_counts(*qs, *rs, I3(*patch), one, one, (ctypes.c_int * 3)()) != ERR_ARG:
        assert "stride" in why      # the case is about a stride: the ring entry points are dense on the query side
        assert _pm(lib, p, qs, rs, patch, ws=False) == ERR_WORKSPACE
        return
    assert _pm(lib, p, qs, rs, patch) == ERR_ARG
    assert _vote(lib, p, rs, qs, patch) == ERR_ARG


def test_the_vote_refuses_from_the_host_path():
    lib = hplib.load()
    keep, p = _p()
    far = ctypes.c_void_p(p.value + (1 << 30))
    for k in ("v", "nn", "fb", "out"):
        assert _vote(lib, p, out_ptr=far, **{k: False}) == ERR_ARG
    assert _vote(lib, p, out_ptr=far, patch=None) == ERR_ARG
    assert _vote(lib, p, out_ptr=far, rstride=None) == ERR_ARG
    assert _vote(lib, p, out_ptr=far, rstride=(1, 0, 1)) == ERR_ARG
    for wrap in ((2, 0, 0), (0, -1, 0), (0, 0, 7)):
        assert _vote(lib, p, out_ptr=far, wrap=wrap) == ERR_ARG
    assert _vote(lib, p, out_ptr=far, qs=(2, 20, 23)) == ERR_ARG               # a ring shorter than the patch
    assert _vote(lib, p, out_ptr=far, vs=(2, 17, 31)) == ERR_ARG
    # out overlapping fallback, v or nn (all three are `p` here), as hpvg_patch_vote_u8 refuses it
    assert _vote(lib, p) == ERR_ARG
    assert _vote(lib, p, out_ptr=ctypes.c_void_p(p.value + 32)) == ERR_ARG


def test_patchmatch_refuses_from_the_host_path():
    lib = hplib.load()
    keep, p = _p()
    assert _pm(lib, p, ws=False) == ERR_WORKSPACE          # the good call gets as far as the workspace
    assert _pm(lib, p, patch=None) == ERR_ARG
    for flags in ((2, 0, 0), (0, -1, 0), (0, 0, 3)):
        assert _pm(lib, p, qwrap=flags) == ERR_ARG and _pm(lib, p, rwrap=flags) == ERR_ARG
    for flags in (None, (0, 0, 0), (1, 1, 1)):
        assert _pm(lib, p, qwrap=flags, rwrap=flags, ws=False) == ERR_WORKSPACE
    for qs, rs in (((1, 1, 65536), (1, 1, 5)), ((1, 1, 5), (1, 65536, 1))):
        assert _pm(lib, p, qs, rs, (1, 1, 1)) == ERR_ARG
    for iters in (-1, 1025):
        assert _pm(lib, p, iters=iters) == ERR_ARG
    assert _pm(lib, p, score=True) == ERR_ARG
    assert _pm(lib, p, score=True, rw=True, ws=False) == ERR_WORKSPACE
    for k in ("q", "r", "d2", "nn"):
        assert _pm(lib, p, **{k: False}) == ERR_ARG
    need = lib.hpvg_patchmatch_ws_bytes(4, 20, 23, 5, 17, 31, I3(3, 7, 7))
    assert _pm(lib, p, ws_bytes=need - 1) == ERR_WORKSPACE and _pm(lib, p, ws_bytes=0) == ERR_WORKSPACE
    assert _pm(lib, p, ws=False, ws_bytes=need) == ERR_WORKSPACE
    odd = ctypes.c_void_p((p.value & ~15) + 8)            # not 16-byte aligned
    assert lib.hpvg_patchmatch_wrap_u8(p, 4, 20, 23, p, 5, 17, 31, I3(3, 7, 7), I3(1, 0, 0), None, None, None, 2, 0, p, p, None, odd,
                                       1 << 40, None) == ERR_WORKSPACE


# --------------------------------------------------------------------------------------------------------------- programs
def test_parsers_and_the_axes_rule():
    p = generate_patchnn.generate_patchnn_parser()
    assert p.parse_args(["--exp-dir", "e"]).wrap is None
    assert p.parse_args(["--exp-dir", "e", "--wrap", "hw"]).wrap == "hw"
    e = evaluate.evaluate_parser()
    assert e.parse_args(["--exp-dir", "e"]).wrap is None and e.parse_args(["--exp-dir", "e", "--wrap", "t"]).wrap == "t"
    for text, flags in FLAGS.items():
        assert generate_patchnn.parse_wrap_axes(text) == flags
    assert generate_patchnn.parse_wrap_axes("wht") == (1, 1, 1)
    for bad in ("", "x", "tt", "thwt", "T", "t h", None):
        with pytest.raises(SystemExit, match="distinct letters"):
            generate_patchnn.parse_wrap_axes(bad)


def test_refusals_in_process(tmp_path):
    clip, out = str(tmp_path / "clip.npy"), str(tmp_path / "o")
    f = generate_patchnn.generate_patchnn
    for bad in ("x", "tt", ""):
        with pytest.raises(SystemExit, match="generate_patchnn: --wrap takes"):
            f(video_path=clip, out=out, wrap=bad)
    with pytest.raises(SystemExit, match="--mask .* do not combine"):
        f(video_path=clip, out=out, wrap="t", mask=str(tmp_path / "hole.npy"))
    with pytest.raises(SystemExit, match="--wrap t needs a clip"):
        f(image_path=str(tmp_path / "i.png"), out=out, wrap="th")
    e = evaluate.evaluate
    with pytest.raises(SystemExit, match="evaluate: --wrap takes"):
        e(samples=clip, real=clip, out=out, wrap="q")
    with pytest.raises(SystemExit, match="--stride must be 1 along a ring axis"):
        e(samples=clip, real=clip, out=out, wrap="t", stride=(2, 1, 1))
    assert not os.path.exists(out)
    with pytest.raises(ValueError):
        generate_patchnn.patchnn_wrap_pad(torch.zeros(2, 9, 9, 3, dtype=torch.uint8), (3, 7, 7), (1, 0, 0))


@pytest.mark.parametrize("flags,message", [
    (["--wrap", "x"], "--wrap takes a non-empty string of distinct letters"),
    (["--wrap", "tt"], "--wrap takes a non-empty string of distinct letters"),
    (["--wrap", "t", "--mask", "m.npy"], "do not combine"),
    (["--wrap", "t", "--image-path", "i.png"], "--wrap t needs a clip")])
def test_the_program_refuses_before_any_device_use(tmp_path, flags, message):
    """A child with no visible device: were the device asked for first, the message would be gpu_device()'s.  None of the files
    exists either, so nothing was read."""
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    source = [] if "--image-path" in flags else ["--video-path", "clip.npy"]
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.generate_patchnn"] + source + ["--out", "o"] + flags,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(str(tmp_path / "o"))
