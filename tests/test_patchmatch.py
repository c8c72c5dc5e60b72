"""The deterministic PatchMatch of `generate_patchnn --search patchmatch`, everything that needs no GPU: the hash and the numpy
restatement of the rule (tests/patchmatch_ref.py) against hand-computed values and the rule's own properties, its convergence
towards the exact search, three seeded defects that the GPU suite's equality check must notice, patchnn_field_resize by hand,
the header / bindings / host refusals of hpvg_patchmatch_u8, and the program's flags."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import generate_patchnn  # noqa: E402
from patchmatch_ref import START_IT, brute_mean_d2, h32, patch_match_ref, patch_matrix, rnd  # noqa: E402
from test_patchnn import BAD, _rand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_WORKSPACE = -1, -2
I3 = ctypes.c_int * 3


# ------------------------------------------------------------------------------------------------------------------ hash
def test_h32_and_rnd_hand_vectors():
    """Computed with plain Python integers, step by step, from the definition in hpvg.h."""
    for x, want in ((0, 0), (1, 0x688990c0), (2, 0xd1132181), (12345, 0x912efcf7), (0xFFFFFFFF, 0x6768824a),
                    (0x9E3779B9, 0x01fce552)):
        assert int(h32(x)) == want
    assert [int(v) for v in h32(np.array([1, 2], np.uint64))] == [0x688990c0, 0xd1132181]
    for (seed, i, it, k, ax), want in (((0, 0, 0, 0, 0), 0), ((7, 5, 2, 3, 1), 0xbcf5cda0), ((-1, 1000000, 1023, 15, 2), 0x7478b7b8),
                                       ((2 ** 40 + 3, 2 ** 31 - 1, START_IT, 0, 2), 0x772b9741)):
        assert int(rnd(seed, i, it, k, ax)) == want
    # seed counts mod 2^32, and i is the flat index
    assert int(rnd(2 ** 32 + 7, 5, 2, 3, 1)) == 0xbcf5cda0
    assert [int(v) for v in rnd(7, np.array([5, 5]), 2, 3, 1)] == [0xbcf5cda0] * 2


# ------------------------------------------------------------------------------------------------- the reference itself
@functools.lru_cache(maxsize=None)
def _small():
    return _rand((4, 12, 15), 70), _rand((3, 11, 17), 71), (2, 3, 3)


def _pair_d2(q, r, patch, nn):
    Q, _ = patch_matrix(q, patch)
    R, _ = patch_matrix(r, patch)
    return ((Q - R[nn.reshape(-1)]) ** 2).sum(1).reshape(nn.shape)


def test_keys_never_increase_and_iters0_is_the_scored_start():
    q, r, patch = _small()
    rg = (2, 9, 15)
    w = (0.25 + 3.75 * np.random.default_rng(72).random(2 * 9 * 15)).astype(np.float32)
    for weights in (None, w):
        info = {}
        d2, nn, score = patch_match_ref(q, r, patch, 5, seed=3, rweight=weights, info=info)
        assert np.array_equal(d2, _pair_d2(q, r, patch, nn)) and nn.min() >= 0 and nn.max() < 270
        keys = info["keys"]
        assert len(keys) == 6
        improved = 0
        for (p0, j0), (p1, j1) in zip(keys[:-1], keys[1:]):
            assert ((p1 < p0) | ((p1 == p0) & (j1 <= j0))).all()
            improved += int((p1 < p0).sum())
        assert improved > 0
        if weights is not None:
            assert score.dtype == np.float32 and np.array_equal(score, d2.astype(np.float32) * w[nn])
        # iters = 0: the start, scored.  The hash start, axis by axis
        d0, n0, _ = patch_match_ref(q, r, patch, 0, seed=3, rweight=weights)
        i = np.arange(n0.size)
        want = [(rnd(3, i, START_IT, 0, ax) % np.uint64(rg[ax])).astype(np.int64) for ax in range(3)]
        assert np.array_equal(n0.reshape(-1), (want[0] * 9 + want[1]) * 15 + want[2])
        assert np.array_equal(d0, _pair_d2(q, r, patch, n0))
        assert np.array_equal(keys[0][1], n0.reshape(-1))
    assert not np.array_equal(patch_match_ref(q, r, patch, 0, seed=4)[1], patch_match_ref(q, r, patch, 0, seed=3)[1])


def test_identity_stays_the_identity():
    q, _, patch = _small()
    n = 3 * 10 * 13
    d2, nn, _ = patch_match_ref(q, q, patch, 3, seed=1, nn_init=np.arange(n))
    assert np.array_equal(nn.reshape(-1), np.arange(n)) and not d2.any()


def test_constant_volumes_end_at_the_smallest_candidate_seen():
    q = np.full((4, 12, 15, 3), 9, np.uint8)
    r = np.full((3, 11, 17, 3), 200, np.uint8)
    info = {}
    d2, nn, _ = patch_match_ref(q, r, (2, 3, 3), 3, seed=5, info=info)
    assert (d2 == 54 * 191 * 191).all()
    assert np.array_equal(nn, info["seen_min"])
    assert (nn < patch_match_ref(q, r, (2, 3, 3), 0, seed=5)[1]).any()


def test_start_entries_out_of_range_are_clamped():
    q, r, patch = _small()
    n, Nr = 3 * 10 * 13, 270
    init = np.random.default_rng(73).integers(0, Nr, size=n)
    bad = init.copy()
    bad[::7], bad[3::7] = -5, Nr + 1000
    good = init.copy()
    good[::7], good[3::7] = 0, Nr - 1
    for iters in (0, 2):
        a, b = patch_match_ref(q, r, patch, iters, seed=2, nn_init=bad), patch_match_ref(q, r, patch, iters, seed=2, nn_init=good)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(patch_match_ref(q, r, patch, 0, nn_init=bad)[1].reshape(-1), good)


# ---------------------------------------------------------------------------------------------------------- convergence
def smooth_pair(image, seed=0):
    """A smooth random volume (a coarse normal field, linearly upsampled by 8) with mild noise, as uint8, and two overlapping
    crops of it: the keys 5 x 32 x 48 (images 1 x 32 x 48) and the query 5 x 28 x 40 (1 x 28 x 40), offset by (8, 12), so the
    query's last 4 rows and 4 columns lie outside the keys and the exact distance is not 0 everywhere."""
    rng = np.random.default_rng(seed)
    T = 1 if image else 5
    coarse = torch.from_numpy(rng.standard_normal((1, 3, T, 7, 9)))
    big = torch.nn.functional.interpolate(coarse, size=(T, 40, 56), mode="trilinear", align_corners=True)[0].permute(1, 2, 3, 0).numpy()
    vol = np.clip(np.round(128 + 60 * big + 2.0 * rng.standard_normal(big.shape)), 0, 255).astype(np.uint8)
    r, q = vol[:, :32, :48], vol[:, 8:36, 12:52]
    return (q[0], r[0]) if image else (q, r)


@pytest.mark.parametrize("image", [False, True])
def test_eight_iterations_from_the_hash_start_come_within_ten_percent_of_the_exact_search(image):
    """The bound of the issue: mean d2 <= 1.10 x the brute-force mean after 8 iterations (its prototype measured 1.005 and
    1.009; 2.0 and 1.2 after 4).  A missing propagation direction or a random search that does not shrink misses it."""
    q, r = smooth_pair(image)
    patch = (1, 7, 7) if image else (3, 7, 7)
    exact = brute_mean_d2(q, r, patch)
    assert exact > 0
    d2 = patch_match_ref(q, r, patch, 8, seed=0)[0]
    ratio = float(d2.mean()) / exact
    print("image" if image else "volume", "mean d2 / exact mean d2 after 8 iterations:", ratio)
    assert 1.0 <= ratio <= 1.10


# ------------------------------------------------------------------------------------------------------- seeded defects
@pytest.mark.parametrize("defect", ["tie_larger", "no_shift", "in_place"])
def test_seeded_defects_change_the_field(defect):
    """Each of these mistakes in a kernel would survive a loose check; the GPU suite's equality with the reference does not let
    them through, because on its kind of inputs they give another field."""
    if defect == "tie_larger":        # constant volumes: every candidate ties
        q, r, patch = np.full((4, 12, 15, 3), 9, np.uint8), np.full((3, 11, 17, 3), 200, np.uint8), (2, 3, 3)
    else:
        q, r, patch = _small()
    good = patch_match_ref(q, r, patch, 3, seed=6)
    bad = patch_match_ref(q, r, patch, 3, seed=6, defect=defect)
    assert not np.array_equal(good[1], bad[1])
    again = patch_match_ref(q, r, patch, 3, seed=6)
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])


# --------------------------------------------------------------------------------------------------------- field resize
def test_field_resize_by_hand():
    f = generate_patchnn.patchnn_field_resize
    # query grid (1, 2, 3) -> (1, 3, 5): rows read 0 1 1, columns 0 1 1 2 2; key grid (1, 2, 3) -> (1, 4, 6): y 0 1 -> 0 3,
    # x 0 1 2 -> 0 3 5 (halves up: (2 * 1 * 5 + 2) // 4 = 3)
    got = f(torch.arange(6, dtype=torch.int32), (1, 2, 3), (1, 2, 3), (1, 3, 5), (1, 4, 6))
    assert got.dtype == torch.int32 and tuple(got.shape) == (1, 3, 5)
    assert got.tolist() == [[[0, 3, 3, 5, 5], [18, 21, 21, 23, 23], [18, 21, 21, 23, 23]]]
    # the same grids: the field itself; entries outside the key grid are clamped first
    nn = torch.tensor([5, 0, 3, 2, 1, 4], dtype=torch.int32)
    assert f(nn, (1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 3)).reshape(-1).tolist() == nn.tolist()
    assert f(torch.tensor([-4, 99, 3, 2, 1, 4]), (1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 3)).reshape(-1).tolist() == [0, 5, 3, 2, 1, 4]
    # sides of 1: a target side of 1 reads source 0, a source key side of 1 maps to 0; t is scaled like any axis
    got = f(torch.tensor([[7], [2]]), (2, 1, 1), (1, 3, 3), (3, 1, 2), (4, 5, 2))
    #   t: 3 targets over 2 sources -> 0 1 1; x: 2 targets over 1 source -> 0 0.  key 7 = (0, 2, 1) -> (0, 4, 1) = 9, 2 = (0, 0, 2) -> 1
    assert got.tolist() == [[[9, 9]], [[1, 1]], [[1, 1]]]
    got = f(torch.tensor([3, 0, 1, 2]), (1, 1, 4), (1, 1, 4), (1, 1, 1), (1, 1, 7))
    assert got.tolist() == [[[6]]]       # target side 1 reads source 0: key x = 3 of 4 -> (2 * 3 * 6 + 3) // 6 = 6
    for bad in (((1, 2), (1, 2, 3), (1, 2, 3), (1, 2, 3)), ((1, 2, 4), (1, 2, 3), (1, 2, 3), (1, 2, 3)),
                ((1, 2, 3), (1, 0, 3), (1, 2, 3), (1, 2, 3))):
        with pytest.raises(ValueError, match="patchnn_field_resize"):
            f(torch.arange(6), *bad)


def test_field_resize_is_the_rule_on_random_grids():
    f = generate_patchnn.patchnn_field_resize
    rng = np.random.default_rng(74)
    for qf, rf, qt, rt in (((3, 9, 12), (3, 8, 15), (3, 13, 17), (3, 11, 21)), ((2, 13, 17), (4, 11, 21), (2, 9, 12), (4, 8, 15)),
                           ((1, 5, 1), (1, 1, 6), (1, 1, 4), (1, 3, 2))):
        nn = rng.integers(0, rf[0] * rf[1] * rf[2], size=qf)
        got = f(torch.from_numpy(nn), qf, rf, qt, rt).numpy()
        for a in np.ndindex(*qt):
            src = tuple((2 * a[k] * (qf[k] - 1) + (qt[k] - 1)) // (2 * (qt[k] - 1)) if qt[k] > 1 else 0 for k in range(3))
            b = np.unravel_index(nn[src], rf)
            nb = tuple((2 * int(b[k]) * (rt[k] - 1) + (rf[k] - 1)) // (2 * (rf[k] - 1)) if rf[k] > 1 else 0 for k in range(3))
            assert got[a] == (nb[0] * rt[1] + nb[1]) * rt[2] + nb[2]
            assert all(0 <= nb[k] < rt[k] for k in range(3))


# ------------------------------------------------------------------------------------------- header, bindings, refusals
def test_exports_are_declared_and_bound():
    declared = hplib.check_symbols()
    assert "hpvg_patchmatch_u8" in declared and "hpvg_patchmatch_ws_bytes" in declared
    with open(hplib.HEADER_PATH) as f:
        text = f.read()
    for word in ("0x7feb352d", "0x846ca68b", "0x9E3779B9", "0x85EBCA6B", "0xFFFFFF", "STRICTLY smaller", "Jacobi"):
        assert word in text      # the rule is the header's contract


def _p():
    dummy = ctypes.create_string_buffer(64)       # never touched: every call below is refused before a launch
    return dummy, ctypes.cast(dummy, ctypes.c_void_p)


def _call(lib, p, qs=(4, 20, 23), rs=(5, 17, 31), patch=(3, 7, 7), q=True, r=True, rw=False, init=False, iters=2, seed=0, d2=True,
          nn=True, score=False, ws=True, ws_bytes=1 << 40):
    g = lambda on: p if on else None   # noqa: E731
    return lib.hpvg_patchmatch_u8(g(q), *qs, g(r), *rs, I3(*patch), g(rw), g(init), iters, seed, g(d2), g(nn), g(score), g(ws),
                                  ws_bytes, None)


@pytest.mark.parametrize("why", sorted(BAD))
def test_the_geometry_refusals_of_the_exact_search(why):
    qs, rs, patch, qstride, rstride = BAD[why]
    lib = hplib.load()
    keep, p = _p()
    one = I3(1, 1, 1)
    dense_refuses = lib.hpvg_patchnn_counts(*qs, *rs, I3(*patch), one, one, (ctypes.c_int * 3)()) == ERR_ARG
    if not dense_refuses:       # the case is about a stride, which this entry point does not have
        assert "stride" in why
        assert lib.hpvg_patchmatch_ws_bytes(*qs, *rs, I3(*patch)) > 0
        return
    assert _call(lib, p, qs, rs, patch) == ERR_ARG
    assert lib.hpvg_patchmatch_ws_bytes(*qs, *rs, I3(*patch)) == 0


def test_every_other_refusal_comes_from_the_host_path():
    lib = hplib.load()
    keep, p = _p()
    assert _call(lib, p, patch=(3, 7, 7), ws=False) == ERR_WORKSPACE      # the good call gets as far as the workspace
    assert lib.hpvg_patchmatch_u8(p, 4, 20, 23, p, 5, 17, 31, None, None, None, 2, 0, p, p, None, p, 1 << 40, None) == ERR_ARG
    # a grid side of 65536 on either side (65535 is taken)
    for qs, rs in (((1, 1, 65536), (1, 1, 5)), ((1, 1, 5), (1, 65536, 1)), ((65536, 1, 1), (1, 1, 5))):
        assert _call(lib, p, qs, rs, (1, 1, 1)) == ERR_ARG
        assert lib.hpvg_patchmatch_ws_bytes(*qs, *rs, I3(1, 1, 1)) == 0
    assert _call(lib, p, (1, 1, 65535), (1, 65535, 1), (1, 1, 1), ws=False) == ERR_WORKSPACE
    assert lib.hpvg_patchmatch_ws_bytes(1, 1, 65535, 1, 65535, 1, I3(1, 1, 1)) > 0
    for iters in (-1, 1025, 1 << 20):
        assert _call(lib, p, iters=iters) == ERR_ARG
    for iters in (0, 1024):
        assert _call(lib, p, iters=iters, ws=False) == ERR_WORKSPACE
    assert _call(lib, p, score=True) == ERR_ARG                             # score without weights
    assert _call(lib, p, score=True, rw=True, ws=False) == ERR_WORKSPACE
    assert _call(lib, p, rw=True, init=True, ws=False) == ERR_WORKSPACE       # weights without score: taken
    for k in ("q", "r", "d2", "nn"):
        assert _call(lib, p, **{k: False}) == ERR_ARG
    need = lib.hpvg_patchmatch_ws_bytes(4, 20, 23, 5, 17, 31, I3(3, 7, 7))
    assert need >= 2 * 3 * 4 * (2 * 14 * 17)                                  # two fields of nn, d2 and score
    assert _call(lib, p, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _call(lib, p, ws_bytes=0) == ERR_WORKSPACE
    assert _call(lib, p, ws=False, ws_bytes=need) == ERR_WORKSPACE
    # the workspace follows the query side only
    assert lib.hpvg_patchmatch_ws_bytes(4, 20, 23, 9, 40, 50, I3(3, 7, 7)) == need
    assert lib.hpvg_patchmatch_ws_bytes(8, 20, 23, 5, 17, 31, I3(3, 7, 7)) > need


# --------------------------------------------------------------------------------------------------------------- parser
def test_parser_defaults_and_choices():
    p = generate_patchnn.generate_patchnn_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.search, a.pm_iters, a.pm_from_level) == ("exact", None, None)      # None: not given (4 and 1 under patchmatch)
    assert (generate_patchnn.PM_ITERS, generate_patchnn.PM_FROM_LEVEL) == (4, 1)
    a = p.parse_args(["--exp-dir", "e", "--search", "patchmatch", "--pm-iters", "8", "--pm-from-level", "2"])
    assert (a.search, a.pm_iters, a.pm_from_level) == ("patchmatch", 8, 2)
    with pytest.raises(SystemExit):
        p.parse_args(["--exp-dir", "e", "--search", "fast"])


def test_refusals_in_process(tmp_path):
    clip, hole, out = str(tmp_path / "clip.npy"), str(tmp_path / "hole.npy"), str(tmp_path / "o")
    f = generate_patchnn.generate_patchnn
    with pytest.raises(SystemExit, match="--mask .* --search patchmatch"):
        f(video_path=clip, out=out, mask=hole, search="patchmatch")        # before any file is read
    for kw in ({"pm_iters": 4}, {"pm_from_level": 1}, {"pm_iters": 2, "pm_from_level": 2}):
        with pytest.raises(SystemExit, match="need --search patchmatch"):
            f(video_path=clip, out=out, **kw)
    with pytest.raises(SystemExit, match="--pm-from-level must be >= 1"):
        f(video_path=clip, out=out, search="patchmatch", pm_from_level=0)
    for bad in (-1, 1025):
        with pytest.raises(SystemExit, match="--pm-iters must lie in"):
            f(video_path=clip, out=out, search="patchmatch", pm_iters=bad)
    with pytest.raises(SystemExit, match="--search must be"):
        f(video_path=clip, out=out, search="fast")
    assert not os.path.exists(out)


@pytest.mark.parametrize("flags,message", [
    (["--search", "patchmatch", "--mask", "hole.npy"], "--search patchmatch does not do"),
    (["--pm-iters", "4"], "need --search patchmatch"),
    (["--pm-from-level", "2"], "need --search patchmatch"),
    (["--search", "exact", "--pm-iters", "4"], "need --search patchmatch")])
def test_the_program_refuses_before_any_device_use(tmp_path, flags, message):
    """A child with no visible device: were the device asked for first, the message would be gpu_device()'s.  The clip and the mask
    do not exist either, so nothing was read."""
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.generate_patchnn", "--video-path", "clip.npy", "--out", "o"] + flags,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(str(tmp_path / "o"))
