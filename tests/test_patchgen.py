"""The two kernels of the patch nearest-neighbour generator (hpvg_patchnn_weighted_u8 / ops.patch_nn_weighted and
hpvg_patch_vote_u8 / ops.patch_vote), one refine step (generate_patchnn.patchnn_refine) and the host-side pieces of generate_patchnn,
against numpy written from the definitions.  Every comparison is torch.equal / ==; there is no tolerance anywhere.

Weighted search: the float64 distance matrix of test_patchnn's yardstick (exact integers) -> float32 (exact below 2^24, round to
nearest even above, as the kernel's conversion) * w in float32 (one IEEE multiply) -> the first argmin along j.  Weights are
drawn from [0.25, 4): the largest product is 441 * 255^2 * 4 = 1.1e8 and the smallest non-zero one 0.25, all normal.

Vote: a scatter over the query grid's patches in numpy int64 (sum and count per voxel), then (2 sum + cnt) // (2 cnt)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import generate_patchnn, ops  # noqa: E402
from patch_ref import brute_weighted, vote_ref  # noqa: E402,F401
from test_patchnn import BAD, _case, _patches, _rand, brute  # noqa: E402

ERR_ARG, ERR_WORKSPACE = -1, -2
I3 = ctypes.c_int * 3
ONE = (1, 1, 1)
WEIGHTED_CASES = ["lane1", "lane8", "ragged", "ragged_strided", "merge", "nq1", "nr1", "image"]


# ------------------------------------------------------------------------------------------------------------ yardsticks
def _weights(n, seed):
    return np.random.default_rng(seed).uniform(0.25, 4.0, size=n).astype(np.float32).clip(0.25, np.nextafter(np.float32(4), np.float32(0)))


@functools.lru_cache(maxsize=None)
def _wcase(name):
    """(q, r, patch, qstride, rstride, w, want_score, want_nn, unweighted_nn) - built once, shared, never modified."""
    q, r, patch, qs, rs, _, nn0 = _case(name)
    Nr = len(_patches(r if r.ndim == 4 else r[None], patch, rs)[0])
    w = _weights(Nr, 100 + WEIGHTED_CASES.index(name))
    score, nn = brute_weighted(q, r, w, patch, qs, rs)
    return q, r, patch, qs, rs, w, score, nn, nn0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------- weighted search
def _run_weighted(q, r, w, patch, qs, rs):
    score, nn = ops.patch_nn_weighted(_dev(q), _dev(r), _dev(w), patch, qs, rs)
    return score.cpu(), nn.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", WEIGHTED_CASES)
def test_weighted_equals_numpy(name):
    """lane1 / lane8: the lane map; ragged(_strided): K padding 441 -> 448 and ragged tiles; merge: 42 row tiles x 41 column
    splits; nq1 / nr1: one patch on a side; image: the [H,W,3] path with patch 1 x 5 x 5."""
    q, r, patch, qs, rs, w, want_score, want_nn, nn0 = _wcase(name)
    if name == "ragged":
        assert want_nn.shape == (2, 14, 17) and w.size == 825
        assert (want_nn != nn0).mean() > 0.5      # the weights decide most winners: a kernel that ignored them cannot pass
    score, nn = _run_weighted(q, r, w, patch, qs, rs)
    assert score.dtype == torch.float32 and nn.dtype == torch.int32
    if q.ndim == 3:
        want_score, want_nn = want_score[0], want_nn[0]
        assert score.dim() == 2
    assert tuple(score.shape) == want_score.shape and tuple(nn.shape) == want_nn.shape
    assert torch.equal(nn.to(torch.int64), torch.from_numpy(want_nn)), name
    assert torch.equal(score.view(torch.int32), torch.from_numpy(want_score.view(np.int32))), name   # bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "ragged_strided", "image"])
def test_unit_weights_reproduce_patch_nn(name):
    q, r, patch, qs, rs = _case(name)[:5]
    qd, rd = _dev(q), _dev(r)
    d2, nn0 = ops.patch_nn(qd, rd, patch, qs, rs)
    Nr = ops.patch_nn_counts((q if q.ndim == 4 else q[None]).shape[:3], (r if r.ndim == 4 else r[None]).shape[:3], patch, qs, rs)[1]
    score, nn = ops.patch_nn_weighted(qd, rd, torch.ones(Nr, device="cuda"), patch, qs, rs)
    assert torch.equal(nn, nn0)
    assert torch.equal(score, d2.to(torch.float32))


@functools.lru_cache(maxsize=None)
def _tie_case(first):
    """The checkerboard construction of test_patchnn's "ties" with grey levels that make two DIFFERENT distances tie: cells of
    a = 40 and b = 220, a constant query of 100.  A window inside an a cell is at d2 = 441 * 60^2 = 1 587 600, one inside a b
    cell at 441 * 120^2 = 4 d2; weights 4 and 1 give both the score 6 350 400 (exact in fp32).  Windows across a cell border
    lie between the two distances and get weight 8, and so does every window of the first frame position, so the smallest
    tied index is not 0.  `first` is the grey level of the board's first cell."""
    t, y, x = np.meshgrid(np.arange(5), np.arange(40), np.arange(48), indexing="ij")
    lo, hi = (40, 220) if first == 40 else (220, 40)
    board = np.where(((y // 8) + (x // 8)) % 2 == 0, lo, hi).astype(np.uint8)
    r = np.ascontiguousarray(np.repeat(board[..., None], 3, axis=3))
    q = np.full((3, 9, 10, 3), 100, np.uint8)
    patch = (3, 7, 7)
    R, grid = _patches(r, patch, ONE)
    w = np.full(len(R), 8.0, np.float32)
    w[(R == 40).all(1)] = 4.0
    w[(R == 220).all(1)] = 1.0
    w[:grid[1] * grid[2]] = 8.0
    return q, r, patch, w, grid


@pytest.mark.gpu
@pytest.mark.parametrize("first", [40, 220])
def test_ties_between_different_distances_resolve_to_smallest_index(first):
    q, r, patch, w, grid = _tie_case(first)
    want_score, want_nn = brute_weighted(q, r, w, patch)
    d2_all = ((_patches(q, patch, ONE)[0][0][None, :] - _patches(r, patch, ONE)[0]) ** 2).sum(1)
    tied = np.flatnonzero(d2_all.astype(np.float32) * w == np.float32(6350400.0))
    assert set(d2_all[tied]) == {1587600.0, 6350400.0} and len(tied) > 100       # two distances, one score
    assert (d2_all.astype(np.float32) * w).min() == np.float32(6350400.0)
    assert (want_nn == tied[0]).all() and tied[0] == grid[1] * grid[2]
    assert d2_all[tied[0]] == (1587600.0 if first == 40 else 6350400.0)           # either distance can be the winner
    score, nn = _run_weighted(q, r, w, patch, ONE, ONE)
    assert torch.equal(nn.to(torch.int64), torch.from_numpy(want_nn))
    assert torch.equal(score, torch.from_numpy(want_score)) and float(score[0, 0, 0]) == 6350400.0


@pytest.mark.gpu
def test_weighted_deterministic_across_runs_and_streams():
    q, r, patch, qs, rs, w, want_score, want_nn, _ = _wcase("merge")
    qd, rd, wd = _dev(q), _dev(r), _dev(w)
    a = ops.patch_nn_weighted(qd, rd, wd, patch)
    b = ops.patch_nn_weighted(qd, rd, wd, patch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.patch_nn_weighted(qd, rd, wd, patch)
    side.synchronize()
    for got in (b, c):
        assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])
    assert torch.equal(a[1].cpu().to(torch.int64), torch.from_numpy(want_nn))


@pytest.mark.gpu
def test_weighted_refuses_bad_weights():
    q, r, patch = _case("nq1")[:3]
    qd, rd = _dev(q), _dev(r)
    Nr = 2 * 3 * 4
    good = torch.ones(Nr, device="cuda")
    assert ops.patch_nn_weighted(qd, rd, good.reshape(2, 3, 4), patch)[1].numel() == 1       # grid-shaped weights are taken
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = good.clone()
        w[Nr // 2] = bad
        with pytest.raises(RuntimeError, match="finite and > 0"):
            ops.patch_nn_weighted(qd, rd, w, patch)
    for w in (good[:-1], good.double(), good.cpu(), good.reshape(4, 6), None):
        with pytest.raises(RuntimeError, match="ref_weight must be float32"):
            ops.patch_nn_weighted(qd, rd, w, patch)


@pytest.mark.gpu
def test_weighted_short_workspace_is_refused():
    q = torch.zeros(3, 8, 8, 3, dtype=torch.uint8, device="cuda")
    w = torch.ones(4, device="cuda")
    score = torch.empty(4, dtype=torch.float32, device="cuda")
    nn = torch.empty(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    one = I3(1, 1, 1)
    need = hplib.call("hpvg_patchnn_ws_bytes", 3, 8, 8, 3, 8, 8, I3(3, 7, 7), one, one)
    f = hplib.load().hpvg_patchnn_weighted_u8
    args = (hplib.ptr(q), 3, 8, 8, hplib.ptr(q), 3, 8, 8, I3(3, 7, 7), one, one, hplib.ptr(w), hplib.ptr(score), hplib.ptr(nn), hplib.ptr(ws))
    assert f(*args, need - 1, hplib.stream()) == ERR_WORKSPACE
    assert f(*args, need, hplib.stream()) == 0
    torch.cuda.synchronize()
    assert nn.cpu().tolist() == [0] * 4 and score.cpu().tolist() == [0.0] * 4      # four copies of one black patch


# ------------------------------------------------------------------------------------------------------------------ vote
@functools.lru_cache(maxsize=None)
def _vcase(name):
    """(values, nn, patch, fallback, qstride, rstride, want, cnt)"""
    rng = np.random.default_rng(40)
    patch, qs, rs = (3, 7, 7), ONE, ONE
    values, fallback = _rand((5, 17, 31), 21), _rand((4, 20, 23), 22)
    if name == "qstride":
        qs = (1, 2, 3)
    elif name == "rstride":
        rs = (2, 1, 2)
    elif name == "image":
        values, fallback, patch = _rand((17, 31), 23)[None], _rand((20, 23), 24)[None], (1, 5, 5)
    Nq, Nr = ops.patch_vote_counts(fallback.shape[:3], values.shape[:3], patch, qs, rs)[:2]
    nn = rng.integers(0, Nr, size=Nq).astype(np.int32)
    if name == "invalid":
        nn[rng.random(Nq) < 0.3] = -1
        nn[rng.random(Nq) < 0.3] = Nr
        nn[:40] = -7            # the corner voxel's only patch, and its neighbours: some voxels lose every vote
        nn[-1] = 2 ** 31 - 1
    return (values, nn, patch, fallback, qs, rs) + vote_ref(values, nn, patch, fallback, qs, rs)


def _run_vote(values, nn, patch, fallback, qs, rs, image=False):
    if image:
        values, fallback = values[0], fallback[0]
    out = ops.patch_vote(_dev(values), _dev(nn), patch, fallback.shape[:-1], _dev(fallback), qs, rs)
    assert out.dtype == torch.uint8 and tuple(out.shape) == fallback.shape
    return out.cpu().numpy()[None] if image else out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense", "qstride", "rstride", "image", "invalid"])
def test_vote_equals_numpy(name):
    values, nn, patch, fallback, qs, rs, want, cnt = _vcase(name)
    uncovered = ops.patch_vote_counts(fallback.shape[:3], values.shape[:3], patch, qs, rs)[2]
    if name == "qstride":
        # W = 23, patch 7, stride 3: the grid's last patch ends at x = 21, so column 22 has no vote; H = 20 at stride 2: row 19
        assert uncovered == (cnt == 0).sum() == 4 * 20 * 23 - 4 * 19 * 22 > 0
        assert np.array_equal(want[cnt == 0], fallback[cnt == 0])
    elif name == "invalid":
        assert uncovered == 0 and (cnt == 0).sum() > 0 and cnt[0, 0, 0] == 0 and (cnt > 0).sum() > cnt.size // 2
    else:
        assert uncovered == 0 == (cnt == 0).sum()
    got = _run_vote(values, nn, patch, fallback, qs, rs, image=(name == "image"))
    assert np.array_equal(got, want), name


@pytest.mark.gpu
def test_vote_extremes_and_half_up():
    v = torch.full((5, 17, 31, 3), 255, dtype=torch.uint8, device="cuda")
    fb = torch.zeros(4, 20, 23, 3, dtype=torch.uint8, device="cuda")
    nn = _dev(_vcase("dense")[1])
    assert int(ops.patch_vote(v, nn, (3, 7, 7), (4, 20, 23), fb).min()) == 255
    # values 0 255 255 0 along x, patch 1 x 1 x 2: value patch 2 is (255, 0).  Both query patches take it, so the middle
    # voxel gets 0 (patch 0, offset 1) and 255 (patch 1, offset 0): 127.5 -> 128
    v = _dev(np.repeat(np.array([0, 255, 255, 0], np.uint8)[None, None, :, None], 3, axis=3))
    fb = torch.full((1, 1, 3, 3), 7, dtype=torch.uint8, device="cuda")
    out = ops.patch_vote(v, torch.tensor([2, 2], dtype=torch.int32, device="cuda"), (1, 1, 2), (1, 1, 3), fb)
    assert out.cpu()[0, 0].tolist() == [[255] * 3, [128] * 3, [0] * 3]


@pytest.mark.gpu
def test_vote_deterministic_and_refuses_aliasing():
    values, nn, patch, fallback, qs, rs, want, _ = _vcase("dense")
    vd, nd, fd = _dev(values), _dev(nn), _dev(fallback)
    a = ops.patch_vote(vd, nd, patch, fallback.shape[:3], fd)
    b = ops.patch_vote(vd, nd, patch, fallback.shape[:3], fd)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)
    geo = (5, 17, 31, hplib.ptr(nd), 4, 20, 23, I3(*patch), I3(*ONE), I3(*ONE), hplib.ptr(fd))
    f = hplib.load().hpvg_patch_vote_u8
    for alias in (fd, vd, nd):        # out over fallback, values or nn: refused before anything is launched
        assert f(hplib.ptr(vd), *geo, hplib.ptr(alias), hplib.stream()) == ERR_ARG
    with pytest.raises(RuntimeError, match="nn must be int32 with 476 entries"):
        ops.patch_vote(vd, nd[:-1], patch, fallback.shape[:3], fd)
    with pytest.raises(RuntimeError, match="out_shape"):
        ops.patch_vote(vd, nd, patch, (4, 20, 22), fd)


# ------------------------------------------------------------------------------------------------------- one refine step
@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.005, float("inf")])
def test_refine_step_equals_numpy_composition(alpha):
    query, keys, values, patch = _rand((4, 20, 23), 1), _rand((5, 17, 31), 2), _rand((5, 17, 31), 11), (3, 7, 7)
    alpha_abs = alpha * 441 * 255 * 255
    if np.isinf(alpha):
        nn = brute(query, keys, patch)[1]
    else:
        m = brute(keys, query, patch)[0]
        w = np.float32(1.0) / (m.astype(np.float32) + np.float32(alpha_abs))
        assert w.dtype == np.float32 and w.min() > 1e-9
        nn = brute_weighted(query, keys, w, patch)[1]
        assert (nn != brute(query, keys, patch)[1]).any()
        # the two intermediate results, bit for bit: the device's divide is the correctly rounded one, and so are the winners
        md = ops.patch_nn(_dev(keys), _dev(query), patch)[0]
        wd = generate_patchnn.patchnn_weights(md, alpha_abs)
        assert wd.dtype == torch.float32 and torch.equal(wd.cpu().view(torch.int32), torch.from_numpy(w.view(np.int32)))
        nnd = ops.patch_nn_weighted(_dev(query), _dev(keys), wd, patch)[1]
        assert torch.equal(nnd.cpu().to(torch.int64), torch.from_numpy(nn))
    want = vote_ref(values, nn, patch, query)[0]
    got = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------- host
def test_new_exports_are_declared_and_bound():
    declared = hplib.check_symbols()
    for name in ("hpvg_patchnn_weighted_u8", "hpvg_patch_vote_u8", "hpvg_patch_vote_counts"):
        assert name in declared


@pytest.mark.parametrize("why", sorted(BAD))
def test_bad_arguments_return_err_arg_from_the_new_entry_points(why):
    qs, rs, patch, qstride, rstride = BAD[why]
    lib = hplib.load()
    dummy = ctypes.create_string_buffer(64)   # never touched: the geometry is refused first
    p = ctypes.cast(dummy, ctypes.c_void_p)
    geo = (I3(*patch), I3(*qstride), I3(*rstride))
    assert lib.hpvg_patchnn_weighted_u8(p, *qs, p, *rs, *geo, p, p, p, p, 64, None) == ERR_ARG
    assert lib.hpvg_patch_vote_u8(p, *rs, p, *qs, *geo, p, ctypes.c_void_p(p.value + 32), None) == ERR_ARG
    assert lib.hpvg_patch_vote_counts(*qs, *rs, *geo, (ctypes.c_long * 3)()) == ERR_ARG


def test_null_pointers_return_err_arg():
    lib = hplib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    geo = (I3(3, 7, 7), I3(*ONE), I3(*ONE))
    for k in (0, 2, 4, 5, 6):    # q, r, rweight, score, nn
        ptrs = [p, (4, 20, 23), p, (5, 17, 31), p, p, p]
        ptrs[k] = None
        assert lib.hpvg_patchnn_weighted_u8(ptrs[0], *ptrs[1], ptrs[2], *ptrs[3], *geo, ptrs[4], ptrs[5], ptrs[6], p, 1 << 40, None) == ERR_ARG
    assert lib.hpvg_patchnn_weighted_u8(p, 4, 20, 23, p, 5, 17, 31, *geo, p, p, p, None, 1 << 40, None) == ERR_WORKSPACE
    for k in range(4):           # v, nn, fallback, out
        ptrs = [p, p, p, ctypes.c_void_p(p.value + 32)]
        ptrs[k] = None
        assert lib.hpvg_patch_vote_u8(ptrs[0], 5, 17, 31, ptrs[1], 4, 20, 23, *geo, ptrs[2], ptrs[3], None) == ERR_ARG
    assert lib.hpvg_patch_vote_counts(4, 20, 23, 5, 17, 31, *geo, None) == ERR_ARG


def test_vote_counts_match_a_numpy_cover():
    for shape in [(1, 9, 11), (4, 20, 23), (7, 16, 40)]:
        for patch in [(1, 1, 1), (1, 5, 5), (3, 7, 7)]:
            if patch[0] > shape[0]:
                continue
            for stride in [(1, 1, 1), (1, 2, 3), (2, 1, 2), (3, 5, 4), (1, 8, 9)]:
                cover = np.zeros(shape, bool)
                n = 0
                for t0 in range(0, shape[0] - patch[0] + 1, stride[0]):
                    for y0 in range(0, shape[1] - patch[1] + 1, stride[1]):
                        for x0 in range(0, shape[2] - patch[2] + 1, stride[2]):
                            cover[t0:t0 + patch[0], y0:y0 + patch[1], x0:x0 + patch[2]] = True
                            n += 1
                got = ops.patch_vote_counts(shape, (7, 16, 40), patch, stride, (1, 1, 1))
                assert got[0] == n and got[2] == int((~cover).sum()), (shape, patch, stride)
                assert got[1] == (8 - patch[0]) * (17 - patch[1]) * (41 - patch[2])


def test_generate_patchnn_parser_defaults_and_arities():
    p = generate_patchnn.generate_patchnn_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.exp_dir, a.video_path, a.image_path, a.out, a.num_samples, a.seed, a.patch, a.ratio, a.min_size, a.iters, a.alpha, a.noise,
            a.size) == ("e", None, None, None, 8, 0, None, 0.75, 16, 10, 0.005, 0.75, None)
    a = p.parse_args(["--video-path", "c.npy", "--out", "o", "--patch", "1", "5", "5", "--size", "6", "40", "64", "--alpha", "inf",
                      "--noise", "0", "--iters", "2", "--num-samples", "3", "--seed", "9", "--ratio", "0.5", "--min-size", "30"])
    assert a.patch == [1, 5, 5] and a.size == [6, 40, 64] and a.alpha == float("inf") and a.noise == 0.0
    assert (a.iters, a.num_samples, a.seed, a.ratio, a.min_size, a.video_path, a.out) == (2, 3, 9, 0.5, 30, "c.npy", "o")
    for bad in (["--patch", "7", "7"], ["--patch", "3", "7", "7", "7"], ["--size", "40", "64"], ["--alpha", "0"], ["--alpha", "-1"],
                ["--alpha", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--exp-dir", "e"] + bad)


def test_pyramid_sizes_by_hand():
    f = generate_patchnn.patchnn_pyramid_sizes
    # 144 * 0.75^7 = 19.2 >= 16 > 144 * 0.75^8 = 14.4: eight levels.  60.75 -> 61, 45.5625 -> 46, 34.17 -> 34, 25.6 -> 26
    assert f((13, 144, 256), 0.75, 16) == [(13, 19, 34), (13, 26, 46), (13, 34, 61), (13, 46, 81), (13, 61, 108), (13, 81, 144),
                                           (13, 108, 192), (13, 144, 256)]
    assert f((6, 40, 48), 0.75, 30) == [(6, 30, 36), (6, 40, 48)]          # 22.5 rounds up to 23 < 30
    assert f((6, 40, 48), 0.75, 23) == [(6, 23, 27), (6, 30, 36), (6, 40, 48)]
    assert f((6, 40, 48), 0.75, 100) == [(6, 40, 48)]                      # at least one level
    assert f((1, 64, 32), 0.5, 8, (1, 7, 7)) == [(1, 16, 8), (1, 32, 16), (1, 64, 32)]
    assert f((4, 10, 10), 0.5, 10) == [(4, 10, 10)]


def test_pyramid_sizes_refuse_a_patch_larger_than_the_coarsest_level():
    f = generate_patchnn.patchnn_pyramid_sizes
    with pytest.raises(ValueError, match="smaller than the patch"):
        f((13, 144, 256), 0.75, 4)            # coarsest 5 x 8 against 7 x 7
    with pytest.raises(ValueError, match="smaller than the patch"):
        f((2, 144, 256), 0.75, 16)            # T = 2 against 3
    with pytest.raises(ValueError, match="smaller than the patch"):
        f((1, 6, 40), 0.75, 100, (1, 7, 7))   # one level, already too small
    assert f((2, 144, 256), 0.75, 64, (1, 7, 7))[0] == (2, 81, 144)
    with pytest.raises(ValueError, match="ratio"):
        f((13, 144, 256), 1.0, 16)


def test_generate_patchnn_needs_one_input_and_an_out():
    with pytest.raises(SystemExit, match="exactly one"):
        generate_patchnn.generate_patchnn()
    with pytest.raises(SystemExit, match="exactly one"):
        generate_patchnn.generate_patchnn(exp_dir="e", video_path="c.npy")
    with pytest.raises(SystemExit, match="need --out"):
        generate_patchnn.generate_patchnn(video_path="c.npy")
