"""Exact patch nearest neighbours (hpvg_patchnn_u8 / ops.patch_nn) against a numpy brute force, and the host-side pieces of the
evaluate program.

The yardstick is written from the definition: both patch matrices gathered with sliding_window_view, |q|^2 + |r|^2 - 2 Q R^T as a
float64 matmul (exact: every value is an integer far below 2^53), argmin along j (numpy returns the first minimum, i.e. the
smallest index).  Every comparison is torch.equal / ==; there is no tolerance anywhere.

The kernel's tile is 128 x 128 patches with a K step of 64 bytes; the column range is split over workgroups until the grid has
about 2048 of them.  The cross-workgroup case of 5 304 x 5 248 patches therefore runs 42 row tiles x 41 column splits, and the
K-padding case (D = 441 -> 448) 7 K steps with ragged row and column tiles."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

from hp_vae_gan_amd import lib as hplib
from hp_vae_gan_amd import evaluate, ops
from patch_ref import _patches, brute  # noqa: F401

ERR_ARG = -1
I3 = ctypes.c_int * 3


# ------------------------------------------------------------------------------------------------------------ yardstick
def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(q, r, patch, qstride, rstride, want_d2, want_nn) - built and brute-forced once, then shared (and never modified)."""
    one = (1, 1, 1)
    if name in ("lane1", "lane8"):
        x, c = np.arange(40)[:, None], np.arange(3)[None, :]
        q = ((7 * x + 3 * c) % 251).astype(np.uint8).reshape(1, 1, 40, 3)
        x = np.arange(37)[:, None]
        r = ((5 * x + 11 * c + 1) % 253).astype(np.uint8).reshape(1, 1, 37, 3)
        args = (q, r, (1, 1, 1) if name == "lane1" else (1, 1, 8), one, one)
    elif name == "ragged":
        args = (_rand((4, 20, 23), 1), _rand((5, 17, 31), 2), (3, 7, 7), one, one)
    elif name == "ragged_strided":
        args = (_rand((4, 20, 23), 1), _rand((5, 17, 31), 2), (3, 7, 7), (1, 2, 3), (2, 1, 2))
    elif name == "merge":
        args = (_rand((6, 40, 45), 3), _rand((6, 38, 47), 4), (3, 7, 7), one, one)
    elif name == "ties":
        t, y, x = np.meshgrid(np.arange(5), np.arange(40), np.arange(48), indexing="ij")
        board = np.where(((y // 8) + (x // 8)) % 2 == 0, 40, 215).astype(np.uint8)
        r = np.repeat(board[..., None], 3, axis=3)
        args = (np.ascontiguousarray(r[1:5, 5:37, 3:43]), r, (3, 7, 7), one, one)
    elif name == "nr1":
        args = (_rand((4, 9, 10), 5), _rand((3, 7, 7), 6), (3, 7, 7), one, one)
    elif name == "nq1":
        args = (_rand((3, 7, 7), 7), _rand((4, 9, 10), 8), (3, 7, 7), one, one)
    elif name == "image":
        args = (_rand((20, 23), 9), _rand((17, 31), 10), (1, 5, 5), one, one)
    else:
        raise KeyError(name)
    return args + brute(*args)


def _run(q, r, patch, qstride, rstride):
    d2, nn = ops.patch_nn(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), patch, qstride, rstride)
    return d2.cpu(), nn.cpu()


def _check(name):
    q, r, patch, qs, rs, want_d2, want_nn = _case(name)
    d2, nn = _run(q, r, patch, qs, rs)
    assert d2.dtype == torch.int32 and nn.dtype == torch.int32
    if q.ndim == 3:
        want_d2, want_nn = want_d2[0], want_nn[0]
    assert tuple(d2.shape) == want_d2.shape and tuple(nn.shape) == want_nn.shape
    assert torch.equal(d2.to(torch.int64), torch.from_numpy(want_d2)), name
    assert torch.equal(nn.to(torch.int64), torch.from_numpy(want_nn)), name
    return d2, nn


# --------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lane1", "lane8"])
def test_lane_map_asymmetric_data(name):
    """Data asymmetric in row, column and k: a transposed or k-permuted fragment cannot pass."""
    _check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "ragged_strided"])
def test_k_padding_and_ragged_tiles(name):
    q, r, patch, qs, rs = _case(name)[:5]
    assert ops.patch_nn_counts(q.shape[:3], r.shape[:3], patch, qs, rs) == ((476, 825, 441) if name == "ragged" else (84, 286, 441))
    _check(name)


@pytest.mark.gpu
def test_cross_workgroup_merge():
    q, r, patch = _case("merge")[:3]
    assert ops.patch_nn_counts(q.shape[:3], r.shape[:3], patch) == (5304, 5248, 441)
    _check("merge")


@pytest.mark.gpu
def test_ties_resolve_to_smallest_index():
    d2, nn = _check("ties")
    assert int((d2 == 0).sum()) == d2.numel()  # a crop: every patch exists in the reference
    want_nn = _case("ties")[6]
    assert len(np.unique(want_nn)) < want_nn.size // 4  # the board repeats: most patches have many exact copies


@pytest.mark.gpu
@pytest.mark.parametrize("qv,rv", [(0, 255), (255, 0)])
def test_extremes(qv, rv):
    patch = (5, 11, 11)
    q = torch.full((5, 12, 13, 3), qv, dtype=torch.uint8, device="cuda")
    r = torch.full((6, 11, 12, 3), rv, dtype=torch.uint8, device="cuda")
    d2, nn = ops.patch_nn(q, r, patch)
    assert tuple(d2.shape) == (1, 2, 3)
    assert 1815 * 255 * 255 == 118020375
    assert torch.equal(d2.cpu(), torch.full((1, 2, 3), 118020375, dtype=torch.int32))
    assert torch.equal(nn.cpu(), torch.zeros(1, 2, 3, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nr1", "nq1", "image"])
def test_small_counts_and_image_path(name):
    d2, nn = _check(name)
    if name == "nr1":
        assert int(nn.abs().sum()) == 0
    if name == "nq1":
        assert d2.numel() == 1
    if name == "image":
        assert d2.dim() == 2


@pytest.mark.gpu
def test_deterministic_across_runs_and_streams():
    q, r, patch, qs, rs, want_d2, want_nn = _case("merge")
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    a = ops.patch_nn(qd, rd, patch)
    b = ops.patch_nn(qd, rd, patch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.patch_nn(qd, rd, patch)
    side.synchronize()
    for got in (b, c):
        assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])
    assert torch.equal(a[1].cpu().to(torch.int64), torch.from_numpy(want_nn))


@pytest.mark.gpu
def test_short_workspace_is_refused():
    q = torch.zeros(3, 8, 8, 3, dtype=torch.uint8, device="cuda")
    out = torch.empty(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    one = I3(1, 1, 1)
    need = hplib.call("hpvg_patchnn_ws_bytes", 3, 8, 8, 3, 8, 8, I3(3, 7, 7), one, one)
    rc = hplib.load().hpvg_patchnn_u8(hplib.ptr(q), 3, 8, 8, hplib.ptr(q), 3, 8, 8, I3(3, 7, 7), one, one, hplib.ptr(out),
                                      hplib.ptr(out), hplib.ptr(ws), need - 1, hplib.stream())
    assert rc == -2


# ----------------------------------------------------------------------------------------------------------------- host
def test_counts_match_sliding_window_view():
    for (T, H, W) in [(1, 9, 11), (4, 20, 23), (7, 16, 40)]:
        vol = np.zeros((T, H, W, 3), np.uint8)
        for patch in [(1, 1, 1), (1, 5, 5), (3, 7, 7), (T, H, W)]:
            if patch[0] > T:
                continue
            for stride in [(1, 1, 1), (1, 2, 3), (2, 1, 2), (3, 5, 4)]:
                grid = _patches(vol, patch, stride)[1]
                n = grid[0] * grid[1] * grid[2]
                assert ops.patch_nn_counts((T, H, W), (T, H, W), patch, stride, (1, 1, 1))[::2] == (n, 3 * patch[0] * patch[1] * patch[2])
                assert ops.patch_nn_counts((T, H, W), (T, H, W), patch, (1, 1, 1), stride)[1] == n


def test_ws_bytes_positive_and_monotone_in_nq():
    one = I3(1, 1, 1)
    prev = 0
    for Tq in range(3, 40, 3):
        b = hplib.call("hpvg_patchnn_ws_bytes", Tq, 20, 23, 5, 17, 31, I3(3, 7, 7), one, one)
        assert b > 0 and b >= prev
        prev = b
    assert prev > hplib.call("hpvg_patchnn_ws_bytes", 3, 20, 23, 5, 17, 31, I3(3, 7, 7), one, one)


BAD = {
    "patch larger than the query": ((2, 20, 23), (5, 17, 31), (3, 7, 7), (1, 1, 1), (1, 1, 1)),
    "patch larger than the reference": ((4, 20, 23), (5, 6, 31), (3, 7, 7), (1, 1, 1), (1, 1, 1)),
    "query stride 0": ((4, 20, 23), (5, 17, 31), (3, 7, 7), (1, 0, 1), (1, 1, 1)),
    "reference stride -1": ((4, 20, 23), (5, 17, 31), (3, 7, 7), (1, 1, 1), (1, 1, -1)),
    "D * 255^2 = 2^31 + 97027": ((1, 101, 109), (1, 101, 109), (1, 101, 109), (1, 1, 1), (1, 1, 1)),   # D = 33 027
    "D far too large": ((11, 55, 55), (11, 55, 55), (11, 55, 55), (1, 1, 1), (1, 1, 1)),
    "Nq = 2^31": ((2048, 1024, 1024), (1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1)),
    "Nr = 2^31": ((1, 1, 1), (2048, 1024, 1024), (1, 1, 1), (1, 1, 1), (1, 1, 1)),
    "patch 0": ((4, 20, 23), (5, 17, 31), (3, 0, 7), (1, 1, 1), (1, 1, 1)),
}


@pytest.mark.parametrize("why", sorted(BAD))
def test_bad_arguments_return_err_arg(why):
    qs, rs, patch, qstride, rstride = BAD[why]
    lib = hplib.load()
    args = (*qs, *rs, I3(*patch), I3(*qstride), I3(*rstride))
    assert lib.hpvg_patchnn_counts(*args, (ctypes.c_int * 3)()) == ERR_ARG
    assert lib.hpvg_patchnn_ws_bytes(*args) == 0
    # the launch entry point refuses the geometry before it touches a pointer or the device
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    assert lib.hpvg_patchnn_u8(p, *qs, p, *rs, I3(*patch), I3(*qstride), I3(*rstride), p, p, p, 64, None) == ERR_ARG


def test_largest_allowed_patch_is_accepted():
    out = (ctypes.c_int * 3)()   # D = 33 024: D * 255^2 = 2^31 - 98 048
    assert hplib.load().hpvg_patchnn_counts(1, 86, 128, 1, 86, 128, I3(1, 86, 128), I3(1, 1, 1), I3(1, 1, 1), out) == 0
    assert list(out) == [1, 1, 33024]


# ------------------------------------------------------------------------------------------------------ evaluate, host side
def test_evaluate_parser_defaults_and_patch_arity():
    p = evaluate.evaluate_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.exp_dir, a.samples, a.real, a.patch, a.stride, a.max_samples, a.out) == ("e", None, None, None, [1, 1, 1], None, None)
    a = p.parse_args(["--samples", "s.npy", "--real", "r.npy", "--patch", "1", "5", "5", "--stride", "1", "2", "2", "--max-samples", "3"])
    assert a.patch == [1, 5, 5] and a.stride == [1, 2, 2] and a.max_samples == 3 and a.exp_dir is None
    for bad in (["--patch", "7", "7"], ["--patch", "3", "7", "7", "7"], ["--stride", "2"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--exp-dir", "e"] + bad)


def test_metric_arithmetic():
    D = 441
    assert evaluate.patch_score(torch.zeros(4, 5, dtype=torch.int32), D) == 0.0
    assert evaluate.patch_score(torch.full((2, 3, 4), D * 255 * 255, dtype=torch.int32), D) == 1.0
    assert evaluate.patch_score(torch.tensor([0, D * 255 * 255], dtype=torch.int32), D) == 0.5
    # sums past 2^31 stay exact
    assert evaluate.patch_score(torch.full((1000,), 118020375, dtype=torch.int32), 1815) == 1.0
    nn = torch.tensor([[0, 3, 3], [7, 7, 0]], dtype=torch.int32)
    assert evaluate.nn_unique_frac(nn, 100) == 3 / 6
    assert evaluate.nn_unique_frac(nn, 4) == 3 / 4
    # diversity: two constant samples 10 and 30 -> per-pixel deviation 10; real half 0, half 100 -> deviation 50
    s = torch.stack([torch.full((2, 4, 4, 3), 10, dtype=torch.uint8), torch.full((2, 4, 4, 3), 30, dtype=torch.uint8)])
    real = torch.cat([torch.zeros(3, 4, 2, 3), torch.full((3, 4, 2, 3), 100.0)], 2).to(torch.uint8)
    assert evaluate.diversity(s, real) == 0.2   # real is cut to the samples' 2 frames
    # the channel MEAN is what varies: samples that differ only in how a fixed sum is spread over the channels have none
    a = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    a[..., 0] = 30
    b = torch.full((1, 4, 4, 3), 10, dtype=torch.uint8)
    assert evaluate.diversity(torch.stack([a, b]), real[:1]) == 0.0
    assert evaluate.diversity(s[:1], real) is None                      # one sample
    assert evaluate.diversity(s, real[:1]) is None                      # real shorter than the samples
    assert evaluate.diversity(s, real[:, :3]) is None                   # other H
    img = torch.stack([torch.full((4, 4, 3), 10, dtype=torch.uint8), torch.full((4, 4, 3), 30, dtype=torch.uint8)])
    assert evaluate.diversity(img, real[0]) == 0.2
