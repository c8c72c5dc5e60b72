"""ops.patch_knn_self and ops.patch_ball_count (hpvg_patchknn_self_u8 / hpvg_patch_ball_count_u8) against the numpy yardstick of
tests/prdc_ref.py.  Every comparison is torch.equal / ==; there is no tolerance anywhere.

The shapes are those of test_patchnn.py, the smallest at which the 128 x 128 tile with its K step of 64 bytes can go wrong: one
row tile with D far below one K step (40 points, patches 1x1x1 and 1x1x8), ragged row and column tiles with D = 441 -> 448
(476 patches; 84 at stride 1 2 3), and 5 304 patches = 42 row tiles, where the column range is split over workgroups and the
lists (or counts) of a row come from many of them.  The checkerboard has many exact duplicates, so multiplicity and the
exclusion of a patch from its own list decide its radii.  k = 1, 3, 4 run the 4-slot instance, k = 5, 8 the 8-slot one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from hp_vae_gan_amd import lib as hplib
from hp_vae_gan_amd import ops

from prdc_ref import dist2, patches, ref_knn_self

pytestmark = pytest.mark.gpu
ONE = (1, 1, 1)
I3 = ctypes.c_int * 3
KS = (1, 3, 4, 5, 8)


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def _board():
    t, y, x = np.meshgrid(np.arange(5), np.arange(40), np.arange(48), indexing="ij")
    board = np.where(((y // 8) + (x // 8)) % 2 == 0, 40, 215).astype(np.uint8)
    return np.repeat(board[..., None], 3, axis=3)


def _lane(n, a, b, c0, mod):
    x, c = np.arange(n)[:, None], np.arange(3)[None, :]
    return ((a * x + b * c + c0) % mod).astype(np.uint8).reshape(1, 1, n, 3)


# ------------------------------------------------------------------------------------------------------ self k-nearest
@functools.lru_cache(maxsize=None)
def _knn_case(name):
    """(vol, patch, stride, N, want [grid..., kmax]) - built once, then shared and never modified; kmax = min(8, N - 1)."""
    if name in ("lane1", "lane8"):
        args = (_lane(40, 7, 3, 0, 251), (1, 1, 1) if name == "lane1" else (1, 1, 8), ONE)
    elif name == "ragged":
        args = (_rand((4, 20, 23), 1), (3, 7, 7), ONE)
    elif name == "ragged_strided":
        args = (_rand((4, 20, 23), 1), (3, 7, 7), (1, 2, 3))
    elif name == "merge":
        args = (_rand((6, 40, 45), 3), (3, 7, 7), ONE)
    elif name == "ties":
        vol = _board().copy()      # a block of noise: the patches that touch it have no copy anywhere
        vol[:, 12:20, 14:22] = _rand((5, 8, 8), 7)
        args = (vol, (3, 7, 7), ONE)
    elif name == "n4":
        args = (_rand((3, 7, 10), 5), (3, 7, 7), ONE)
    elif name == "n9":
        args = (_rand((3, 9, 9), 6), (3, 7, 7), ONE)
    elif name == "image":
        args = (_rand((20, 23), 9), (1, 5, 5), ONE)
    else:
        raise KeyError(name)
    vol, patch, stride = args
    N = len(patches(vol[None] if vol.ndim == 3 else vol, patch, stride)[0])
    want = ref_knn_self(vol, patch, min(8, N - 1), stride)
    return vol, patch, stride, N, want[0] if vol.ndim == 3 else want


def _check_knn(name, ks=KS):
    vol, patch, stride, N, want = _knn_case(name)
    dev = torch.from_numpy(vol).cuda()
    for k in ks:
        if k >= N:
            continue
        got = ops.patch_knn_self(dev, patch, k, stride)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape[:-1] + (k,), (name, k)
        assert torch.equal(got.cpu().to(torch.int64), torch.from_numpy(want[..., :k])), (name, k)
    return N, want


@pytest.mark.parametrize("name", ["lane1", "lane8"])
def test_knn_lane_map_asymmetric_data(name):
    N, _ = _check_knn(name)
    assert N == (40 if name == "lane1" else 33)


@pytest.mark.parametrize("name", ["ragged", "ragged_strided"])
def test_knn_k_padding_and_ragged_tiles(name):
    N, _ = _check_knn(name)
    assert N == (476 if name == "ragged" else 84)


def test_knn_lists_merge_across_workgroups():
    N, want = _check_knn("merge")
    assert N == 5304 and int(want.min()) > 0


def test_knn_duplicates_count_with_multiplicity_and_self_is_excluded():
    N, want = _check_knn("ties")
    flat = want.reshape(N, -1)
    zeros = (flat == 0).sum(1)
    assert N == 4284 and int((zeros == 8).sum()) > N // 2     # most patches have eight exact copies elsewhere ...
    assert int((zeros == 0).sum()) > 100                      # ... those on the noise have none: counting self would give them a 0


def test_knn_n_equals_k_plus_one_and_the_image_path():
    assert _check_knn("n4", (1, 3))[0] == 4
    assert _check_knn("n9", (4, 5, 8))[0] == 9
    N, want = _check_knn("image")
    assert N == 16 * 19 and want.ndim == 3


def test_knn_is_the_same_on_a_second_run_and_another_stream():
    vol, patch, stride, _, _ = _knn_case("merge")
    dev = torch.from_numpy(vol).cuda()
    a = ops.patch_knn_self(dev, patch, 5)
    b = ops.patch_knn_self(dev, patch, 5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.patch_knn_self(dev, patch, 5)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_knn_refusals():
    vol = torch.from_numpy(_knn_case("n4")[0]).cuda()
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(RuntimeError, match=r"patch_knn_self: k must be an int in \[1, 8\]"):
            ops.patch_knn_self(vol, (3, 7, 7), k)
    for k in (4, 5, 8):
        with pytest.raises(RuntimeError, match="patch_knn_self: 4 patches cannot have %d neighbours" % k):
            ops.patch_knn_self(vol, (3, 7, 7), k)
    with pytest.raises(RuntimeError, match="hpvg_patchnn_counts failed: HPVG_ERR_ARG"):
        ops.patch_knn_self(vol, (4, 7, 7), 1)
    with pytest.raises(RuntimeError, match="vol must be uint8"):
        ops.patch_knn_self(vol.to(torch.int32), (3, 7, 7), 1)
    # the C entry itself, with real pointers
    out = torch.empty(4 * 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    lib, one, patch = hplib.load(), I3(1, 1, 1), I3(3, 7, 7)
    for k in (0, 9, 4):
        assert lib.hpvg_patchknn_self_ws_bytes(3, 7, 10, patch, one, k) == 0
        assert lib.hpvg_patchknn_self_u8(hplib.ptr(vol), 3, 7, 10, patch, one, k, hplib.ptr(out), hplib.ptr(ws), ws.numel(),
                                         hplib.stream()) == -1
    need = lib.hpvg_patchknn_self_ws_bytes(3, 7, 10, patch, one, 3)
    assert lib.hpvg_patchknn_self_u8(hplib.ptr(vol), 3, 7, 10, patch, one, 3, hplib.ptr(out), hplib.ptr(ws), need - 1,
                                     hplib.stream()) == -2


# ---------------------------------------------------------------------------------------------------------- ball count
@functools.lru_cache(maxsize=None)
def _ball_case(name):
    """(q, r, patch, qstride, rstride, {radii name: (radius int32 [Nr], want int64 [Nq])}) - built once, never modified."""
    if name == "ragged":
        args = (_rand((4, 20, 23), 1), _rand((5, 17, 31), 2), (3, 7, 7), ONE, ONE)
    elif name == "ragged_strided":
        args = (_rand((4, 20, 23), 1), _rand((5, 17, 31), 2), (3, 7, 7), (1, 2, 3), (2, 1, 2))
    elif name == "merge":
        args = (_rand((6, 40, 45), 3), _rand((6, 38, 47), 4), (3, 7, 7), ONE, ONE)
    elif name == "ties":
        r = _board()
        args = (np.ascontiguousarray(r[1:5, 5:37, 3:43]), r, (3, 7, 7), ONE, ONE)
    else:
        raise KeyError(name)
    q, r, patch, qs, rs = args
    Q, R = patches(q, patch, qs)[0], patches(r, patch, rs)[0]
    d = dist2(Q, R)
    Nq, Nr, D = len(Q), len(R), Q.shape[1]
    rng = np.random.default_rng(11)
    radii = {"zero": np.zeros(Nr, np.int64), "full": np.full(Nr, D * 255 * 255, np.int64),
             # a radius per key over the range of the actual distances: taken at another index, the counts change
             "random": rng.integers(int(d.min()), int(d.max()) + 1, size=Nr),
             # the distance of an actual pair: every key has a query exactly ON its sphere
             "equal": d[rng.integers(0, Nq, size=Nr), np.arange(Nr)]}
    return q, r, patch, qs, rs, {n: (rad.astype(np.int32), (d <= rad[None, :]).sum(1)) for n, rad in radii.items()}


def _check_ball(name):
    q, r, patch, qs, rs, radii = _ball_case(name)
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    grid = patches(q, patch, qs)[1]
    for n, (rad, want) in radii.items():
        got = ops.patch_ball_count(qd, rd, torch.from_numpy(rad).cuda(), patch, qs, rs)
        assert got.dtype == torch.int32 and tuple(got.shape) == grid, (name, n)
        assert torch.equal(got.cpu().to(torch.int64).reshape(-1), torch.from_numpy(want)), (name, n)
    return radii


@pytest.mark.parametrize("name", ["ragged", "ragged_strided"])
def test_ball_count_ragged_tiles(name):
    radii = _check_ball(name)
    Nq, Nr = (476, 825) if name == "ragged" else (84, 286)
    assert len(radii["full"][1]) == Nq and set(radii["full"][1].tolist()) == {Nr}      # padded columns never count
    assert int(radii["zero"][1].sum()) == 0                                           # random volumes share no patch
    want = radii["random"][1]
    assert int(want.min()) < Nr and int(want.max()) > 0
    assert len(set(want.tolist())) > 8
    assert int(radii["equal"][1].sum()) >= Nr


def test_ball_count_adds_up_across_workgroups():
    radii = _check_ball("merge")
    assert len(radii["full"][1]) == 5304 and set(radii["full"][1].tolist()) == {5248}
    assert len(set(radii["random"][1].tolist())) > 100


def test_ball_count_radius_zero_counts_the_exact_duplicates():
    radii = _check_ball("ties")
    want = radii["zero"][1]
    assert int(want.min()) >= 1 and int(want.max()) > 8        # a crop of the board: every patch exists, most many times


def test_ball_count_radius_grid_shaped_and_image_path():
    q, r = _rand((20, 23), 9), _rand((17, 31), 10)
    patch = (1, 5, 5)
    d = dist2(patches(q[None], patch)[0], patches(r[None], patch)[0])
    rad = np.random.default_rng(5).integers(int(d.min()), int(d.max()) + 1, size=d.shape[1])
    got = ops.patch_ball_count(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(),
                               torch.from_numpy(rad.astype(np.int32).reshape(13, 27)).cuda(), patch)
    assert tuple(got.shape) == (16, 19)
    assert torch.equal(got.cpu().to(torch.int64).reshape(-1), torch.from_numpy((d <= rad[None, :]).sum(1)))


def test_ball_count_refusals():
    q, r, patch, qs, rs, radii = _ball_case("ragged_strided")
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    rad = torch.from_numpy(radii["random"][0]).cuda()
    bad = rad.clone()
    bad[17] = -1
    with pytest.raises(RuntimeError, match="patch_ball_count: every ref_radius must be >= 0"):
        ops.patch_ball_count(qd, rd, bad, patch, qs, rs)
    for wrong in (rad[:-1], torch.cat([rad, rad[:1]]), rad.to(torch.int64), rad.to(torch.float32), rad.cpu(), rad.tolist()):
        with pytest.raises(RuntimeError, match=r"patch_ball_count: ref_radius must be int32 \[286\]"):
            ops.patch_ball_count(qd, rd, wrong, patch, qs, rs)
    with pytest.raises(RuntimeError, match="hpvg_patchnn_counts failed: HPVG_ERR_ARG"):
        ops.patch_ball_count(qd, rd, rad, patch, (1, 0, 1), rs)


def test_ball_count_clears_its_output_itself():
    q, r, patch, qs, rs, radii = _ball_case("ragged_strided")
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    rad, want = radii["random"]
    radd = torch.from_numpy(rad).cuda()
    count = torch.full((84,), 12345, dtype=torch.int32, device="cuda")          # garbage before the first call
    ws = torch.empty(4 << 20, dtype=torch.uint8, device="cuda")
    args = (hplib.ptr(qd), *q.shape[:3], hplib.ptr(rd), *r.shape[:3], I3(*patch), I3(*qs), I3(*rs), hplib.ptr(radd), hplib.ptr(count))
    need = hplib.call("hpvg_patch_ball_count_ws_bytes", *q.shape[:3], *r.shape[:3], I3(*patch), I3(*qs), I3(*rs))
    assert 0 < need <= ws.numel()
    for _ in range(2):
        hplib.call("hpvg_patch_ball_count_u8", *args, hplib.ptr(ws), ws.numel(), hplib.stream())
        assert torch.equal(count.cpu().to(torch.int64), torch.from_numpy(want))
    assert hplib.load().hpvg_patch_ball_count_u8(*args, hplib.ptr(ws), need - 1, hplib.stream()) == -2
