"""Exact sliced Wasserstein patch distance: the projection histograms (hpvg_patchproj_hist_u8 / ops.patch_proj_hist) and the W1
numerator (hpvg_hist_w1_i32 / ops.hist_w1) against numpy written from the definition, and the host-side pieces of evaluate --swd.

The yardstick: the patch matrix gathered with sliding_window_view (test_patchnn._patches), (patches - 128) @ S.T in int64,
np.bincount per direction over NB = 256 D + 1 bins; np.cumsum and num_p = sum_b |Nb cA_p(b) - Na cB_p(b)| in Python integers.
Every comparison is torch.equal / ==; there is no tolerance anywhere.

The kernel's tile is 128 patches x 128 directions with a K step of 64 bytes, one workgroup per 128 patches walking the direction
tiles; the W1 kernel walks the bins in chunks of 1024."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from patch_ref import ref_hist, ref_num  # noqa: E402
from test_patchnn import _case as _nn_case  # noqa: E402
from test_patchnn import _patches, _rand  # noqa: E402

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import evaluate, ops  # noqa: E402

ERR_ARG, ERR_WS = -1, -2
I3 = ctypes.c_int * 3
ONE = (1, 1, 1)


# ------------------------------------------------------------------------------------------------------------ yardstick
def _dirs(P, D, seed):
    """Random {-1, 0, +1} directions, none all-zero (row p gets a +1 at k = p % D where the draw left it empty)."""
    S = np.random.default_rng(seed).integers(-1, 2, size=(P, D), dtype=np.int8)
    for p in np.flatnonzero(~S.any(1)):
        S[p, p % D] = 1
    return S


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vol, patch, stride, S, want_hist, N) - built once, then shared (and never modified)."""
    if name in ("lane8_q", "lane8_r"):
        # 24 rows +e_k and 24 rows -e_k (48 directions: every byte of the patch on its own, with either sign), then 4 mixed rows
        q, r, patch = _nn_case("lane8")[:3]
        eye = np.eye(24, dtype=np.int8)
        args = (q if name == "lane8_q" else r, patch, ONE, np.concatenate([eye, -eye, _dirs(4, 24, 11)]))
    elif name == "ragged":
        args = (_rand((4, 20, 23), 1), (3, 7, 7), ONE, _dirs(130, 441, 12))
    elif name == "ragged_strided":
        args = (_rand((4, 20, 23), 1), (3, 7, 7), (1, 2, 3), _dirs(130, 441, 12))
    elif name == "other":      # the second volume of the unequal-count W1 case
        args = (_rand((5, 17, 31), 2), (3, 7, 7), ONE, _dirs(130, 441, 12)[:6])
    elif name == "image":
        args = (_rand((20, 23), 9), (1, 5, 5), ONE, _dirs(7, 75, 13))
    elif name == "n1":
        args = (_rand((3, 7, 7), 7), (3, 7, 7), ONE, _dirs(5, 441, 14))
    elif name == "p1":
        args = (_rand((4, 9, 10), 5), (3, 7, 7), ONE, _dirs(1, 441, 15))
    elif name in ("tiny_a", "tiny_b"):   # D = 3: NB = 769, less than one chunk of the W1 kernel
        q, r = _nn_case("lane1")[:2]
        args = (q if name == "tiny_a" else r, (1, 1, 1), ONE, np.array([[1, 1, 1], [1, 0, -1], [0, -1, 0]], np.int8))
    else:
        raise KeyError(name)
    return args + ref_hist(args[0], args[1], args[3], args[2])


def _hist(vol, patch, S, stride=ONE):
    return ops.patch_proj_hist(torch.from_numpy(vol).cuda(), patch, torch.from_numpy(S).cuda(), stride)


def _check(name):
    vol, patch, stride, S, want, N = _case(name)
    got = _hist(vol, patch, S, stride)
    D = S.shape[1]
    assert got.dtype == torch.int32 and tuple(got.shape) == (S.shape[0], 256 * D + 1) == want.shape
    got = got.cpu()
    # padding rows (zero rows of the last 128-patch tile) would land in bin 128 D; padding directions have no row at all
    assert torch.equal(got.sum(1, dtype=torch.int64), torch.full((S.shape[0],), N, dtype=torch.int64)), name
    assert torch.equal(got[:, 128 * D], torch.from_numpy(want[:, 128 * D])), name
    assert torch.equal(got, torch.from_numpy(want)), name
    return got


# ------------------------------------------------------------------------------------------------ histogram kernel (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lane8_q", "lane8_r"])
def test_lane_and_k_map(name):
    """One-hot directions read single bytes of the patch: a direction packed in another k order than the patches, or a
    transposed accumulator map, cannot pass.  (D = 24 has 48 signed one-hot rows; the mixed rows come on top: P = 52.)"""
    vol, patch, stride, S, want, N = _case(name)
    assert S.shape == (52, 24) and N == (33 if name == "lane8_q" else 30)
    _check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "ragged_strided"])
def test_k_padding_ragged_row_tile_two_direction_tiles(name):
    vol, patch, stride, S, want, N = _case(name)
    assert S.shape == (130, 441) and N == (476 if name == "ragged" else 84)
    _check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 255])
def test_range_ends(value):
    """byte - 128 = -128 / +127 on every k: all-(+1) and all-(-1) directions reach bins 0 and 256 D / 255 D and D."""
    patch, D = (3, 7, 7), 441
    vol = np.full((3, 8, 9, 3), value, np.uint8)
    S = np.stack([np.ones(D, np.int8), -np.ones(D, np.int8)])
    got = _hist(vol, patch, S).cpu()
    assert tuple(got.shape) == (2, 256 * D + 1)
    bins = (0, 256 * D) if value == 0 else (255 * D, D)
    want = np.zeros((2, 256 * D + 1), np.int32)
    want[0, bins[0]] = want[1, bins[1]] = 6
    assert np.array_equal(want, ref_hist(vol, patch, S)[0])
    assert torch.equal(got, torch.from_numpy(want))


@pytest.mark.gpu
def test_many_increments_on_one_bin():
    """A constant volume: 5 304 patches in 42 row tiles, all of them on one bin per direction."""
    patch, D = (3, 7, 7), 441
    vol = np.full((6, 40, 45, 3), 77, np.uint8)
    S = _dirs(5, D, 16)
    got = _hist(vol, patch, S).cpu()
    want = np.zeros((5, 256 * D + 1), np.int32)
    for p in range(5):
        want[p, (77 - 128) * int(S[p].astype(np.int64).sum()) + 128 * D] = 5304
    assert int((got != 0).sum()) == 5
    assert torch.equal(got, torch.from_numpy(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["image", "n1", "p1"])
def test_edges(name):
    vol, patch, stride, S, want, N = _case(name)
    assert N == {"image": 16 * 19, "n1": 1, "p1": 2 * 3 * 4}[name]
    _check(name)


@pytest.mark.gpu
def test_deterministic_across_runs_and_streams():
    vol, patch, stride, S, want, N = _case("ragged")
    v, s = torch.from_numpy(vol).cuda(), torch.from_numpy(S).cuda()
    a = ops.patch_proj_hist(v, patch, s)
    b = ops.patch_proj_hist(v, patch, s)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.patch_proj_hist(v, patch, s)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a.cpu(), torch.from_numpy(want))


@pytest.mark.gpu
def test_stale_histogram_memory_is_cleared_by_the_library():
    vol, patch, stride, S, want, N = _case("p1")
    v, s = torch.from_numpy(vol).cuda(), torch.from_numpy(S).cuda()
    NB = want.shape[1]
    # one element more than the histogram in front and behind: the 16-byte body of the clear starts mid-tensor, and the guards stay
    buf = torch.full((NB + 2,), -559038737, dtype=torch.int32, device="cuda")
    need = hplib.call("hpvg_patchproj_ws_bytes", 4, 9, 10, I3(*patch), I3(1, 1, 1), 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    hplib.call("hpvg_patchproj_hist_u8", hplib.ptr(v), 4, 9, 10, I3(*patch), I3(1, 1, 1), hplib.ptr(s), 1, hplib.ptr(buf[1:NB + 1]),
               hplib.ptr(ws), need, hplib.stream())
    buf = buf.cpu()
    assert torch.equal(buf[1:NB + 1], torch.from_numpy(want[0]))
    assert int(buf[0]) == -559038737 and int(buf[NB + 1]) == -559038737


@pytest.mark.gpu
def test_short_or_misaligned_workspace_is_refused():
    v = torch.zeros(3, 8, 8, 3, dtype=torch.uint8, device="cuda")
    s = torch.ones(1, 441, dtype=torch.int8, device="cuda")
    hist = torch.zeros(112897, dtype=torch.int32, device="cuda")
    need = hplib.call("hpvg_patchproj_ws_bytes", 3, 8, 8, I3(3, 7, 7), I3(1, 1, 1), 1)
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    f = hplib.load().hpvg_patchproj_hist_u8
    args = (hplib.ptr(v), 3, 8, 8, I3(3, 7, 7), I3(1, 1, 1), hplib.ptr(s), 1, hplib.ptr(hist))
    assert f(*args, hplib.ptr(ws), need - 1, hplib.stream()) == ERR_WS
    assert f(*args, hplib.ptr(ws[1:]), need, hplib.stream()) == ERR_WS
    assert f(*args, None, need, hplib.stream()) == ERR_WS


# ------------------------------------------------------------------------------------------------------- W1 kernel (GPU)
def _w1(hA, Na, hB, Nb):
    num = ops.hist_w1(torch.from_numpy(hA).cuda(), Na, torch.from_numpy(hB).cuda(), Nb)
    assert num.dtype == torch.int64 and tuple(num.shape) == (hA.shape[0],)
    return num.cpu().tolist()


@pytest.mark.gpu
def test_w1_identical_volumes_give_zero():
    vol, patch, stride, S, want, N = _case("ragged")
    h = _hist(vol, patch, S)
    assert ops.hist_w1(h, N, h.clone(), N).cpu().tolist() == [0] * 130


@pytest.mark.gpu
def test_w1_unequal_counts():
    """(4, 20, 23) against (5, 17, 31): Na = 476, Nb = 825, the kernel's histograms into the kernel's W1."""
    va, patch, _, Sa, wa, Na = _case("ragged")
    vb, _, _, Sb, wb, Nb = _case("other")
    assert (Na, Nb) == (476, 825) and np.array_equal(Sa[:6], Sb)
    want = ref_num(wa[:6], Na, wb, Nb)
    assert min(want) > 0
    ha, hb = _hist(va, patch, Sb), _hist(vb, patch, Sb)
    assert ops.hist_w1(ha, Na, hb, Nb).cpu().tolist() == want
    assert ops.hist_w1(hb, Nb, ha, Na).cpu().tolist() == want   # symmetric


@pytest.mark.gpu
def test_w1_fewer_bins_than_one_chunk():
    va, patch, _, S, wa, Na = _case("tiny_a")
    vb, _, _, _, wb, Nb = _case("tiny_b")
    assert wa.shape == (3, 769) and (Na, Nb) == (40, 37)
    assert _w1(wa, Na, wb, Nb) == ref_num(wa, Na, wb, Nb)


@pytest.mark.gpu
def test_w1_closed_form_shift():
    """b = a + 37 without clipping, direction all +1 (and all -1): every projection moves by 37 D, so W1 = 37 D exactly."""
    patch, D, c = (3, 7, 7), 441, 37
    a = np.random.default_rng(21).integers(0, 201, size=(4, 12, 13, 3), dtype=np.uint8)
    b = (a + c).astype(np.uint8)
    S = np.stack([np.ones(D, np.int8), -np.ones(D, np.int8)])
    N = 2 * 6 * 7
    num = ops.hist_w1(_hist(a, patch, S), N, _hist(b, patch, S), N).cpu().tolist()
    assert num == [N * N * c * D] * 2


@pytest.mark.gpu
def test_w1_last_bin_contributes_nothing_and_a_point_mass_distance():
    NB, Na, Nb = 256 * 441 + 1, 476, 825
    hA, hB = np.zeros((2, NB), np.int32), np.zeros((2, NB), np.int32)
    hA[0, NB - 1], hB[0, NB - 1] = Na, Nb         # both distributions on the last bin: 0
    hA[1, 5], hB[1, 5 + 3000] = Na, Nb            # point masses 3000 bins apart (the carry crosses two chunk boundaries)
    assert _w1(hA, Na, hB, Nb) == [0, Na * Nb * 3000]


@pytest.mark.gpu
def test_w1_largest_numerator_the_entry_point_accepts():
    """Na * Nb * 256 D just below 2^63, all of A on the first bin and all of B on the last: num = Na * Nb * 256 D."""
    NB, Na = 769, 1 << 27
    Nb = (2 ** 63 - 1) // (768 * Na)
    assert Nb < 2 ** 31 and Na * (Nb + 1) * 768 >= 2 ** 63
    hA, hB = np.zeros((1, NB), np.int32), np.zeros((1, NB), np.int32)
    hA[0, 0], hB[0, NB - 1] = Na, Nb
    assert _w1(hA, Na, hB, Nb) == [Na * Nb * 768]


# ----------------------------------------------------------------------------------------------------------------- host
def test_swd_directions():
    a, b, c = evaluate.swd_directions(16, 441, 3), evaluate.swd_directions(16, 441, 3), evaluate.swd_directions(16, 441, 4)
    assert a.dtype == np.int8 and a.shape == (16, 441)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert set(np.unique(a)) == {-1, 0, 1}
    # D = 3: one row in 27 comes out all-zero on the first draw, so 4 000 rows hold some with certainty and they are redrawn
    d = evaluate.swd_directions(4000, 3, 0)
    first = np.random.default_rng(0).integers(-1, 2, size=(4000, 3), dtype=np.int8)
    assert (~first.any(1)).sum() > 50
    assert d.shape == (4000, 3) and d.any(1).all() and set(np.unique(d)) == {-1, 0, 1}
    assert np.array_equal(d[first.any(1)], first[first.any(1)])   # rows that were fine keep their first draw


def test_swd_score_arithmetic():
    dirs = np.array([[1, 0, 0, 0], [1, -1, 1, -1], [0, 1, 1, 0]], np.int8)   # nnz 1, 4, 2
    assert evaluate.swd_score([0, 0, 0], 5, 7, dirs) == 0.0
    # W1 = 255 along e_0 alone: black against white is one full intensity range
    assert evaluate.swd_score([5 * 7 * 255], 5, 7, dirs[:1]) == 1.0
    assert evaluate.swd_score([5 * 7 * 255, 5 * 7 * 255 * 4, 0], 5, 7, dirs) == (1.0 + 2.0 + 0.0) / 3
    want = ((10 / (5 * 7 * 255)) / 1.0 + (20 / (5 * 7 * 255)) / 2.0 + (30 / (5 * 7 * 255)) / np.sqrt(2.0)) / 3
    assert evaluate.swd_score(torch.tensor([10, 20, 30]), 5, 7, dirs) == want
    # numerators and counts past 2^53 stay exact up to the one rounding of the quotient
    Na = Nb = 2 ** 27
    assert evaluate.swd_score([Na * Nb * 768 - 1], Na, Nb, dirs[:1]) == (Na * Nb * 768 - 1) / (Na * Nb * 255)
    with pytest.raises(ValueError):
        evaluate.swd_score([1, 2], 5, 7, dirs)


def test_evaluate_parser_swd_flags():
    p = evaluate.evaluate_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.swd, a.swd_seed) == (0, 0)
    a = p.parse_args(["--exp-dir", "e", "--swd", "512", "--swd-seed", "7"])
    assert (a.swd, a.swd_seed) == (512, 7)
    with pytest.raises(SystemExit):
        p.parse_args(["--exp-dir", "e", "--swd", "many"])


def test_bins_and_ws_bytes_queries():
    lib = hplib.load()
    assert lib.hpvg_patchproj_bins(I3(3, 7, 7)) == 112897 == ops.patch_proj_bins((3, 7, 7))
    assert lib.hpvg_patchproj_bins(I3(1, 1, 1)) == 769
    assert lib.hpvg_patchproj_bins(I3(1, 86, 128)) == 256 * 33024 + 1     # the largest D the i8 path takes
    assert lib.hpvg_patchproj_bins(I3(1, 101, 109)) == 0                  # D = 33 027
    assert lib.hpvg_patchproj_bins(I3(3, 0, 7)) == 0 and lib.hpvg_patchproj_bins(None) == 0
    with pytest.raises(RuntimeError, match="patch"):
        ops.patch_proj_bins((3, 0, 7))

    def al(v):
        return (v + 255) // 256 * 256
    one = I3(1, 1, 1)
    # (4, 20, 23): N = 476 -> 512 rows of 448 bytes; P directions -> P padded to 128 rows of 448 bytes
    for P, Ppad in [(1, 128), (128, 128), (129, 256), (512, 512)]:
        assert lib.hpvg_patchproj_ws_bytes(4, 20, 23, I3(3, 7, 7), one, P) == al(512 * 448) + al(Ppad * 448)
    assert lib.hpvg_patchproj_ws_bytes(4, 20, 23, I3(3, 7, 7), I3(1, 2, 3), 1) == al(128 * 448) + al(128 * 448)   # N = 84
    assert lib.hpvg_patchproj_ws_bytes(13, 144, 256, I3(3, 7, 7), one, 512) == al(379520 * 448) + al(512 * 448)


BAD_HIST = {
    "patch larger than the volume": ((2, 20, 23), (3, 7, 7), (1, 1, 1), 4),
    "stride 0": ((4, 20, 23), (3, 7, 7), (1, 0, 1), 4),
    "stride -1": ((4, 20, 23), (3, 7, 7), (1, 1, -1), 4),
    "patch 0": ((4, 20, 23), (3, 0, 7), (1, 1, 1), 4),
    "D * 255^2 = 2^31 + 97027": ((1, 101, 109), (1, 101, 109), (1, 1, 1), 4),
    "N = 2^31": ((2048, 1024, 1024), (1, 1, 1), (1, 1, 1), 4),
    "P = 0": ((4, 20, 23), (3, 7, 7), (1, 1, 1), 0),
    "P = -3": ((4, 20, 23), (3, 7, 7), (1, 1, 1), -3),
}


@pytest.mark.parametrize("why", sorted(BAD_HIST))
def test_hist_bad_arguments_return_err_arg(why):
    vol, patch, stride, P = BAD_HIST[why]
    lib = hplib.load()
    assert lib.hpvg_patchproj_ws_bytes(*vol, I3(*patch), I3(*stride), P) == 0
    # the launch entry point refuses before it touches a pointer or the device
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    assert lib.hpvg_patchproj_hist_u8(p, *vol, I3(*patch), I3(*stride), p, P, p, p, 1 << 40, None) == ERR_ARG


def test_hist_null_pointers_misaligned_histogram_and_workspace_are_refused():
    lib = hplib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    a = p.value + (-p.value) % 16
    geo = ((4, 20, 23), I3(3, 7, 7), I3(1, 1, 1))
    need = lib.hpvg_patchproj_ws_bytes(*geo[0], geo[1], geo[2], 4)

    def f(vol, dirs, hist, ws, nbytes):
        return lib.hpvg_patchproj_hist_u8(vol, *geo[0], geo[1], geo[2], dirs, 4, hist, ws, nbytes, None)
    assert f(None, a, a, a, need) == ERR_ARG and f(a, None, a, a, need) == ERR_ARG and f(a, a, None, a, need) == ERR_ARG
    assert f(a, a, a + 2, a, need) == ERR_ARG         # int32 histogram on a 2-byte boundary
    assert f(a, a, a, a, need - 1) == ERR_WS and f(a, a, a, a + 4, need) == ERR_WS and f(a, a, a, None, need) == ERR_WS


def test_w1_bad_arguments_return_err_arg():
    lib = hplib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def f(Na, Nb, P, NB, a=p, b=p, num=p):
        return lib.hpvg_hist_w1_i32(a, Na, b, Nb, P, NB, num, None)
    NB = 112897
    assert f(476, 825, 0, NB) == ERR_ARG and f(476, 825, -1, NB) == ERR_ARG
    assert f(0, 825, 4, NB) == ERR_ARG and f(476, -1, 4, NB) == ERR_ARG
    assert f(1 << 31, 825, 4, NB) == ERR_ARG and f(476, 1 << 31, 4, NB) == ERR_ARG
    for bad_nb in (0, 1, 768, 770, NB - 1, NB + 1, 256 * 440 + 1, 256 * 33027 + 1):   # not 256 D + 1 with D = 3 pt ph pw in range
        assert f(476, 825, 4, bad_nb) == ERR_ARG, bad_nb
    assert f(476, 825, 4, NB, a=None) == ERR_ARG and f(476, 825, 4, NB, b=None) == ERR_ARG and f(476, 825, 4, NB, num=None) == ERR_ARG


def test_w1_refuses_numerators_past_int64_for_a_geometry_patch_nn_accepts():
    """Two 1290^3 volumes of 1 x 1 x 1 patches: hpvg_patchnn_counts takes them (N = 2 146 689 000 < 2^31), but
    Na * Nb * 256 D = 3.5e21 does not fit the int64 numerator."""
    lib = hplib.load()
    out = (ctypes.c_int * 3)()
    assert lib.hpvg_patchnn_counts(1290, 1290, 1290, 1290, 1290, 1290, I3(1, 1, 1), I3(1, 1, 1), I3(1, 1, 1), out) == 0
    N = 1290 ** 3
    assert list(out) == [N, N, 3] and lib.hpvg_patchproj_bins(I3(1, 1, 1)) == 769
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    assert lib.hpvg_hist_w1_i32(p, N, p, N, 1, 769, p, None) == ERR_ARG
    # the bound itself: Na * Nb * 768 >= 2^63 is refused from the first product that reaches it
    Na = 1 << 27
    Nb = (2 ** 63 - 1) // (768 * Na) + 1
    assert Na * Nb * 768 >= 2 ** 63 > Na * (Nb - 1) * 768
    assert lib.hpvg_hist_w1_i32(p, Na, p, Nb, 1, 769, p, None) == ERR_ARG
    assert lib.hpvg_hist_w1_i32(p, Nb, p, Na, 1, 769, p, None) == ERR_ARG


def test_ops_argument_checks_name_the_argument():
    vol = torch.zeros(4, 9, 10, 3, dtype=torch.uint8)
    dirs = torch.ones(2, 441, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="patch_proj_hist: vol on cpu"):
        ops.patch_proj_hist(vol, (3, 7, 7), dirs)
    with pytest.raises(RuntimeError, match="patch_proj_hist: vol must be uint8"):
        ops.patch_proj_hist(vol.float(), (3, 7, 7), dirs)
    for bad in (torch.ones(2, 440, dtype=torch.int8), torch.ones(441, dtype=torch.int8), torch.ones(2, 441, dtype=torch.int32),
                torch.ones(0, 441, dtype=torch.int8)):
        with pytest.raises(RuntimeError, match=r"patch_proj_hist: dirs must be int8 \[P, 441\]"):
            ops.patch_proj_hist(vol, (3, 7, 7), bad)
    two = dirs.clone()
    two[1, 7] = 2
    with pytest.raises(RuntimeError, match="patch_proj_hist: dirs entries must be -1, 0 or \\+1"):
        ops.patch_proj_hist(vol, (3, 7, 7), two)
    two[1, 7] = -128
    with pytest.raises(RuntimeError, match="magnitude 128"):
        ops.patch_proj_hist(vol, (3, 7, 7), two)
    with pytest.raises(RuntimeError, match="patch_proj_hist: stride must have 3 entries"):
        ops.patch_proj_hist(vol, (3, 7, 7), dirs, stride=(1, 1))
    h = torch.zeros(2, 769, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="hist_w1: histA on cpu"):
        ops.hist_w1(h, 5, h, 5)
    with pytest.raises(RuntimeError, match="hist_w1: histB must be int32"):
        ops.hist_w1(h, 5, h.long(), 5)
    with pytest.raises(RuntimeError, match="hist_w1: histA .* and histB .* must have one shape"):
        ops.hist_w1(h, 5, h[:1], 5)
