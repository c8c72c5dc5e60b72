"""hpvg_patchmatch_u8 / ops.patch_match on the GPU against the numpy restatement of the rule (tests/patchmatch_ref.py): d2, nn and
score must be torch.equal to it - the field is defined bit for bit, so there is no tolerance anywhere.  Every reference is
computed once and shared.

The kernel's tile is 8 x 32 query patches at one t, a patch line is read as whole 4-byte words plus a tail, and a patch whose
tile does not fit 64 KB of LDS reads the query from global memory: the cases put grid sides off the tile, lines with and
without a tail, key axes of length 1, and one such long patch."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import ops  # noqa: E402
from patchmatch_ref import patch_match_ref  # noqa: E402
from test_patchnn import _rand  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_WORKSPACE = -1, -2
I3 = ctypes.c_int * 3


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(n, seed):
    return (0.25 + 3.75 * np.random.default_rng(seed).random(n)).astype(np.float32)      # [0.25, 4)


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(q, r, patch, iters, seed, w, init) and the reference's (d2, nn, score) - built once, then shared and never modified."""
    c = dict(patch=(3, 7, 7), iters=3, seed=11, w=None, init=None)
    if name in ("ragged", "weighted", "warm", "iters0"):
        # query grid 3 x 17 x 35 (three tiles of 8 rows, two of 32 columns, every edge ragged), key grid 2 x 13 x 24
        c.update(q=_rand((5, 23, 41), 80), r=_rand((4, 19, 30), 81))
        if name == "weighted":
            c.update(w=_weights(2 * 13 * 24, 82))
        elif name == "warm":
            init = np.random.default_rng(83).integers(0, 624, size=3 * 17 * 35).astype(np.int32)
            init[::5], init[2::5] = -3, 624 + 17        # out of range on both sides: clamped to 0 and 623
            c.update(init=init, iters=1)
        elif name == "iters0":
            c.update(iters=0)
    elif name == "image":        # [H,W,3]: kT = 1, line = 21 bytes
        c.update(q=_rand((29, 37), 84), r=_rand((31, 26), 85), patch=(1, 7, 7))
    elif name == "thin_keys":    # key grid 1 x 1 x 34: every offset along t and y clamps
        c.update(q=_rand((4, 12, 20), 86), r=_rand((3, 7, 40), 87))
    elif name == "small_patch":  # D = 54, line = 9 bytes: two words and a tail of one
        c.update(q=_rand((4, 10, 12), 88), r=_rand((3, 9, 17), 89), patch=(2, 3, 3))
    elif name == "line_of_whole_words":   # pw = 4: line = 12 bytes, no tail
        c.update(q=_rand((3, 11, 37), 90), r=_rand((2, 9, 21), 91), patch=(2, 2, 4))
    elif name == "wide":         # query grid 1 x 3 x 134: five tiles along x; key grid 1 x 2 x 194: radii 194, 97, ... 1 (eight)
        c.update(q=_rand((3, 9, 140), 92), r=_rand((3, 8, 200), 93))
    elif name == "wide_weighted":
        c.update(q=_rand((3, 9, 140), 92), r=_rand((3, 8, 200), 93), w=_weights(2 * 194, 94))
    elif name == "long_patch":   # pt = 290: the tile would need 222 KB of LDS, so the query is read from global memory
        c.update(q=_rand((300, 9, 40), 95), r=_rand((295, 5, 20), 96), patch=(290, 1, 1), iters=2)
    elif name == "long_patch_weighted":
        c.update(q=_rand((300, 9, 40), 95), r=_rand((295, 5, 20), 96), patch=(290, 1, 1), iters=2, w=_weights(6 * 5 * 20, 97))
    elif name == "ties":         # constant volumes: every candidate ties, the smallest index seen wins
        c.update(q=np.full((5, 23, 41, 3), 9, np.uint8), r=np.full((4, 19, 30, 3), 200, np.uint8))
    elif name == "extremes":     # d2 = D * 255^2 = 28 676 025 everywhere
        c.update(q=np.zeros((5, 23, 41, 3), np.uint8), r=np.full((4, 19, 30, 3), 255, np.uint8))
    else:
        raise KeyError(name)
    want = patch_match_ref(c["q"], c["r"], c["patch"], c["iters"], c["seed"], c["w"], c["init"])
    return c, want


def _run(c, iters=None):
    out, nn = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], c["iters"] if iters is None else iters, c["seed"], _dev(c["w"]),
                              _dev(c["init"]))
    return out.cpu(), nn.cpu()


@pytest.mark.parametrize("name", ["ragged", "image", "thin_keys", "small_patch", "line_of_whole_words", "wide", "wide_weighted",
                                  "weighted", "warm", "iters0", "ties", "extremes", "long_patch", "long_patch_weighted"])
def test_field_equals_the_reference(name):
    c, (d2, nn, score) = _case(name)
    out, got_nn = _run(c)
    assert got_nn.dtype == torch.int32 and tuple(got_nn.shape) == nn.shape
    assert torch.equal(got_nn.to(torch.int64), torch.from_numpy(nn))
    if c["w"] is None:
        assert out.dtype == torch.int32 and torch.equal(out.to(torch.int64), torch.from_numpy(d2))
    else:
        assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), torch.from_numpy(score.view(np.int32)))
    if name == "extremes":
        assert int(out.min()) == int(out.max()) == 441 * 255 * 255
    if name == "image":
        assert out.dim() == 2
    if name == "warm":
        assert (c["init"] < 0).any() and (c["init"] >= 624).any()


def test_weighted_call_also_writes_the_exact_distance():
    """ops.patch_match returns the score; the C entry point writes d2 beside it."""
    c, (d2, nn, score) = _case("weighted")
    q, r, w = _dev(c["q"]), _dev(c["r"]), _dev(c["w"])
    n = nn.size
    od2, onn = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    osc = torch.empty(n, dtype=torch.float32, device="cuda")
    need = hplib.call("hpvg_patchmatch_ws_bytes", 5, 23, 41, 4, 19, 30, I3(3, 7, 7))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    f = hplib.load().hpvg_patchmatch_u8
    args = (hplib.ptr(q), 5, 23, 41, hplib.ptr(r), 4, 19, 30, I3(3, 7, 7), hplib.ptr(w), None, c["iters"], c["seed"], hplib.ptr(od2),
            hplib.ptr(onn))
    assert f(*args, hplib.ptr(osc), hplib.ptr(ws), need - 1, hplib.stream()) == ERR_WORKSPACE
    assert f(*args, hplib.ptr(osc), hplib.ptr(ws), need, hplib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(od2.cpu().to(torch.int64), torch.from_numpy(d2.reshape(-1)))
    assert torch.equal(onn.cpu().to(torch.int64), torch.from_numpy(nn.reshape(-1)))
    assert torch.equal(osc.cpu().view(torch.int32), torch.from_numpy(score.reshape(-1).view(np.int32)))
    od2.fill_(-7)
    assert f(*args, None, hplib.ptr(ws), need, hplib.stream()) == 0       # weights without a score output
    torch.cuda.synchronize()
    assert torch.equal(od2.cpu().to(torch.int64), torch.from_numpy(d2.reshape(-1)))
    assert f(*args[:9], None, *args[10:], hplib.ptr(osc), hplib.ptr(ws), need, hplib.stream()) == ERR_ARG     # score without weights


def test_two_runs_and_another_stream_give_equal_results():
    for name in ("ragged", "weighted"):
        c, _ = _case(name)
        a = _run(c)
        b = _run(c)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            d = _run(c)
        side.synchronize()
        for got in (b, d):
            assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])


@pytest.mark.parametrize("name", ["ragged", "weighted"])
def test_one_more_iteration_never_raises_a_key(name):
    c, _ = _case(name)
    prev = _run(c, 0)
    lowered = 0
    for n in range(1, 5):
        cur = _run(c, n)
        assert bool(((cur[0] < prev[0]) | ((cur[0] == prev[0]) & (cur[1] <= prev[1]))).all())
        lowered += int((cur[0] < prev[0]).sum())
        prev = cur
    assert lowered > 0


def test_seed_and_start_matter():
    c, _ = _case("ragged")
    q, r = _dev(c["q"]), _dev(c["r"])
    a = ops.patch_match(q, r, c["patch"], 0, 1)[1]
    assert not torch.equal(a, ops.patch_match(q, r, c["patch"], 0, 2)[1])
    assert torch.equal(a, ops.patch_match(q, r, c["patch"], 0, 1 + 2 ** 32)[1])       # seeds count mod 2^32
    init = torch.full((3 * 17 * 35,), 77, dtype=torch.int32, device="cuda")
    assert bool((ops.patch_match(q, r, c["patch"], 0, 1, nn_init=init)[1] == 77).all())
    assert bool((ops.patch_match(q, r, c["patch"], 0, 1, nn_init=init.reshape(3, 17, 35))[1] == 77).all())


def test_wrapper_refuses_bad_weights_starts_and_iteration_counts():
    c, _ = _case("ragged")
    q, r, patch = _dev(c["q"]), _dev(c["r"]), c["patch"]
    Nr, Nq = 624, 1785
    good = torch.ones(Nr, device="cuda")
    assert ops.patch_match(q, r, patch, 1, 0, good.reshape(2, 13, 24))[0].dtype == torch.float32      # grid-shaped weights are taken
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = good.clone()
        w[Nr // 2] = bad
        with pytest.raises(RuntimeError, match="finite and > 0"):
            ops.patch_match(q, r, patch, 1, 0, w)
    for w in (good[:-1], good.double(), good.cpu(), good.reshape(24, 26)):
        with pytest.raises(RuntimeError, match="ref_weight must be float32"):
            ops.patch_match(q, r, patch, 1, 0, w)
    init = torch.zeros(Nq, dtype=torch.int32, device="cuda")
    for bad in (init[:-1], init.long(), init.cpu(), [0] * Nq):
        with pytest.raises(RuntimeError, match="nn_init must be int32 with 1785 entries"):
            ops.patch_match(q, r, patch, 1, 0, None, bad)
    for iters in (-1, 1025):
        with pytest.raises(RuntimeError, match="iters"):
            ops.patch_match(q, r, patch, iters)
    with pytest.raises(RuntimeError, match="hpvg_patchnn_counts failed"):
        ops.patch_match(q, r, (6, 7, 7), 1)                                # a patch larger than a volume
    with pytest.raises(RuntimeError, match="uint8"):
        ops.patch_match(q.float(), r, patch, 1)
