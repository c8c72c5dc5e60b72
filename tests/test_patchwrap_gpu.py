"""hpvg_patch_vote_wrap_u8 / hpvg_patchmatch_wrap_u8 (ops.patch_vote(..., wrap), ops.patch_match(..., qwrap, rwrap)) on the GPU
against the numpy restatement of the ring contract (tests/patchwrap_ref.py).  Everything is exact: bytes, d2, nn and the bits of
the score."""
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
import offset_buf as OB  # noqa: E402
from patchwrap_ref import patch_match_wrap_ref, periodic_grid, vote_wrap_ref  # noqa: E402
from test_patchnn import _rand  # noqa: E402

pytestmark = pytest.mark.gpu
I3 = ctypes.c_int * 3
FLAGS = {None: None, "0": (0, 0, 0), "t": (1, 0, 0), "hw": (0, 1, 1), "thw": (1, 1, 1), "w": (0, 0, 1), "tw": (1, 0, 1),
         "th": (1, 1, 0), "h": (0, 1, 0)}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- vote
@functools.lru_cache(maxsize=None)
def _vcase(name):
    """dict(values, fallback, patch, wrap, rstride, nn) and the reference's bytes - built once, shared, never modified."""
    c = dict(values=_rand((4, 12, 14), 20), patch=(3, 7, 7), rstride=(1, 1, 1), image=False)
    if name == "ring_as_long_as_the_patch":       # S == p on t: grid 3 x 1 x 3
        c.update(fallback=_rand((3, 7, 9), 21), wrap="t")
    elif name == "one_longer_than_the_patch":     # S = p + 1 on every axis: grid 4 x 8 x 10
        c.update(fallback=_rand((4, 8, 10), 22), wrap="thw")
    elif name == "image":
        c.update(values=_rand((1, 20, 23), 23), fallback=_rand((1, 12, 15), 24), patch=(1, 5, 5), wrap="hw", image=True)
    elif name == "one_row_of_rings":              # only w is a ring, the other grid sides are 1: grid 1 x 1 x 12
        c.update(fallback=_rand((3, 7, 12), 25), patch=(3, 7, 5), wrap="w")
    elif name == "rstride":                       # values grid 2 x 3 x 8 at stride (1, 2, 1)
        c.update(fallback=_rand((5, 9, 11), 26), wrap="th", rstride=(1, 2, 1))
    elif name in ("skipped_entries", "all_invalid"):
        c.update(fallback=_rand((5, 9, 11), 27), wrap="tw")
    else:
        raise KeyError(name)
    wrap = FLAGS[c["wrap"]]
    vg = tuple((s - p) // st + 1 for s, p, st in zip(c["values"].shape[:3], c["patch"], c["rstride"]))
    Nr = vg[0] * vg[1] * vg[2]
    grid = periodic_grid(c["fallback"].shape[:3], c["patch"], wrap)
    rng = np.random.default_rng(28)
    nn = rng.integers(0, Nr, size=grid).astype(np.int32)
    if name == "skipped_entries":
        nn.reshape(-1)[::3], nn.reshape(-1)[1::7] = -1 - rng.integers(0, 5), Nr + rng.integers(0, 5)
    elif name == "all_invalid":
        nn.reshape(-1)[::2], nn.reshape(-1)[1::2] = -1, Nr
    c.update(nn=nn, Nr=Nr)
    return c, vote_wrap_ref(c["values"], nn, c["patch"], c["fallback"], wrap, c["rstride"])


@pytest.mark.parametrize("name", ["ring_as_long_as_the_patch", "one_longer_than_the_patch", "image", "one_row_of_rings", "rstride",
                                  "skipped_entries", "all_invalid"])
def test_vote_equals_the_reference(name):
    c, (want, cnt) = _vcase(name)
    v, fb = (c["values"][0], c["fallback"][0]) if c["image"] else (c["values"], c["fallback"])
    out = ops.patch_vote(_dev(v), _dev(c["nn"]), c["patch"], fb.shape[:-1], _dev(fb), rstride=c["rstride"], wrap=FLAGS[c["wrap"]])
    assert out.dtype == torch.uint8 and tuple(out.shape) == fb.shape
    assert np.array_equal(out.cpu().numpy(), want[0] if c["image"] else want)
    if name == "ring_as_long_as_the_patch":
        assert (cnt == cnt[:1]).all() and cnt.max() == 3 * 1 * 3          # every t patch covers every frame
    if name == "one_longer_than_the_patch":
        assert (cnt == 3 * 7 * 7).all()
    if name == "skipped_entries":
        assert (c["nn"] < 0).any() and (c["nn"] >= c["Nr"]).any() and 0 < cnt.min() < cnt.max()
    if name == "all_invalid":
        assert (cnt == 0).all() and np.array_equal(want, c["fallback"])


def test_vote_at_odd_byte_offsets_inside_guard_bands():
    """out, v and fallback each start at an odd byte inside an int32 payload between guard bands (tests/offset_buf.py): the
    launch writes its bytes and nothing else."""
    c, (want, _) = _vcase("one_longer_than_the_patch")

    def inside(nbytes, odd, data=None):
        words = (nbytes + odd + 3) // 4 + 1
        if data is None:
            payload = OB.out_like((words,), torch.int32, 1, device="cuda")
        else:
            payload = OB.embed(torch.full((words,), -1, dtype=torch.int32, device="cuda"), 1)
        view = payload.view(torch.uint8)[odd:odd + nbytes]
        if data is not None:
            view.copy_(_dev(data).reshape(-1))
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        return payload, view
    _, v = inside(c["values"].size, 1, c["values"])
    _, fb = inside(c["fallback"].size, 3, c["fallback"])
    payload, out = inside(c["fallback"].size, 5)
    before = payload.view(torch.uint8).clone()
    nn = _dev(c["nn"])
    hplib.call("hpvg_patch_vote_wrap_u8", hplib.ptr(v), *c["values"].shape[:3], hplib.ptr(nn), *c["fallback"].shape[:3],
               I3(*c["patch"]), I3(*c["rstride"]), I3(1, 1, 1), hplib.ptr(fb), hplib.ptr(out), hplib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    after = payload.view(torch.uint8)
    assert OB.guards_intact(payload) and torch.equal(after[:5], before[:5]) and torch.equal(after[5 + out.numel():], before[5 + out.numel():])


def test_vote_without_rings_is_the_plain_vote():
    values, fb = _dev(_rand((4, 12, 14), 30)), _dev(_rand((5, 9, 11), 31))
    nn = _dev(np.random.default_rng(32).integers(-2, 2 * 6 * 8 + 3, size=3 * 3 * 5).astype(np.int32))
    for rstride in ((1, 1, 1), (1, 2, 1)):
        plain = ops.patch_vote(values, nn, (3, 7, 7), (5, 9, 11), fb, rstride=rstride)
        assert torch.equal(ops.patch_vote(values, nn, (3, 7, 7), (5, 9, 11), fb, rstride=rstride, wrap=(0, 0, 0)), plain)
    with pytest.raises(RuntimeError, match="qstride"):
        ops.patch_vote(values, nn, (3, 7, 7), (5, 9, 11), fb, qstride=(1, 2, 1), wrap=(1, 0, 0))
    with pytest.raises(RuntimeError, match="each 0 or 1"):
        ops.patch_vote(values, nn, (3, 7, 7), (5, 9, 11), fb, wrap=(2, 0, 0))
    with pytest.raises(RuntimeError, match="nn must be int32 with 75 entries"):
        ops.patch_vote(values, nn, (3, 7, 7), (5, 9, 11), fb, wrap=(1, 0, 0))     # ring t: the grid is 5 x 3 x 5, nn has 3 x 3 x 5


# ----------------------------------------------------------------------------------------------------------- PatchMatch
def _weights(n, seed):
    return (0.25 + 3.75 * np.random.default_rng(seed).random(n)).astype(np.float32)      # [0.25, 4)


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(q, r, patch, iters, seed, w, init, qwrap, rwrap) - q and r are the padded volumes - and the reference's
    (d2, nn, score); built once, then shared and never modified."""
    c = dict(patch=(3, 7, 7), iters=3, seed=11, w=None, init=None, qwrap=None, rwrap=None)
    ragged = dict(q=_rand((5, 23, 41), 80), r=_rand((4, 19, 30), 81))     # grids 3 x 17 x 35 and 2 x 13 x 24, ragged against 8 x 32
    if name.startswith("ragged_"):
        _, qf, rf = name.split("_")
        c.update(ragged, qwrap={"n": None}.get(qf, qf), rwrap={"n": None}.get(rf, rf))
    elif name == "weighted":
        c.update(ragged, qwrap="thw", rwrap="t", w=_weights(2 * 13 * 24, 82))
    elif name == "warm":
        init = np.random.default_rng(83).integers(0, 624, size=3 * 17 * 35).astype(np.int32)
        init[::5], init[2::5] = -3, 624 + 17
        c.update(ragged, qwrap="t", rwrap="thw", init=init, iters=1)
    elif name == "iters0":
        c.update(ragged, qwrap="thw", rwrap="thw", iters=0)
    elif name == "key_side_of_one":      # key grid 1 x 1 x 34, t and h rings of one position
        c.update(q=_rand((4, 12, 20), 86), r=_rand((3, 7, 40), 87), rwrap="thw")
    elif name == "query_side_of_one":    # query grid 1 x 3 x 24, t a ring of one position: the neighbour is the patch itself
        c.update(q=_rand((3, 9, 30), 88), r=_rand((4, 12, 20), 89), qwrap="tw", rwrap="h")
    elif name == "wide":                 # key grid 1 x 2 x 194: R = 194 exceeds two sides, the offsets wrap many times
        c.update(q=_rand((3, 9, 140), 92), r=_rand((3, 8, 200), 93), rwrap="tw")
    elif name == "long_patch":           # pt = 290: the query is read from global memory
        c.update(q=_rand((300, 9, 40), 95), r=_rand((295, 5, 20), 96), patch=(290, 1, 1), iters=2, qwrap="thw", rwrap="thw")
    elif name == "no_flags":
        c.update(ragged, qwrap="0", rwrap=None)
    else:
        raise KeyError(name)
    want = patch_match_wrap_ref(c["q"], c["r"], c["patch"], c["iters"], c["seed"], c["w"], c["init"], FLAGS[c["qwrap"]],
                                FLAGS[c["rwrap"]])
    return c, want


def _run(c):
    out, nn = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], c["iters"], c["seed"], _dev(c["w"]), _dev(c["init"]),
                              qwrap=FLAGS[c["qwrap"]], rwrap=FLAGS[c["rwrap"]])
    return out.cpu(), nn.cpu()


@pytest.mark.parametrize("name", ["ragged_t_n", "ragged_thw_n", "ragged_n_t", "ragged_n_thw", "ragged_thw_thw", "key_side_of_one",
                                  "query_side_of_one", "wide", "weighted", "warm", "iters0", "long_patch"])
def test_field_equals_the_reference(name):
    c, (d2, nn, score) = _case(name)
    out, got_nn = _run(c)
    assert got_nn.dtype == torch.int32 and tuple(got_nn.shape) == nn.shape
    assert torch.equal(got_nn.to(torch.int64), torch.from_numpy(nn))
    if c["w"] is None:
        assert out.dtype == torch.int32 and torch.equal(out.to(torch.int64), torch.from_numpy(d2))
    else:
        assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), torch.from_numpy(score.view(np.int32)))
    if c["iters"] > 0:
        # the flags change this field: the plain search gives another one
        plain = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], c["iters"], c["seed"], _dev(c["w"]), _dev(c["init"]))[1]
        assert not torch.equal(plain.cpu(), got_nn)


def test_flags_zero_are_the_plain_search():
    c, (d2, nn, _) = _case("no_flags")
    out, got_nn = _run(c)
    plain = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], c["iters"], c["seed"])
    assert torch.equal(out, plain[0].cpu()) and torch.equal(got_nn, plain[1].cpu())
    assert torch.equal(got_nn.to(torch.int64), torch.from_numpy(nn)) and torch.equal(out.to(torch.int64), torch.from_numpy(d2))
    w = _dev(_weights(2 * 13 * 24, 82))
    a = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], 2, 5, w, qwrap=None, rwrap=(0, 0, 0))
    b = ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], 2, 5, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError, match="each 0 or 1"):
        ops.patch_match(_dev(c["q"]), _dev(c["r"]), c["patch"], 2, 5, rwrap=(0, 3, 0))


def test_two_runs_and_another_stream_give_equal_results():
    for name in ("ragged_thw_thw", "weighted"):
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
