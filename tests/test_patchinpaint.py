"""The subset search (hpvg_patchnn_subset_u8 / ops.patch_nn_subset), the mask count (hpvg_patch_mask_count_u8 / ops.patch_mask_count),
one inpainting step and a whole inpainting with a known answer (generate_patchnn.patchnn_inpaint), and the host-side pieces of
`generate_patchnn --mask`, against numpy written from the definitions.  Every comparison is torch.equal / ==; there is no
tolerance anywhere.

Subset search: test_patchnn's float64 distance matrix restricted to the selected rows of both patch matrices, the first argmin
along the selected keys translated back through rsel (the lists ascend, so that is the smallest grid index among equals), and
-1 / -1 for every query patch that is not selected.  The tile is 128 x 128 patches, so list lengths of 127, 128, 129 and 130
sit on its edges and 1 / N - 1 on the ends."""
import ctypes
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import generate_patchnn, ops  # noqa: E402
from patch_ref import brute_subset, count_ref  # noqa: E402
from test_patchgen import vote_ref  # noqa: E402
from test_patchnn import BAD, _patches, _rand  # noqa: E402

ERR_ARG, ERR_WORKSPACE = -1, -2
I3 = ctypes.c_int * 3
ONE = (1, 1, 1)


# ------------------------------------------------------------------------------------------------------------ yardsticks
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sel(N, n, seed):
    return np.sort(np.random.default_rng(seed).choice(N, size=n, replace=False)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _base():
    """The base case: q (4,18,22), r (5,20,17), patch (2,5,5): D = 150 (padded to 192), Nq = 756, Nr = 832."""
    q, r, patch = _rand((4, 18, 22), 31), _rand((5, 20, 17), 32), (2, 5, 5)
    assert (len(_patches(q, patch, ONE)[0]), len(_patches(r, patch, ONE)[0])) == (756, 832)
    return q, r, patch


def _check_subset(q, r, patch, qsel, rsel, qs=ONE, rs=ONE):
    want_d2, want_nn = brute_subset(q, r, patch, qsel, rsel, qs, rs)
    d2, nn = ops.patch_nn_subset(_dev(q), _dev(r), patch, None if qsel is None else _dev(qsel), None if rsel is None else _dev(rsel),
                                 qs, rs)
    assert d2.dtype == torch.int32 and nn.dtype == torch.int32
    if q.ndim == 3:
        want_d2, want_nn = want_d2[0], want_nn[0]
    assert tuple(d2.shape) == want_d2.shape and tuple(nn.shape) == want_nn.shape
    assert torch.equal(d2.cpu().to(torch.int64), torch.from_numpy(want_d2))
    assert torch.equal(nn.cpu().to(torch.int64), torch.from_numpy(want_nn))
    return d2.cpu(), nn.cpu()


# ------------------------------------------------------------------------------------------------------------ mask count
@pytest.mark.gpu
@pytest.mark.parametrize("shape,patch,stride", [((4, 20, 24), (3, 7, 7), (1, 1, 1)), ((4, 20, 24), (3, 7, 7), (2, 3, 1)),
                                                ((1, 17, 19), (1, 5, 5), (1, 1, 1))])
def test_mask_count_equals_numpy(shape, patch, stride):
    rng = np.random.default_rng(50)
    box = np.zeros(shape, np.uint8)
    box[shape[0] // 2, 5:9, 8:13] = rng.integers(1, 256, size=(4, 5))      # any nonzero byte counts, once
    for mask in (box, (rng.random(shape) < 0.5).astype(np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)):
        want = count_ref(mask, patch, stride)
        got = ops.patch_mask_count(_dev(mask), patch, stride)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        assert torch.equal(got.cpu().to(torch.int64), torch.from_numpy(want))
    assert (count_ref(box, patch, stride) == 0).any() and (count_ref(box, patch, stride) == 20).any()
    if shape[0] == 1:
        got = ops.patch_mask_count(_dev(box[0]), patch, stride)         # the [H,W] form
        assert got.dim() == 2 and torch.equal(got.cpu().to(torch.int64), torch.from_numpy(count_ref(box, patch, stride)[0]))


# --------------------------------------------------------------------------------------------------------- subset search
@pytest.mark.gpu
@pytest.mark.parametrize("nr", [1, 128, 130, 700])
@pytest.mark.parametrize("nq", [1, 127, 128, 129, 755])
def test_subset_equals_brute_force_on_the_selected_rows(nq, nr):
    q, r, patch = _base()
    qsel, rsel = _sel(756, nq, 1000 + nq), _sel(832, nr, 2000 + nr)
    d2, nn = _check_subset(q, r, patch, qsel, rsel)
    assert int((nn >= 0).sum()) == nq == int((d2 >= 0).sum())
    assert set(nn.reshape(-1)[torch.from_numpy(qsel).long()].tolist()) <= set(rsel.tolist())


@pytest.mark.gpu
def test_one_list_only():
    q, r, patch = _base()
    _check_subset(q, r, patch, _sel(756, 300, 1), None)
    d2, nn = _check_subset(q, r, patch, None, _sel(832, 300, 2))
    assert int(nn.min()) >= 0


@pytest.mark.gpu
def test_null_lists_reproduce_patch_nn():
    q, r, patch = _base()
    qd, rd = _dev(q), _dev(r)
    a, b = ops.patch_nn(qd, rd, patch), ops.patch_nn_subset(qd, rd, patch)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    full = torch.arange(756, dtype=torch.int32, device="cuda"), torch.arange(832, dtype=torch.int32, device="cuda")
    c = ops.patch_nn_subset(qd, rd, patch, *full)                         # the identity lists too
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.gpu
def test_strided_grids():
    q, r, patch = _base()
    qs, rs = (1, 2, 3), (2, 1, 2)
    Nq, Nr, _ = ops.patch_nn_counts(q.shape[:3], r.shape[:3], patch, qs, rs)
    assert (Nq, Nr) == (3 * 7 * 6, 2 * 16 * 7)
    _check_subset(q, r, patch, _sel(Nq, 50, 3), _sel(Nr, 129, 4), qs, rs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["image", "d27", "d441"])
def test_other_patch_sizes(name):
    if name == "image":        # the [H,W,3] form, D = 147
        q, r, patch = _rand((30, 33), 33), _rand((30, 33), 34), (1, 7, 7)
    elif name == "d27":        # one K step, mostly padding
        q, r, patch = _rand((2, 12, 13), 35), _rand((2, 11, 14), 36), (1, 3, 3)
    else:                      # 441 -> 448: seven K steps
        q, r, patch = _rand((4, 12, 13), 37), _rand((4, 12, 13), 38), (3, 7, 7)
    Nq, Nr, D = ops.patch_nn_counts((q if q.ndim == 4 else q[None]).shape[:3], (r if r.ndim == 4 else r[None]).shape[:3], patch)
    assert D == {"image": 147, "d27": 27, "d441": 441}[name]
    d2, nn = _check_subset(q, r, patch, _sel(Nq, Nq // 3, 5), _sel(Nr, Nr // 2, 6))
    assert d2.dim() == (2 if name == "image" else 3)


@pytest.mark.gpu
def test_ties_resolve_to_the_smallest_selected_index():
    q, _, patch = _base()
    r = np.full((5, 20, 17, 3), 77, np.uint8)
    rsel = _sel(832, 130, 7)
    assert rsel[0] > 0
    nn = _check_subset(q, r, patch, None, rsel)[1]
    assert int((nn == int(rsel[0])).sum()) == nn.numel()
    # two identical halves: patch j of frames 0:2 is patch j + 416 of frames 2:4, and the query is the first half
    half = _rand((2, 20, 17), 39)
    r = np.concatenate([half, half], 0)
    per = 16 * 13
    assert len(_patches(r, patch, ONE)[0]) == 3 * per
    both = _check_subset(half, r, patch, None, None)[1].reshape(-1)
    assert both.tolist() == list(range(per))                               # the first copy wins
    second = _check_subset(half, r, patch, None, np.arange(per, 3 * per, dtype=np.int32))[1].reshape(-1)
    assert second.tolist() == list(range(2 * per, 3 * per))                # the first copy deselected: the second answers
    keep = np.sort(np.concatenate([_sel(per, 100, 8), np.arange(per, 3 * per)])).astype(np.int32)
    mixed = _check_subset(half, r, patch, _sel(per, 150, 9), keep)[1].reshape(-1)
    kept = set(keep[:100].tolist())
    for i in np.flatnonzero(mixed.numpy() >= 0):
        assert int(mixed[i]) == (i if i in kept else i + 2 * per)


@pytest.mark.gpu
def test_subset_deterministic_across_runs_and_streams():
    q, r, patch = _base()
    qd, rd, qsel, rsel = _dev(q), _dev(r), _dev(_sel(756, 400, 10)), _dev(_sel(832, 700, 11))
    a = ops.patch_nn_subset(qd, rd, patch, qsel, rsel)
    b = ops.patch_nn_subset(qd, rd, patch, qsel, rsel)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.patch_nn_subset(qd, rd, patch, qsel, rsel)
    side.synchronize()
    for got in (b, c):
        assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])


@pytest.mark.gpu
def test_wrapper_refuses_bad_lists():
    q, r, patch = _base()
    qd, rd = _dev(q), _dev(r)
    good = torch.tensor([3, 5, 9], dtype=torch.int32, device="cuda")
    assert int((ops.patch_nn_subset(qd, rd, patch, good, good)[1] >= 0).sum()) == 3
    for bad in ([5, 3, 9], [3, 3, 9], [3, 5, 756], [-1, 5, 9]):        # unsorted, duplicate, out of range
        t = torch.tensor(bad, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match="qsel must be strictly ascending"):
            ops.patch_nn_subset(qd, rd, patch, t, good)
    with pytest.raises(RuntimeError, match="rsel must be strictly ascending"):
        ops.patch_nn_subset(qd, rd, patch, good, torch.tensor([3, 5, 832], dtype=torch.int32, device="cuda"))
    assert int(ops.patch_nn_subset(qd, rd, patch, good, torch.tensor([831], dtype=torch.int32, device="cuda"))[1].max()) == 831
    for bad in (good[:0], good.long(), good.reshape(1, 3), good.cpu(), [3, 5, 9]):    # empty, not int32, not 1-D, not there
        with pytest.raises(RuntimeError, match="rsel must be a non-empty 1-D int32 tensor"):
            ops.patch_nn_subset(qd, rd, patch, good, bad)


# ------------------------------------------------------------------------------------------------------ one inpaint step
@functools.lru_cache(maxsize=None)
def _step_case():
    shape, patch = (4, 20, 23), (3, 7, 7)
    mask = np.zeros(shape, bool)
    mask[:, 2:6, 3:8] = True
    return _rand(shape, 41), _rand(shape, 42), _rand(shape, 43), mask, patch


def _step_ref(query, keys, values, mask, patch, key_mask):
    c, ck = count_ref(mask, patch).reshape(-1), count_ref(key_mask, patch).reshape(-1)
    qsel, rsel = np.flatnonzero(c > 0).astype(np.int32), np.flatnonzero(ck == 0).astype(np.int32)
    assert 0 < len(qsel) < c.size and 0 < len(rsel) < c.size
    nn = brute_subset(query, keys, patch, qsel, rsel)[1]
    voted = vote_ref(values, nn, patch, query)[0]
    return np.where(mask[..., None], voted, query), qsel, rsel


@pytest.mark.gpu
def test_inpaint_step_equals_numpy_composition():
    query, keys, values, mask, patch = _step_case()
    want, qsel, rsel = _step_ref(query, keys, values, mask, patch, mask)
    assert (want != query).any() and np.array_equal(want[~mask], query[~mask])
    got = generate_patchnn.patchnn_inpaint_step(_dev(query), _dev(keys), _dev(values), _dev(mask), patch, _dev(qsel), _dev(rsel))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_blurred_key_step_uses_the_patches_that_avoid_B():
    """Two levels (4,15,17) -> (4,20,23): the plan's lists against numpy, then the first step of level 1 with them."""
    query, keys, values, mask, patch = _step_case()
    sizes = [(4, 15, 17), (4, 20, 23)]
    M0 = generate_patchnn.patchnn_mask_resize(mask, sizes[0])
    B1 = mask | generate_patchnn.patchnn_mask_resize(M0, sizes[1])
    assert B1.sum() > mask.sum()
    plan = generate_patchnn.patchnn_inpaint_plan(_dev(mask), sizes, patch)
    want, qsel, rsel_first = _step_ref(query, keys, values, mask, patch, B1)
    for lv, M in zip(plan, (M0, mask)):
        c = count_ref(M, patch).reshape(-1)
        assert np.array_equal(lv["mask"].cpu().numpy(), M)
        assert lv["qsel"].dtype == torch.int32 and np.array_equal(lv["qsel"].cpu().numpy(), np.flatnonzero(c > 0))
        assert np.array_equal(lv["rsel"].cpu().numpy(), np.flatnonzero(c == 0))
    assert "rsel_first" not in plan[0] and np.array_equal(plan[1]["rsel_first"].cpu().numpy(), rsel_first)
    assert len(rsel_first) < plan[1]["rsel"].numel()
    got = generate_patchnn.patchnn_inpaint_step(_dev(query), _dev(keys), _dev(values), plan[1]["mask"], patch, plan[1]["qsel"],
                                                plan[1]["rsel_first"])
    assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------- known answer
@pytest.mark.gpu
@pytest.mark.parametrize("hole", [(17, 23, 20, 26), (10, 22, 15, 29)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_periodic_texture_is_restored_byte_for_byte(seed, hole):
    """An 8 x 8 tile repeated to 40 x 48: every patch of the image has exact copies that avoid the hole, so the hole's border
    patches find them and the vote brings the missing bytes.  In numpy the small hole closes in one step and the large one in
    two, so the third step's queries all have an exact copy among the keys: the score is 0."""
    tile = np.random.default_rng(seed).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    img = np.tile(tile, (5, 6, 1))
    assert img.shape == (40, 48, 3)
    mask = np.zeros((40, 48), bool)
    mask[hole[0]:hole[1], hole[2]:hole[3]] = True
    out, score = generate_patchnn.patchnn_inpaint(_dev(img), _dev(mask), patch=(1, 7, 7), min_size=100, noise=0, iters=3)
    assert out.dtype == torch.uint8 and tuple(out.shape) == img.shape
    assert np.array_equal(out.cpu().numpy(), img)
    assert score == 0.0


# ----------------------------------------------------------------------------------------------------------------- host
def test_new_exports_are_declared_and_bound():
    declared = hplib.check_symbols()
    for name in ("hpvg_patch_mask_count_u8", "hpvg_patchnn_subset_ws_bytes", "hpvg_patchnn_subset_u8"):
        assert name in declared


def _p():
    dummy = ctypes.create_string_buffer(64)       # never touched: every call below is refused before a launch
    return dummy, ctypes.cast(dummy, ctypes.c_void_p)


@pytest.mark.parametrize("why", sorted(BAD))
def test_bad_geometry_returns_err_arg_from_the_new_entry_points(why):
    qs, rs, patch, qstride, rstride = BAD[why]
    lib = hplib.load()
    keep, p = _p()
    geo = (I3(*patch), I3(*qstride), I3(*rstride))
    assert lib.hpvg_patchnn_subset_u8(p, *qs, p, *rs, *geo, None, 0, None, 0, p, p, p, 1 << 40, None) == ERR_ARG
    assert lib.hpvg_patchnn_subset_u8(p, *qs, p, *rs, *geo, p, 1, p, 1, p, p, p, 1 << 40, None) == ERR_ARG
    assert lib.hpvg_patchnn_subset_ws_bytes(*qs, *rs, *geo, -1, -1) == 0
    assert lib.hpvg_patchnn_subset_ws_bytes(*qs, *rs, *geo, 1, 1) == 0
    # the mask count has one side: whichever side of the pair is the refused one
    refused = 0
    for shape, stride in ((qs, qstride), (rs, rstride)):
        if lib.hpvg_patchnn_counts(*shape, *shape, I3(*patch), I3(*stride), I3(*stride), (ctypes.c_int * 3)()) == ERR_ARG:
            assert lib.hpvg_patch_mask_count_u8(p, *shape, I3(*patch), I3(*stride), p, None) == ERR_ARG
            refused += 1
    assert refused >= 1


def test_null_pointers_and_workspace():
    lib = hplib.load()
    keep, p = _p()
    geo = (I3(3, 7, 7), I3(*ONE), I3(*ONE))
    for k in range(4):           # q, r, d2, nn
        a = [p, p, p, p]
        a[k] = None
        assert lib.hpvg_patchnn_subset_u8(a[0], 4, 20, 23, a[1], 5, 17, 31, *geo, None, 0, None, 0, a[2], a[3], p, 1 << 40, None) == ERR_ARG
    assert lib.hpvg_patch_mask_count_u8(None, 4, 20, 23, geo[0], geo[1], p, None) == ERR_ARG
    assert lib.hpvg_patch_mask_count_u8(p, 4, 20, 23, geo[0], geo[1], None, None) == ERR_ARG
    assert lib.hpvg_patch_mask_count_u8(p, 4, 20, 23, None, geo[1], p, None) == ERR_ARG
    assert lib.hpvg_patch_mask_count_u8(p, 4, 20, 23, geo[0], None, p, None) == ERR_ARG
    # a null or short workspace, for whole grids and for lists (p is 16-byte aligned or not: the size is tested first)
    for lists, counts in (((None, 0, None, 0), (-1, -1)), ((p, 100, p, 200), (100, 200))):
        need = lib.hpvg_patchnn_subset_ws_bytes(4, 20, 23, 5, 17, 31, *geo, *counts)
        assert need > 0
        args = (p, 4, 20, 23, p, 5, 17, 31, *geo, *lists, p, p)
        assert lib.hpvg_patchnn_subset_u8(*args, None, 1 << 40, None) == ERR_WORKSPACE
        assert lib.hpvg_patchnn_subset_u8(*args, p, need - 1, None) == ERR_WORKSPACE
        assert lib.hpvg_patchnn_subset_u8(*args, p, 0, None) == ERR_WORKSPACE


def test_selection_counts():
    lib = hplib.load()
    keep, p = _p()
    shapes = (4, 20, 23, 5, 17, 31)
    geo = (I3(3, 7, 7), I3(*ONE), I3(*ONE))
    Nq, Nr = 476, 825
    full = lib.hpvg_patchnn_ws_bytes(*shapes, *geo)
    assert full > 0 and lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, -1, -1) == full
    assert lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, Nq, Nr) == full
    one = lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, 1, 1)
    assert 0 < one < full
    assert one < lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, 1, -1) < full          # sized by each count on its own
    assert one < lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, -1, 1) < full
    assert lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, 128, 128) < lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, 129, 128)
    for nq, nr in ((0, 1), (1, 0), (Nq + 1, 1), (1, Nr + 1)):
        assert lib.hpvg_patchnn_subset_ws_bytes(*shapes, *geo, nq, nr) == 0
        assert lib.hpvg_patchnn_subset_u8(p, *shapes[:3], p, *shapes[3:], *geo, p, nq, p, nr, p, p, p, 1 << 40, None) == ERR_ARG
    for nq, nr in ((-5, 1), (1, -5)):      # a negative count is a null list only in the ws query
        assert lib.hpvg_patchnn_subset_u8(p, *shapes[:3], p, *shapes[3:], *geo, p, nq, p, nr, p, p, p, 1 << 40, None) == ERR_ARG
    # a null list's count is ignored: these get as far as the workspace test
    assert lib.hpvg_patchnn_subset_u8(p, *shapes[:3], p, *shapes[3:], *geo, None, 0, None, Nr + 7, p, p, None, 0, None) == ERR_WORKSPACE
    assert lib.hpvg_patchnn_subset_u8(p, *shapes[:3], p, *shapes[3:], *geo, p, Nq, p, Nr, p, p, None, 0, None) == ERR_WORKSPACE


# ---- mask resize
def _conn(S, O):
    """The rule, written out pair by pair."""
    c = np.zeros((O, S), bool)
    for o in range(O):
        for i in range(S):
            c[o, i] = O == 1 or S == 1 or abs(i * (O - 1) - o * (S - 1)) < max(O - 1, S - 1)
    return c


def test_mask_resize_hand_case_and_identity():
    f = generate_patchnn.patchnn_mask_resize
    want = np.array([[1, 1, 0, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 1]], bool)
    assert np.array_equal(_conn(7, 4), want)
    for i in range(7):
        m = np.zeros((2, 7, 7), bool)
        m[1, 3, i] = True
        got = f(m, (2, 7, 4))
        assert got.dtype == np.bool_ and got.shape == (2, 7, 4)
        assert not got[0].any() and np.array_equal(got[1, 3], want[:, i]) and got[1].sum() == want[:, i].sum()
        m = np.zeros((1, 7, 5), bool)
        m[0, i, 2] = True
        assert np.array_equal(f(m, (1, 4, 5))[0, :, 2], want[:, i])
    m = np.random.default_rng(60).random((3, 9, 11)) < 0.3
    assert np.array_equal(f(m, (3, 9, 11)), m)
    t = f(torch.from_numpy(m), (3, 5, 17))                      # a tensor gives a tensor
    assert isinstance(t, torch.Tensor) and t.dtype == torch.bool and np.array_equal(t.numpy(), f(m, (3, 5, 17)))
    for bad in ((2, 9, 11), (3, 0, 11), (9, 11)):
        with pytest.raises(ValueError, match="patchnn_mask_resize"):
            f(m, bad)
    with pytest.raises(ValueError, match="patchnn_mask_resize"):
        f(m.astype(np.uint8), (3, 9, 11))


def test_mask_resize_is_the_rule_and_contains_what_the_linear_resize_reads():
    f = generate_patchnn.patchnn_mask_resize
    rng = np.random.default_rng(61)
    for (S_h, S_w), (O_h, O_w) in [((19, 34), (26, 46)), ((26, 46), (19, 34)), ((40, 48), (30, 36)), ((30, 36), (40, 48)),
                                   ((1, 9), (5, 1)), ((7, 7), (4, 13)), ((12, 5), (12, 9)), ((2, 39), (39, 2))]:
        for density in (0.02, 0.3):
            m = rng.random((2, S_h, S_w)) < density
            m[0, rng.integers(S_h), rng.integers(S_w)] = True
            got = f(m, (2, O_h, O_w))
            ch, cw = _conn(S_h, O_h), _conn(S_w, O_w)
            want = np.einsum("oi,tij,pj->top", ch.astype(np.int64), m.astype(np.int64), cw.astype(np.int64)) > 0
            assert np.array_equal(got, want), ((S_h, S_w), (O_h, O_w))
            assert got[0].any()                                             # a non-empty mask stays non-empty
            # floor and ceil of the exact align-corners source coordinate, per axis
            reads = []
            for S, O in ((S_h, O_h), (S_w, O_w)):
                x = [Fraction(o * (S - 1), O - 1) if O > 1 else Fraction(0) for o in range(O)]
                reads.append([(int(v.numerator // v.denominator), int(-((-v.numerator) // v.denominator))) for v in x])
            for oy, ys in enumerate(reads[0]):
                for ox, xs in enumerate(reads[1]):
                    read = m[:, list(ys)][:, :, list(xs)].any((1, 2))
                    assert (got[:, oy, ox] >= read).all()
    for S in range(2, 40):       # when downsizing every source has a connected output: no set voxel vanishes
        for O in range(1, S + 1):
            assert _conn(S, O).any(0).all(), (S, O)


# ---- the program's host side
def test_parser_has_mask_and_keeps_its_defaults():
    p = generate_patchnn.generate_patchnn_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert a.mask is None
    assert (a.exp_dir, a.video_path, a.image_path, a.out, a.num_samples, a.seed, a.patch, a.ratio, a.min_size, a.iters, a.alpha, a.noise,
            a.size, a.save_levels) == ("e", None, None, None, 8, 0, None, 0.75, 16, 10, 0.005, 0.75, None, False)
    assert p.parse_args(["--exp-dir", "e", "--mask", "hole.npy"]).mask == "hole.npy"
    with pytest.raises(SystemExit):
        p.parse_args(["--exp-dir", "e", "--mask"])


def test_mask_refusals_that_need_no_device(tmp_path):
    """--mask with another --size, an empty and an all-hole mask end the program before gpu_device() is asked (which would end it
    too where there is no GPU, with another message)."""
    clip, hole = str(tmp_path / "clip.npy"), str(tmp_path / "hole.npy")
    np.save(clip, np.zeros((6, 40, 48, 3), np.uint8))
    m = np.zeros((6, 40, 48), np.uint8)
    m[2:4, 10:20, 10:22] = 1
    np.save(hole, m)
    with pytest.raises(SystemExit, match="--size .* is not the mask's"):
        generate_patchnn.generate_patchnn(video_path=clip, out=str(tmp_path / "o"), mask=hole, size=(6, 40, 64))
    np.save(hole, np.zeros((6, 40, 48), bool))
    with pytest.raises(SystemExit, match="--mask is empty"):
        generate_patchnn.generate_patchnn(video_path=clip, out=str(tmp_path / "o"), mask=hole)
    np.save(hole, np.full((6, 40, 48, 3), [0, 0, 9], np.uint8))       # [...,3]: any nonzero channel is hole
    with pytest.raises(SystemExit, match="--mask is all hole"):
        generate_patchnn.generate_patchnn(video_path=clip, out=str(tmp_path / "o"), mask=hole)
    np.save(hole, np.zeros((6, 40, 48), np.float32))
    with pytest.raises(SystemExit, match="--mask must be bool or uint8"):
        generate_patchnn.generate_patchnn(video_path=clip, out=str(tmp_path / "o"), mask=hole)
    assert not os.path.exists(str(tmp_path / "o"))


def test_load_mask_forms(tmp_path):
    f = generate_patchnn.load_mask
    m = np.zeros((3, 8, 9), bool)
    m[1, 2:4, 5] = True
    for k, arr in enumerate((m, m.astype(np.uint8) * 200, np.stack([m * 0, m * 7, m * 0], -1).astype(np.uint8))):
        path = str(tmp_path / ("m%d.npy" % k))
        np.save(path, arr)
        got = f(path, (3, 8, 9))
        assert got.dtype == np.bool_ and np.array_equal(got, m)
    path = str(tmp_path / "img.npy")
    np.save(path, m[1])
    assert np.array_equal(f(path, (1, 8, 9)), m[1:2])
    from PIL import Image
    png = str(tmp_path / "hole.png")
    Image.fromarray(m[1].astype(np.uint8) * 255).save(png)
    assert np.array_equal(f(png, (1, 8, 9)), m[1:2])
    frames = tmp_path / "frames"
    frames.mkdir()
    for t in range(3):
        Image.fromarray(m[t].astype(np.uint8) * 255).save(str(frames / ("%02d.png" % t)))
    assert np.array_equal(f(str(frames), (3, 8, 9)), m)
    with pytest.raises(SystemExit, match="must have the real volume's shape"):
        f(str(frames), (3, 8, 10))
    # an [H,W,3] array reads as a volume of W = 3 and as an image mask; the real volume's shape decides
    path = str(tmp_path / "hw3.npy")
    arr = np.zeros((8, 9, 3), np.uint8)
    arr[2, 5, 1] = 1
    np.save(path, arr)
    forms = generate_patchnn.mask_forms(path)
    assert [m.shape for m in forms] == [(8, 9, 3), (1, 8, 9)] and all(m.dtype == np.bool_ for m in forms)
    assert f(path, (1, 8, 9)).sum() == 1 and f(path, (1, 8, 9))[0, 2, 5] and np.array_equal(f(path, (8, 9, 3)), arr != 0)
    np.save(path, np.zeros((2, 3, 4, 5, 3), np.uint8))
    with pytest.raises(SystemExit, match="--mask must be"):
        generate_patchnn.mask_forms(path)
