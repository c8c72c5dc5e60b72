"""hpvg_nnf_chunks_i32 / ops.nnf_chunks on the GPU against the union-find yardstick of tests/nnf_chunks_ref.py.

Every field is synthetic (no search), built once with its yardstick answer and shared; every comparison is torch.equal / ==.
Fields are written as a displacement in GRID units per patch: nn = the flat key index of (grid coordinate + displacement).
The serpentine case spans 80 workgroups of 256 threads, so one chunk's pieces are merged from different XCDs."""
import functools

import numpy as np
import pytest
import torch

from hp_vae_gan_amd import ops

from nnf_chunks_ref import pair_count, ref_chunks

pytestmark = pytest.mark.gpu
ONE = (1, 1, 1)


def _coords(grid):
    return np.meshgrid(*(np.arange(n, dtype=np.int64) for n in grid), indexing="ij")


def _field(grid, kgrid, dt, dy, dx):
    """int32 nn over `grid`: the key index of (t + dt, y + dy, x + dx); every key coordinate must lie in kgrid."""
    t, y, x = _coords(grid)
    b = (t + dt, y + dy, x + dx)
    assert all(int(c.min()) >= 0 and int(c.max()) < k for c, k in zip(b, kgrid))
    return ((b[0] * kgrid[1] + b[1]) * kgrid[2] + b[2]).astype(np.int32)


def _serpentine():
    grid, kgrid = (1, 128, 160), (1, 130, 162)
    _, y, x = _coords(grid)
    snake = (y % 2 == 0) | ((y % 4 == 1) & (x == grid[2] - 1) & (y < grid[1] - 1)) | ((y % 4 == 3) & (x == 0) & (y < grid[1] - 1))
    d = np.where(snake, 1, np.where((y + x) % 2 == 0, 0, 2))   # the wall alternates two other displacements: singletons
    assert int(snake.sum()) == 64 * 160 + 63
    return _field(grid, kgrid, 0, d, d), kgrid


@functools.lru_cache(maxsize=None)
def _case(name):
    """(nn, kgrid, qstride, rstride, d2, max_d2, (labels, sizes, stats) of the yardstick) - built once, never modified."""
    qs, rs, d2, max_d2 = ONE, ONE, None, None
    if name == "single":
        nn, kg = np.zeros((1, 1, 1), np.int32), (1, 1, 1)
    elif name == "identity":
        kg = (3, 9, 11)
        nn = np.arange(3 * 9 * 11, dtype=np.int32).reshape(kg)
    elif name == "shifted":
        kg = (4, 12, 15)
        nn = _field((3, 9, 11), kg, 1, 2, 3)
    elif name.startswith("stripes_"):
        g = (3, 5, 6)
        t, y, x = _coords(g)
        if name == "stripes_x":     # the displacement depends on (t, y) alone, and differs for any two of them
            kg, d = (3, 5, 6 + 15), (0, 0, t * 5 + y)
        elif name == "stripes_y":
            kg, d = (3, 5 + 18, 6), (0, t * 6 + x, 0)
        else:
            kg, d = (3 + 30, 5, 6), (y * 6 + x, 0, 0)
        nn = _field(g, kg, *d)
    elif name == "wrap":
        g, kg = (2, 6, 8), (2, 6, 14)
        _, _, x = _coords(g)
        nn = _field(g, kg, 0, 0, np.where((x == 0) | (x == 7), 0, x))
    elif name == "strided_voxel":   # b = (t, 2y + 1, 3x + 2): voxel displacement (t, 1, 2), grid displacement all over the place
        g, kg, qs, rs = (2, 4, 5), (2, 8, 15), (1, 2, 3), (2, 1, 1)
        t, y, x = _coords(g)
        nn = _field(g, kg, 0, y + 1, 2 * x + 2)
    elif name == "strided_grid":    # b = a + (0, 1, 2): one grid displacement, voxel displacement (t, 1 - y, 2 - 2x)
        g, kg, qs, rs = (2, 4, 5), (2, 8, 15), (1, 2, 3), (2, 1, 1)
        nn = _field(g, kg, 0, 1, 2)
    elif name == "random_uniform":
        kg = (4, 20, 25)
        nn = np.random.default_rng(11).integers(0, 4 * 20 * 25, size=(3, 18, 22)).astype(np.int32)
    elif name == "random_three":
        g, kg = (3, 18, 22), (4, 20, 24)
        pick = np.random.default_rng(12).integers(0, 3, size=g)
        disp = np.array([(0, 0, 0), (1, 1, 2), (0, 2, 1)])[pick]
        nn = _field(g, kg, disp[..., 0], disp[..., 1], disp[..., 2])
    elif name.startswith("excluded_"):
        kg = (3, 6, 7)
        nn = np.arange(3 * 6 * 7, dtype=np.int32).reshape(kg).copy()
        if name == "excluded_minus1":
            nn[:, 3, :] = -1
        elif name == "excluded_nr":
            nn[:, 3, :] = 3 * 6 * 7
        else:
            d2 = np.zeros(kg, np.int32)
            d2[:, 3, :] = 5 if name == "excluded_d2_gt4" else 1
            max_d2 = 4 if name == "excluded_d2_gt4" else 0
            if name == "excluded_d2_negative":
                d2[:, 3, :] = -3
    elif name == "serpentine":
        nn, kg = _serpentine()
    else:
        raise KeyError(name)
    return nn, kg, qs, rs, d2, max_d2, ref_chunks(nn, kg, qs, rs, d2, max_d2)


def _run(name):
    nn, kg, qs, rs, d2, max_d2, _ = _case(name)
    dev = torch.device("cuda")
    return ops.nnf_chunks(torch.from_numpy(nn).to(dev), kg, qstride=qs, rstride=rs,
                          d2=None if d2 is None else torch.from_numpy(d2).to(dev), max_d2=max_d2)


def _check(name):
    labels, sizes, stats = _run(name)
    want = _case(name)[6]
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and stats.dtype == torch.int64
    assert stats.cpu().tolist() == want[2].tolist()
    assert torch.equal(labels.cpu(), torch.from_numpy(want[0]))
    assert torch.equal(sizes.cpu(), torch.from_numpy(want[1]))
    return labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().tolist()


def test_single():
    labels, sizes, stats = _check("single")
    assert labels.tolist() == [[[0]]] and sizes.tolist() == [[[1]]] and stats == [1, 1, 0, 1, 1, 1]


def test_identity_is_one_chunk_in_place():
    labels, sizes, stats = _check("identity")
    Nq, E = 3 * 9 * 11, pair_count((3, 9, 11))
    assert stats == [Nq, Nq, E, 1, Nq, Nq * Nq] and not labels.any() and sizes.reshape(-1)[0] == Nq


def test_shifted_is_one_chunk_out_of_place():
    _, _, stats = _check("shifted")
    Nq = 3 * 9 * 11
    assert stats == [Nq, 0, pair_count((3, 9, 11)), 1, Nq, Nq * Nq]


@pytest.mark.parametrize("axis", ["t", "y", "x"])
def test_stripes_fix_the_axis_and_raster_order(axis):
    labels, sizes, stats = _check("stripes_" + axis)
    g = (3, 5, 6)
    t, y, x = _coords(g)
    flat = (t * g[1] + y) * g[2] + x
    a = "tyx".index(axis)
    start = flat - (t, y, x)[a] * (30, 6, 1)[a]    # the line's first patch
    assert np.array_equal(labels, start)
    n = g[a]
    assert stats[3:] == [90 // n, n, 90 // n * n * n] and stats[2] == 90 // n * (n - 1)
    assert np.array_equal(sizes, np.where(flat == start, n, 0))


def test_row_ends_are_not_linked():
    labels, _, stats = _check("wrap")
    assert stats[3] == 8 and stats[4] == 12                       # every column is a chunk of its own
    assert labels[0, 0, 7] == 7 and labels[0, 1, 0] == 0 and labels[1, 5, 7] == 7


def test_strides_enter_the_displacement():
    _, _, stats = _check("strided_voxel")
    assert stats[3:] == [2, 20, 800] and stats[1] == 0            # one chunk per t plane: 2 b_t - t differs
    _, _, stats = _check("strided_grid")
    assert stats[2:] == [0, 40, 1, 40]


@pytest.mark.parametrize("name", ["random_uniform", "random_three"])
def test_random_fields(name):
    _, _, stats = _check(name)
    assert stats[0] == 3 * 18 * 22
    if name == "random_three":
        assert 1 < stats[4] < stats[0] and stats[3] > 10          # many interlocking mid-sized chunks, as intended


@pytest.mark.parametrize("how", ["minus1", "nr", "d2_gt0", "d2_gt4", "d2_negative"])
def test_excluded_plane_cuts_the_chunk_in_two(how):
    labels, sizes, stats = _check("excluded_" + how)
    assert (labels[:, 3, :] == -1).all() and (sizes[:, 3, :] == 0).all()
    assert stats[0] == 126 - 21 and stats[3] == 2 and stats[4] == 63   # y < 3: 3 * 3 * 7, y > 3: 3 * 2 * 7
    assert set(np.unique(labels).tolist()) == {-1, 0, 28}


def test_null_d2_keeps_everything():
    nn, kg = _case("excluded_d2_gt0")[:2]
    got = ops.nnf_chunks(torch.from_numpy(nn).cuda(), kg)
    assert got[2].cpu().tolist() == [126, 126, pair_count(kg), 1, 126, 126 * 126]


def test_serpentine_across_workgroups():
    labels, sizes, stats = _check("serpentine")
    assert stats[3] == 1 + 10177 and stats[4] == 10303 and stats[5] == 10303 * 10303 + 10177
    assert sizes[0, 0, 0] == 10303 and labels[0, 126, 159] == 0


@pytest.mark.parametrize("name", ["serpentine", "random_three", "random_uniform"])
def test_two_runs_are_identical(name):
    a, b = _run(name), _run(name)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_image_form():
    nn, kg = _case("serpentine")[:2]
    dev_nn = torch.from_numpy(nn).cuda()
    l3, s3, st3 = ops.nnf_chunks(dev_nn, kg)
    l2, s2, st2 = ops.nnf_chunks(dev_nn[0], kg)
    assert l2.shape == (128, 160) and s2.shape == (128, 160)
    assert torch.equal(l2, l3[0]) and torch.equal(s2, s3[0]) and torch.equal(st2, st3)


def test_errors_are_raised_by_name():
    nn = torch.zeros(2, 3, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="nnf_chunks: nn must be"):
        ops.nnf_chunks(nn.to(torch.int64), (2, 3, 4))
    with pytest.raises(RuntimeError, match="nnf_chunks: nn must be"):
        ops.nnf_chunks(nn.reshape(-1), (2, 3, 4))
    with pytest.raises(RuntimeError, match="nnf_chunks: nn is on cpu"):
        ops.nnf_chunks(nn.cpu(), (2, 3, 4))
    with pytest.raises(RuntimeError, match="nnf_chunks: d2 and max_d2 go together"):
        ops.nnf_chunks(nn, (2, 3, 4), d2=nn)
    with pytest.raises(RuntimeError, match="nnf_chunks: d2 must be int32"):
        ops.nnf_chunks(nn, (2, 3, 4), d2=nn[0], max_d2=0)
    with pytest.raises(RuntimeError, match="nnf_chunks: max_d2"):
        ops.nnf_chunks(nn, (2, 3, 4), d2=nn, max_d2=-1)
    with pytest.raises(RuntimeError, match="nnf_chunks: ref_grid"):
        ops.nnf_chunks(nn, (2, 0, 4))
    with pytest.raises(RuntimeError, match="nnf_chunks: ref_grid must have 3 entries"):
        ops.nnf_chunks(nn, (3, 4))
    with pytest.raises(RuntimeError, match="nnf_chunks: strides"):
        ops.nnf_chunks(nn, (2, 3, 4), qstride=(1, 0, 1))
