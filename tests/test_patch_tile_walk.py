"""The step from one column tile to the next inside a workgroup of the patch searches (pnn_tile_products called twice by the
same workgroup: the first LDS store of the next tile after the last reads of the previous one, and for the self search the
jt == blockIdx.x diagonal in the middle of a walk).  The split rule gives every workgroup one column tile until row tiles x
column tiles > 2048, so no smaller case reaches it.  Two image pairs, random bytes, dense grids:
  patch 1 x 7 x 7: 5824 patches a side, D = 147 -> 3 K steps (the last one reads LDS buffer 0), 46 x 46 tiles, 23 splits of 2;
  patch 1 x 5 x 5: 6138 patches a side, D = 75 -> 2 K steps (the last one reads LDS buffer 1), 48 x 48 tiles, 24 splits of 2.
Every comparison is torch.equal against the numpy yardsticks of patch_ref.py / prdc_ref.py; there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from hp_vae_gan_amd import ops

from patch_ref import brute, brute_weighted
from prdc_ref import ref_ball_count, ref_knn_self

pytestmark = pytest.mark.gpu
PATCHES = ((1, 7, 7), (1, 5, 5))
TILE, BK, TARGET_WGS = 128, 64, 2048     # PNN_TILE, PNN_BK, PNN_TARGET_WGS of csrc/patchnn.hip


@functools.lru_cache(maxsize=None)
def _images():
    """(query [70,97,3], ref [97,70,3]) - built once, then shared and never modified"""
    rng = np.random.default_rng(11)
    return (rng.integers(0, 256, size=(70, 97, 3), dtype=np.uint8), rng.integers(0, 256, size=(97, 70, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _ref_knn(patch):
    """int64 [gH][gW][8] of the ref image - computed once and shared by the k-nearest and the ball count tests"""
    return ref_knn_self(_images()[1], patch, 8)[0]


def _walk(nrt, nct):
    """(splits, tiles per split) as pnn_splits of csrc/patchnn.hip chooses them"""
    splits = max(1, min(nct, -(-TARGET_WGS // nrt)))
    per = -(-nct // splits)
    return -(-nct // per), per


@pytest.mark.parametrize("patch,n,ksteps,tiles,splits", [((1, 7, 7), 5824, 3, 46, 23), ((1, 5, 5), 6138, 2, 48, 24)])
def test_the_shapes_walk_two_column_tiles_per_workgroup(patch, n, ksteps, tiles, splits):
    q, r = _images()
    Nq, Nr, D = ops.patch_nn_counts((1,) + q.shape[:2], (1,) + r.shape[:2], patch)
    assert (Nq, Nr) == (n, n) and -(-D // BK) == ksteps
    assert -(-n // TILE) == tiles and _walk(tiles, tiles) == (splits, 2)


@pytest.mark.parametrize("patch", PATCHES)
def test_patch_nn(patch):
    q, r = _images()
    d2, nn = ops.patch_nn(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), patch)
    want_d2, want_nn = brute(q, r, patch)
    assert torch.equal(d2.cpu().to(torch.int64), torch.from_numpy(want_d2[0]))
    assert torch.equal(nn.cpu().to(torch.int64), torch.from_numpy(want_nn[0]))


@pytest.mark.parametrize("patch", PATCHES)
def test_patch_nn_weighted(patch):
    q, r = _images()
    n = ops.patch_nn_counts((1,) + q.shape[:2], (1,) + r.shape[:2], patch)[1]
    w = np.random.default_rng(12).uniform(0.5, 2.0, size=n).astype(np.float32)
    score, nn = ops.patch_nn_weighted(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), torch.from_numpy(w).cuda(), patch)
    want_score, want_nn = brute_weighted(q, r, w, patch)
    assert torch.equal(score.cpu(), torch.from_numpy(want_score[0]))
    assert torch.equal(nn.cpu().to(torch.int64), torch.from_numpy(want_nn[0]))


@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("patch", PATCHES)
def test_patch_knn_self(patch, k):
    got = ops.patch_knn_self(torch.from_numpy(_images()[1]).cuda(), patch, k)
    assert torch.equal(got.cpu().to(torch.int64), torch.from_numpy(_ref_knn(patch)[..., :k]))


@pytest.mark.parametrize("patch", PATCHES)
def test_patch_ball_count(patch):
    q, r = _images()
    radius = np.ascontiguousarray(_ref_knn(patch)[..., 2])     # the k = 3 radii of the ref's own patches
    got = ops.patch_ball_count(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), torch.from_numpy(radius.astype(np.int32)).cuda(),
                               patch)
    assert torch.equal(got.cpu().to(torch.int64), torch.from_numpy(ref_ball_count(q, r, radius, patch)[0]))
