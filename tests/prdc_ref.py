"""The yardstick of evaluate --prdc, written from the definitions with numpy (no device, no project code).

d2 is the exact squared patch distance: both patch matrices gathered with sliding_window_view, |q|^2 + |r|^2 - 2 Q R^T as a
float64 matmul (exact: every value is an integer far below 2^53).

  rad_X[j]   the k-th smallest d2(x_j, x_j') over j' != j (the diagonal is excluded by INDEX, np.sort along j': other patches
             at distance 0 count, each once), optionally raised to the floor
  precision  #{i : exists j, d2(s_i, r_j) <= rad_R[j]} / Ns
  density    sum_i #{j : d2(s_i, r_j) <= rad_R[j]} / (k Ns)
  recall     #{j : exists i, d2(r_j, s_i) <= rad_S[i]} / Nr
  coverage   #{j : min_i d2(r_j, s_i) <= rad_R[j]} / Nr

R: the real volume's patches on the dense grid; S: the sample's on the strided grid.  Each quotient is a Python int / int."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ONE = (1, 1, 1)


def patches(vol, patch, stride=ONE):
    """(float64 [N][D] patch matrix, grid) of a uint8 [T][H][W][3] volume, patches in (t, y, x) raster order of the strided grid."""
    win = sliding_window_view(vol, tuple(patch) + (3,))[:, :, :, 0]
    win = win[::stride[0], ::stride[1], ::stride[2]]
    grid = tuple(win.shape[:3])
    return win.reshape(grid[0] * grid[1] * grid[2], -1).astype(np.float64), grid


def dist2(Q, R):
    """int64 [Nq][Nr]"""
    d = (Q * Q).sum(1)[:, None] + (R * R).sum(1)[None, :] - 2.0 * (Q @ R.T)
    return d.astype(np.int64)


def _vol(v):
    return v[None] if v.ndim == 3 else v


def ref_knn_self(vol, patch, k, stride=ONE):
    """int64 [gT][gH][gW][k]: the k smallest d2 to the other patches of the same grid, ascending, with multiplicity."""
    X, grid = patches(_vol(vol), patch, stride)
    N = len(X)
    assert N > k >= 1
    d = dist2(X, X)
    d[np.arange(N), np.arange(N)] = np.iinfo(np.int64).max    # the diagonal, by index
    out = np.sort(d, axis=1)[:, :k]
    return out.reshape(grid + (k,))


def ref_ball_count(q, r, radius, patch, qstride=ONE, rstride=ONE):
    """int64, shaped as the query grid: #{j : d2(q_i, r_j) <= radius[j]}"""
    Q, grid = patches(_vol(q), patch, qstride)
    R, _ = patches(_vol(r), patch, rstride)
    rad = np.asarray(radius).reshape(-1).astype(np.int64)
    assert len(rad) == len(R)
    return (dist2(Q, R) <= rad[None, :]).sum(1).reshape(grid)


def ref_prdc(real, smp, patch, k, stride=ONE, floor=None):
    """dict: precision, recall, density, coverage (Python floats from int / int) and the arrays behind them: count (int64, the
    sample grid: balls of R that hold s_i), real_radius (int64, the real grid, floored), real_covered (bool, the real grid),
    zero_radius (the number of real patches whose UNFLOORED radius is 0)."""
    R, rgrid = patches(_vol(real), patch, ONE)
    S, sgrid = patches(_vol(smp), patch, stride)
    Nr, Ns, D = len(R), len(S), R.shape[1]
    rad_R = ref_knn_self(real, patch, k, ONE).reshape(Nr, k)[:, k - 1]
    rad_S = ref_knn_self(smp, patch, k, stride).reshape(Ns, k)[:, k - 1]
    zero = int((rad_R == 0).sum())
    if floor is not None:
        fl = int(np.floor(float(floor) * (D * 255 * 255)))
        rad_R, rad_S = np.maximum(rad_R, fl), np.maximum(rad_S, fl)
    d = dist2(S, R)                                   # [Ns][Nr]
    inside = d <= rad_R[None, :]
    count = inside.sum(1)
    covered = d.min(0) <= rad_R
    reached = (d <= rad_S[:, None]).any(0)
    return {"precision": int((count > 0).sum()) / Ns, "density": int(count.sum()) / (k * Ns),
            "recall": int(reached.sum()) / Nr, "coverage": int(covered.sum()) / Nr,
            "count": count.reshape(sgrid), "real_radius": rad_R.reshape(rgrid), "real_covered": covered.reshape(rgrid),
            "zero_radius": zero}


# ------------------------------------------------------------------------------------------------------------ fixtures
def smooth_volume(shape=(5, 24, 28), seed=0):
    """A smooth uint8 [T][H][W][3] volume: a few low-frequency waves per channel, seeded phases."""
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    out = np.empty(tuple(shape) + (3,), np.float64)
    for c in range(3):
        f = rng.uniform(0.15, 0.45, size=(3, 3))
        ph = rng.uniform(0, 2 * np.pi, size=3)
        out[..., c] = sum(np.sin(f[w, 0] * t + f[w, 1] * y + f[w, 2] * x + ph[w]) for w in range(3))
    out = (out - out.min()) / (out.max() - out.min())
    return np.round(out * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def program_fixture():
    """(real, samples [3]) of the program tests, built once and never modified: the copy, the volume whose right half is a copy
    of its left half (mode collapse), and a noisy copy."""
    real = smooth_volume()
    half = real.copy()
    half[:, :, 14:] = real[:, :, :14]
    noise = np.random.default_rng(1).integers(-6, 7, size=real.shape)
    noisy = np.clip(real.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return real, np.stack([real, half, noisy])


@functools.lru_cache(maxsize=None)
def program_want(k=3, stride=ONE, floor=None, patch=(3, 7, 7)):
    real, S = program_fixture()
    return tuple(ref_prdc(real, s, patch, k, stride, floor) for s in S)
