"""The numpy restatements of the byte-tensor patch kernels, written from the definitions in include/hpvg.h and shared by the
suites that check them (tests/test_patchnn.py, test_patchgen.py, test_patchinpaint.py, test_patchswd.py,
test_byte_offset_launches.py): the exact search and its weighted and subset forms, the vote, the mask count, the projection
histograms and their W1 numerators.  Everything is exact integer (or single-rounding fp32) arithmetic: the comparisons built on
these are equalities."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ONE = (1, 1, 1)


def _patches(vol, patch, stride):
    """float64 [N][D] patch matrix of a uint8 [T][H][W][3] volume, patches in (t, y, x) raster order of the strided grid."""
    win = sliding_window_view(vol, tuple(patch) + (3,))[:, :, :, 0]
    win = win[::stride[0], ::stride[1], ::stride[2]]
    grid = win.shape[:3]
    return win.reshape(grid[0] * grid[1] * grid[2], -1).astype(np.float64), grid


def brute(q, r, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    if q.ndim == 3:
        q, r = q[None], r[None]
    Q, grid = _patches(q, patch, qstride)
    R, _ = _patches(r, patch, rstride)
    rn = (R * R).sum(1)
    d2 = np.empty(len(Q), np.int64)
    nn = np.empty(len(Q), np.int64)
    for i0 in range(0, len(Q), 1024):
        Qc = Q[i0:i0 + 1024]
        dist = (Qc * Qc).sum(1)[:, None] + rn[None, :] - 2.0 * (Qc @ R.T)
        j = dist.argmin(1)
        nn[i0:i0 + 1024] = j
        d2[i0:i0 + 1024] = dist[np.arange(len(Qc)), j]
    return d2.reshape(grid), nn.reshape(grid)


def brute_weighted(q, r, w, patch, qstride=ONE, rstride=ONE):
    """(score float32, nn int64) shaped as the query grid: min_j float32(d2_ij) * w[j] and the first j that attains it."""
    if q.ndim == 3:
        q, r = q[None], r[None]
    Q, grid = _patches(q, patch, qstride)
    R, _ = _patches(r, patch, rstride)
    w = np.asarray(w, np.float32).reshape(-1)
    assert w.shape == (len(R),)
    rn = (R * R).sum(1)
    score = np.empty(len(Q), np.float32)
    nn = np.empty(len(Q), np.int64)
    for i0 in range(0, len(Q), 1024):
        Qc = Q[i0:i0 + 1024]
        dist = (Qc * Qc).sum(1)[:, None] + rn[None, :] - 2.0 * (Qc @ R.T)     # exact integers in float64
        s = dist.astype(np.float32) * w[None, :]
        assert s.dtype == np.float32
        j = s.argmin(1)
        nn[i0:i0 + 1024] = j
        score[i0:i0 + 1024] = s[np.arange(len(Qc)), j]
    return score.reshape(grid), nn.reshape(grid)


def vote_ref(values, nn, patch, fallback, qstride=ONE, rstride=ONE):
    """numpy vote: values / fallback uint8 [T,H,W,3], nn flat indices into values' grid (entries outside [0, Nr) are skipped)."""
    pt, ph, pw = patch
    win = sliding_window_view(values, tuple(patch) + (3,))[:, :, :, 0][::rstride[0], ::rstride[1], ::rstride[2]]
    V = win.reshape(-1, pt, ph, pw, 3).astype(np.int64)
    T, H, W = fallback.shape[:3]
    total = np.zeros((T, H, W, 3), np.int64)
    cnt = np.zeros((T, H, W, 1), np.int64)
    i = 0
    for t0 in range(0, T - pt + 1, qstride[0]):
        for y0 in range(0, H - ph + 1, qstride[1]):
            for x0 in range(0, W - pw + 1, qstride[2]):
                j = int(nn.reshape(-1)[i])
                i += 1
                if 0 <= j < len(V):
                    total[t0:t0 + pt, y0:y0 + ph, x0:x0 + pw] += V[j]
                    cnt[t0:t0 + pt, y0:y0 + ph, x0:x0 + pw] += 1
    assert i == nn.size
    out = (2 * total + cnt) // (2 * np.maximum(cnt, 1))
    return np.where(cnt > 0, out, fallback).astype(np.uint8), cnt[..., 0]


def brute_subset(q, r, patch, qsel=None, rsel=None, qstride=ONE, rstride=ONE):
    """(d2, nn) int64 shaped as the query grid: brute force between the selected rows, nn in r's grid, -1 / -1 elsewhere."""
    if q.ndim == 3:
        q, r = q[None], r[None]
    Q, grid = _patches(q, patch, qstride)
    R, _ = _patches(r, patch, rstride)
    qi = np.arange(len(Q)) if qsel is None else np.asarray(qsel, np.int64)
    ri = np.arange(len(R)) if rsel is None else np.asarray(rsel, np.int64)
    Qs, Rs = Q[qi], R[ri]
    dist = (Qs * Qs).sum(1)[:, None] + (Rs * Rs).sum(1)[None, :] - 2.0 * (Qs @ Rs.T)     # exact integers in float64
    j = dist.argmin(1)
    d2 = np.full(len(Q), -1, np.int64)
    nn = np.full(len(Q), -1, np.int64)
    d2[qi] = dist[np.arange(len(qi)), j]
    nn[qi] = ri[j]
    return d2.reshape(grid), nn.reshape(grid)


def count_ref(mask, patch, stride=ONE):
    win = sliding_window_view(mask != 0, tuple(patch))[::stride[0], ::stride[1], ::stride[2]]
    return win.sum((3, 4, 5)).astype(np.int64)


def ref_hist(vol, patch, S, stride=ONE):
    """(int32 [P][NB] histograms, N) of a uint8 volume's patch projections on the rows of S, from the definition."""
    if vol.ndim == 3:
        vol = vol[None]
    X = _patches(vol, patch, stride)[0].astype(np.int64) - 128
    N, D = X.shape
    assert S.shape[1] == D
    proj = X @ S.T.astype(np.int64) + 128 * D
    assert proj.min() >= 0 and proj.max() <= 256 * D
    return np.stack([np.bincount(proj[:, p], minlength=256 * D + 1) for p in range(S.shape[0])]).astype(np.int32), N


def ref_num(hA, Na, hB, Nb):
    """Python-integer numerators sum_b |Nb cA(b) - Na cB(b)| of two [P][NB] histograms."""
    out = []
    for a, b in zip(hA, hB):
        cA, cB = np.cumsum(a.astype(np.int64)).astype(object), np.cumsum(b.astype(np.int64)).astype(object)
        out.append(int(np.abs(int(Nb) * cA - int(Na) * cB).sum()))
    return out
