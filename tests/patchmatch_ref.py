"""numpy restatement of the deterministic PatchMatch rule of hpvg_patchmatch_u8 (include/hpvg.h), vectorised per candidate over
all query patches: every candidate of the rule is one pass that scores it for all patches at once and replaces the running
best where its key is strictly smaller.  Integers are int64 / uint64 holding 32-bit values; weighted scores are numpy float32
(one conversion, one multiply).  `defect` seeds one of three mistakes on purpose, for the tests that show the equality check
would notice them."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

M32 = 0xFFFFFFFF
START_IT = 0xFFFFFF


def h32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def rnd(seed, i, it, k, ax):
    """uint64 array (values < 2^32) for the flat query indices i."""
    i = np.asarray(i, dtype=np.uint64)
    c = ((int(it) * 64 + int(k) * 4 + int(ax)) * 0x85EBCA6B + (int(seed) & M32)) & M32
    return h32((i * np.uint64(0x9E3779B9) + np.uint64(c)) & np.uint64(M32))


def patch_matrix(vol, patch):
    """int64 [N][D] patches of a uint8 [T][H][W][3] volume in (t, y, x) raster order of the dense grid, and the grid."""
    win = sliding_window_view(vol, tuple(patch) + (3,))[:, :, :, 0]
    grid = win.shape[:3]
    return win.reshape(grid[0] * grid[1] * grid[2], -1).astype(np.int64), grid


def brute_mean_d2(q, r, patch):
    """Mean over the query patches of the exact nearest distance (the convergence yardstick)."""
    if q.ndim == 3:
        q, r = q[None], r[None]
    Q, _ = patch_matrix(q, patch)
    R, _ = patch_matrix(r, patch)
    Qf, Rf = Q.astype(np.float64), R.astype(np.float64)
    rn = (Rf * Rf).sum(1)
    best = np.empty(len(Q))
    for i0 in range(0, len(Q), 1024):
        Qc = Qf[i0:i0 + 1024]
        best[i0:i0 + 1024] = ((Qc * Qc).sum(1)[:, None] + rn[None, :] - 2.0 * (Qc @ Rf.T)).min(1)
    return float(best.mean())


def patch_match_ref(q, r, patch, iters, seed=0, rweight=None, nn_init=None, defect=None, info=None):
    """(d2 int64, nn int64, score float32 or None), shaped as the query grid (images: without the leading 1).
    defect: None, 'tie_larger' (ties go to the larger index), 'no_shift' (propagation without - s e_ax) or 'in_place' (the
    propagation reads the field being written).  info: a dict that receives `seen_min`, per patch the smallest index among the
    start and every candidate scored, and `keys`, the per-iteration (primary, nn) pairs (start first)."""
    image = q.ndim == 3
    if image:
        q, r = q[None], r[None]
    Q, qg = patch_matrix(q, patch)
    R, rg = patch_matrix(r, patch)
    Nq, Nr = len(Q), len(R)
    i = np.arange(Nq, dtype=np.int64)
    a = np.stack(np.unravel_index(i, qg))                 # [3][Nq]
    w = None if rweight is None else np.asarray(rweight, np.float32).reshape(-1)
    assert w is None or w.shape == (Nr,)

    def flat(c):
        return (c[0] * rg[1] + c[1]) * rg[2] + c[2]

    def primary(rows, j):
        d = ((Q[rows] - R[j]) ** 2).sum(1)
        return d, (d if w is None else d.astype(np.float32) * w[j])

    if nn_init is None:
        b = np.stack([(rnd(seed, i, START_IT, 0, ax) % np.uint64(rg[ax])).astype(np.int64) for ax in range(3)])
    else:
        b = np.stack(np.unravel_index(np.clip(np.asarray(nn_init, np.int64).reshape(-1), 0, Nr - 1), rg)).astype(np.int64)
    bj = flat(b)
    bd, bp = primary(i, bj)
    seen = bj.copy()
    keys = [(bp.copy(), bj.copy())]

    def consider(c, valid):
        nonlocal bd, bp, bj, b
        rows = np.flatnonzero(valid)
        if not len(rows):
            return
        cj = flat(c[:, rows])
        seen[rows] = np.minimum(seen[rows], cj)
        d, p = primary(rows, cj)
        tie = (cj > bj[rows]) if defect == "tie_larger" else (cj < bj[rows])
        better = (p < bp[rows]) | ((p == bp[rows]) & tie)
        win = rows[better]
        bd[win], bp[win], bj[win] = d[better], p[better], cj[better]
        b[:, win] = c[:, rows][:, better]

    R0 = max(rg)
    for it in range(iters):
        old = b if defect == "in_place" else b.copy()
        for ax in range(3):
            for s in (-1, 1):
                na = a.copy()
                na[ax] += s
                inside = (na[ax] >= 0) & (na[ax] < qg[ax])
                nb = np.where(inside, (na[0] * qg[1] + na[1]) * qg[2] + na[2], 0)
                c = old[:, nb].copy()
                if defect != "no_shift":
                    c[ax] -= s
                consider(c, inside & (c[ax] >= 0) & (c[ax] < rg[ax]))
        k = 0
        while (R0 >> k) >= 1:
            rk = R0 >> k
            c = np.stack([np.clip(b[ax] + (rnd(seed, i, it, k, ax) % np.uint64(2 * rk + 1)).astype(np.int64) - rk, 0, rg[ax] - 1)
                          for ax in range(3)])
            consider(c, np.ones(Nq, bool))
            k += 1
        keys.append((bp.copy(), bj.copy()))
    if info is not None:
        info["seen_min"] = seen.reshape(qg[1:] if image else qg)
        info["keys"] = keys
    shape = qg[1:] if image else qg
    score = None if w is None else bp.astype(np.float32).reshape(shape)
    return bd.reshape(shape), bj.reshape(shape), score
