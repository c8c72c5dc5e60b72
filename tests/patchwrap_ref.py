"""numpy restatement of the ring contract of include/hpvg.h (generate_patchnn --wrap): the circular pad, the vote onto a ring
(hpvg_patch_vote_wrap_u8), PatchMatch between rings (hpvg_patchmatch_wrap_u8), one refine step composed of them, and the
seam coherence of `evaluate --wrap`.  The PatchMatch rule is written with the pieces of patchmatch_ref.py (hash, patch
matrix); everything is integer arithmetic or numpy float32, so every comparison against it is exact.  `defect` seeds one of
three mistakes on purpose, for the tests that show the equality checks would notice them."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from patchmatch_ref import START_IT, patch_matrix, rnd
from patch_ref import brute, brute_weighted

NONE = (0, 0, 0)


def wrap_pad(vol, patch, wrap):
    """uint8 [T,H,W,3] with its first p - 1 slices appended along every ring axis, in the order t, y, x."""
    out = vol
    for ax in range(3):
        if wrap[ax] and patch[ax] > 1:
            assert out.shape[ax] >= patch[ax]
            out = np.concatenate([out, np.take(out, np.arange(patch[ax] - 1), axis=ax)], axis=ax)
    return np.ascontiguousarray(out)


def periodic_grid(size, patch, wrap):
    return tuple(int(s) if w else int(s) - int(p) + 1 for s, p, w in zip(size, patch, wrap))


def vote_wrap_ref(values, nn, patch, fallback, wrap, rstride=(1, 1, 1), defect=None):
    """(out uint8 shaped as fallback, cnt): the vote into the circularly padded box - every periodic-grid patch is a dense patch
    of it - whose pad is then folded back onto the first slices, sums AND counts, before the one rounding.
    defect 'no_seam_votes': the pad is cut off instead, so the votes of the patches that cross a seam never reach the first
    slices."""
    pt, ph, pw = patch
    win = sliding_window_view(values, tuple(patch) + (3,))[:, :, :, 0][::rstride[0], ::rstride[1], ::rstride[2]]
    V = win.reshape(-1, pt, ph, pw, 3).astype(np.int64)
    size = fallback.shape[:3]
    grid = periodic_grid(size, patch, wrap)
    box = tuple(g + p - 1 for g, p in zip(grid, patch))
    total = np.zeros(box + (3,), np.int64)
    cnt = np.zeros(box + (1,), np.int64)
    flat = np.asarray(nn).reshape(-1)
    assert flat.size == grid[0] * grid[1] * grid[2]
    i = 0
    for t0 in range(grid[0]):
        for y0 in range(grid[1]):
            for x0 in range(grid[2]):
                j = int(flat[i])
                i += 1
                if 0 <= j < len(V):
                    total[t0:t0 + pt, y0:y0 + ph, x0:x0 + pw] += V[j]
                    cnt[t0:t0 + pt, y0:y0 + ph, x0:x0 + pw] += 1
    for ax in range(3):
        S, extra = size[ax], box[ax] - size[ax]
        if extra:
            assert wrap[ax] and extra == patch[ax] - 1 <= S
            folded = []
            for a in (total, cnt):
                head = np.take(a, np.arange(S), axis=ax).copy()
                if defect != "no_seam_votes":
                    idx = [slice(None)] * 4
                    idx[ax] = slice(0, extra)
                    head[tuple(idx)] += np.take(a, np.arange(S, S + extra), axis=ax)
                folded.append(head)
            total, cnt = folded
    out = (2 * total + cnt) // (2 * np.maximum(cnt, 1))
    return np.where(cnt > 0, out, fallback).astype(np.uint8), cnt[..., 0]


def patch_match_wrap_ref(q, r, patch, iters, seed=0, rweight=None, nn_init=None, qwrap=None, rwrap=None, defect=None):
    """(d2 int64, nn int64, score float32 or None) shaped as the query grid (images: without the leading 1): patch_match_ref's
    rule on volumes that arrive circularly padded, with the ring changes of hpvg_patchmatch_wrap_u8: on a qwrap axis the
    neighbour is taken modulo the query grid side and never skipped; on an rwrap axis the propagated candidate and the random
    candidate are taken modulo the key grid side instead of being skipped / clamped.
    defect: None, 'prop_no_wrap' (propagation ignores both flag sets) or 'clamp_not_mod' (the random search clamps on a ring)."""
    qwrap, rwrap = tuple(qwrap or NONE), tuple(rwrap or NONE)
    image = q.ndim == 3
    if image:
        q, r = q[None], r[None]
    Q, qg = patch_matrix(q, patch)
    R, rg = patch_matrix(r, patch)
    Nq, Nr = len(Q), len(R)
    i = np.arange(Nq, dtype=np.int64)
    a = np.stack(np.unravel_index(i, qg))
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

    def consider(c, valid):
        nonlocal bd, bp, bj, b
        rows = np.flatnonzero(valid)
        if not len(rows):
            return
        cj = flat(c[:, rows])
        d, p = primary(rows, cj)
        better = (p < bp[rows]) | ((p == bp[rows]) & (cj < bj[rows]))
        win = rows[better]
        bd[win], bp[win], bj[win] = d[better], p[better], cj[better]
        b[:, win] = c[:, rows][:, better]

    prop = defect != "prop_no_wrap"
    R0 = max(rg)
    for it in range(iters):
        old = b.copy()
        for ax in range(3):
            for s in (-1, 1):
                na = a.copy()
                na[ax] += s
                if qwrap[ax] and prop:
                    na[ax] %= qg[ax]
                    inside = np.ones(Nq, bool)
                else:
                    inside = (na[ax] >= 0) & (na[ax] < qg[ax])
                nb = np.where(inside, (na[0] * qg[1] + na[1]) * qg[2] + na[2], 0)
                c = old[:, nb].copy()
                c[ax] -= s
                if rwrap[ax] and prop:
                    c[ax] %= rg[ax]
                consider(c, inside & (c[ax] >= 0) & (c[ax] < rg[ax]))
        k = 0
        while (R0 >> k) >= 1:
            rk = R0 >> k
            cs = []
            for ax in range(3):
                v = b[ax] + (rnd(seed, i, it, k, ax) % np.uint64(2 * rk + 1)).astype(np.int64) - rk
                cs.append(v % rg[ax] if rwrap[ax] and defect != "clamp_not_mod" else np.clip(v, 0, rg[ax] - 1))   # numpy's % is >= 0
            consider(np.stack(cs), np.ones(Nq, bool))
            k += 1
    shape = qg[1:] if image else qg
    score = None if w is None else bp.astype(np.float32).reshape(shape)
    return bd.reshape(shape), bj.reshape(shape), score


def refine_wrap_ref(query, keys, values, patch, alpha_abs, wrap, search="exact", pm_iters=2, seed=0, fwd=None, rev=None,
                    defect=None):
    """(result, fwd field, rev field, seed after) of one generator step whose query is a ring along `wrap`: both searches on the
    padded query (exhaustive, or patch_match_wrap_ref with the flags on the query's side), weights 1 / (float32(m) +
    float32(alpha_abs)), and the vote onto the ring with the query as fallback.  wrap all zero: the plain step."""
    padded = wrap_pad(query, patch, wrap)
    rnn = None
    if search == "patchmatch":
        if np.isinf(alpha_abs):
            nn = patch_match_wrap_ref(padded, keys, patch, pm_iters, seed, None, fwd, qwrap=wrap, defect=defect)[1]
            seed += 1
        else:
            m, rnn, _ = patch_match_wrap_ref(keys, padded, patch, pm_iters, seed, None, rev, rwrap=wrap, defect=defect)
            w = np.float32(1.0) / (m.astype(np.float32) + np.float32(alpha_abs))
            nn = patch_match_wrap_ref(padded, keys, patch, pm_iters, seed + 1, w.reshape(-1), fwd, qwrap=wrap, defect=defect)[1]
            seed += 2
    elif np.isinf(alpha_abs):
        nn = brute(padded, keys, patch)[1]
    else:
        m, rnn = brute(keys, padded, patch)
        w = np.float32(1.0) / (m.astype(np.float32) + np.float32(alpha_abs))
        assert w.dtype == np.float32
        nn = brute_weighted(padded, keys, w.reshape(-1), patch)[1]
    out = vote_wrap_ref(values, nn, patch, query, wrap, defect=defect)[0]
    return out, nn, rnn, seed


def seam_ref(sample, real, patch, wrap, stride=(1, 1, 1)):
    """(seam_patches, seam_coherence) of `evaluate --wrap`: the patches of the sample's periodic grid at `stride` that cross at
    least one seam, and the mean over them of the exact nearest distance to real's dense patches over D * 255^2 (one Python
    int / int division; None without such patches)."""
    assert all(s == 1 for s, w in zip(stride, wrap) if w)
    d2 = brute(wrap_pad(sample, patch, wrap), real, patch, qstride=stride)[0]
    cross = np.zeros(d2.shape, bool)
    for ax in range(3):
        if wrap[ax]:
            idx = [slice(None)] * 3
            idx[ax] = slice(sample.shape[ax] - patch[ax] + 1, None)
            cross[tuple(idx)] = True
    n = int(cross.sum())
    D = 3 * patch[0] * patch[1] * patch[2]
    return n, (int(d2[cross].sum()) / (n * D * 255 * 255) if n else None)
