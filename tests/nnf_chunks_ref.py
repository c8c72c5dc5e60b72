"""The yardstick of hpvg_nnf_chunks_i32 / ops.nnf_chunks: a numpy / pure-Python union-find written from the definition.

nn: integers over the query patch grid (gT, gH, gW) (a 2-D array is gT = 1), indices into the key grid ref_grid = (kT, kH, kW).
Patch i at grid coordinate a with nn[i] at key coordinate b has the displacement b * rstride - a * qstride.  It is kept iff
0 <= nn[i] < Nr and (d2 is None or 0 <= d2[i] <= max_d2).  Two patches that differ by +1 along exactly one grid axis are a pair;
a pair is coherent iff both are kept and their displacements are equal; chunks are the connected components of the kept patches
under coherent pairs.  labels = the smallest flat index of the patch's chunk (-1 where not kept), sizes = the chunk's size at
labels[i] == i and 0 elsewhere, stats = (kept, in_place, coherent_pairs, chunks, largest, sum of size^2)."""
import numpy as np


def pair_count(grid):
    gT, gH, gW = grid
    return (gT - 1) * gH * gW + gT * (gH - 1) * gW + gT * gH * (gW - 1)


def displacements(nn, ref_grid, qstride=(1, 1, 1), rstride=(1, 1, 1), d2=None, max_d2=None):
    """(kept bool [gT,gH,gW], delta int64 [gT,gH,gW,3]); delta is meaningless where not kept."""
    nn = np.asarray(nn).astype(np.int64)
    if nn.ndim == 2:
        nn = nn[None]
    kT, kH, kW = (int(e) for e in ref_grid)
    kept = (nn >= 0) & (nn < kT * kH * kW)
    if d2 is not None:
        d = np.asarray(d2).astype(np.int64).reshape(nn.shape)
        kept &= (d >= 0) & (d <= int(max_d2))
    j = np.where(kept, nn, 0)
    b = np.stack([j // (kH * kW), (j // kW) % kH, j % kW], -1)
    a = np.stack(np.meshgrid(*(np.arange(n, dtype=np.int64) for n in nn.shape), indexing="ij"), -1)
    return kept, b * np.asarray(rstride, np.int64) - a * np.asarray(qstride, np.int64)


def ref_chunks(nn, ref_grid, qstride=(1, 1, 1), rstride=(1, 1, 1), d2=None, max_d2=None, wrap_defect=False):
    """(labels int32, sizes int32, stats int64 [6]) shaped as nn.  wrap_defect=True plants the bug of linking flat neighbours
    across the end of a row or plane (for the test that such a result is told apart)."""
    shape = np.asarray(nn).shape
    kept, delta = displacements(nn, ref_grid, qstride, rstride, d2, max_d2)
    grid = kept.shape
    N = kept.size
    flat = np.arange(N, dtype=np.int64).reshape(grid)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(u, v):
        u, v = find(u), find(v)
        if u != v:
            parent[max(u, v)] = min(u, v)

    pairs = 0
    for axis in range(3):
        lo = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        hi = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        coh = kept[lo] & kept[hi] & (delta[lo] == delta[hi]).all(-1)
        pairs += int(coh.sum())
        for u, v in zip(flat[lo][coh].tolist(), flat[hi][coh].tolist()):
            union(u, v)
    if wrap_defect:
        k, d = kept.reshape(-1), delta.reshape(-1, 3)
        for u in range(N - 1):
            if k[u] and k[u + 1] and (d[u] == d[u + 1]).all():
                union(u, u + 1)
    keptf = kept.reshape(-1)
    labels = np.array([find(i) if keptf[i] else -1 for i in range(N)], np.int64)
    sizes = np.bincount(labels[labels >= 0], minlength=N).astype(np.int64)
    roots = sizes[sizes > 0]
    in_place = int((kept & (delta == 0).all(-1)).sum())
    stats = np.array([int(keptf.sum()), in_place, pairs, len(roots), int(roots.max()) if len(roots) else 0,
                      int((roots * roots).sum())], np.int64)
    return labels.astype(np.int32).reshape(shape), sizes.astype(np.int32).reshape(shape), stats


def same(got, want):
    """Whether two (labels, sizes, stats) results are equal in every entry."""
    return all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g), np.asarray(w))
               for g, w in zip(got, want)) and len(got) == len(want) == 3
