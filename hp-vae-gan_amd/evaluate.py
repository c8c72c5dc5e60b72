"""`python -m hp_vae_gan_amd.evaluate --exp-dir run/<clip>/<checkname>/experiment_<n>` (after `generate`), or
`--samples S.npy --real R.npy` without an experiment: patch nearest-neighbour coherence / completeness, nn_unique_frac and
diversity of the samples against the training clip, written to metrics.json; with --chunks also the copied-region statistics of
the nearest-neighbour field; with --prdc K also the patch sets' precision, recall, density and coverage at k = K; with --wrap AXES
also seam_coherence, the coherence of the patches that cross the seam of samples that are rings along those axes; with --scales K
also coherence / completeness at K coarser scales of an antialiased pyramid (the patch metrics alone are blind to layout)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import ops
from .programs import default_patch, gpu_device, load_opt, load_u8_frames, parse_wrap_axes, patchnn_wrap_pad, real_volume, write_frames


def evaluate_parser():
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.evaluate",
                                description="Score samples against the training clip: exact patch nearest-neighbour "
                                "coherence / completeness (bidirectional similarity) and SinGAN's diversity.")
    p.add_argument('--exp-dir', default=None, help='experiment_<n> directory (gives the samples\' default place and the real volume)')
    p.add_argument('--samples', default=None, help='samples.npy, uint8 [N,T,H,W,3] or [N,H,W,3] (default: <exp-dir>/eval/samples/'
                   'samples.npy, as `generate` writes it)')
    p.add_argument('--real', default=None, help='the real clip / image (.npy, frame directory or image file); with --exp-dir it '
                   'replaces the run\'s input and is trimmed, sampled and resized like it; without, it is used as it is')
    p.add_argument('--patch', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='patch (default 3 7 7, images 1 7 7)')
    p.add_argument('--stride', type=int, nargs=3, default=[1, 1, 1], metavar=('T', 'H', 'W'),
                   help='stride of the query side of each direction (the other side is always dense)')
    p.add_argument('--max-samples', type=int, default=None, help='score only the first N samples')
    p.add_argument('--out', default=None, help='directory of metrics.json (default: beside the samples)')
    p.add_argument('--swd', type=int, default=0, metavar='P', help='also report the exact sliced Wasserstein distance between the '
                   'patch distributions over P random directions with entries in {-1, 0, +1} (default 0: off)')
    p.add_argument('--swd-seed', type=int, default=0, help='seed of the directions')
    p.add_argument('--chunks', action='store_true', help='also report the copied regions of each sample: the connected components '
                   'of its patch grid under "neighbours whose nearest neighbours have the same displacement"')
    p.add_argument('--chunk-tol', type=_nonneg_float, default=None, metavar='X', help='with --chunks (which it implies): only patches '
                   'whose squared distance is at most floor(X * D * 255^2), X in the unit of coherence, belong to a chunk '
                   '(default: every patch does)')
    p.add_argument('--save-chunks', action='store_true', help='with --chunks (which it implies): write chunks.npz (labels, sizes, '
                   'nn) and one source_XXXX.gif / .png per sample, coloured by where each patch came from')
    p.add_argument('--prdc', type=_prdc_k, default=0, metavar='K', help='also report precision, recall, density and coverage of '
                   'each sample\'s patch set against the real one, every patch\'s radius being the distance to its K-th nearest '
                   'other patch of its own volume (1 <= K <= {}; default 0: off)'.format(ops.PATCH_KNN_MAX_K))
    p.add_argument('--prdc-floor', type=_nonneg_float, default=None, metavar='X', help='with --prdc (required): no radius below '
                   'floor(X * D * 255^2), X in the unit of coherence (default: none; saturated regions have radius 0)')
    p.add_argument('--save-prdc', action='store_true', help='with --prdc (without it: nothing): write prdc.npz (count per sample patch, '
                   'real_radius and real_covered on the real grid)')
    p.add_argument('--wrap', default=None, metavar='AXES', help='the samples are rings along these axes (distinct letters of t, h, w; '
                   'what `generate_patchnn --wrap` makes): also report seam_coherence, the coherence of the patches that cross a seam '
                   '(last slice into first).  --stride must be 1 on a ring axis; no t for images')
    p.add_argument('--scales', type=_scales_k, default=0, metavar='K', help='also report coherence and completeness at K coarser '
                   'scales: for k = 1..K every sample and the real volume are resized, each from its own full size, to (T, round(H R^k), '
                   'round(W R^k)) by the exact antialiased resize and searched with the same patch and --stride (default 0: off)')
    p.add_argument('--scale-ratio', type=_scale_ratio, default=None, metavar='R', help='with --scales (required): the size ratio '
                   'between two scales, in (0, 1) (default {})'.format(SCALE_RATIO))
    return p


SCALE_RATIO = 0.5   # --scale-ratio


def _scales_k(text):
    v = int(text)
    if v < 0:
        raise argparse.ArgumentTypeError("must be >= 0 (0: off), got %s" % text)
    return v


def _scale_ratio(text):
    v = float(text)
    if not 0.0 < v < 1.0:
        raise argparse.ArgumentTypeError("must lie in (0, 1), got %s" % text)
    return v


def scale_sizes(size, K, ratio=SCALE_RATIO):
    """[(T, H_k, W_k)] for k = 1..K of a (T, H, W) volume: H_k = floor(H ratio^k + 0.5), W_k alike; T is kept.  Host only."""
    T, H, W = (int(e) for e in size)
    return [(T, int(math.floor(H * float(ratio) ** k + 0.5)), int(math.floor(W * float(ratio) ** k + 0.5))) for k in range(1, int(K) + 1)]


def scales_check(K, ratio=None, sizes=(), patch=None):
    """Refuse what --scales cannot score, as the program's exit: --scale-ratio without --scales, K < 0, a ratio outside (0, 1)
    and, once the volumes' sizes and the patch are known, a K whose coarsest volume is smaller than the patch (the message
    names the largest K that fits).  Returns the ratio in force (None when off)."""
    K = int(K or 0)
    if K < 0:
        raise SystemExit("evaluate: --scales K must be >= 0, got {}".format(K))
    if K == 0:
        if ratio is not None:
            raise SystemExit("evaluate: --scale-ratio needs --scales K")
        return None
    ratio = SCALE_RATIO if ratio is None else float(ratio)
    if not 0.0 < ratio < 1.0:
        raise SystemExit("evaluate: --scale-ratio must lie in (0, 1), got {}".format(ratio))
    if patch is not None:
        fits = lambda k: all(all(s >= p for s, p in zip(scale_sizes(size, k, ratio)[-1], patch)) for size in sizes)   # noqa: E731
        if not fits(K):
            best = max([k for k in range(1, K) if fits(k)], default=0)
            raise SystemExit("evaluate: --scales {}: the volume at scale {} is smaller than the patch {}; the largest K that fits "
                             "is {}".format(K, K, list(patch), best))
    return ratio


def _nonneg_float(text):
    v = float(text)
    if not (v >= 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError("must be a finite number >= 0, got %s" % text)
    return v


def _prdc_k(text):
    v = int(text)
    if not 0 <= v <= ops.PATCH_KNN_MAX_K:
        raise argparse.ArgumentTypeError("must be in [1, %d] (0: off), got %s" % (ops.PATCH_KNN_MAX_K, text))
    return v


def patch_score(d2, D):
    """coherence / completeness of one direction: mean_i d2[i] / (D * 255^2), from the integer sum (exactly 0.0 for a copy and
    exactly 1.0 for black against white)."""
    d2 = torch.as_tensor(d2)
    return int(d2.sum(dtype=torch.int64)) / (d2.numel() * int(D) * 255 * 255)


def nn_unique_frac(nn, Nr):
    """Distinct nearest-neighbour indices over min(Nq, Nr): low for a sample stitched from a few source patches."""
    nn = torch.as_tensor(nn)
    return int(torch.unique(nn).numel()) / min(int(nn.numel()), int(Nr))


def diversity(samples, real):
    """SinGAN's diversity: the mean over pixels of the standard deviation across samples of the channel-mean intensity, over the
    standard deviation of that intensity over the real volume (population standard deviations).  samples: uint8 [N,T,H,W,3] /
    [N,H,W,3], real: [T',H,W,3] / [H,W,3]; None when there are fewer than 2 samples, H or W differ, or the real volume is
    shorter than the samples (its first T frames are used)."""
    samples, real = torch.as_tensor(samples), torch.as_tensor(real)
    if samples.shape[0] < 2 or samples.dim() != real.dim() + 1:
        return None
    if samples.dim() == 5:
        T = samples.shape[1]
        if real.shape[0] < T:
            return None
        real = real[:T]
    if tuple(samples.shape[1:]) != tuple(real.shape):
        return None
    s = samples.to(torch.float64).mean(-1)
    r = real.to(torch.float64).mean(-1)
    denom = float(r.std(unbiased=False))
    if denom == 0.0:
        return None
    return float(s.std(0, unbiased=False).mean()) / denom


def swd_directions(P, D, seed):
    """int8 [P][D] directions for the sliced Wasserstein distance: entries drawn uniformly from {-1, 0, +1} by
    numpy.random.default_rng(seed) on the host, all-zero rows drawn again."""
    rng = np.random.default_rng(seed)
    dirs = rng.integers(-1, 2, size=(int(P), int(D)), dtype=np.int8)
    while True:
        zero = np.flatnonzero(~dirs.any(1))
        if len(zero) == 0:
            return dirs
        dirs[zero] = rng.integers(-1, 2, size=(len(zero), int(D)), dtype=np.int8)


def swd_score(num, Na, Nb, dirs):
    """Sliced Wasserstein distance from the integer numerators of ops.hist_w1: the mean over directions of
    num[p] / (Na * Nb * 255 * sqrt(nnz_p)), i.e. W1 along the unit vector dirs[p] / sqrt(nnz_p) in units of the full intensity
    range.  Exactly 0.0 when every numerator is 0 (equal patch multisets)."""
    num = [int(v) for v in (num.tolist() if hasattr(num, "tolist") else num)]
    nnz = [int(v) for v in np.count_nonzero(np.asarray(dirs), axis=1)]
    if len(num) != len(nnz) or not num:
        raise ValueError("swd_score: %d numerators for %d directions" % (len(num), len(nnz)))
    scale = int(Na) * int(Nb) * 255
    return sum((n / scale) / math.sqrt(z) for n, z in zip(num, nnz)) / len(num)   # n / scale: Python's correctly rounded int / int


def seam_patches(size, patch, stride, wrap):
    """(flat indices, grid): the patches that cross at least one seam of a (T, H, W) volume that is a ring along the axes flagged
    in wrap = (wt, wh, ww).  The grid is the periodic one at `stride` - every position of a ring axis (stride 1 there), the
    positions 0, s, 2 s, ... <= S - p of another - which is the strided grid of the circularly padded volume; a patch crosses
    the seam of a ring axis iff its coordinate there is > S - p.  Indices: ascending int64 numpy, raster order.  Host only."""
    coords, grid = [], []
    for S, p, s, w in zip(size, patch, stride, wrap):
        if w and int(s) != 1:
            raise ValueError("seam_patches: the stride along a ring axis must be 1, got %s" % (tuple(stride),))
        n = int(S) if w else (int(S) - int(p)) // int(s) + 1
        grid.append(n)
        coords.append(np.arange(n) > int(S) - int(p) if w else np.zeros(n, bool))
    cross = coords[0][:, None, None] | coords[1][None, :, None] | coords[2][None, None, :]
    return np.flatnonzero(cross.reshape(-1)).astype(np.int64), tuple(grid)


def pair_count(grid):
    """E: the pairs of 6-neighbours of a patch grid (gT, gH, gW)."""
    gT, gH, gW = (int(e) for e in grid)
    return (gT - 1) * gH * gW + gT * (gH - 1) * gW + gT * gH * (gW - 1)


def chunk_metrics(stats, Nq, E, kept_frac=False):
    """The per-sample chunk scores from the integers of ops.nnf_chunks, stats = (kept, in_place, coherent_pairs, chunks, largest,
    sum of size^2), each one Python int / int division: nnf_coherence = coherent_pairs / E (None for a grid without pairs),
    chunks, largest_chunk_frac = largest / Nq, chunk_frac = sum_sq / Nq^2 (the expected share of the grid taken up by the chunk
    of a random patch: 1.0 for a rigid copy, about 1 / Nq for an incoherent field), in_place_frac = in_place / Nq; with
    kept_frac also chunk_kept_frac = kept / Nq."""
    kept, in_place, pairs, chunks, largest, sum_sq = (int(v) for v in (stats.tolist() if hasattr(stats, "tolist") else stats))
    Nq, E = int(Nq), int(E)
    m = {"nnf_coherence": pairs / E if E > 0 else None, "chunks": chunks, "largest_chunk_frac": largest / Nq,
         "chunk_frac": sum_sq / (Nq * Nq), "in_place_frac": in_place / Nq}
    if kept_frac:
        m["chunk_kept_frac"] = kept / Nq
    return m


def prdc_check(k, floor=None, Ns=None, Nr=None):
    """Refuse what --prdc cannot score, as the program's exit: --prdc-floor without --prdc, K outside
    [1, ops.PATCH_KNN_MAX_K], a floor < 0 and, once the patch counts are known, a side with no more than K patches (its K-th
    neighbour does not exist).  k == 0 without a floor is "off" and passes."""
    k = int(k or 0)
    if k == 0:
        if floor is not None:
            raise SystemExit("evaluate: --prdc-floor needs --prdc K")
        return
    if not 1 <= k <= ops.PATCH_KNN_MAX_K:
        raise SystemExit("evaluate: --prdc K must be in [1, {}], got {}".format(ops.PATCH_KNN_MAX_K, k))
    if floor is not None and not (float(floor) >= 0.0 and math.isfinite(float(floor))):
        raise SystemExit("evaluate: --prdc-floor must be a finite number >= 0, got {}".format(floor))
    for name, n in (("sample", Ns), ("real volume", Nr)):
        if n is not None and int(n) <= k:
            raise SystemExit("evaluate: --prdc {}: the {} has {} patches, and every patch needs k = {} others".format(k, name, int(n), k))


def prdc_metrics(inside, ball_sum, reached, covered, Ns, Nr, k):
    """The four per-sample scores from integer counts, each one Python int / int division: precision = inside / Ns (sample
    patches inside some real patch's ball), density = ball_sum / (k Ns) (the balls that hold a sample patch, summed),
    recall = reached / Nr (real patches inside some sample patch's ball), coverage = covered / Nr (real patches whose own ball
    holds a sample patch)."""
    inside, ball_sum, reached, covered, Ns, Nr, k = (int(v) for v in (inside, ball_sum, reached, covered, Ns, Nr, k))
    return {"precision": inside / Ns, "recall": reached / Nr, "density": ball_sum / (k * Ns), "coverage": covered / Nr}


def source_colours(nn, ref_grid):
    """uint8 [..., 3] shaped as nn's patch grid: (R, G, B) = the (x, y, t) key coordinate of each patch's nearest neighbour,
    coordinate c of an axis of k positions as the byte (2 * 255 * c + (k - 1)) // (2 * (k - 1)), 0 when k == 1."""
    kT, kH, kW = (int(e) for e in ref_grid)
    j = nn.to(torch.int64).clamp(0, kT * kH * kW - 1)
    coords = ((j % kW, kW), ((j // kW) % kH, kH), (j // (kW * kH), kT))
    return torch.stack([(2 * 255 * c + (k - 1)) // (2 * (k - 1)) if k > 1 else torch.zeros_like(c) for c, k in coords], -1).to(torch.uint8)


def evaluate(exp_dir=None, samples=None, real=None, patch=None, stride=(1, 1, 1), max_samples=None, out=None, swd=0, swd_seed=0,
             chunks=False, chunk_tol=None, save_chunks=False, prdc=0, prdc_floor=None, save_prdc=False, wrap=None, scales=0,
             scale_ratio=None):
    """Score `samples` against the real volume; writes metrics.json (and, with exp_dir, the real volume used as real.npy) into
    `out` and returns the metrics.  swd > 0: also the sliced Wasserstein patch distance over that many directions.
    chunks (implied by chunk_tol / save_chunks): also the copied-region statistics of the coherence direction's field.
    prdc = k > 0: also precision / recall / density / coverage of the patch sets (prdc_floor is refused without it, save_prdc
    does nothing without it).  wrap: the --wrap string (letters of t, h, w): the samples are rings along those axes, and every
    sample also gets seam_patches (the patches of its periodic grid, at `stride`, that cross a seam) and seam_coherence (the
    mean over those of the exact nearest distance to the real volume's dense patches, over D * 255^2; None without such
    patches), searched on the circularly padded sample with ops.patch_nn_subset.
    scales = K > 0 (scale_ratio, default 0.5, is refused without it): for k = 1..K every sample and the real volume are resized
    from their own full sizes by ops.volume_resize_u8 to scale_sizes() and coherence / completeness are computed there with the
    same patch and stride; every per_sample entry gains `scales` (a list of scale, size, coherence, completeness) and the
    metrics `scales` (the means and Nq / Nr per scale), scale_ratio and scales_seconds."""
    scales = int(scales or 0)
    scale_ratio = scales_check(scales, scale_ratio)
    rings = None
    if wrap is not None:
        try:
            rings = parse_wrap_axes(wrap)
        except SystemExit as e:
            raise SystemExit("evaluate: {}".format(e))
        if any(w and int(s) != 1 for w, s in zip(rings, stride)):
            raise SystemExit("evaluate: --wrap {}: --stride must be 1 along a ring axis, got {}".format(wrap, list(stride)))
    prdc_check(prdc, prdc_floor)
    prdc = int(prdc or 0)
    if exp_dir is None and (samples is None or real is None):
        raise SystemExit("evaluate: give --exp-dir, or both --samples and --real")
    spath = samples or os.path.join(exp_dir, 'eval', 'samples', 'samples.npy')
    if not os.path.isfile(spath):
        raise SystemExit("evaluate: no samples at {}; run `python -m hp_vae_gan_amd.generate --exp-dir {}` first "
                         "(or pass --samples)".format(spath, exp_dir or '<experiment>'))
    device = gpu_device()
    arr = np.load(spath, allow_pickle=False)
    if arr.dtype != np.uint8 or arr.ndim not in (4, 5) or arr.shape[-1] != 3:
        raise SystemExit("evaluate: samples must be uint8 [N,T,H,W,3] or [N,H,W,3], got {} {}".format(arr.dtype, arr.shape))
    if max_samples:
        arr = arr[:max_samples]
    video = arr.ndim == 5
    if rings is not None and rings[0] and not video:
        raise SystemExit("evaluate: --wrap t needs clips: an image has no time axis")
    out = out or os.path.dirname(os.path.abspath(spath))
    os.makedirs(out, exist_ok=True)
    if exp_dir is not None:
        opt = load_opt(exp_dir)
        if (opt.dims == 3) != video:
            raise SystemExit("evaluate: the samples' rank does not match the experiment ({}-D)".format(opt.dims))
        real_dev = real_volume(opt, real, device)
        np.save(os.path.join(out, 'real.npy'), real_dev.cpu().numpy())
    else:
        real_dev = load_u8_frames(real, device, not video, "evaluate: --real must be uint8 [...,3]")
        if real_dev.dim() != arr.ndim - 1:
            raise SystemExit("evaluate: --real {} does not match samples {}".format(tuple(real_dev.shape), arr.shape))
    patch = tuple(patch) if patch else default_patch(video)
    stride = tuple(stride)
    samples_dev = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    vol = (lambda t: tuple(t.shape[:3])) if video else (lambda t: (1,) + tuple(t.shape[:2]))
    coh_counts = ops.patch_nn_counts(vol(samples_dev[0]), vol(real_dev), patch, qstride=stride)
    com_counts = ops.patch_nn_counts(vol(real_dev), vol(samples_dev[0]), patch, qstride=stride)
    D = coh_counts[2]
    if scales:
        scales_check(scales, scale_ratio, (vol(samples_dev[0]), vol(real_dev)), patch)
        as_vol = (lambda t: t) if video else (lambda t: t[None])
        ssizes, rsizes = scale_sizes(vol(samples_dev[0]), scales, scale_ratio), scale_sizes(vol(real_dev), scales, scale_ratio)
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0.record()
        real_scaled = [ops.volume_resize_u8(as_vol(real_dev), s) for s in rsizes]
        k1.record()
        k1.synchronize()
        scales_seconds = k0.elapsed_time(k1) / 1e3
        scale_counts = [ops.patch_nn_counts(s, r, patch, qstride=stride) for s, r in zip(ssizes, rsizes)]
    chunks = bool(chunks or chunk_tol is not None or save_chunks)
    if chunks:
        ref_grid = tuple(v - p + 1 for v, p in zip(vol(real_dev), patch))   # the real side is dense
        max_d2 = None if chunk_tol is None else min(int(math.floor(float(chunk_tol) * (D * 255 * 255))), 2 ** 31 - 1)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        chunk_seconds, saved = 0.0, []
    if prdc:
        # S: the sample's patches on the strided grid, R: the real volume's on the dense grid (as for --swd)
        Ns, Nr = coh_counts[0], coh_counts[1]
        prdc_check(prdc, prdc_floor, Ns, Nr)
        one = (1, 1, 1)
        grid3 = lambda t, st: tuple((v - p) // s + 1 for v, p, s in zip(vol(t), patch, st))   # noqa: E731
        floor_d2 = None if prdc_floor is None else min(int(math.floor(float(prdc_floor) * (D * 255 * 255))), 2 ** 31 - 1)
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p0.record()
        rad_real = ops.patch_knn_self(real_dev, patch, prdc)[..., prdc - 1]
        zero_radius = int((rad_real == 0).sum())
        rad_real = (rad_real if floor_d2 is None else rad_real.clamp(min=floor_d2)).contiguous()
        p1.record()
        p1.synchronize()
        prdc_seconds, prdc_saved = p0.elapsed_time(p1) / 1e3, []
    if rings is not None:
        seam_idx, _ = seam_patches(vol(samples_dev[0]), patch, stride, rings)
        seam_sel = torch.from_numpy(seam_idx).to(device=device, dtype=torch.int32)
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        seam_seconds = 0.0
    per_sample = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    seconds = 0.0
    for smp in samples_dev:
        e0.record()
        d2c, nnc = ops.patch_nn(smp, real_dev, patch, qstride=stride)
        d2r, _ = ops.patch_nn(real_dev, smp, patch, qstride=stride)
        e1.record()
        e1.synchronize()
        seconds += e0.elapsed_time(e1) / 1e3
        per_sample.append({"coherence": patch_score(d2c, D), "completeness": patch_score(d2r, D),
                           "nn_unique_frac": nn_unique_frac(nnc, coh_counts[1])})
        if rings is not None:
            per_sample[-1].update({"seam_patches": int(seam_sel.numel()), "seam_coherence": None})
            if seam_sel.numel():
                s0.record()
                d2s, _ = ops.patch_nn_subset(patchnn_wrap_pad(smp, patch, rings), real_dev, patch, seam_sel, None, qstride=stride)
                d2s = d2s.reshape(-1)[seam_sel.long()]
                s1.record()
                s1.synchronize()
                seam_seconds += s0.elapsed_time(s1) / 1e3
                per_sample[-1]["seam_coherence"] = patch_score(d2s, D)
        if scales:
            k0.record()
            rows = []
            for k, (ss, rk) in enumerate(zip(ssizes, real_scaled)):
                sk = ops.volume_resize_u8(as_vol(smp), ss)
                rows.append((k + 1, ss, ops.patch_nn(sk, rk, patch, qstride=stride)[0], ops.patch_nn(rk, sk, patch, qstride=stride)[0]))
            k1.record()
            k1.synchronize()
            scales_seconds += k0.elapsed_time(k1) / 1e3
            per_sample[-1]["scales"] = [{"scale": k, "size": list(ss if video else ss[1:]), "coherence": patch_score(dc, D),
                                         "completeness": patch_score(dr, D)} for k, ss, dc, dr in rows]
        if chunks:
            c0.record()
            labels, sizes, stats = ops.nnf_chunks(nnc, ref_grid, qstride=stride, d2=None if max_d2 is None else d2c, max_d2=max_d2)
            c1.record()
            c1.synchronize()
            chunk_seconds += c0.elapsed_time(c1) / 1e3
            grid = tuple(nnc.shape) if video else (1,) + tuple(nnc.shape)
            per_sample[-1].update(chunk_metrics(stats.cpu(), coh_counts[0], pair_count(grid), max_d2 is not None))
            if save_chunks:
                saved.append((labels.cpu().numpy().reshape(grid), sizes.cpu().numpy().reshape(grid), nnc.cpu().numpy().reshape(grid),
                              source_colours(nnc, ref_grid).cpu().numpy()))
        if prdc:
            p0.record()
            rad_smp = ops.patch_knn_self(smp, patch, prdc, stride)[..., prdc - 1]
            rad_smp = (rad_smp if floor_d2 is None else rad_smp.clamp(min=floor_d2)).contiguous()
            count = ops.patch_ball_count(smp, real_dev, rad_real, patch, qstride=stride)     # balls of R that hold s_i
            reach = ops.patch_ball_count(real_dev, smp, rad_smp, patch, rstride=stride)      # balls of S that hold r_j
            # min_i d2(r_j, s_i) over the strided sample grid; at stride 1 1 1 that is the completeness search
            near = d2r if stride == one else ops.patch_nn(real_dev, smp, patch, rstride=stride)[0]
            covered = near <= rad_real
            ints = torch.stack([(count > 0).sum(), count.sum(dtype=torch.int64), (reach > 0).sum(), covered.sum()])
            p1.record()
            p1.synchronize()
            prdc_seconds += p0.elapsed_time(p1) / 1e3
            per_sample[-1].update(prdc_metrics(*ints.tolist(), Ns, Nr, prdc))
            if save_prdc:
                prdc_saved.append((count.cpu().numpy().reshape(grid3(smp, stride)), covered.cpu().numpy()))
    n = len(per_sample)
    metrics = {"samples": os.path.abspath(spath), "num_samples": n, "patch": list(patch), "stride": list(stride),
               "Nq": coh_counts[0], "Nr": coh_counts[1], "D": D, "Nq_completeness": com_counts[0], "Nr_completeness": com_counts[1],
               "per_sample": per_sample, "patchnn_seconds": seconds, "diversity": diversity(samples_dev, real_dev)}
    for k in ("coherence", "completeness", "nn_unique_frac"):
        metrics[k] = sum(p[k] for p in per_sample) / n
    swd_text = ""
    if swd and swd > 0:
        # the sample side carries the stride, the real side stays dense (as for coherence); its histograms are made once
        dirs = swd_directions(swd, D, swd_seed)
        dirs_dev = torch.from_numpy(dirs).to(device)
        Ns, Nr = coh_counts[0], coh_counts[1]
        e0.record()
        hist_real = ops.patch_proj_hist(real_dev, patch, dirs_dev)
        nums = [ops.hist_w1(ops.patch_proj_hist(smp, patch, dirs_dev, stride), Ns, hist_real, Nr) for smp in samples_dev]
        e1.record()
        e1.synchronize()
        for p, num in zip(per_sample, nums):
            p["swd"] = swd_score(num.cpu(), Ns, Nr, dirs)
        metrics.update({"swd": sum(p["swd"] for p in per_sample) / n, "swd_directions": int(swd), "swd_seed": int(swd_seed),
                        "swd_seconds": e0.elapsed_time(e1) / 1e3})
        swd_text = " swd {:.6f}".format(metrics["swd"])
    chunk_text = ""
    if chunks:
        for k in ("nnf_coherence", "chunks", "largest_chunk_frac", "chunk_frac", "in_place_frac") + \
                (("chunk_kept_frac",) if max_d2 is not None else ()):
            vals = [p[k] for p in per_sample]
            metrics[k] = None if any(v is None for v in vals) else sum(vals) / n
        metrics.update({"chunk_tol": None if chunk_tol is None else float(chunk_tol), "chunk_seconds": chunk_seconds})
        chunk_text = " chunk_frac {:.6f} nnf_coherence {}".format(
            metrics["chunk_frac"], "n/a" if metrics["nnf_coherence"] is None else "{:.6f}".format(metrics["nnf_coherence"]))
        if save_chunks:
            np.savez(os.path.join(out, 'chunks.npz'), labels=np.stack([s[0] for s in saved]), sizes=np.stack([s[1] for s in saved]),
                     nn=np.stack([s[2] for s in saved]))
            for i, s in enumerate(saved):
                write_frames(s[3], os.path.join(out, 'source_{:04d}{}'.format(i, '.gif' if video else '.png')), 10)
    prdc_text = ""
    if prdc:
        for k in ("precision", "recall", "density", "coverage"):
            metrics[k] = sum(p[k] for p in per_sample) / n
        metrics.update({"prdc_k": prdc, "prdc_floor": None if prdc_floor is None else float(prdc_floor),
                        "prdc_zero_radius_frac": zero_radius / Nr, "prdc_seconds": prdc_seconds})
        prdc_text = " precision {:.6f} recall {:.6f} density {:.6f} coverage {:.6f}".format(
            metrics["precision"], metrics["recall"], metrics["density"], metrics["coverage"])
        if save_prdc:
            rgrid = grid3(real_dev, one)
            np.savez(os.path.join(out, 'prdc.npz'), count=np.stack([s[0] for s in prdc_saved]),
                     real_radius=rad_real.cpu().numpy().reshape(rgrid),
                     real_covered=np.stack([s[1].reshape(rgrid) for s in prdc_saved]))
    seam_text = ""
    if rings is not None:
        vals = [p["seam_coherence"] for p in per_sample]
        metrics.update({"seam_coherence": None if any(v is None for v in vals) else sum(vals) / n, "wrap": wrap,
                        "seam_seconds": seam_seconds})
        seam_text = " seam_coherence {}".format("n/a" if metrics["seam_coherence"] is None else "{:.6f}".format(metrics["seam_coherence"]))
    scales_text = ""
    if scales:
        metrics["scales"] = [{"scale": k + 1, "size": list(ssizes[k] if video else ssizes[k][1:]),
                              "real_size": list(rsizes[k] if video else rsizes[k][1:]),
                              "coherence": sum(p["scales"][k]["coherence"] for p in per_sample) / n,
                              "completeness": sum(p["scales"][k]["completeness"] for p in per_sample) / n,
                              "Nq": scale_counts[k][0], "Nr": scale_counts[k][1]} for k in range(scales)]
        metrics.update({"scale_ratio": scale_ratio, "scales_seconds": scales_seconds})
        scales_text = "".join(" coherence@{} {:.6f}".format(s["scale"], s["coherence"]) for s in metrics["scales"])
    with open(os.path.join(out, 'metrics.json'), 'w') as f:
        json.dump(metrics, f, indent=1, sort_keys=True)
    print("evaluate: {} samples, patch {} stride {}: coherence {:.6f} completeness {:.6f} nn_unique_frac {:.4f} diversity {}{}{}{}{}{} "
          "({:.3f} s in patch_nn) -> {}".format(n, list(patch), list(stride), metrics["coherence"], metrics["completeness"],
                                               metrics["nn_unique_frac"],
                                               "n/a" if metrics["diversity"] is None else "{:.4f}".format(metrics["diversity"]),
                                               swd_text, chunk_text, prdc_text, seam_text, scales_text, seconds, os.path.join(out, 'metrics.json')))
    return metrics


def main(argv=None):
    a = evaluate_parser().parse_args(argv)
    evaluate(a.exp_dir, a.samples, a.real, a.patch, a.stride, a.max_samples, a.out, a.swd, a.swd_seed, a.chunks, a.chunk_tol,
             a.save_chunks, a.prdc, a.prdc_floor, a.save_prdc, a.wrap, a.scales, a.scale_ratio)
    return 0


if __name__ == "__main__":
    sys.exit(main())
