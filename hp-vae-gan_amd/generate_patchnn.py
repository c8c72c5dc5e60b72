"""`python -m hp_vae_gan_amd.generate_patchnn --exp-dir run/<clip>/<checkname>/experiment_<n>` (or `--video-path clip.npy --out
dir`, `--image-path img.png --out dir`): training-free samples of the clip by coarse-to-fine patch nearest neighbours (GPNN /
VGPNN); writes samples.npy, one GIF / PNG per sample and patchnn.json.  With `--mask hole.npy` the samples are completions of
the masked region of the clip (patch inpainting) and every other voxel stays as it is.  With `--search patchmatch` the levels
above the coarsest search by a deterministic PatchMatch (linear in the patch count) instead of exhaustively.  With `--wrap AXES`
(letters of t, h, w) the samples are rings along those axes: `--wrap t` makes clips whose last frame continues into the first
(seamless loops), `--wrap hw` tileable textures.  With `--antialias` every resize of the run is the exact antialiased integer
resize (ops.volume_resize_u8: the coarse levels are low-passed, not subsampled), and with `--t-ratio R` the pyramid also
scales T (a spatio-temporal pyramid).  With `--guide PATH --guide-level N` every sample starts from the given volume at pyramid
level N instead of from noise (structural analogies, sketch-to-video, editing), and with `--guide-mask hole.npy` it is kept only
inside the feathered hole (ops.mask_blend)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import ops
from . import utils as hp_utils
from . import datasets
from .programs import (add_guide_flags, check_guide_flags, default_patch, gpu_device, load_guide_frames, load_opt, load_u8_frames,
                       mask_forms, parse_wrap_axes, patchnn_wrap_pad, pick_mask, real_volume,
                       refuse_trivial_mask as _refuse_trivial_mask, wrap_triple as _wrap3, write_samples)


# The training-free counterpart of the trained generator: GPNN (Granot et al., "Drop the GAN", CVPR 2022) and its video form
# VGPNN (Haim et al., ECCV 2022) on the exact patch engine of `evaluate`.  Everything is a uint8 volume [T,H,W,3]; an image is
# the volume with T = 1.  Coarse to fine over a pyramid of the real volume (spatial by default: T is kept; --t-ratio scales T
# too, VGPNN's spatio-temporal pyramid), every level repeats one step: search, for each patch of the current guess, the key
# patch that minimises d2 / (alpha_abs + the key's distance to ITS nearest guess patch) (the completeness normalisation: key
# patches the guess does not use yet become cheap), then vote the value patches of the winners into the next guess.
PM_ITERS = 4        # --pm-iters: a warm-started search at the finest level is within 1.05 of the exact mean d2 after 4
PM_FROM_LEVEL = 1   # --pm-from-level
PM_SEED_STRIDE = 1000003


def generate_patchnn_parser():
    def alpha(s):
        v = float(s)
        if not v > 0:
            raise argparse.ArgumentTypeError("--alpha must be > 0 (inf: no completeness normalisation)")
        return v
    p = argparse.ArgumentParser(prog="python -m hp_vae_gan_amd.generate_patchnn",
                                description="Training-free samples of one clip / image by coarse-to-fine patch nearest "
                                "neighbours (GPNN / VGPNN) on the exact patch engine of `evaluate`.")
    p.add_argument('--exp-dir', default=None, help='experiment_<n> directory: the real volume is the one `evaluate` compares against')
    p.add_argument('--video-path', default=None, help='a clip taken as it is (.npy [N,H,W,3] uint8 or a frame directory); needs --out')
    p.add_argument('--image-path', default=None, help='an image taken as it is (.npy [H,W,3] uint8 or an image file); needs --out')
    p.add_argument('--out', default=None, help='output directory (default: <exp-dir>/eval/samples_patchnn)')
    p.add_argument('--num-samples', type=int, default=8, help='number of samples')
    p.add_argument('--seed', type=int, default=0, help='sample i draws its noise under seed + i')
    p.add_argument('--patch', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='patch (default 3 7 7, images 1 7 7)')
    p.add_argument('--ratio', type=float, default=0.75, help='size ratio between two levels of the pyramid')
    p.add_argument('--min-size', type=int, default=16, help='the coarsest level keeps min(H, W) >= this')
    p.add_argument('--iters', type=int, default=10, help='refine steps per level')
    p.add_argument('--alpha', type=alpha, default=0.005, help='completeness normalisation, in units of D * 255^2 (the unit of '
                   '`evaluate`\'s coherence); inf turns it off')
    p.add_argument('--noise', type=float, default=0.75, help='standard deviation, in units of 255, of the noise added to the coarsest guess')
    p.add_argument('--size', type=int, nargs=3, default=None, metavar=('T', 'H', 'W'), help='size of the samples (default: the real '
                   'volume\'s; another size retargets)')
    p.add_argument('--save-levels', action='store_true', help='also write levels.npz: the real pyramid (level_<l>) and the blurred '
                   'keys of every level above the coarsest (keys_<l>)')
    p.add_argument('--mask', default=None, help='fill a hole instead of sampling the whole volume: a mask of the real volume\'s '
                   '(T, H, W) (.npy [T,H,W] / [H,W] bool or uint8, or [...,3], an image file or a frame directory; nonzero = hole). '
                   'Only patches that overlap the hole are searched, only patches that avoid it answer, and voxels outside the '
                   'hole are kept; the search is the plain nearest neighbour (--alpha is not used)')
    p.add_argument('--search', choices=('exact', 'patchmatch'), default='exact', help='exact: every step searches all keys '
                   '(quadratic in the patch count); patchmatch: from --pm-from-level on, the deterministic PatchMatch '
                   '(linear in the patch count), started from the previous step\'s field')
    p.add_argument('--pm-iters', type=int, default=None, help='PatchMatch iterations per search (default %d); only with '
                   '--search patchmatch' % PM_ITERS)
    p.add_argument('--pm-from-level', type=int, default=None, help='first pyramid level searched by PatchMatch, >= 1 (default %d; '
                   'level 0 is always exact); only with --search patchmatch' % PM_FROM_LEVEL)
    p.add_argument('--wrap', default=None, metavar='AXES', help='make the samples rings along these axes: distinct letters of t, h, w '
                   '(t: a clip that loops without a seam; hw: a texture that tiles).  The patches that cross a seam are searched '
                   'and voted like any others; the real clip stays as it is.  Not with --mask; no t for an image')
    p.add_argument('--antialias', action='store_true', help='every resize of the run (real levels, blurred keys, the guess '
                   'between levels, the coarsest guess under --size, the resize of --mask) is the exact antialiased integer resize: '
                   'a coarse voxel averages everything it stands for under a triangle filter; upsizing stays linear interpolation')
    p.add_argument('--t-ratio', type=float, default=1.0, metavar='R', help='also scale T between two levels of the pyramid: the level '
                   'k steps below the finest has min(T, max(F, round(T R^k))) frames, F = --min-frames; R in (0, 1], 1.0 keeps T.  '
                   'Not for an image, and not with --mask (the mask resize keeps T)')
    p.add_argument('--min-frames', type=int, default=None, metavar='F', help='no level of a --t-ratio pyramid has fewer frames '
                   '(default: patch T + 1; at least patch T); only with --t-ratio below 1')
    add_guide_flags(p)
    p.add_argument('--guide-noise', type=float, default=None, metavar='S', help='standard deviation, in units of 255, of the noise '
                   'added to the guide at --guide-level (default 0; --noise is not used in a guided run); only with --guide')
    return p


def patchnn_wrap_grid(size, patch, wrap):
    """The sides of the periodic patch grid of a (T, H, W) volume: the whole side on a ring axis, S - p + 1 elsewhere."""
    w = _wrap3(wrap) or (0, 0, 0)
    return tuple(int(s) if f else int(s) - int(p) + 1 for s, p, f in zip(size, patch, w))


def patchnn_level_frames(T, k, t_ratio=1.0, min_frames=None, patch_t=3):
    """Frames of the level k steps below the finest of a T-frame volume: min(T, max(F, floor(T t_ratio^k + 0.5))) with
    F = min_frames (default patch_t + 1); T itself for t_ratio == 1.0.  Refuses t_ratio outside (0, 1], min_frames < patch_t and
    min_frames with t_ratio == 1.0.  Host only."""
    T, t_ratio = int(T), float(t_ratio)
    if not 0.0 < t_ratio <= 1.0:
        raise ValueError("patchnn_pyramid_sizes: t_ratio must lie in (0, 1], got %r" % (t_ratio,))
    if t_ratio == 1.0:
        if min_frames is not None:
            raise ValueError("patchnn_pyramid_sizes: min_frames needs a t_ratio below 1")
        return T
    F = int(patch_t) + 1 if min_frames is None else int(min_frames)
    if F < int(patch_t):
        raise ValueError("patchnn_pyramid_sizes: min_frames must be at least the patch's T = %d, got %d" % (int(patch_t), F))
    return min(T, max(F, int(math.floor(T * t_ratio ** k + 0.5))))


def patchnn_pyramid_sizes(shape, ratio, min_size, patch=(3, 7, 7), t_ratio=1.0, min_frames=None):
    """[(T, H, W)] of the pyramid of a (T, H, W) volume from coarse to fine: level l of L has (H, W) scaled by ratio^(L-1-l) and
    rounded (halves up), the finest is the volume itself and T is kept.  L is the largest count whose coarsest level has
    min(H, W) >= min_size (at least 1).  Refuses a coarsest level smaller than the patch.  Host only.
    t_ratio < 1 (a spatio-temporal pyramid): the level k = L-1-l steps below the finest has patchnn_level_frames(T, k, t_ratio,
    min_frames, patch T) frames; L is still decided by the spatial sides.  t_ratio == 1.0: exactly the sizes above."""
    T, H, W = (int(e) for e in shape)
    ratio = float(ratio)
    if not 0.0 < ratio < 1.0:
        raise ValueError("patchnn_pyramid_sizes: ratio must lie in (0, 1), got %r" % (ratio,))
    if min(T, H, W) < 1:
        raise ValueError("patchnn_pyramid_sizes: bad volume %s" % ((T, H, W),))

    patchnn_level_frames(T, 0, t_ratio, min_frames, patch[0])   # the refusals, whatever L turns out to be

    def at(k):
        return (patchnn_level_frames(T, k, t_ratio, min_frames, patch[0]), int(math.floor(H * ratio ** k + 0.5)),
                int(math.floor(W * ratio ** k + 0.5)))
    L = 1
    while min(at(L)[1:]) >= max(int(min_size), 1):
        L += 1
    sizes = [at(L - 1 - l) for l in range(L)]
    if any(s < p for s, p in zip(sizes[0], patch)):
        raise ValueError("patchnn_pyramid_sizes: the coarsest level %s is smaller than the patch %s (raise min_size)"
                         % (sizes[0], tuple(patch)))
    return sizes


def _resize_u8(vol, size, antialias=False):
    """uint8 [T,H,W,3] -> uint8 [*size, 3]: the trilinear align-corners resize (ops.UpsampleAC, fp32), rounded and clamped.
    antialias: the exact antialiased integer resize instead (ops.volume_resize_u8, one launch)."""
    size = tuple(int(e) for e in size)
    if tuple(vol.shape[:3]) == size:
        return vol.contiguous()
    if antialias:
        return ops.volume_resize_u8(vol, size)
    x = vol.permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()
    with torch.no_grad():
        y = ops.UpsampleAC.apply(x, size, None, 0.0)
    return torch.round(y).clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 3, 0).contiguous()


def patchnn_real_levels(real, sizes, antialias=False):
    """(levels, keys) of the real volume [T,H,W,3]: levels[l] is the full-size volume resized to sizes[l]; keys[l] (l > 0) is
    levels[l-1] resized to sizes[l], the blurred keys of the first step of level l (keys[0] is levels[0]).  antialias: both by
    the exact antialiased resize (_resize_u8)."""
    levels = [_resize_u8(real, s, antialias) for s in sizes]
    keys = [levels[0]] + [_resize_u8(levels[l - 1], sizes[l], antialias) for l in range(1, len(sizes))]
    return levels, keys


def patchnn_weights(m, alpha_abs):
    """w = 1 / (float32(m) + float32(alpha_abs)) for the int32 distances m: one fp32 add and one correctly rounded fp32 divide
    per key patch (the generator's results are defined bit for bit, so this must equal numpy's float32 arithmetic)."""
    return 1.0 / (m.to(torch.float32) + torch.tensor(alpha_abs, dtype=torch.float32, device=m.device))


def patchnn_field_resize(nn, qgrid_from, rgrid_from, qgrid_to, rgrid_to):
    """A nearest-neighbour field carried to another pair of dense patch grids, in integer arithmetic (torch, any device).  nn: an
    integer tensor with prod(qgrid_from) entries, indices into the key grid rgrid_from (clamped into it).  Per axis, target
    query coordinate a (grid side Gt) reads the source (side Gf) at (2 a (Gf - 1) + (Gt - 1)) // (2 (Gt - 1)) - the nearest
    source coordinate under the align-corners map, halves up; 0 when Gt = 1 - and the key coordinate b' found there (side Kf)
    becomes (2 b' (Kt - 1) + (Kf - 1)) // (2 (Kf - 1)) in the target key grid (side Kt; 0 when Kf = 1).  Returns int32 shaped
    qgrid_to."""
    qf, rf, qt, rt = (tuple(int(e) for e in g) for g in (qgrid_from, rgrid_from, qgrid_to, rgrid_to))
    if any(len(g) != 3 or min(g) < 1 for g in (qf, rf, qt, rt)) or nn.numel() != qf[0] * qf[1] * qf[2]:
        raise ValueError("patchnn_field_resize: grids of 3 sides >= 1 and a field of prod(qgrid_from) entries, got %s %s %s %s, %d"
                         % (qf, rf, qt, rt, nn.numel()))
    dev = nn.device
    src = nn.reshape(qf).to(torch.int64).clamp(0, rf[0] * rf[1] * rf[2] - 1)
    for axis in range(3):
        a = torch.arange(qt[axis], dtype=torch.int64, device=dev)
        idx = (2 * a * (qf[axis] - 1) + (qt[axis] - 1)) // (2 * (qt[axis] - 1)) if qt[axis] > 1 else torch.zeros_like(a)
        src = src.index_select(axis, idx)
    b = [src // (rf[1] * rf[2]), (src // rf[2]) % rf[1], src % rf[2]]
    for axis in range(3):
        b[axis] = (2 * b[axis] * (rt[axis] - 1) + (rf[axis] - 1)) // (2 * (rf[axis] - 1)) if rf[axis] > 1 else torch.zeros_like(b[axis])
    return ((b[0] * rt[1] + b[1]) * rt[2] + b[2]).to(torch.int32).contiguous()


def patchnn_search_state(seed=0, index=0):
    """What the PatchMatch steps of one sample carry from step to step: `fwd` (guess -> keys) and `rev` (keys -> guess), the
    kept int32 fields (None: not known yet, the search starts from the hash), and the seed rule: PatchMatch search number n of
    the sample (0-based, in launch order: a step's reverse search comes before its forward search) runs under the seed
    (seed + index) * 1000003 + n."""
    return {"fwd": None, "rev": None, "base": (int(seed) + int(index)) * PM_SEED_STRIDE, "count": 0}


def _next_seed(state):
    s = state["base"] + state["count"]
    state["count"] += 1
    return s


def patchnn_refine(query, keys, values, patch, alpha_abs, return_score=False, search='exact', pm_iters=PM_ITERS,
                   pm_from_level=PM_FROM_LEVEL, level=None, state=None, wrap=None):
    """One GPNN step on uint8 volumes (or images): m = for every key patch the distance to its nearest query patch,
    w = 1 / (float32(m) + float32(alpha_abs)), nn = the weighted nearest key of every query patch, result = the vote of the
    value patches nn (keys and values share one grid) with the query as fallback.  alpha_abs = inf: the plain nearest key,
    one search.  return_score: also the mean of the minimised quantity (d2 * w; d2 for inf).
    search = 'patchmatch' (and level None or >= max(pm_from_level, 1); below that the step is the exact one): both searches are
    ops.patch_match with pm_iters iterations - m is the d2 of patch_match(keys, query) started from state['rev'], the forward
    search is patch_match(query, keys, ref_weight=w) started from state['fwd'] - each under its own seed
    (patchnn_search_state).  state: that dict, updated in place with the fields of this step's searches, exact ones included
    (None: a fresh one, i.e. hash starts under seeds 0 and 1).
    wrap = (wt, wh, ww): the query (the guess) is a ring along the flagged axes.  Both searches then run on the circularly padded
    query (patchnn_wrap_pad), whose dense grid is the query's periodic grid - PatchMatch with that grid's ring flags on the
    query's side - and the vote goes onto the ring (ops.patch_vote(..., wrap)), into the query's own size.  The fields in
    `state` live on the periodic grid.  Keys and values are never rings.  None: the step it always was."""
    wrap = _wrap3(wrap)
    padded = query if wrap is None else patchnn_wrap_pad(query, patch, wrap)
    if search not in ("exact", "patchmatch"):
        raise ValueError("patchnn_refine: search must be 'exact' or 'patchmatch', got %r" % (search,))
    pm = search == "patchmatch" and (level is None or int(level) >= max(int(pm_from_level), 1))
    if pm and state is None:
        state = patchnn_search_state()
    rev = None
    if pm:
        if math.isinf(alpha_abs):
            score, nn = ops.patch_match(padded, keys, patch, pm_iters, _next_seed(state), None, state["fwd"], qwrap=wrap)
        else:
            m, rev = ops.patch_match(keys, padded, patch, pm_iters, _next_seed(state), None, state["rev"], rwrap=wrap)
            score, nn = ops.patch_match(padded, keys, patch, pm_iters, _next_seed(state), patchnn_weights(m, alpha_abs), state["fwd"],
                                        qwrap=wrap)
    elif math.isinf(alpha_abs):
        score, nn = ops.patch_nn(padded, keys, patch)
    else:
        m, rev = ops.patch_nn(keys, padded, patch)
        score, nn = ops.patch_nn_weighted(padded, keys, patchnn_weights(m, alpha_abs), patch)
    if state is not None:
        state["fwd"], state["rev"] = nn, rev
    if wrap is None:
        out = ops.patch_vote(values, nn, patch, tuple(query.shape[:-1]), query)
    else:
        out = ops.patch_vote(values, nn, patch, tuple(query.shape[:-1]), query, wrap=wrap)
    if return_score:
        return out, float(score.to(torch.float64).mean())
    return out


def patchnn_sample_sizes(sizes, real_shape, size, patch, ratio=0.75, t_ratio=1.0, min_frames=None, start=0):
    """The (T, H, W) of every level of a sample of (T, H, W) = size beside the real pyramid `sizes` of a volume of real_shape:
    `sizes` itself for size None or the real shape, else per level the sample's sides scaled as patchnn_pyramid_sizes scales the
    real ones.  Refuses (ValueError) a sample whose coarsest used level `start` is smaller than the patch.  Host only."""
    L = len(sizes)
    if size is None or tuple(size) == tuple(real_shape):
        return sizes
    St, Sh, Sw = (int(e) for e in size)
    qsizes = [(patchnn_level_frames(St, L - 1 - l, t_ratio, min_frames, patch[0]),
               int(math.floor(Sh * ratio ** (L - 1 - l) + 0.5)), int(math.floor(Sw * ratio ** (L - 1 - l) + 0.5)))
              for l in range(L)]
    if any(s < p for s, p in zip(qsizes[start], patch)):
        raise ValueError("patchnn_synthesize: the sample's coarsest level %s is smaller than the patch %s" % (qsizes[start], tuple(patch)))
    return qsizes


def patchnn_synthesize(real, size=None, patch=None, ratio=0.75, min_size=16, iters=10, noise=0.75, alpha=0.005, seed=0, index=0,
                       pyramid=None, search='exact', pm_iters=PM_ITERS, pm_from_level=PM_FROM_LEVEL, wrap=None, antialias=False,
                       t_ratio=1.0, min_frames=None, guide=None, guide_level=None, guide_noise=0.0):
    """One sample of the uint8 device volume `real` ([T,H,W,3]; images [H,W,3]) -> (sample, mean final score).  size: the
    sample's (T, H, W) (default real's).  The coarsest guess is real level 0 (resized to the sample's coarsest size) plus
    noise * 255 * N(0, 1) drawn under torch.manual_seed(seed + index); level 0 runs `iters` steps with keys = values = real
    level 0; level l > 0 starts from the previous result resized, runs one step with the blurred keys (real level l-1 resized
    to level l) and values real level l, then iters - 1 steps with keys = values = real level l.  pyramid: a
    (sizes, levels, keys) triple of patchnn_pyramid_sizes / patchnn_real_levels to reuse between samples.
    search = 'patchmatch': the steps of level max(pm_from_level, 1) and above search by PatchMatch (patchnn_refine) with
    pm_iters iterations, each started from the previous step's fields; between levels both fields go through
    patchnn_field_resize (the guess's and the keys' grids may differ: retargeting).  Seeds: patchnn_search_state(seed, index).
    The default 'exact' computes what it always did.
    wrap = (wt, wh, ww): the sample is a ring along the flagged axes - every step is patchnn_refine(..., wrap=wrap) and the
    PatchMatch fields live on the guess's periodic grids.  The resize between levels and the coarsest noise stay as they are
    (not periodic): the steps that follow re-vote every voxel.
    antialias: every resize (real levels, blurred keys, coarsest guess, the guess between levels) is ops.volume_resize_u8.
    t_ratio / min_frames: the pyramid scales T as well (patchnn_pyramid_sizes); a sample of another size scales its own T by the
    same rule.  A given `pyramid` must have been made with the same three settings.
    guide (a uint8 device volume [T,H,W,3]; images [H,W,3]) with guide_level = N in 0 .. L - 1: the sample starts from the guide
    instead of from noise.  The guide's (T, H, W) is the sample's size (a `size` that differs is refused); the levels below N are
    skipped; the guess at level N is the guide resized to the sample's level-N size plus guide_noise * 255 * N(0, 1), drawn under
    seed + index as the coarsest noise is (`noise` is not used); level N is this run's coarsest level - `iters` steps with
    keys = values = real level N, always exact - and PatchMatch starts at max(pm_from_level, N + 1); the finer levels run as
    they always do.  guide None: the function it always was."""
    wrap = _wrap3(wrap)
    image = real.dim() == 3
    vol = real[None] if image else real
    patch = tuple(patch) if patch else default_patch(not image)
    if pyramid is None:
        sizes = patchnn_pyramid_sizes(vol.shape[:3], ratio, min_size, patch, t_ratio, min_frames)
        pyramid = (sizes,) + patchnn_real_levels(vol, sizes, antialias)
    sizes, levels, keys = pyramid
    L = len(sizes)
    start = 0
    if guide is not None:
        gvol = guide[None] if guide.dim() == 3 else guide
        if guide.dim() != real.dim() or gvol.dtype != torch.uint8 or gvol.dim() != 4 or gvol.shape[-1] != 3 or gvol.device != vol.device:
            raise ValueError("patchnn_synthesize: the guide must be uint8 %s on %s like the real volume, got %s %s on %s"
                             % ("[H,W,3]" if image else "[T,H,W,3]", vol.device, guide.dtype, tuple(guide.shape), guide.device))
        if size is not None and tuple(int(e) for e in size) != tuple(gvol.shape[:3]):
            raise ValueError("patchnn_synthesize: the guide's size %s is the sample's: size %s differs"
                             % (tuple(gvol.shape[:3]), tuple(size)))
        if guide_level is None or isinstance(guide_level, bool) or not 0 <= int(guide_level) < L:
            raise ValueError("patchnn_synthesize: guide_level must lie in 0 .. %d (the pyramid has %d levels), got %r"
                             % (L - 1, L, guide_level))
        size, start = tuple(int(e) for e in gvol.shape[:3]), int(guide_level)
    elif guide_level is not None or guide_noise:
        raise ValueError("patchnn_synthesize: guide_level and guide_noise need a guide")
    qsizes = patchnn_sample_sizes(sizes, vol.shape[:3], size, patch, ratio, t_ratio, min_frames, start)
    alpha_abs = float(alpha) * 3 * patch[0] * patch[1] * patch[2] * 255 * 255
    iters = max(int(iters), 1)
    if guide is None:
        q = _resize_u8(levels[0], qsizes[0], antialias)
    else:
        q, noise, pm_from_level = _resize_u8(gvol, qsizes[start], antialias), guide_noise, max(int(pm_from_level), start + 1)
    if noise:
        torch.manual_seed(int(seed) + int(index))
        with ops.noise_stream(q.device):
            z = ops.normal_(torch.empty(q.shape, dtype=torch.float32, device=q.device))
        q = torch.round(q.to(torch.float32) + (float(noise) * 255.0) * z).clamp_(0, 255).to(torch.uint8)
    state = patchnn_search_state(seed, index) if search == "patchmatch" else None
    score = None
    for l in range(start, L):
        if l > start:
            q = _resize_u8(q, qsizes[l], antialias)
            if state is not None:
                qf, qt = (patchnn_wrap_grid(qsizes[k], patch, wrap) for k in (l - 1, l))
                rf, rt = (tuple(s - p + 1 for s, p in zip(sizes[k], patch)) for k in (l - 1, l))
                if state["fwd"] is not None:
                    state["fwd"] = patchnn_field_resize(state["fwd"], qf, rf, qt, rt)
                if state["rev"] is not None:
                    state["rev"] = patchnn_field_resize(state["rev"], rf, qf, rt, qt)
        for it in range(iters):
            k = keys[l] if (l > start and it == 0) else levels[l]
            q, score = patchnn_refine(q, k, levels[l], patch, alpha_abs, return_score=True, search=search, pm_iters=pm_iters,
                                      pm_from_level=pm_from_level, level=l, state=state, wrap=wrap)
    return (q[0] if image else q), score


# Patch inpainting (the hole-filling application of GPNN, after Wexler et al.'s space-time completion): the same coarse-to-fine
# steps, but at every level only the patches that overlap the hole are queries, only the patches that avoid it are keys
# (ops.patch_nn_subset: the contraction shrinks to |queries| x |keys|), and only the hole's voxels take the vote.
def patchnn_mask_resize(mask, size):
    """A bool mask [T,H,W] (torch tensor on any device, or numpy array) at another (T, H, W) with the same T, in exact integer
    arithmetic and separable: along an axis of S source and O output positions, output o is connected to source i iff
    |i (O - 1) - o (S - 1)| < max(O - 1, S - 1) (every pair when O or S is 1), and an output voxel is set iff some connected
    source voxel - connected along both axes - is set.  Equal sizes give the mask itself; the connected set holds floor and
    ceil of the align-corners source coordinate o (S - 1) / (O - 1), i.e. every voxel the linear resize of the volume reads
    for that output; and when downsizing every source is connected to some output, so a set voxel never vanishes."""
    if isinstance(mask, np.ndarray):
        return patchnn_mask_resize(torch.from_numpy(np.ascontiguousarray(mask)), size).numpy()
    size = tuple(int(e) for e in size)
    if mask.dim() != 3 or mask.dtype != torch.bool or len(size) != 3 or size[0] != mask.shape[0] or min(size) < 1:
        raise ValueError("patchnn_mask_resize: a bool [T,H,W] mask and a (T, H, W) with the same T, got %s %s -> %s"
                         % (mask.dtype, tuple(mask.shape), size))
    out = mask
    for axis in (1, 2):
        S, O = int(out.shape[axis]), size[axis]
        if S == O:
            continue
        i, o = np.arange(S, dtype=np.int64)[None, :], np.arange(O, dtype=np.int64)[:, None]
        conn = np.abs(i * (O - 1) - o * (S - 1)) < max(O - 1, S - 1) if min(O, S) > 1 else np.ones((O, S), bool)
        lo, hi = conn.argmax(1), S - conn[:, ::-1].argmax(1)      # the connected sources of o are the run [lo, hi)
        assert (conn.sum(1) == hi - lo).all() and (hi > lo).all()
        pre = torch.zeros([e + (a == axis) for a, e in enumerate(out.shape)], dtype=torch.int32, device=out.device)
        pre.narrow(axis, 1, S).copy_(torch.cumsum(out.to(torch.int32), axis))
        hi_t = torch.from_numpy(hi).to(out.device)
        lo_t = torch.from_numpy(lo).to(out.device)
        out = (pre.index_select(axis, hi_t) - pre.index_select(axis, lo_t)) > 0
    return out.contiguous()


def _flat_i32(cond):
    return torch.nonzero(cond.reshape(-1)).reshape(-1).to(torch.int32)


def patchnn_inpaint_plan(mask, sizes, patch):
    """What the levels of patchnn_inpaint need of the mask [T,H,W] (bool, on the device), one dict per level: `mask` = M_l, the
    mask at sizes[l] (patchnn_mask_resize of the full mask; the finest is the mask itself); `qsel` = the patches that overlap
    M_l, the queries; `rsel` = the patches that avoid it, the keys of an ordinary step; `rsel_first` (l > 0) = the patches
    that avoid B_l = M_l | resize(M_{l-1}), the keys of the level's first step, whose key volume is real level l-1 resized: a
    voxel of it is clean only where every voxel that resize read was known.  All three are ascending flat int32 grid
    indices.  An empty key set raises ValueError."""
    plan = []
    for l, size in enumerate(sizes):
        M = patchnn_mask_resize(mask, size)
        c = ops.patch_mask_count(M.to(torch.uint8), patch).reshape(-1)
        lv = {"mask": M, "qsel": _flat_i32(c > 0), "rsel": _flat_i32(c == 0)}
        if l > 0:
            B = M | patchnn_mask_resize(plan[-1]["mask"], size)
            lv["rsel_first"] = _flat_i32(ops.patch_mask_count(B.to(torch.uint8), patch) == 0)
        if any(lv[k].numel() == 0 for k in lv if k.startswith("rsel")):
            raise ValueError("patchnn_inpaint: the hole leaves no whole patch at level %d %s" % (l, tuple(size)))
        if lv["qsel"].numel() == 0:
            raise ValueError("patchnn_inpaint: the mask is empty")
        plan.append(lv)
    return plan


def patchnn_inpaint_step(query, keys, values, mask, patch, qsel, rsel, return_score=False):
    """One inpainting step on uint8 volumes [T,H,W,3]: nn = for the query patches qsel (those that overlap the hole) the nearest
    of the key patches rsel (those that avoid it), voted = the vote of the value patches nn with the query as fallback, and the
    result takes voted inside the bool mask [T,H,W] and the query elsewhere.  return_score: also the mean d2 of the queries."""
    d2, nn = ops.patch_nn_subset(query, keys, patch, qsel, rsel)
    voted = ops.patch_vote(values, nn, patch, tuple(query.shape[:-1]), query)
    out = torch.where(mask[..., None], voted, query)
    if return_score:
        return out, float(d2.reshape(-1)[qsel.long()].to(torch.float64).mean())
    return out


def patchnn_inpaint(real, mask, patch=None, ratio=0.75, min_size=16, iters=10, noise=0.75, seed=0, index=0, pyramid=None,
                    return_levels=False, antialias=False):
    """One completion of the hole `mask` (bool [T,H,W], images [H,W]; True = hole) of the uint8 device volume `real` ([T,H,W,3];
    images [H,W,3]) -> (sample, mean d2 of the last step's queries[, every level's result]).  Sizes, real levels and blurred
    keys are patchnn_synthesize's.  The coarsest guess is real level 0 with the hole set to the per-channel mean of the known
    voxels ((2 sum + n) // (2 n)) plus noise * 255 * N(0, 1), rounded and clamped; the noise is drawn for the whole volume
    under torch.manual_seed(seed + index) as patchnn_synthesize draws it.  Every step is patchnn_inpaint_step with the level's
    lists (patchnn_inpaint_plan): the plain nearest neighbour - a completeness term would pull every key of the clip into the
    hole.  Between levels the hole is the previous result resized and everything else real level l.  pyramid: a
    (sizes, levels, keys) or (sizes, levels, keys, plan) tuple to reuse between samples.  antialias: the real levels, the keys
    and the resize between levels are ops.volume_resize_u8, whose footprint is exactly the mask resize's connection rule: M_l
    covers every voxel that level l's resize of the full-size volume read, B_l every voxel the blurred keys read."""
    image = real.dim() == 3
    vol = real[None] if image else real
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != tuple(real.shape[:-1]) or \
            mask.device != real.device:
        raise ValueError("patchnn_inpaint: mask must be bool %s on %s, got %s %s on %s"
                         % (tuple(real.shape[:-1]), real.device, getattr(mask, "dtype", type(mask)), tuple(getattr(mask, "shape", ())),
                            getattr(mask, "device", None)))
    mask = mask[None] if image else mask
    patch = tuple(patch) if patch else default_patch(not image)
    if pyramid is None:
        sizes = patchnn_pyramid_sizes(vol.shape[:3], ratio, min_size, patch)
        pyramid = (sizes,) + patchnn_real_levels(vol, sizes, antialias)
    sizes, levels, keys = pyramid[:3]
    plan = pyramid[3] if len(pyramid) > 3 else patchnn_inpaint_plan(mask, sizes, patch)
    iters = max(int(iters), 1)
    M = plan[0]["mask"][..., None]
    known = (~M).to(torch.int64)
    n = known.sum()
    mean = (2 * (levels[0].to(torch.int64) * known).sum((0, 1, 2)) + n) // (2 * n)
    fill = mean.to(torch.float32).expand(levels[0].shape)
    if noise:
        torch.manual_seed(int(seed) + int(index))
        with ops.noise_stream(vol.device):
            z = ops.normal_(torch.empty(levels[0].shape, dtype=torch.float32, device=vol.device))
        fill = fill + (float(noise) * 255.0) * z
    q = torch.where(M, torch.round(fill).clamp_(0, 255).to(torch.uint8), levels[0])
    score, results = None, []
    for l, lv in enumerate(plan):
        if l > 0:
            q = torch.where(lv["mask"][..., None], _resize_u8(q, sizes[l], antialias), levels[l])
        for it in range(iters):
            first = l > 0 and it == 0
            last = l == len(plan) - 1 and it == iters - 1
            q = patchnn_inpaint_step(q, keys[l] if first else levels[l], levels[l], lv["mask"], patch, lv["qsel"],
                                     lv["rsel_first"] if first else lv["rsel"], return_score=last)
            if last:
                q, score = q
        results.append(q[0] if image else q)
    if return_levels:
        return results[-1], score, results
    return results[-1], score


def load_mask(path, shape):
    """The hole mask at `path` of a volume of (T, H, W) = shape as a host bool array [T,H,W] (programs.mask_forms, pick_mask)."""
    return pick_mask(mask_forms(path), shape)


def _host_real_shape(exp_dir, video_path, image_path):
    """((T, H, W), image) of the real volume a run will load, from the host alone: the input's frames as they are, or for an
    experiment directory what programs.real_volume makes of the run's input."""
    if exp_dir is None:
        ra = datasets.load_frames(video_path or image_path)
        image = image_path is not None
        if ra.ndim not in (3, 4) or ra.shape[-1] != 3:
            raise SystemExit("generate_patchnn: the input must be uint8 [N,H,W,3] or [H,W,3], got {} {}".format(ra.dtype, ra.shape))
        if image or ra.ndim == 3:
            return (1,) + tuple(ra.shape[-3:-1]), image
        return tuple(ra.shape[:3]), False
    opt = load_opt(exp_dir)
    h, w = datasets._stage_size(opt, opt.stop_scale)
    if opt.dims != 3:
        return (1, h, w), True
    frames = datasets.load_frames(opt.video_path)
    start = getattr(opt, "start_frame", 0)
    n = len(frames[start:start + opt.max_frames] if getattr(opt, "max_frames", None) else frames[start:])
    every = opt.sampling_rates[hp_utils.get_fps_td_by_index(opt.stop_scale, opt)[2]]
    return (len(range(0, n, every)), h, w), False


def generate_patchnn(exp_dir=None, video_path=None, image_path=None, out=None, num_samples=8, seed=0, patch=None, ratio=0.75,
                     min_size=16, iters=10, alpha=0.005, noise=0.75, size=None, save_levels=False, mask=None, search='exact',
                     pm_iters=None, pm_from_level=None, wrap=None, antialias=False, t_ratio=1.0, min_frames=None, guide=None,
                     guide_level=None, guide_mask=None, guide_feather=None, guide_noise=None):
    """Write samples.npy (uint8 [N,T,H,W,3], images [N,H,W,3]: what `evaluate --samples` reads), one GIF / PNG per sample and
    patchnn.json (the settings, the level sizes, seconds per sample from HIP events, the mean final score per sample).  mask: the
    path of a hole mask of the real volume; the samples are then completions of the hole (patchnn_inpaint), land in
    <exp-dir>/eval/samples_patchinpaint by default, and patchnn.json also records the mask, its voxels and per level the query
    and key patches.  search = 'patchmatch': patchnn_synthesize's PatchMatch steps, with pm_iters (default 4) iterations per
    search from level pm_from_level (default 1) on; patchnn.json then also records search, pm_iters and pm_from_level.  Not
    with a mask (the subset search has no PatchMatch form), and the two pm_* settings only with it.  wrap: the --wrap string
    (letters of t, h, w): the samples are rings along those axes (patchnn_synthesize's wrap); patchnn.json then records it.  Not
    with a mask, and no t for an image.  antialias: every resize is ops.volume_resize_u8.  t_ratio < 1 (with min_frames): the
    pyramid scales T too; not for an image and not with a mask.  patchnn.json records antialias when it is set, and t_ratio and
    min_frames (the value in force) when t_ratio is below 1.
    guide (a path: .npy, a frame directory or an image file) with guide_level = N: every sample starts from the guide at level N
    (patchnn_synthesize's guide) plus guide_noise (default 0) instead of from the coarsest level plus `noise`; the guide's
    (T, H, W) is the sample's size.  guide_mask (the forms of `mask`, the sample's shape) with guide_feather (default 1 5 5, images
    0 5 5): every finished sample becomes ops.mask_blend(sample, guide, mask, feather) - the sample inside the hole, the guide
    away from it.  Not with `mask`.  The samples land in <exp-dir>/eval/samples_patchnn_guide<N> by default and patchnn.json also
    records guide, guide_level, guide_noise, guide_mask and guide_feather."""
    t_ratio = 1.0 if t_ratio is None else float(t_ratio)
    if not 0.0 < t_ratio <= 1.0:
        raise SystemExit("generate_patchnn: --t-ratio must lie in (0, 1], got {}".format(t_ratio))
    if t_ratio == 1.0:
        if min_frames is not None:
            raise SystemExit("generate_patchnn: --min-frames needs --t-ratio below 1")
    else:
        if image_path is not None:
            raise SystemExit("generate_patchnn: --t-ratio needs a clip: an image has no time axis")
        if mask is not None:
            raise SystemExit("generate_patchnn: --t-ratio does not combine with --mask: the mask resize (patchnn_mask_resize) "
                             "keeps T and refuses another")
        if min_frames is not None and int(min_frames) < (int(patch[0]) if patch else default_patch(True)[0]):
            raise SystemExit("generate_patchnn: --min-frames must be at least the patch's T = {}, got {}".format(
                int(patch[0]) if patch else default_patch(True)[0], min_frames))
    rings = None
    if wrap is not None:
        try:
            rings = parse_wrap_axes(wrap)
        except SystemExit as e:
            raise SystemExit("generate_patchnn: {}".format(e))
        if mask is not None:
            raise SystemExit("generate_patchnn: --wrap makes the whole sample a ring, --mask keeps everything outside a hole: "
                             "they do not combine")
        if rings[0] and image_path is not None:
            raise SystemExit("generate_patchnn: --wrap t needs a clip: an image has no time axis")
    if search not in ("exact", "patchmatch"):
        raise SystemExit("generate_patchnn: --search must be exact or patchmatch, got {!r}".format(search))
    if search == "exact" and (pm_iters is not None or pm_from_level is not None):
        raise SystemExit("generate_patchnn: --pm-iters and --pm-from-level need --search patchmatch")
    if search == "patchmatch":
        if mask is not None:
            raise SystemExit("generate_patchnn: --mask searches a subset of the patches, which --search patchmatch does not do; "
                             "use --search exact")
        pm_iters = PM_ITERS if pm_iters is None else int(pm_iters)
        pm_from_level = PM_FROM_LEVEL if pm_from_level is None else int(pm_from_level)
        if not 0 <= pm_iters <= 1024:
            raise SystemExit("generate_patchnn: --pm-iters must lie in [0, 1024], got {}".format(pm_iters))
        if pm_from_level < 1:
            raise SystemExit("generate_patchnn: --pm-from-level must be >= 1 (level 0 is always exact), got {}".format(pm_from_level))
    given = [a for a in (exp_dir, video_path, image_path) if a is not None]
    if len(given) != 1:
        raise SystemExit("generate_patchnn: give exactly one of --exp-dir, --video-path and --image-path")
    if exp_dir is None and out is None:
        raise SystemExit("generate_patchnn: --video-path / --image-path need --out")
    gframes = gmask = gfeather = None
    if guide is None and guide_noise is not None:
        raise SystemExit("generate_patchnn: --guide-noise needs --guide")
    if guide is not None or guide_level is not None or guide_mask is not None or guide_feather is not None:
        # everything the guide's flags and files decide, before the device is touched
        host = _host_real_shape(exp_dir, video_path, image_path)
        gfeather, gforms = check_guide_flags("generate_patchnn", guide, guide_level, guide_mask, guide_feather, host[1])
        if mask is not None:
            raise SystemExit("generate_patchnn: --guide starts every voxel from the guide, --mask fills a hole of the real volume: "
                             "they do not combine (use --guide-mask to keep the guide outside a hole)")
        guide_noise = 0.0 if guide_noise is None else float(guide_noise)
        if not guide_noise >= 0 or math.isinf(guide_noise):
            raise SystemExit("generate_patchnn: --guide-noise must be finite and >= 0, got {}".format(guide_noise))
        gframes = load_guide_frames("generate_patchnn", guide)
        if host[1] and gframes.shape[0] != 1:
            raise SystemExit("generate_patchnn: the guide of an image run is one image, got {} frames".format(gframes.shape[0]))
        if size is not None and tuple(size) != tuple(gframes.shape[:3]):
            raise SystemExit("generate_patchnn: the guide's size {} is the samples': --size {} differs".format(
                tuple(gframes.shape[:3]), tuple(size)))
        size = tuple(int(e) for e in gframes.shape[:3])
        gpatch = tuple(patch) if patch else default_patch(not host[1])
        try:
            gsizes = patchnn_pyramid_sizes(host[0], ratio, min_size, gpatch, t_ratio, min_frames)
            if not 0 <= int(guide_level) < len(gsizes):
                raise ValueError("--guide-level must lie in 0 .. {} (the pyramid of the real volume {} has {} levels), got {}".format(
                    len(gsizes) - 1, tuple(host[0]), len(gsizes), guide_level))
            patchnn_sample_sizes(gsizes, host[0], size, gpatch, ratio, t_ratio, min_frames, int(guide_level))
        except ValueError as e:
            raise SystemExit("generate_patchnn: {}".format(e))
        if gforms is not None:
            gmask = pick_mask(gforms, size, "generate_patchnn: --guide-mask", "the guide's")
            _refuse_trivial_mask([gmask], "generate_patchnn: --guide-mask")
    hole = forms = None
    if mask is not None:
        # what the mask alone decides, before the device is touched.  The mask has the real volume's shape (checked below, once
        # that is known), so a --size that no reading of the mask has cannot be the real size; and a mask is refused as empty
        # or all hole here only when every reading that can still be the real volume's is.
        forms = mask_forms(mask)
        if size is not None:
            forms = [m for m in forms if tuple(m.shape) == tuple(size)]
            if not forms:
                raise SystemExit("generate_patchnn: --mask fills a hole of the real volume: --size {} is not the mask's {}".format(
                    tuple(size), " or ".join(str(tuple(m.shape)) for m in mask_forms(mask))))
        _refuse_trivial_mask(forms)
    device = gpu_device()
    fps = 10
    if exp_dir is not None:
        opt = load_opt(exp_dir)
        real = real_volume(opt, None, device)
        if opt.dims == 3:
            fps = hp_utils.get_fps_td_by_index(opt.stop_scale, opt)[0]
        out = out or os.path.join(exp_dir, 'eval', 'samples_patchinpaint' if mask is not None else
                                  'samples_patchnn_guide{}'.format(int(guide_level)) if guide is not None else 'samples_patchnn')
    else:
        real = load_u8_frames(video_path or image_path, device, image_path is not None,
                              "generate_patchnn: the input must be uint8 [N,H,W,3] or [H,W,3]", ranks=(3, 4))
        if video_path is not None and real.dim() == 3:
            real = real[None]   # one frame given as a clip
    image = real.dim() == 3
    if image and rings is not None and rings[0]:
        raise SystemExit("generate_patchnn: --wrap t needs a clip: an image has no time axis")
    if image and t_ratio != 1.0:
        raise SystemExit("generate_patchnn: --t-ratio needs a clip: an image has no time axis")
    vol = real[None] if image else real
    patch = tuple(patch) if patch else default_patch(not image)
    size = tuple(size) if size else tuple(vol.shape[:3])
    try:
        sizes = patchnn_pyramid_sizes(vol.shape[:3], ratio, min_size, patch, t_ratio, min_frames)
    except ValueError as e:
        raise SystemExit("generate_patchnn: {}".format(e))
    if image and size[0] != 1:
        raise SystemExit("generate_patchnn: an image's --size has T = 1")
    pyramid = (sizes,) + patchnn_real_levels(vol, sizes, antialias)
    if mask is not None:
        hole = pick_mask(forms, vol.shape[:3])
        _refuse_trivial_mask([hole])
        hole = torch.from_numpy(hole).to(device)
        try:
            pyramid = pyramid + (patchnn_inpaint_plan(hole, sizes, patch),)
        except ValueError as e:
            raise SystemExit("generate_patchnn: {}".format(e))
    gkw = {}
    if guide is not None:
        gdev = torch.from_numpy(gframes).to(device)
        gkw = {"guide": gdev, "guide_level": int(guide_level), "guide_noise": guide_noise}
        if gmask is not None:
            gmask = torch.from_numpy(gmask).to(device)
    os.makedirs(out, exist_ok=True)
    if save_levels:
        np.savez(os.path.join(out, 'levels.npz'), **{"level_%d" % l: v.cpu().numpy() for l, v in enumerate(pyramid[1])},
                 **{"keys_%d" % l: v.cpu().numpy() for l, v in enumerate(pyramid[2]) if l > 0})
    samples, seconds, scores = [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(num_samples):
        e0.record()
        try:
            if mask is not None:
                smp, score = patchnn_inpaint(vol, hole, patch, ratio, min_size, iters, noise, seed, i, pyramid, antialias=antialias)
            else:
                pm = {"search": search, "pm_iters": pm_iters, "pm_from_level": pm_from_level} if search == "patchmatch" else {}
                if rings is not None:
                    pm["wrap"] = rings
                if antialias:
                    pm["antialias"] = True
                if t_ratio != 1.0:
                    pm.update({"t_ratio": t_ratio, "min_frames": min_frames})
                smp, score = patchnn_synthesize(vol, size, patch, ratio, min_size, iters, noise, alpha, seed, i, pyramid, **pm, **gkw)
                if gmask is not None:
                    smp = ops.mask_blend(smp, gdev, gmask, gfeather)
        except ValueError as e:
            raise SystemExit("generate_patchnn: {}".format(e))
        e1.record()
        e1.synchronize()
        seconds.append(e0.elapsed_time(e1) / 1e3)
        scores.append(score)
        samples.append((smp[0] if image else smp).cpu().numpy())
    arr = np.stack(samples)
    write_samples(out, arr, fps)
    info = {"input": os.path.abspath(exp_dir or video_path or image_path), "real_shape": list(vol.shape[:3]), "size": list(size),
            "num_samples": int(num_samples), "seed": int(seed), "patch": list(patch), "ratio": float(ratio), "min_size": int(min_size),
            "iters": int(iters), "alpha": (float(alpha) if math.isfinite(alpha) else "inf"), "noise": float(noise),
            "level_sizes": [list(s) for s in sizes], "seconds_per_sample": seconds, "final_score_per_sample": scores,
            "final_score": "mean over the sample's patches of the last step's minimum: d2 / (alpha D 255^2 + the key's distance "
                           "to its nearest sample patch); plain d2 for alpha = inf"}
    if mask is not None:
        info.update({"mask": os.path.abspath(mask), "hole_voxels": int(hole.sum()), "alpha": "inf",
                     "active_patches": [int(lv["qsel"].numel()) for lv in pyramid[3]],
                     "valid_keys": [int(lv["rsel"].numel()) for lv in pyramid[3]]})
    if search == "patchmatch":
        info.update({"search": search, "pm_iters": pm_iters, "pm_from_level": pm_from_level})
    if wrap is not None:
        info["wrap"] = wrap
    if antialias:
        info["antialias"] = True
    if t_ratio != 1.0:
        info.update({"t_ratio": t_ratio, "min_frames": patch[0] + 1 if min_frames is None else int(min_frames)})
    if guide is not None:
        info.update({"guide": os.path.abspath(guide), "guide_level": int(guide_level), "guide_noise": guide_noise,
                     "guide_mask": os.path.abspath(guide_mask) if guide_mask is not None else None,
                     "guide_feather": list(gfeather) if gfeather is not None else None})
    with open(os.path.join(out, 'patchnn.json'), 'w') as f:
        json.dump(info, f, indent=1, sort_keys=True)
    print("wrote {} patch nearest-neighbour samples {} ({} levels, {:.3f} s per sample) to {}".format(
        len(arr), tuple(arr.shape[1:]), len(sizes), sum(seconds) / max(len(seconds), 1), out))
    return arr


def main(argv=None):
    a = generate_patchnn_parser().parse_args(argv)
    generate_patchnn(a.exp_dir, a.video_path, a.image_path, a.out, a.num_samples, a.seed, a.patch, a.ratio, a.min_size, a.iters,
                     a.alpha, a.noise, a.size, a.save_levels, a.mask, a.search, a.pm_iters, a.pm_from_level, a.wrap, a.antialias, a.t_ratio,
                     a.min_frames, a.guide, a.guide_level, a.guide_mask, a.guide_feather, a.guide_noise)
    return 0


if __name__ == "__main__":
    sys.exit(main())
