"""numpy restatements for guided sampling (generate --guide, generate_patchnn --guide).

`mask_blend_ref` is the contract of hpvg_mask_blend_u8 (include/hpvg.h) read aloud: per voxel a walk over its clipped box, and
for every voxel of that box a walk over ITS clipped box - nothing separable, so it shares no shortcut with the kernel.  `defect`
seeds one of three mistakes on purpose, for the tests that show the equality checks would notice them.  `far_from_hole` is the
set on which the contract promises the second volume untouched.

`synthesize_guided_ref` is the guided schedule of generate_patchnn.patchnn_synthesize on an antialiased pyramid, composed of the
existing restatements (patch_ref / patchwrap_ref steps, volresize_ref resizes); `generator_guided_ref` is the float64 forward of
GeneratorHPVAEGAN.refinement_layers from level N, composed of ring_ref's pieces."""
import math

import numpy as np
import torch

from patchwrap_ref import periodic_grid, refine_wrap_ref
from ring_ref import _stack, ring_resize_ref
from volresize_ref import resize as vol_resize

DEFECTS = ("no_dilation", "n_unclipped", "round_down")


def _box(v, shape, radius):
    return [range(max(0, v[k] - radius[k]), min(shape[k] - 1, v[k] + radius[k]) + 1) for k in range(3)]


def mask_blend_ref(a, b, mask, radius, defect=None):
    """uint8 [T,H,W,3] x 2, mask [T,H,W] (nonzero = hole), radius (rt, rh, rw) -> uint8 [T,H,W,3]:
    out = (2 (c a + (n - c) b) + n) // (2 n), c = the voxels u of box(v) whose own box holds a hole voxel, n = |box(v)|."""
    assert defect is None or defect in DEFECTS
    a, b, hole = np.asarray(a), np.asarray(b), np.asarray(mask) != 0
    assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == hole.shape + (3,) and len(radius) == 3
    shape = hole.shape
    dil = np.zeros(shape, bool)
    for t in range(shape[0]):
        for y in range(shape[1]):
            for x in range(shape[2]):
                if defect == "no_dilation":
                    dil[t, y, x] = hole[t, y, x]
                else:
                    bt, by, bx = _box((t, y, x), shape, radius)
                    dil[t, y, x] = hole[bt.start:bt.stop, by.start:by.stop, bx.start:bx.stop].any()
    out = np.zeros(a.shape, np.uint8)
    for t in range(shape[0]):
        for y in range(shape[1]):
            for x in range(shape[2]):
                bt, by, bx = _box((t, y, x), shape, radius)
                c = int(dil[bt.start:bt.stop, by.start:by.stop, bx.start:bx.stop].sum())
                n = len(bt) * len(by) * len(bx)
                if defect == "n_unclipped":
                    n = (2 * radius[0] + 1) * (2 * radius[1] + 1) * (2 * radius[2] + 1)
                for k in range(3):
                    num = 2 * (c * int(a[t, y, x, k]) + (n - c) * int(b[t, y, x, k])) + (0 if defect == "round_down" else n)
                    out[t, y, x, k] = num // (2 * n)
    return out


def far_from_hole(mask, radius):
    """bool [T,H,W]: the voxels farther than 2 r_ax from EVERY hole voxel along some axis (the axis may differ from hole voxel to
    hole voxel), i.e. those no hole voxel has within 2 r on all three axes at once."""
    hole = np.asarray(mask) != 0
    far = np.ones(hole.shape, bool)
    idx = np.indices(hole.shape)
    for u in np.argwhere(hole):
        near = np.ones(hole.shape, bool)
        for k in range(3):
            near &= np.abs(idx[k] - u[k]) <= 2 * radius[k]
        far &= ~near
    return far


# ------------------------------------------------------------------------------------------------------ the patch schedule
def pyramid_sizes(shape, ratio, min_size):
    """generate_patchnn.patchnn_pyramid_sizes for t_ratio = 1: [(T, H, W)] coarse to fine."""
    T, H, W = shape

    def at(k):
        return (T, int(math.floor(H * ratio ** k + 0.5)), int(math.floor(W * ratio ** k + 0.5)))
    L = 1
    while min(at(L)[1:]) >= max(int(min_size), 1):
        L += 1
    return [at(L - 1 - l) for l in range(L)]


def _resize(vol, size):
    return np.ascontiguousarray(vol) if tuple(vol.shape[:3]) == tuple(size) else vol_resize(vol, size)


def field_resize_ref(nn, qf, rf, qt, rt):
    """generate_patchnn.patchnn_field_resize in numpy: the field read at the nearest source query coordinate (align corners, halves
    up) and its key coordinates carried to the target key grid by the same rule."""
    src = np.clip(np.asarray(nn, np.int64).reshape(qf), 0, rf[0] * rf[1] * rf[2] - 1)
    for ax in range(3):
        a = np.arange(qt[ax], dtype=np.int64)
        idx = (2 * a * (qf[ax] - 1) + (qt[ax] - 1)) // (2 * (qt[ax] - 1)) if qt[ax] > 1 else np.zeros_like(a)
        src = np.take(src, idx, axis=ax)
    b = [src // (rf[1] * rf[2]), (src // rf[2]) % rf[1], src % rf[2]]
    for ax in range(3):
        b[ax] = (2 * b[ax] * (rt[ax] - 1) + (rf[ax] - 1)) // (2 * (rf[ax] - 1)) if rf[ax] > 1 else np.zeros_like(b[ax])
    return (b[0] * rt[1] + b[1]) * rt[2] + b[2]


def synthesize_guided_ref(real, guide, level, z, guide_noise, patch, ratio, min_size, iters, alpha, seed=0, index=0, search="exact",
                          pm_iters=4, pm_from_level=1, wrap=(0, 0, 0)):
    """The guided sample of patchnn_synthesize(antialias=True) as uint8 [T,H,W,3].  z: the float32 N(0, 1) draw of the guess at
    `level` (the test takes it from the device stream under seed + index; None for guide_noise 0).  Levels below `level` are
    skipped, level `level` is exact with keys = values = the real level, PatchMatch starts at max(pm_from_level, level + 1), the
    n-th PatchMatch search runs under (seed + index) * 1000003 + n."""
    sizes = pyramid_sizes(real.shape[:3], ratio, min_size)
    L = len(sizes)
    levels = [_resize(real, s) for s in sizes]
    keys = [levels[0]] + [_resize(levels[l - 1], sizes[l]) for l in range(1, L)]
    St, Sh, Sw = guide.shape[:3]
    if tuple(guide.shape[:3]) == tuple(real.shape[:3]):
        qsizes = sizes
    else:
        qsizes = [(St, int(math.floor(Sh * ratio ** (L - 1 - l) + 0.5)), int(math.floor(Sw * ratio ** (L - 1 - l) + 0.5)))
                  for l in range(L)]
    alpha_abs = np.float32(float(alpha) * 3 * patch[0] * patch[1] * patch[2] * 255 * 255)
    q = _resize(guide, qsizes[level])
    if guide_noise:
        f = q.astype(np.float32) + np.float32(float(guide_noise) * 255.0) * np.asarray(z, np.float32)
        assert f.dtype == np.float32
        q = np.clip(np.round(f), 0, 255).astype(np.uint8)
    pm_first = max(int(pm_from_level), level + 1)
    pm_seed, fwd, rev = (int(seed) + int(index)) * 1000003, None, None
    for l in range(level, L):
        if l > level:
            q = _resize(q, qsizes[l])
            if search == "patchmatch":
                qf, qt = (periodic_grid(qsizes[k], patch, wrap) for k in (l - 1, l))
                rf, rt = (tuple(s - p + 1 for s, p in zip(sizes[k], patch)) for k in (l - 1, l))
                fwd = None if fwd is None else field_resize_ref(fwd, qf, rf, qt, rt)
                rev = None if rev is None else field_resize_ref(rev, rf, qf, rt, qt)
        for it in range(iters):
            k = keys[l] if (l > level and it == 0) else levels[l]
            how = "patchmatch" if search == "patchmatch" and l >= pm_first else "exact"
            q, fwd, rev, pm_seed = refine_wrap_ref(q, k, levels[l], patch, alpha_abs, wrap, how, pm_iters, pm_seed, fwd, rev)
    return q


# --------------------------------------------------------------------------------------------------- the trained generator
def generator_guided_ref(netG, x_start, start, noise_amps, sizes, ring, noises):
    """Float64 CPU forward of GeneratorHPVAEGAN.refinement_layers(start, x_start, amps, 'rand'): per level l = start + 1 .. L,
    up = resize(x, sizes[l]), up_noisy = up + amp_l * noise where the level injects noise (3-D: from the first GAN level on; 2-D:
    every level), x = tanh(block(up_noisy) + up); BatchNorm on batch statistics.  start = 0 with the decoder's output is the
    unguided pass (ring_ref.generator_ring_ref).  noises: the recorded level noises of the levels that run, in order."""
    nd = x_start.dim() - 2
    ring = [int(f) for f in ring]
    wrap3 = [0] * (3 - nd) + ring
    x = x_start.detach().double().cpu()
    noises = list(noises)
    for idx, block in enumerate(netG.body):
        if idx < start:
            continue
        size = [int(s) for s in sizes[idx + 1]]
        a = x.numpy() if nd == 3 else x.numpy()[:, :, None]
        up = torch.from_numpy(np.ascontiguousarray(ring_resize_ref(a, [1] * (3 - nd) + size, wrap3)))
        up = up if nd == 3 else up[:, :, 0]
        up_noisy = up
        if nd == 2 or netG.opt.vae_levels <= idx + 1:
            nz = noises.pop(0).detach().double().cpu()
            assert tuple(nz.shape) == tuple(up.shape), (tuple(nz.shape), tuple(up.shape))
            up_noisy = up + float(noise_amps[idx + 1]) * nz
        x = torch.tanh(_stack(block, up_noisy, ring) + up)
    assert not noises, "%d recorded noises were not used" % len(noises)
    return x
