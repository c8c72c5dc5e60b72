"""Guided sampling on the GPU: ops.mask_blend / hpvg_mask_blend_u8 against the plain numpy definition (tests/guide_ref.py) by
equality, with every tensor at every byte offset 0..3 inside guard bands; its refusals and its properties as bits; the trained
path on a small random-weight generator (the guide through the dataset's front end, the guided pass against float64); and the
guided schedule of patchnn_synthesize against the numpy schedule."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import offset_buf as OB  # noqa: E402
from guide_ref import far_from_hole, generator_guided_ref, mask_blend_ref, synthesize_guided_ref  # noqa: E402
from helpers import RTOL, rel_err  # noqa: E402
from hp_vae_gan_amd import datasets, generate, generate_patchnn, ops  # noqa: E402
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import networks_2d, networks_3d  # noqa: E402
from make_golden import make_opt  # noqa: E402
from ring_ref import generator_ring_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ERR_ARG = hplib._CONSTANTS["HPVG_ERR_ARG"]
ERR_UNSUPPORTED = hplib._CONSTANTS["HPVG_ERR_UNSUPPORTED"]
ERR_WORKSPACE = hplib._CONSTANTS["HPVG_ERR_WORKSPACE"]


def _i3(v):
    return (ctypes.c_int * 3)(*[int(e) for e in v])


def _rc(name, *args):
    """the raw return code of an entry point (hplib.call raises on any but 0)"""
    return getattr(hplib.load(), name)(*args)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ mask_blend
SHAPES = [(3, 5, 7), (1, 9, 8), (4, 1, 6), (2, 70, 3)]
RADII = [(0, 0, 0), (1, 1, 1), (1, 2, 3), (0, 3, 3), (2, 64, 1)]
MASKS = ["one", "corner", "random", "empty", "full"]


def _mask(kind, shape, rng):
    m = np.zeros(shape, np.uint8)
    if kind == "one":
        m[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
    elif kind == "corner":
        m[-1, -1, 0] = 200
    elif kind == "random":
        m = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    elif kind == "full":
        m[:] = 255
    return m


def test_new_entry_points_are_declared_and_bound():
    names = hplib.check_symbols()
    assert "hpvg_mask_blend_u8" in names and "hpvg_mask_blend_ws_bytes" in names


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_blend_equals_the_definition_at_every_byte_offset(shape):
    """Every radius and mask of the lists above; per case four placements, so that each of a, b, mask and out starts at every
    byte offset 0..3, each placement run twice (offset_buf.byte_rule: guards 0x00 / 0xFF around the inputs, two sentinels in the
    output), guards bit-intact after each."""
    rng = np.random.default_rng(sum(shape))
    T, H, W = shape
    a, b = (rng.integers(0, 256, shape + (3,)).astype(np.uint8) for _ in range(2))
    for radius in RADII:
        nbytes = hplib.call("hpvg_mask_blend_ws_bytes", T, H, W, _i3(radius))
        assert (nbytes == 0) == (radius == (0, 0, 0))
        ws = ops._scratch(nbytes, DEV)
        for kind in MASKS:
            mask = _mask(kind, shape, rng)
            want = torch.from_numpy(mask_blend_ref(a, b, mask, radius))

            def launch(ins, outs):
                hplib.call("hpvg_mask_blend_u8", hplib.ptr(ins["a"]), hplib.ptr(ins["b"]), hplib.ptr(ins["mask"]), T, H, W, _i3(radius),
                           hplib.ptr(outs["out"]), *ws, hplib.stream())
                torch.cuda.synchronize()
            for k in range(4):
                offs = {"a": k, "b": (k + 1) % 4, "mask": (k + 2) % 4, "out": (k + 3) % 4}
                OB.byte_rule(launch, {"a": torch.from_numpy(a), "b": torch.from_numpy(b), "mask": torch.from_numpy(mask)},
                             {"out": shape + (3,)}, {"out": want}, offs, DEV, "mask_blend %s r %s %s offsets %s" % (shape, radius, kind, offs))
            got = ops.mask_blend(_dev(a), _dev(b), _dev(mask), radius)
            assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), (shape, radius, kind)


def test_mask_blend_images_bool_masks_and_python_refusals():
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 256, (9, 8, 3)).astype(np.uint8) for _ in range(2))
    mask = rng.random((9, 8)) < 0.2
    want = torch.from_numpy(mask_blend_ref(a[None], b[None], mask[None], (0, 2, 1))[0])
    assert torch.equal(ops.mask_blend(_dev(a), _dev(b), _dev(mask), (2, 1)).cpu(), want)
    assert torch.equal(ops.mask_blend(_dev(a), _dev(b), _dev(mask.astype(np.uint8) * 9), (0, 2, 1)).cpu(), want)
    for bad in ((1, 2, 1), (2,), (0, 65, 1), (0, -1, 1)):
        with pytest.raises(RuntimeError, match="mask_blend"):
            ops.mask_blend(_dev(a), _dev(b), _dev(mask), bad)
    with pytest.raises(RuntimeError, match="mask_blend: mask must be"):
        ops.mask_blend(_dev(a), _dev(b), _dev(mask[:-1]), (2, 1))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.mask_blend(_dev(a), _dev(b[:-1]), _dev(mask), (2, 1))
    with pytest.raises(RuntimeError):
        ops.mask_blend(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(mask), (2, 1))     # host tensors


def test_mask_blend_refusals_return_their_codes_without_a_launch():
    T, H, W = 3, 5, 7
    V = T * H * W
    buf = torch.full((16 * V,), 0x5A, dtype=torch.uint8, device=DEV)
    a, b, out, m = buf[:3 * V], buf[3 * V:6 * V], buf[6 * V:9 * V], buf[9 * V:10 * V]
    p, s, r = hplib.ptr, hplib.stream(), _i3((1, 2, 3))
    nbytes = hplib.call("hpvg_mask_blend_ws_bytes", T, H, W, r)
    assert nbytes >= 6 * V and nbytes % 16 == 0
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    w = (p(ws), nbytes)
    f = "hpvg_mask_blend_u8"
    for bad in ((0, H, W), (T, 0, W), (T, H, -1)):
        assert _rc(f, p(a), p(b), p(m), *bad, r, p(out), *w, s) == ERR_ARG, bad
        assert hplib.call("hpvg_mask_blend_ws_bytes", *bad, r) == 0
    for bad in ((-1, 0, 0), (0, 65, 0), (0, 0, 1000)):
        assert _rc(f, p(a), p(b), p(m), T, H, W, _i3(bad), p(out), *w, s) == ERR_ARG, bad
        assert hplib.call("hpvg_mask_blend_ws_bytes", T, H, W, _i3(bad)) == 0
    assert _rc(f, p(a), p(b), p(m), T, H, W, None, p(out), *w, s) == ERR_ARG
    for args in ((None, p(b), p(m), p(out)), (p(a), None, p(m), p(out)), (p(a), p(b), None, p(out)), (p(a), p(b), p(m), None)):
        assert _rc(f, args[0], args[1], args[2], T, H, W, r, args[3], *w, s) == ERR_ARG
    # out overlapping an input: in place, and out starting inside one
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(a), *w, s) == ERR_ARG
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(buf[3 * V + 5:]), *w, s) == ERR_ARG
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(buf[7 * V + 1:]), *w, s) == ERR_ARG            # its tail lies on the mask
    # 2^31 voxels: refused on the host
    assert _rc(f, p(a), p(b), p(m), 1 << 11, 1 << 10, 1 << 10, r, p(out), *w, s) == ERR_UNSUPPORTED
    assert hplib.call("hpvg_mask_blend_ws_bytes", 1 << 11, 1 << 10, 1 << 10, r) == 0
    # workspace: null, misaligned, one byte short; radius 0 takes a null one
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(out), None, nbytes, s) == ERR_WORKSPACE
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(out), p(ws[1:]), nbytes, s) == ERR_WORKSPACE
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(out), p(ws), nbytes - 1, s) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())                                                              # nothing was launched
    assert _rc(f, p(a), p(b), p(m), T, H, W, _i3((0, 0, 0)), p(out), None, 0, s) == 0
    assert _rc(f, p(a), p(b), p(m), T, H, W, r, p(out), *w, s) == 0
    torch.cuda.synchronize()


def test_mask_blend_properties_as_bits():
    rng = np.random.default_rng(11)
    shape, radius = (6, 40, 52), (1, 3, 4)
    a, b = (rng.integers(0, 256, shape + (3,)).astype(np.uint8) for _ in range(2))
    mask = np.zeros(shape, bool)
    mask[2:4, 10:17, 20:31] = True
    mask[5, 39, 0] = True
    out = ops.mask_blend(_dev(a), _dev(b), _dev(mask), radius).cpu().numpy()
    assert np.array_equal(out[mask], a[mask])                                  # a on the hole
    far = far_from_hole(mask, radius)
    assert 0 < far.sum() < far.size and np.array_equal(out[far], b[far])       # b beyond 2 r
    between = ~far & ~mask
    assert (out[between] != a[between]).any() and (out[between] != b[between]).any()
    assert np.array_equal(out, mask_blend_ref(a, b, mask, radius))
    # a and b swapped, nothing else changed: the formula with the volumes exchanged (the weights c / n stay)
    swapped = ops.mask_blend(_dev(b), _dev(a), _dev(mask), radius).cpu().numpy()
    assert np.array_equal(swapped, mask_blend_ref(b, a, mask, radius))
    assert np.array_equal(swapped[mask], b[mask]) and np.array_equal(swapped[far], a[far])
    # with a = 255 and b = 0 the two results are the rounded weights w and 255 - w up to the shared half: they sum to 255 or 256
    hi, lo = _dev(np.full_like(a, 255)), _dev(np.zeros_like(a))
    w1 = ops.mask_blend(hi, lo, _dev(mask), radius).cpu().numpy().astype(int)
    w0 = ops.mask_blend(lo, hi, _dev(mask), radius).cpu().numpy().astype(int)
    assert set(np.unique(w1 + w0)) <= {255, 256} and np.array_equal((w1 + w0 == 256), (w1 + w0 == 256) & between[..., None])
    # deterministic
    assert np.array_equal(ops.mask_blend(_dev(a), _dev(b), _dev(mask), radius).cpu().numpy(), out)


# ---------------------------------------------------------------------------------------------------------- trained path
def _small_opt(dims):
    opt = make_opt(device=DEV, dims=dims, generator="GeneratorHPVAEGAN", hflip=False, start_frame=0, max_frames=1000, data_rep=1)
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    return opt


def _small_generator(dims=3, levels=3, seed=0):
    torch.manual_seed(seed)
    opt = _small_opt(dims)
    netG = (networks_3d if dims == 3 else networks_2d).GeneratorHPVAEGAN(opt)
    for _ in range(levels):
        netG.init_next_stage()
    return opt, netG.to(DEV)


def _frames(dims, seed=0):
    rng = np.random.default_rng(seed)
    n = 14 if dims == 3 else 1
    base = rng.integers(0, 256, (n, 9, 12, 3)).astype(np.float64)
    return np.clip(np.kron(base, np.ones((1, 4, 4, 1))) + rng.normal(0, 6, (n, 36, 48, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("dims", [3, 2])
def test_the_guide_made_from_the_training_frames_is_the_datasets_item(dims):
    opt = _small_opt(dims)
    opt.frames = _frames(dims)
    ds = (datasets.SingleVideoDataset if dims == 3 else datasets.SingleImageDataset)(opt, device=DEV)
    assert opt.ar == 0.75
    for N in range(3):
        opt.scale_idx = N
        if dims == 3:
            opt.fps_index = hu.get_fps_td_by_index(N, opt)[2]
            ds.generate_frames(N)
        item = ds[0]
        item = item[0] if N > 0 else item
        x, u8 = generate.guide_tensors(opt, opt.frames, N, DEV, finest=3)
        shape = hu.images.level_shape_3d(N, opt) if dims == 3 else hu.images.level_shape_2d(N, opt)
        assert list(x.shape) == [3] + shape and torch.equal(x, item), (dims, N)
        fine = hu.images.level_shape_3d(3, opt) if dims == 3 else [1] + hu.images.level_shape_2d(3, opt)
        assert u8.dtype == torch.uint8 and list(u8.shape) == fine + [3]


class _Recorded:
    """noise_source that draws from a CPU generator and keeps what it drew"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.drawn = []

    def __call__(self, ref):
        n = torch.randn(tuple(ref.shape), generator=self.g)
        self.drawn.append(n)
        return n.to(ref.device)


@pytest.mark.parametrize("dims", [3, 2])
def test_guided_pass_against_float64_is_no_worse_than_twice_the_unguided_pass(dims):
    """The bound is the ring tests' rule: the scaled error (max |got - ref| / max |ref|) of the unguided pass against the float64
    restatement is measured here, and the guided pass - the same levels from N on, fewer of them - is allowed twice that."""
    amps = [1.0, 0.1, 0.1, 0.1]
    opt, netG = _small_generator(dims)
    netG.train()
    trained = [netG._level_size(l) for l in range(4)]
    z = torch.randn((2, opt.latent_dim, *trained[0]), generator=torch.Generator().manual_seed(3))
    src = _Recorded(11)
    netG.noise_source = src
    with torch.no_grad():
        got, _ = netG(z.to(DEV), amps, noise_init=z.to(DEV), mode="rand")
    plain = rel_err(got, generator_ring_ref(netG, z, amps, trained, (0,) * dims, src.drawn))
    assert 0 < plain <= RTOL, plain
    opt.ar = 0.75
    frames = _frames(dims, 1)
    for N in range(3):
        x = generate.guide_tensors(opt, frames, N, DEV)[0]
        x = x[None].expand(2, *x.shape).contiguous()
        src = _Recorded(20 + N)
        netG.noise_source = src
        with torch.no_grad():
            got, _ = netG(z.to(DEV), amps, noise_init=z.to(DEV), sample_init=(N, x.clone()), mode="rand")
        ref = generator_guided_ref(netG, x, N, amps, trained, (0,) * dims, src.drawn)
        assert tuple(got.shape) == tuple(ref.shape) == (2, 3, *trained[-1])
        guided = rel_err(got, ref)
        print("%d-D generator vs float64, max |got - ref| / max |ref|: unguided %.3e, guided from level %d %.3e" % (dims, plain, N, guided))
        assert guided <= 2 * plain, (N, guided, plain)
        # the guide matters, and so does the level noise above it
        other = generate.guide_tensors(opt, _frames(dims, 2), N, DEV)[0]
        with torch.no_grad():
            moved, _ = netG(z.to(DEV), amps, noise_init=z.to(DEV), sample_init=(N, other[None].expand(2, *other.shape).contiguous()),
                            mode="rand")
        assert not torch.equal(moved, got)


# ------------------------------------------------------------------------------------------------------------ patch path
PATCH, RATIO, MIN_SIZE, ITERS = (3, 5, 5), 0.75, 8, 2


def _clip(shape, seed):
    rng = np.random.default_rng(seed)
    t, h, w = shape
    base = rng.integers(0, 256, (t, h // 4 + 1, w // 4 + 1, 3)).astype(np.float64)
    big = np.kron(base, np.ones((1, 4, 4, 1)))[:, :h, :w]
    return np.clip(big + rng.normal(0, 10, big.shape), 0, 255).astype(np.uint8)


def _synth(real, size=None, **kw):
    return generate_patchnn.patchnn_synthesize(real, size, PATCH, RATIO, MIN_SIZE, ITERS, **kw)[0]


def test_guide_the_clip_at_level_0_without_noise_is_the_unguided_sample_without_noise():
    real = _dev(_clip((5, 20, 24), 0))
    assert len(generate_patchnn.patchnn_pyramid_sizes((5, 20, 24), RATIO, MIN_SIZE, PATCH)) == 4
    want = _synth(real, noise=0)
    got = _synth(real, guide=real, guide_level=0, guide_noise=0)
    assert torch.equal(got, want)
    assert torch.equal(_synth(real, noise=0.75, guide=real, guide_level=0), want)      # --noise is not used in a guided run


def test_guide_the_clip_at_the_finest_level_returns_the_clip():
    real = _dev(_clip((5, 20, 24), 0))
    for search in ("exact", "patchmatch"):
        assert torch.equal(_synth(real, guide=real, guide_level=3, guide_noise=0, search=search), real)


def test_patchnn_synthesize_guide_refusals():
    real = _dev(_clip((5, 20, 24), 0))
    for kw in (dict(guide=real, guide_level=4), dict(guide=real, guide_level=-1), dict(guide=real), dict(guide_level=1),
               dict(guide_noise=0.5), dict(guide=real[0], guide_level=1), dict(guide=real, guide_level=1, size=(5, 20, 25)),
               dict(guide=_dev(_clip((5, 9, 30), 1)), guide_level=0)):
        with pytest.raises(ValueError, match="patchnn_synthesize"):
            _synth(real, **kw)


@pytest.mark.parametrize("search,wrap", [("exact", None), ("patchmatch", None), ("patchmatch", (1, 0, 0))])
def test_guide_of_another_size_at_a_middle_level_equals_the_numpy_schedule(search, wrap):
    """An antialiased pyramid, so that every resize of the schedule is exact integer arithmetic; the level's noise is drawn
    from the device stream under seed + index as the function draws it, and handed to the numpy schedule."""
    real, guide = _clip((5, 20, 24), 0), _clip((5, 16, 30), 1)
    level, noise, seed, index = 1, 0.3, 4, 2
    torch.manual_seed(seed + index)
    with ops.noise_stream(DEV):
        z = ops.normal_(torch.empty((5, 9, 17, 3), dtype=torch.float32, device=DEV)).cpu().numpy()
    want = synthesize_guided_ref(real, guide, level, z, noise, PATCH, RATIO, MIN_SIZE, ITERS, 0.005, seed, index, search, 2, 1,
                                 wrap or (0, 0, 0))
    got, score = generate_patchnn.patchnn_synthesize(_dev(real), None, PATCH, RATIO, MIN_SIZE, ITERS, 0.75, 0.005, seed, index, None,
                                                     search, 2, 1, wrap, True, guide=_dev(guide), guide_level=level, guide_noise=noise)
    assert got.shape == (5, 16, 30, 3) and np.isfinite(score)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert not np.array_equal(want, synthesize_guided_ref(real, guide, level, None, 0, PATCH, RATIO, MIN_SIZE, ITERS, 0.005, seed, index,
                                                          search, 2, 1, wrap or (0, 0, 0)))
