"""generate --size / --wrap on the GPU: the circular pad at every word offset inside guard bands, the ring resize against
float64 and its roll property as bits, modules/_nets.Conv with `ring` against the circular convolution, a small generator at
another size and on a ring against the float64 restatement of the sampling path, and the program end to end (fresh child
processes on an experiment directory written without training).  References: tests/ring_ref.py."""
import ctypes
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import conv_ref as R  # noqa: E402
import offset_buf as OB  # noqa: E402
from helpers import RTOL, rel_err  # noqa: E402
from hp_vae_gan_amd import checkpoint, generate, ops, programs  # noqa: E402
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import _nets, networks_2d, networks_3d  # noqa: E402
from make_golden import make_opt  # noqa: E402
from ring_ref import generator_ring_ref, ring_conv_ref, ring_pad_ref, ring_resize_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TAU = 1e-5      # the project's rule: |got - ref| <= TAU * A


def _i3(v):
    return (ctypes.c_int * 3)(*[int(e) for e in v])


def _rc(name, *args):
    """the raw return code of an entry point (hplib.call raises on any but 0)"""
    return getattr(hplib.load(), name)(*args)


ERR_ARG = hplib._CONSTANTS["HPVG_ERR_ARG"]
ERR_UNSUPPORTED = hplib._CONSTANTS["HPVG_ERR_UNSUPPORTED"]


# ------------------------------------------------------------------------------------------------------------- ring pad
PAD_CASES = [(3, (1, 1, 1), (1, 1, 1)), (2, (2, 5, 7), (1, 0, 1)), (3, (4, 6, 33), (3, 3, 3)), (2, (1, 5, 9), (0, 1, 1))]


@pytest.mark.parametrize("nc,sp,pad", PAD_CASES)
def test_ring_pad_equals_the_reference_at_every_offset(nc, sp, pad):
    g = torch.Generator().manual_seed(nc * 100 + sp[2])
    x = torch.randn((nc,) + sp, generator=g)
    want = torch.from_numpy(ring_pad_ref(x.numpy(), pad)).float()
    big = tuple(s + 2 * p for s, p in zip(sp, pad))
    assert tuple(want.shape) == (nc,) + big
    for so in OB.OFFSETS:
        for do in OB.OFFSETS:
            src = OB.embed(x, so, device=DEV)
            dst = OB.out_like((nc,) + big, torch.float32, do, device=DEV)
            hplib.call("hpvg_ring_pad_f32", hplib.ptr(src), nc, *sp, _i3(pad), hplib.ptr(dst), hplib.stream())
            torch.cuda.synchronize()
            what = "ring_pad %s pad %s, offsets %d -> %d" % (sp, pad, so, do)
            OB.assert_written(dst, what)
            assert OB.guards_intact(src), what + ": the input's guard band was written"
            assert torch.equal(dst.cpu(), want), what


def test_ring_pad_through_ops_2d_and_3d():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((2, 3, 4, 6, 5), generator=g)
    got = ops.ring_pad(x.to(DEV), (2, 0, 7))
    assert torch.equal(got.cpu(), torch.from_numpy(ring_pad_ref(x.numpy(), (2, 0, 7))).float())
    assert torch.equal(ops.ring_crop(got, (2, 0, 7)).cpu(), x)
    x2 = torch.randn((2, 3, 6, 5), generator=g)
    got2 = ops.ring_pad(x2.to(DEV), (1, 3))
    assert torch.equal(got2.cpu(), torch.from_numpy(ring_pad_ref(x2.numpy()[:, :, None], (0, 1, 3))[:, :, 0]).float())
    assert torch.equal(ops.ring_crop(got2, (1, 3)).cpu(), x2)


def test_ring_pad_refusals():
    x = torch.zeros(2 * 2 * 5 * 7 + 1024, device=DEV)
    out = torch.zeros(2 * 4 * 5 * 9, device=DEV)
    p, s = hplib.ptr, hplib.stream()
    ok = _i3((1, 0, 1))
    assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, ok, p(out), s) == 0
    assert _rc("hpvg_ring_pad_f32", None, 2, 2, 5, 7, ok, p(out), s) == ERR_ARG
    assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, ok, None, s) == ERR_ARG
    assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, None, p(out), s) == ERR_ARG
    for bad in ((0, 2, 5, 7), (2, 0, 5, 7), (2, 2, 0, 7), (2, 2, 5, 0), (2, 2, 5, -3)):
        assert _rc("hpvg_ring_pad_f32", p(x), *bad, ok, p(out), s) == ERR_ARG, bad
    for bad in ((-1, 0, 1), (1, -1, 1), (1, 0, -2)):
        assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, _i3(bad), p(out), s) == ERR_ARG, bad
    # out overlapping x: in place, and out starting inside x
    assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, ok, p(x), s) == ERR_ARG
    assert _rc("hpvg_ring_pad_f32", p(x), 2, 2, 5, 7, ok, p(x[100:]), s) == ERR_ARG
    assert _rc("hpvg_ring_pad_f32", p(x[100:]), 2, 2, 5, 7, ok, p(x), s) == ERR_ARG      # x starting inside out
    # 2^31 elements: refused on the host, nothing is launched
    assert _rc("hpvg_ring_pad_f32", p(x), 1 << 31, 1, 1, 1, _i3((0, 0, 0)), p(out), s) == ERR_UNSUPPORTED
    assert _rc("hpvg_ring_pad_f32", p(x), 1 << 20, 2, 32, 16, _i3((0, 0, 8)), p(out), s) == ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_ring_ops_refuse_a_backward():
    x = torch.randn((1, 2, 3, 4, 5), device=DEV, requires_grad=True)
    for fn in (lambda: ops.ring_pad(x, (1, 1, 1)), lambda: ops.upsample_ring(x, (6, 4, 5), (1, 0, 0)),
               lambda: ops.ring_crop(x, (1, 1, 1))):
        with pytest.raises(RuntimeError, match="no backward"):
            fn()
    with torch.no_grad():
        assert ops.ring_pad(x, (1, 1, 1)).shape == (1, 2, 5, 6, 7)


# ---------------------------------------------------------------------------------------------------------- ring resize
def test_ring_resize_without_flags_is_upsample_ac_bit_for_bit():
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 3, 3, 5, 7), generator=g).to(DEV)
    want = ops.UpsampleAC.apply(x, (4, 7, 9), None, 0.0)
    got = ops.upsample_ring(x, (4, 7, 9), (0, 0, 0))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    null = torch.empty_like(want)
    hplib.call("hpvg_upsample_linear_ring_f32", hplib.ptr(x), 6, 3, 5, 7, hplib.ptr(null), 4, 7, 9, None, hplib.stream())
    assert torch.equal(null.view(torch.int32), want.view(torch.int32))
    for bad in ((2, 0, 0), (0, -1, 0), (0, 0, 3)):
        assert _rc("hpvg_upsample_linear_ring_f32", hplib.ptr(x), 6, 3, 5, 7, hplib.ptr(null), 4, 7, 9, _i3(bad),
                   hplib.stream()) == ERR_ARG


@pytest.mark.parametrize("src,dst", [((4, 5, 6), (7, 5, 11)), ((6, 5, 8), (4, 5, 3)), ((1, 4, 4), (3, 4, 8))])
@pytest.mark.parametrize("flags", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_ring_resize_against_float64(src, dst, flags):
    g = torch.Generator().manual_seed(sum(src) * 7 + sum(flags))
    x = torch.randn((2, 3) + src, generator=g)
    ref, A = ring_resize_ref(x.numpy(), dst, flags, with_scale=True)
    got = ops.upsample_ring(x.to(DEV), dst, flags).cpu().double().numpy()
    assert got.shape == ref.shape
    worst = float(np.max(np.abs(got - ref) / A))
    print("ring resize %s -> %s flags %s: worst |got - ref| / A = %.3e" % (src, dst, flags, worst))
    assert np.all(np.abs(got - ref) <= TAU * A), worst
    if all(s == d for s, d, f in zip(src, dst, flags)):
        assert np.array_equal(got, x.double().numpy())


@pytest.mark.parametrize("k", [2, 3])
def test_ring_resize_roll_property_as_bits(k):
    g = torch.Generator().manual_seed(k)
    x = torch.randn((2, 3, 4, 5, 6), generator=g).to(DEV)
    for ax, flags in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        size = list(x.shape[2:])
        size[ax] *= k
        y = ops.upsample_ring(x, size, flags)
        for r in (1, 3):
            rolled = ops.upsample_ring(torch.roll(x, r, 2 + ax).contiguous(), size, flags)
            assert torch.equal(rolled.view(torch.int32), torch.roll(y, k * r, 2 + ax).contiguous().view(torch.int32)), (ax, r)
    # all three at once
    size = [s * k for s in x.shape[2:]]
    y = ops.upsample_ring(x, size, (1, 1, 1))
    rolled = ops.upsample_ring(torch.roll(x, (1, 2, 3), (2, 3, 4)).contiguous(), size, (1, 1, 1))
    assert torch.equal(rolled.view(torch.int32), torch.roll(y, (k, 2 * k, 3 * k), (2, 3, 4)).contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------- Conv with ring
CONV_CASES = [(3, f, k, sp) for f in ((1, 0, 1), (1, 1, 1)) for k in (3, 5, 7) for sp in ((3, 6, 9), (1, 6, 9))] + \
             [(2, (1, 1), 3, (6, 9))]


@pytest.mark.parametrize("dims,ring,k,sp", CONV_CASES)
def test_conv_with_ring_is_the_circular_convolution(dims, ring, k, sp):
    torch.manual_seed(k * 10 + dims)
    conv = _nets.Conv(dims, 5, 6, k, k // 2).to(DEV)
    x = torch.randn((2, 5) + sp)
    ref, A = ring_conv_ref(x, conv.weight, conv.bias, ring)
    with torch.no_grad():
        plain = conv(x.to(DEV))
        conv.ring = ring
        got = conv(x.to(DEV))
    assert got.shape == plain.shape
    worst = R.check(got.cpu(), ref, A, "Conv(ring=%s, k=%d) on %s" % (ring, k, sp))
    print("Conv ring %s k %d %s: worst |got - ref| / A = %.3e" % (ring, k, sp, worst))
    # the zero-padded conv is something else (unless every ring axis has no neighbours to wrap to and none to pad: never here)
    assert R.err_ratio(plain.cpu(), ref, A)[0] > 100 * TAU
    conv.ring = (0,) * dims
    with torch.no_grad():
        assert torch.equal(conv(x.to(DEV)), plain)           # all flags zero: today's path


# ------------------------------------------------------------------------------------------------------------ generator
def _small_opt(dims):
    opt = make_opt(device=DEV, dims=dims, generator="GeneratorHPVAEGAN")
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


class _Recorded:
    """noise_source that draws from a CPU generator and keeps what it drew"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.drawn = []

    def __call__(self, ref):
        n = torch.randn(tuple(ref.shape), generator=self.g)
        self.drawn.append(n)
        return n.to(ref.device)


def _run_generator(netG, amps, sizes, ring, seed):
    netG.train()
    netG.level_sizes = None if sizes is None else [list(s) for s in sizes]
    trained = [netG._level_size(l) for l in range(len(netG.body) + 1)] if sizes is None else sizes
    if ring is not None:
        generate.set_ring(netG, ring)
    src = _Recorded(seed)
    netG.noise_source = src
    z = torch.randn((2, netG.opt.latent_dim, *trained[0]), generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        got, _ = netG(z.to(DEV), amps, noise_init=z.to(DEV), mode="rand")
    ref = generator_ring_ref(netG, z, amps, trained, ring or (0,) * netG.dims, src.drawn)
    assert tuple(got.shape) == tuple(ref.shape) == (2, 3, *trained[-1])
    return rel_err(got, ref)


def test_generator_at_another_size_and_on_a_ring_against_float64():
    """The bound: the worst scaled error (max |got - ref| / max |ref|) of the plain path - trained sizes, no ring - against the
    float64 restatement is measured first; the --size and the ring paths are allowed twice that (the pad and the crop are exact
    copies and the ring resize has the op count of the plain one, so more than a factor of 2 is a defect, not rounding)."""
    amps = [1.0, 0.1, 0.1, 0.1]
    opt, netG = _small_generator()
    trained = [netG._level_size(l) for l in range(4)]
    plain = _run_generator(netG, amps, None, None, 11)
    fine = trained[-1]
    sizes = generate.level_sizes(trained, [2 * fine[0], fine[1], (3 * fine[2]) // 2])
    assert sizes[-1] == [2 * fine[0], fine[1], (3 * fine[2]) // 2] and sizes[0] != trained[0]
    resized = _run_generator(netG, amps, sizes, None, 11)
    _, netR = _small_generator()                      # the same weights (same seed), its convs on a t ring
    ring = _run_generator(netR, amps, None, (1, 0, 0), 11)
    print("generator vs float64, max |got - ref| / max |ref|: plain %.3e, --size %s %.3e, ring t %.3e" % (
        plain, "x".join(map(str, sizes[-1])), resized, ring))
    assert 0 < plain <= RTOL, plain                    # the suite's own measure: the restatement is the path that runs
    assert resized <= 2 * plain, (resized, plain)
    assert ring <= 2 * plain, (ring, plain)


def test_generator_2d_on_an_hw_ring_against_float64():
    amps = [1.0, 0.1, 0.1, 0.1]
    _, netG = _small_generator(dims=2)
    err = _run_generator(netG, amps, None, (1, 1), 5)
    print("2-D generator on an hw ring vs float64: %.3e" % err)
    assert err <= RTOL


# -------------------------------------------------------------------------------------------------------------- program
def _child(args, cwd, timeout=120, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    print("%s: %.1f s, exit %d" % (" ".join(args[:1] + args[3:]), time.time() - t0, r.returncode))
    if ok:
        assert r.returncode == 0, (args, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _write_experiment(path, dims, program=None, weights=True):
    """An experiment directory as a trainer leaves it, without training: opt.json, and netG.pth / Noise_Amps.pth of a freshly
    initialised small generator with three body levels through checkpoint's own writer."""
    opt, netG = _small_generator(dims)
    opt.scale_idx = 3
    opt.Noise_Amps = [1.0, 0.1, 0.1, 0.1]
    if program:
        opt.program = program
    os.makedirs(os.path.join(path, "eval"))
    saved = programs.json_settings(opt)
    with open(os.path.join(path, "opt.json"), "w") as f:
        json.dump(saved, f, indent=1, sort_keys=True)
    if weights:
        trainer = types.SimpleNamespace(netG=netG, netD=None, optimizerG=types.SimpleNamespace(state_dict=lambda: {}))
        checkpoint.save_stage(path, opt, trainer)
    return path, [netG._level_size(l) for l in range(4)]


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ring"))
    path, trained = _write_experiment(os.path.join(tmp, "exp"), 3)
    plain = os.path.join(path, "eval", "samples")
    _child(["hp_vae_gan_amd.generate", "--exp-dir", path, "--num-samples", "3", "--seed", "7"], tmp)
    return types.SimpleNamespace(tmp=tmp, path=path, trained=trained, plain=plain)


def _gen(exp, flags, out=None, seed=7):
    args = ["hp_vae_gan_amd.generate", "--exp-dir", exp.path, "--num-samples", "3", "--seed", str(seed)] + flags
    _child(args + (["--out", out] if out else []), exp.tmp)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_program_without_flags_writes_no_new_file(exp):
    assert sorted(os.listdir(exp.plain)) == ["sample_0000.gif", "sample_0001.gif", "sample_0002.gif", "samples.npy"]
    assert sorted(os.listdir(os.path.join(exp.path, "eval"))) == ["samples"]
    assert list(np.load(os.path.join(exp.plain, "samples.npy")).shape) == [3] + exp.trained[-1] + [3]


def test_program_size_at_the_trained_size_reproduces_the_flagless_bytes(exp):
    T, H, W = exp.trained[-1]
    _gen(exp, ["--size", str(T), str(H), str(W)])
    out = os.path.join(exp.path, "eval", "samples_%dx%dx%d" % (T, H, W))
    assert _bytes(os.path.join(out, "samples.npy")) == _bytes(os.path.join(exp.plain, "samples.npy"))
    with open(os.path.join(out, "generate.json")) as f:
        meta = json.load(f)
    assert meta["size"] == [T, H, W] and meta["level_sizes"] == exp.trained and meta["wrap"] is None
    assert meta["seed"] == 7 and meta["num_samples"] == 3 and meta["batch_size"] == 2 and meta["seconds_per_sample"] > 0


@pytest.mark.parametrize("which", ["size", "wrap", "both"])
def test_program_flags_shape_metadata_and_determinism(exp, which):
    T, H, W = exp.trained[-1]
    size = [2 * T, H, (3 * W) // 2] if which != "wrap" else [T, H, W]
    flags = (["--size"] + [str(s) for s in size] if which != "wrap" else []) + (["--wrap", "t"] if which != "size" else [])
    _gen(exp, flags)
    _gen(exp, flags, out=os.path.join(exp.tmp, "again_" + which))
    name = "samples_%dx%dx%d" % tuple(size) + ("_wrapt" if which != "size" else "")
    out = os.path.join(exp.path, "eval", name)
    arr = np.load(os.path.join(out, "samples.npy"))
    assert arr.dtype == np.uint8 and list(arr.shape) == [3] + size + [3]
    assert _bytes(os.path.join(out, "samples.npy")) == _bytes(os.path.join(exp.tmp, "again_" + which, "samples.npy"))
    assert sorted(os.listdir(out)) == ["generate.json", "sample_0000.gif", "sample_0001.gif", "sample_0002.gif", "samples.npy"]
    with open(os.path.join(out, "generate.json")) as f:
        meta = json.load(f)
    assert meta["size"] == size and meta["level_sizes"] == generate.level_sizes(exp.trained, size)
    assert meta["wrap"] == (None if which == "size" else "t")
    if which == "wrap":   # the ring changes the samples; the trained size and seed are those of the flagless run
        assert not np.array_equal(arr, np.load(os.path.join(exp.plain, "samples.npy")))


REFUSALS = [(3, None, ["--wrap", "q"]), (3, None, ["--wrap", "tt"]), (3, None, ["--size", "13", "30"]),
            (3, None, ["--size", "13", "0", "40"]), (2, None, ["--wrap", "t"]), (2, None, ["--size", "13", "30", "40"]),
            (3, "train_video_baselines", ["--size", "13", "30", "40"]), (3, "train_video_baselines", ["--wrap", "t"])]


@pytest.mark.parametrize("dims,program,flags", REFUSALS)
def test_program_refusals_exit_nonzero_and_leave_no_directory(tmp_path, dims, program, flags):
    path, _ = _write_experiment(str(tmp_path / "exp"), dims, program, weights=False)    # refused before anything is loaded
    r = _child(["hp_vae_gan_amd.generate", "--exp-dir", path, "--num-samples", "1", "--out", str(tmp_path / "out")] + flags,
               str(tmp_path), ok=False)
    assert r.returncode != 0 and "Traceback" not in r.stderr and ("--size" in r.stderr or "--wrap" in r.stderr), r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "out")) and os.listdir(os.path.join(path, "eval")) == []
    assert sorted(os.listdir(str(tmp_path))) == ["exp"]
