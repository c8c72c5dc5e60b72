"""Cost of `generate --wrap` at the benchmark's size, 13 x 144 x 256, batch 2 (development tool, not a test).  HIP events, warm-up,
median of `reps` with every repetition listed.

  1. One sampling pass of GeneratorHPVAEGAN (the benchmark's video config: nfc 64, latent 128, all levels; freshly initialised
     weights - the time does not depend on them - or --exp-dir E for a trained run) as `generate` runs it: train mode, no_grad,
     noise from the library's stream.  Plain, then with rings t and thw; milliseconds per sample.
  2. hpvg_ring_pad_f32 and the crop (hpvg_box_copy_f32) on the finest level's 64-channel activation [2, 64, 13, 144, 256] for
     rings t and thw, and hpvg_upsample_linear_ring_f32 on the last resize of the pyramid: bytes moved (read + write) and the
     achieved rate against the 6.29 TB/s float4 copy of profiles/snapshot_cost.txt.
With --plain-only just the plain pass of 1. is timed, through nothing this tool's commit added: run it on the parent commit and
on this tree in one session to see that a flagless `generate` costs what it did.
usage: python tools/perf_generate_ring.py [out.txt] [--reps N] [--plain-only] [--append] [--exp-dir E]"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import ops  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import networks_3d  # noqa: E402

argv = sys.argv[1:]


def flag(name, n=0):
    if name not in argv:
        return None
    k = argv.index(name)
    vals = argv[k + 1:k + 1 + n]
    del argv[k:k + 1 + n]
    return vals if n else True


reps = int((flag("--reps", 1) or [7])[0])
plain_only, append = flag("--plain-only"), flag("--append")
exp_dir = (flag("--exp-dir", 1) or [None])[0]
out_path = argv[0] if argv else None
COPY_RATE = 6.29e12   # bytes / s: the measured float4 copy of profiles/snapshot_cost.txt
DEV = torch.device("cuda", 0)
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def fmt(ms):
    return "[" + ", ".join("%.3f" % v for v in ms) + "]"


if exp_dir:
    from hp_vae_gan_amd import generate
    opt, netG = generate.load_generator(exp_dir, DEV)
    amps = opt.Noise_Amps
else:
    torch.manual_seed(0)
    opt = bench._video_opt(DEV)
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    netG = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(opt.stop_scale):
        netG.init_next_stage()
    netG = netG.to(DEV)
    amps = [1.0] + [0.1] * opt.stop_scale
netG.train()
B = 2
sizes = [netG._level_size(l) for l in range(len(netG.body) + 1)]
say("generator: %d levels, %s -> %s, batch %d, %s weights" % (len(sizes), sizes[0], sizes[-1], B, "trained" if exp_dir else "fresh"))


def one_pass():
    with torch.no_grad(), ops.noise_stream(DEV):
        z = hu.generate_noise(size=[B, opt.latent_dim, *sizes[0]], device=DEV)
        fake, _ = netG(z, amps, noise_init=z, mode="rand")
    return fake


med, ms = timed(one_pass)
say("generate pass, plain: median %.3f ms = %.3f ms per sample of %s" % (med, med / B, fmt(ms)))
if not plain_only:
    from hp_vae_gan_amd import generate
    plain_med = med
    for axes in ("t", "thw"):
        generate.set_ring(netG, tuple(int(c in axes) for c in "thw"))
        med, ms = timed(one_pass)
        say("generate pass, --wrap %s: median %.3f ms = %.3f ms per sample (x %.3f of plain) of %s" % (
            axes, med, med / B, med / plain_med, fmt(ms)))
    generate.set_ring(netG, (0, 0, 0))

    say("")
    say("kernels on the finest level's activation [2, 64, 13, 144, 256] (copy rate %.2f TB/s):" % (COPY_RATE / 1e12))
    T, H, W = sizes[-1]
    NC = B * 64
    x = torch.randn((B, 64, T, H, W), device=DEV)
    for axes in ("t", "thw"):
        pad = tuple(int(c in axes) for c in "thw")
        big = (T + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2])
        out = torch.empty((B, 64) + big, device=DEV)
        back = torch.empty_like(x)
        parr = (ctypes.c_int * 3)(*pad)
        nbytes = 4 * (x.numel() + out.numel())
        med, ms = timed(lambda: hplib.call("hpvg_ring_pad_f32", hplib.ptr(x), NC, T, H, W, parr, hplib.ptr(out), hplib.stream()))
        say("hpvg_ring_pad_f32 ring %-3s: %d bytes, median %.4f ms = %.2f TB/s = %.0f %% of the copy rate, of %s" % (
            axes, nbytes, med, nbytes / med / 1e9, 100 * nbytes / (med * 1e-3) / COPY_RATE, fmt(ms)))
        med, ms = timed(lambda: hplib.call("hpvg_box_copy_f32", hplib.ptr(out), hplib.ptr(back), NC, *big, T, H, W, -pad[0], -pad[1],
                                           -pad[2], hplib.stream()))
        say("hpvg_box_copy_f32 crop %-3s: %d bytes, median %.4f ms = %.2f TB/s = %.0f %% of the copy rate, of %s" % (
            axes, nbytes, med, nbytes / med / 1e9, 100 * nbytes / (med * 1e-3) / COPY_RATE, fmt(ms)))
        assert torch.equal(back, x)
    Ts, Hs, Ws = sizes[-2]
    src = torch.randn((B, 3, Ts, Hs, Ws), device=DEV)
    dst = torch.empty((B, 3, T, H, W), device=DEV)
    nbytes = 4 * (src.numel() + dst.numel())
    for axes in ("", "t", "thw"):
        warr = (ctypes.c_int * 3)(*[int(c in axes) for c in "thw"])
        med, ms = timed(lambda: hplib.call("hpvg_upsample_linear_ring_f32", hplib.ptr(src), B * 3, Ts, Hs, Ws, hplib.ptr(dst), T, H, W,
                                           warr, hplib.stream()))
        say("hpvg_upsample_linear_ring_f32 %s -> %s ring %-4s: %d bytes, median %.4f ms = %.2f TB/s, of %s" % (
            sizes[-2], sizes[-1], axes or "none", nbytes, med, nbytes / med / 1e9, fmt(ms)))

if out_path:
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n")
