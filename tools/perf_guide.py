"""Cost of guided sampling at the benchmark's size, 13 x 144 x 256 (development tool, not a test).  HIP events, warm-up, median of
`reps` (default 5) with every repetition listed.

  1. ops.mask_blend (hpvg_mask_blend_u8) on 13 x 144 x 256 byte volumes with a box hole: radius (1, 5, 5) (the default feather) and
     (0, 0, 0) (the hard composite, one kernel), as time and as bytes / s over the 10 bytes per voxel the composite cannot avoid
     (a, b and out 3 each, the mask 1), beside the 6.29 TB/s float4 copy of profiles/snapshot_cost.txt; then one radius at a time,
     which shows what each axis' dilation and count passes cost.
  2. One sampling pass of GeneratorHPVAEGAN (the benchmark's video config, freshly initialised weights, batch 2) as `generate`
     runs it, unguided and with sample_init at the middle level, and the composite of its batch on top.
  3. One sample of patchnn_synthesize (patch 3 7 7, --search patchmatch, iters 4) unguided and guided at the middle level, and the
     composite on top.
usage: python tools/perf_guide.py [out.txt] [--reps N]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import generate_patchnn, ops  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import networks_3d  # noqa: E402

argv = sys.argv[1:]
reps = 5
if "--reps" in argv:
    k = argv.index("--reps")
    reps = int(argv[k + 1])
    del argv[k:k + 2]
out_path = argv[0] if argv else None
COPY_RATE = 6.29e12   # bytes / s: the measured float4 copy of profiles/snapshot_cost.txt
DEV = torch.device("cuda", 0)
SHAPE = (13, 144, 256)
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
    return "[" + ", ".join("%.4f" % v for v in ms) + "]"


# ---- 1. the kernel
rng = np.random.default_rng(0)
a, b = (torch.from_numpy(rng.integers(0, 256, SHAPE + (3,)).astype(np.uint8)).to(DEV) for _ in range(2))
hole = torch.zeros(SHAPE, dtype=torch.uint8, device=DEV)
hole[4:9, 40:100, 80:180] = 1
V = SHAPE[0] * SHAPE[1] * SHAPE[2]
say("mask_blend on %s uint8 volumes, hole %d voxels; %d bytes per call at 10 bytes per voxel; copy rate %.2f TB/s" % (
    SHAPE, int(hole.sum()), 10 * V, COPY_RATE / 1e12))
for radius in ((1, 5, 5), (0, 0, 0), (0, 0, 5), (0, 5, 0), (1, 0, 0)):
    med, ms = timed(lambda: ops.mask_blend(a, b, hole, radius))
    rate = 10 * V / (med * 1e-3)
    say("  radius %-9s: median %.4f ms = %.3f TB/s = %.1f %% of the copy rate, of %s" % (
        radius, med, rate / 1e12, 100 * rate / COPY_RATE, fmt(ms)))

# ---- 2. the trained generator
torch.manual_seed(0)
opt = bench._video_opt(DEV)
hu.adjust_scales2image(opt.img_size, opt)
opt.stop_scale_time = opt.stop_scale
netG = networks_3d.GeneratorHPVAEGAN(opt)
for _ in range(opt.stop_scale):
    netG.init_next_stage()
netG = netG.to(DEV).train()
amps = [1.0] + [0.1] * opt.stop_scale
B = 2
sizes = [netG._level_size(l) for l in range(len(netG.body) + 1)]
N = len(netG.body) // 2
x_guide = torch.tanh(torch.randn((B, 3, *sizes[N]), device=DEV))
say("")
say("generator: %d levels, %s -> %s, batch %d, fresh weights; guide at level %d %s" % (len(sizes), sizes[0], sizes[-1], B, N, sizes[N]))


def one_pass(guided):
    with torch.no_grad(), ops.noise_stream(DEV):
        z = hu.generate_noise(size=[B, opt.latent_dim, *sizes[0]], device=DEV)
        kw = {"sample_init": (N, x_guide.clone())} if guided else {}
        fake, _ = netG(z, amps, noise_init=z, mode="rand", **kw)
    return fake


plain, ms = timed(lambda: one_pass(False))
say("generate pass, unguided: median %.3f ms = %.3f ms per sample, of %s" % (plain, plain / B, fmt(ms)))
med, ms = timed(lambda: one_pass(True))
say("generate pass, --guide-level %d: median %.3f ms = %.3f ms per sample (x %.3f of unguided), of %s" % (N, med, med / B, med / plain, fmt(ms)))
fake = one_pass(True)
fine = tuple(sizes[-1])
ga = torch.from_numpy(rng.integers(0, 256, fine + (3,)).astype(np.uint8)).to(DEV)
gh = torch.zeros(fine, dtype=torch.uint8, device=DEV)
gh[4:9, 40:100, 80:180] = 1
med, ms = timed(lambda: [ops.mask_blend(s, ga, gh, (1, 5, 5)) for s in ops.video_to_u8(fake)])
say("  --guide-mask on top (to bytes, %d composites): median %.3f ms = %.3f ms per sample, of %s" % (B, med, med / B, fmt(ms)))

# ---- 3. the patch generator
base = rng.integers(0, 256, (SHAPE[0], SHAPE[1] // 8 + 1, SHAPE[2] // 8 + 1, 3)).astype(np.float64)
clip = np.kron(base, np.ones((1, 8, 8, 1)))[:, :SHAPE[1], :SHAPE[2]]
real = torch.from_numpy(np.clip(clip + rng.normal(0, 8, clip.shape), 0, 255).astype(np.uint8)).to(DEV)
patch = (3, 7, 7)
psizes = generate_patchnn.patchnn_pyramid_sizes(SHAPE, 0.75, 16, patch)
pyramid = (psizes,) + generate_patchnn.patchnn_real_levels(real, psizes)
PN = len(psizes) // 2
say("")
say("patchnn_synthesize: clip %s, patch %s, %d levels, --search patchmatch, iters 4; guide at level %d %s" % (
    SHAPE, patch, len(psizes), PN, psizes[PN]))


def one_sample(guided):
    kw = {"guide": a, "guide_level": PN, "guide_noise": 0.25} if guided else {}
    return generate_patchnn.patchnn_synthesize(real, None, patch, 0.75, 16, 4, 0.75, 0.005, 0, 0, pyramid, "patchmatch", **kw)[0]


plain, ms = timed(lambda: one_sample(False), warm=1)
say("one sample, unguided: median %.2f ms, of %s" % (plain, fmt(ms)))
med, ms = timed(lambda: one_sample(True), warm=1)
say("one sample, --guide-level %d: median %.2f ms (x %.3f of unguided), of %s" % (PN, med, med / plain, fmt(ms)))
smp = one_sample(True)
med, ms = timed(lambda: ops.mask_blend(smp, a, hole, (1, 5, 5)))
say("  --guide-mask on top: median %.4f ms, of %s" % (med, fmt(ms)))

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
