"""The antialiased space-time pyramid of generate_patchnn at the benchmarked size - a 13 x 144 x 256 clip, patch 3 x 7 x 7
(development tool, not a test): (a) hpvg_volume_resize_u8 against the seven-launch fp32 path (generate_patchnn._resize_u8) on the
finest upscale and on the coarsest level made from the full-size volume (per call, 20 calls between two events); (b) one full sample with the program's defaults, with
--antialias and with --antialias --t-ratio 0.85, under both searches; (c) `evaluate --scales 2`'s numbers on those samples.
HIP events, warm-up, median of `reps`.  The clip is the smooth multi-scale one of tools/perf_patchmatch.py.  With --compare, the
`(d) one full sample` lines of two tools/perf_patchgen.py outputs (the parent commit's and this tree's, taken in the same
session) are copied in and the tree's median is checked against the parent's own min-max spread.
usage: python tools/perf_patchpyramid.py [out.txt] [reps] [--compare parent_patchgen.txt tree_patchgen.txt]"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import evaluate, generate_patchnn, ops  # noqa: E402

argv = sys.argv[1:]
compare = None
if "--compare" in argv:
    k = argv.index("--compare")
    compare = argv[k + 1:k + 3]
    argv = argv[:k]
out_path = argv[0] if len(argv) > 0 else None
reps = int(argv[1]) if len(argv) > 1 else 5
T, H, W = 13, 144, 256
PATCH = (3, 7, 7)
dev = torch.device("cuda")
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def timed(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms


def fmt(ms, digits=3):
    return "[" + ", ".join("%.*f" % (digits, m) for m in ms) + "]"


def clip(seed):
    """tools/perf_patchmatch.py's clip: smooth, multi-scale, drifting over t, with mild noise."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    vol = torch.zeros(1, 3, T, H, W)
    for cells, amp in ((4, 50.0), (12, 30.0), (36, 14.0)):
        coarse = torch.randn(1, 3, max(T // 4, 2), cells * 9 // 16 + 2, cells + 2, generator=g)
        vol += amp * torch.nn.functional.interpolate(coarse, size=(T, H, W), mode="trilinear", align_corners=True)
    vol += 2.0 * torch.randn(vol.shape, generator=g)
    return (128 + vol).round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 3, 0).contiguous()


real = clip(0).to(dev)
say("patch pyramid perf: clip %s (the smooth multi-scale clip of tools/perf_patchmatch.py), patch %s" % ((T, H, W), PATCH))

# ---- (a) the resize alone
sizes = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH)
sizes_t = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH, 0.85)
below = torch.randint(0, 256, sizes[-2] + (3,), dtype=torch.uint8, device=dev)
for name, src, size in (("the finest upscale", below, sizes[-1]), ("the coarsest level from full size", real, sizes[0]),
                        ("the coarsest level from full size, T scaled", real, sizes_t[0])):
    dmax, reads = ops.volume_resize_check(tuple(src.shape[:3]), size)
    # 20 calls between the two events, so that the figure is the stream's time per call and not one enqueue's host time
    med_k, ms_k = (lambda m, ms: (m / 20, [v / 20 for v in ms]))(*timed(lambda: [ops.volume_resize_u8(src, size) for _ in range(20)], 2, reps))
    med_o, ms_o = (lambda m, ms: (m / 20, [v / 20 for v in ms]))(*timed(lambda: [generate_patchnn._resize_u8(src, size) for _ in range(20)], 2, reps))
    nbytes = 3.0 * (src.shape[0] * src.shape[1] * src.shape[2] + size[0] * size[1] * size[2])
    say("(a) %s, %s -> %s (at most %d source voxels per output, %s per output): ops.volume_resize_u8 median %.3f ms of %s "
        "(%.1f GB/s of source + output bytes); the fp32 path (permute, to-float, UpsampleAC, round, clamp, to-u8, permute: 2 source "
        "voxels per axis whatever the ratio) median %.3f ms of %s; x%.2f"
        % (name, tuple(src.shape[:3]), tuple(size), reads, "a wave" if reads >= 64 else "a thread", med_k, fmt(ms_k), nbytes / med_k / 1e6,
           med_o, fmt(ms_o), med_o / med_k))

# ---- (b) one sample, (c) its scores at three scales
CONFIGS = (("default", {}), ("--antialias", {"antialias": True}), ("--antialias --t-ratio 0.85", {"antialias": True, "t_ratio": 0.85}))
D = 3 * PATCH[0] * PATCH[1] * PATCH[2]
ssizes = evaluate.scale_sizes((T, H, W), 2)
real_scaled = [real] + [ops.volume_resize_u8(real, s) for s in ssizes]


def scores(smp):
    out = []
    for k, rk in enumerate(real_scaled):
        sk = smp if k == 0 else ops.volume_resize_u8(smp, ssizes[k - 1])
        out.append((evaluate.patch_score(ops.patch_nn(sk, rk, PATCH)[0], D), evaluate.patch_score(ops.patch_nn(rk, sk, PATCH)[0], D)))
    return out


for search in ("exact", "patchmatch"):
    for name, kw in CONFIGS:
        sz = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH, kw.get("t_ratio", 1.0))
        pyramid = (sz,) + generate_patchnn.patchnn_real_levels(real, sz, kw.get("antialias", False))
        last = [None]

        def sample():
            last[0] = generate_patchnn.patchnn_synthesize(real, None, PATCH, 0.75, 16, 10, 0.75, 0.005, 0, 1, pyramid, search=search, **kw)[0]
        med, ms = timed(sample, 1, reps)
        sc = scores(last[0])
        say("(b) one sample, search %-10s %-27s (%d levels %s ... %s): median %.1f ms of %s" % (search, name, len(sz), sz[0], sz[-1], med, fmt(ms, 1)))
        say("(c)     seed 0 + 1, coherence / completeness at full size %.6f / %.6f, at scale 1 %s %.6f / %.6f, at scale 2 %s %.6f / %.6f"
            % (sc[0] + (ssizes[0],) + sc[1] + (ssizes[1],) + sc[2]))
med_e, ms_e = timed(lambda: [ops.volume_resize_u8(real, s) for s in ssizes], 3, reps)
say("(c) evaluate --scales 2 adds per volume the two resizes (median %.3f ms of %s) and per sample the searches at %s and %s"
    % (med_e, fmt(ms_e), ssizes[0], ssizes[1]))

if compare:
    def line(path):
        with open(path) as f:
            for ln in f:
                if ln.startswith("(d) one full sample"):
                    m = re.search(r"median ([0-9.]+) ms of \[(.*?)\]", ln)
                    return ln.strip()[:200], float(m.group(1)), [float(v) for v in m.group(2).split(",")]
        raise SystemExit("no '(d) one full sample' line in %s" % path)
    pl, pmed, pall = line(compare[0])
    tl, tmed, tall = line(compare[1])
    lo, hi = min(pall), max(pall)
    say("(d) the default path (tools/perf_patchgen.py (d), one full sample), same session:")
    say("  parent commit: median %.1f ms of %s" % (pmed, fmt(pall, 1)))
    say("  this tree:     median %.1f ms of %s" % (tmed, fmt(tall, 1)))
    say("  this tree's median %s the parent's min-max spread [%.1f, %.1f] ms"
        % ("lies within" if lo <= tmed <= hi else ("lies below (faster than)" if tmed < lo else "LIES ABOVE"), lo, hi))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
