"""The patch nearest-neighbour generator's pieces at the benchmarked size - a 13 x 144 x 256 guess against a 13 x 144 x 256 real
volume, patch 3 x 7 x 7, dense (development tool, not a test): one hpvg_patchnn_u8 direction, one hpvg_patchnn_weighted_u8 pass
(the C entry points, so the two differ by the kernels alone; ops.patch_nn_weighted's weight check is timed apart), one
ops.patch_vote, and one full sample of generate_patchnn.patchnn_synthesize with the program's defaults.  HIP events, warm-up, median
of `reps`.  With --compare, the `hpvg_patchnn_u8` lines of two tools/perf_patchnn.py outputs (the parent commit's and this
tree's, taken in the same session) are copied in and the tree's median is checked against the parent's own min-max spread
widened by 2 %.
usage: python tools/perf_patchgen.py [out.txt] [reps] [--compare parent_patchnn.txt tree_patchnn.txt]"""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import generate_patchnn, ops  # noqa: E402

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
I8_PEAK = 5.0e15   # multiply-add ops / s, dense (tools/perf_patchnn.py)
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


def fmt(ms, digits=1):
    return "[" + ", ".join("%.*f" % (digits, m) for m in ms) + "]"


torch.manual_seed(0)
guess = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
real = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
Nq, Nr, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
macs = float(Nq) * Nr * D
weights = torch.rand(Nr, device=dev) * 3.75 + 0.25
say("patchgen perf: guess %s vs real %s, patch %s dense: Nq = Nr = %d, D = %d, %.3e multiply-adds per search"
    % ((T, H, W), (T, H, W), PATCH, Nq, D, macs))

# (a) and (b) time the two C entry points on preallocated outputs and one workspace, so their difference is the kernels' alone;
# (b') is what ops.patch_nn_weighted adds on top: the finite-and-positive check of the weights (one reduction and its host read)
I3 = ctypes.c_int * 3
pa, one = I3(*PATCH), I3(1, 1, 1)
ws = ops.workspace(hplib.call("hpvg_patchnn_ws_bytes", T, H, W, T, H, W, pa, one, one), dev)
d2_out = torch.empty(Nq, dtype=torch.int32, device=dev)
sc_out = torch.empty(Nq, dtype=torch.float32, device=dev)
nn_out = torch.empty(Nq, dtype=torch.int32, device=dev)


def unweighted():
    hplib.call("hpvg_patchnn_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(d2_out), hplib.ptr(nn_out),
               hplib.ptr(ws), ws.numel(), hplib.stream())


def weighted():
    hplib.call("hpvg_patchnn_weighted_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(weights),
               hplib.ptr(sc_out), hplib.ptr(nn_out), hplib.ptr(ws), ws.numel(), hplib.stream())


med_u, ms_u = timed(unweighted, 2, reps)
say("(a) hpvg_patchnn_u8, one direction (pack + i8 MFMA min + unpack): median %.1f ms of %s = %.1f %% of the i8 dense peak"
    % (med_u, fmt(ms_u), 100.0 * 2 * macs / (med_u / 1e3) / I8_PEAK))
med_w, ms_w = timed(weighted, 2, reps)
say("(b) hpvg_patchnn_weighted_u8, one pass (the same launches, weighted epilogue): median %.1f ms of %s = %.1f %% of the i8 dense "
    "peak; x%.3f of (a)" % (med_w, fmt(ms_w), 100.0 * 2 * macs / (med_w / 1e3) / I8_PEAK, med_w / med_u))
med_c, ms_c = timed(lambda: bool((torch.isfinite(weights) & (weights > 0)).all()), 2, reps)
med_o, ms_o = timed(lambda: ops.patch_nn_weighted(guess, real, weights, PATCH), 2, reps)
say("(b') ops.patch_nn_weighted = (b) + the weight check (%d weights: median %.3f ms of %s) + two output allocations: median %.1f ms "
    "of %s" % (Nr, med_c, fmt(ms_c, 3), med_o, fmt(ms_o)))
# static facts of the compiled gfx950 kernels (hipcc -S, instructions outside / inside the K loop per 128 x 128 column tile)
say("    where (b) - (a) comes from, per column tile and wave, counted in the compiled kernels: the K loop is the same 7 x 57 "
    "instructions (8 MFMAs per step); outside it the unweighted kernel issues 637 (605 vector: per accumulator element shift, "
    "subtract, min, compare, 2 selects, plus 64 accumulator reads and 128 accumulator clears) and the weighted one 703 (641 vector: "
    "per element add of the row norm, shift, subtract, v_cvt_f32_i32, half a v_pk_mul_f32, fp32 compare, 2 selects, plus 140 moves "
    "that clear the accumulators and pair the operands of the packed multiply; 8 ds_read_b128 of the row norms, 7 more waits and 6 "
    "nops): 1102 against 1036 issued instructions = x1.064, at the same two waves per SIMD (214 / 232 registers).  The epilogue is "
    "vector-ALU work that this wave's MFMAs wait for; the SIMD's other wave can issue MFMAs meanwhile, so the measured ratio stays a "
    "little below the instruction ratio.  A first form that selected +inf per "
    "element for padded columns compiled to 64 exec-mask branches per tile, each waiting on its own LDS read: x1.237 (148.6 ms)")
nn = ops.patch_nn(guess, real, PATCH)[1]
med_v, ms_v = timed(lambda: ops.patch_vote(real, nn, PATCH, (T, H, W), guess), 2, reps)
votes = float(T * H * W) * PATCH[0] * PATCH[1] * PATCH[2]
say("(c) ops.patch_vote (%d voxels, up to %d covering patches each): median %.3f ms of %s = %.1f G votes/s"
    % (T * H * W, PATCH[0] * PATCH[1] * PATCH[2], med_v, fmt(ms_v, 3), votes / med_v / 1e6))

sizes = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH)
pyramid = (sizes,) + generate_patchnn.patchnn_real_levels(real, sizes)
index = [0]


def sample():
    index[0] += 1
    return generate_patchnn.patchnn_synthesize(real, None, PATCH, 0.75, 16, 10, 0.75, 0.005, 0, index[0], pyramid)


med_s, ms_s = timed(sample, 1, reps)
searches = sum(2 * 10 * float(s[0] - 2) * (s[1] - 6) * (s[2] - 6) * (s[0] - 2) * (s[1] - 6) * (s[2] - 6) * D for s in sizes)
say("(d) one full sample, defaults (ratio 0.75, min size 16: %d levels %s ... %s; 10 steps per level, alpha 0.005, i.e. two "
    "searches and one vote per step): median %.1f ms of %s; %.3e multiply-adds = %.1f %% of the i8 dense peak end to end"
    % (len(sizes), sizes[0], sizes[-1], med_s, fmt(ms_s), searches, 100.0 * 2 * searches / (med_s / 1e3) / I8_PEAK))

if compare:
    def line(path):
        with open(path) as f:
            for ln in f:
                if ln.startswith("hpvg_patchnn_u8"):
                    m = re.search(r"median ([0-9.]+) ms of \[(.*)\]", ln)
                    return ln.strip(), float(m.group(1)), [float(v.strip(" '")) for v in m.group(2).split(",")]
        raise SystemExit("no hpvg_patchnn_u8 line in %s" % path)
    pl, pmed, pall = line(compare[0])
    tl, tmed, tall = line(compare[1])
    lo, hi = min(pall) * 0.98, max(pall) * 1.02
    say("the existing path (tools/perf_patchnn.py, both directions), same session:")
    say("  parent commit: " + pl)
    say("  this tree:     " + tl)
    say("  this tree's median %.1f ms %s the parent's min-max spread widened by 2 %% [%.1f, %.1f] ms"
        % (tmed, "lies within" if lo <= tmed <= hi else ("lies below (faster than)" if tmed < lo else "LIES ABOVE"), lo, hi))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
