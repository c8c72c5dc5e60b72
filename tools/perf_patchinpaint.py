"""Patch inpainting's search at the benchmarked size - 13 x 144 x 256 volumes, patch 3 x 7 x 7, a box hole of 46 x 81 over every
frame (10 % of the voxels) - (development tool, not a test): hpvg_patchnn_u8 on the full grids, hpvg_patchnn_subset_u8 on the
hole's lists (queries: the patches that overlap the hole; keys: the patches that avoid it; the C entry points on preallocated
outputs and one workspace, so the two differ by the compaction alone), and one full sample of generate_patchnn.patchnn_inpaint
with the program's defaults.  HIP events, warm-up, median of `reps`.  The subset search must be faster than the full one.  With
--compare, the `hpvg_patchnn_u8` lines of two tools/perf_patchnn.py outputs (the parent commit's and this tree's, taken in the
same session) are copied in and the tree's median is checked against the parent's own min-max spread widened by 2 %.
usage: python tools/perf_patchinpaint.py [out.txt] [reps] [--compare parent_patchnn.txt tree_patchnn.txt]"""
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
HOLE = (49, 95, 87, 168)   # rows, columns: 46 x 81, centred
dev = torch.device("cuda")
lines = []
failed = []


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
mask = torch.zeros(T, H, W, dtype=torch.bool, device=dev)
mask[:, HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = True
Nq, Nr, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
count = ops.patch_mask_count(mask.to(torch.uint8), PATCH).reshape(-1)
qsel = torch.nonzero(count > 0).reshape(-1).to(torch.int32)
rsel = torch.nonzero(count == 0).reshape(-1).to(torch.int32)
nq, nr = qsel.numel(), rsel.numel()
macs_full, macs_sub = float(Nq) * Nr * D, float(nq) * nr * D
say("patchinpaint perf: volumes %s, patch %s dense: N = %d patches, D = %d; hole %d x %d over every frame = %.1f %% of the voxels: "
    "%d queries (%.1f %% of the patches), %d keys (%.1f %%)"
    % ((T, H, W), PATCH, Nq, D, HOLE[1] - HOLE[0], HOLE[3] - HOLE[2], 100.0 * float(mask.sum()) / mask.numel(), nq, 100.0 * nq / Nq,
       nr, 100.0 * nr / Nr))

I3 = ctypes.c_int * 3
pa, one = I3(*PATCH), I3(1, 1, 1)
full_bytes = hplib.call("hpvg_patchnn_ws_bytes", T, H, W, T, H, W, pa, one, one)
sub_bytes = hplib.call("hpvg_patchnn_subset_ws_bytes", T, H, W, T, H, W, pa, one, one, nq, nr)
ws = ops.workspace(full_bytes, dev)
d2_out = torch.empty(Nq, dtype=torch.int32, device=dev)
nn_out = torch.empty(Nq, dtype=torch.int32, device=dev)


def full():
    hplib.call("hpvg_patchnn_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(d2_out), hplib.ptr(nn_out),
               hplib.ptr(ws), ws.numel(), hplib.stream())


def subset():
    hplib.call("hpvg_patchnn_subset_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(qsel), nq,
               hplib.ptr(rsel), nr, hplib.ptr(d2_out), hplib.ptr(nn_out), hplib.ptr(ws), ws.numel(), hplib.stream())


med_f, ms_f = timed(full, 2, reps)
say("(a) hpvg_patchnn_u8 on the full grids (pack + i8 MFMA min + unpack): median %.1f ms of %s; %.3e multiply-adds, workspace %.1f MB"
    % (med_f, fmt(ms_f), macs_full, full_bytes / 1e6))
med_s, ms_s = timed(subset, 2, reps)
say("(b) hpvg_patchnn_subset_u8 on the hole's lists (gather pack + the same min kernel + fill + scatter): median %.2f ms of %s; "
    "%.3e multiply-adds, workspace %.1f MB" % (med_s, fmt(ms_s, 2), macs_sub, sub_bytes / 1e6))
verdict = "the subset search is faster than the full search" if med_s < med_f else "THE SUBSET SEARCH IS NOT FASTER"
say("    multiply-adds (b) / (a) = %.3f, time (b) / (a) = %.3f: %s" % (macs_sub / macs_full, med_s / med_f, verdict))
if not med_s < med_f:
    failed.append("subset search not faster")
# the result the timing stands for: the full search's rows, where the two must agree (every key selected for this check)
full()
want = d2_out.clone()
hplib.call("hpvg_patchnn_subset_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(qsel), nq, None, 0,
           hplib.ptr(d2_out), hplib.ptr(nn_out), hplib.ptr(ws), ws.numel(), hplib.stream())
same = bool((d2_out[qsel.long()] == want[qsel.long()]).all()) and int((d2_out >= 0).sum()) == nq
say("    queries only (every key): d2 of the %d selected rows %s the full search's, %d rows at -1"
    % (nq, "equals" if same else "DIFFERS FROM", int((d2_out < 0).sum())))
if not same:
    failed.append("subset result differs")

sizes = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH)
levels, keys = generate_patchnn.patchnn_real_levels(real, sizes)
plan = generate_patchnn.patchnn_inpaint_plan(mask, sizes, PATCH)
pyramid = (sizes, levels, keys, plan)
index = [0]


def sample():
    index[0] += 1
    return generate_patchnn.patchnn_inpaint(real, mask, PATCH, 0.75, 16, 10, 0.75, 0, index[0], pyramid)


med_i, ms_i = timed(sample, 1, reps)
# ops.patch_nn_subset checks both lists on every call (one device reduction and its host read each), so (c) holds two host
# synchronisations per step; timed apart on the finest level's lists
fin = plan[-1]
med_k, ms_k = timed(lambda: (ops._patch_sel(fin["qsel"], "qsel", Nq, real.device), ops._patch_sel(fin["rsel"], "rsel", Nr, real.device)), 2, reps)
steps = 10 * len(sizes)
work = sum(float(lv["qsel"].numel()) * ((lv["rsel_first"].numel() if l else 0) + (9 if l else 10) * lv["rsel"].numel()) * D
           for l, lv in enumerate(plan))
say("(c) one full --mask sample, defaults (ratio 0.75, min size 16: %d levels %s ... %s; 10 steps per level, one subset search, one "
    "vote and one select per step): median %.1f ms of %s; %.3e multiply-adds (profiles/patchgen_perf.txt (d): an unconditional "
    "sample with its two full searches per step)" % (len(sizes), sizes[0], sizes[-1], med_i, fmt(ms_i), work))
say("    (c) includes ops.patch_nn_subset's check of both lists on every call, two host synchronisations per step, %d per sample: "
    "at the finest level (%d + %d entries) median %.3f ms of %s per step" % (2 * steps, fin["qsel"].numel(), fin["rsel"].numel(),
                                                                          med_k, fmt(ms_k, 3)))

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
    if tmed > hi:
        failed.append("existing path slower")
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
if failed:
    raise SystemExit("perf_patchinpaint: " + "; ".join(failed))
