"""The deterministic PatchMatch search (hpvg_patchmatch_u8) against the exhaustive one at the generator's size - a T x 144 x 256
guess against a T x 144 x 256 real volume, patch 3 x 7 x 7, dense (development tool, not a test).  HIP events around the C entry
points on preallocated outputs, warm-up, median of `reps` with every repetition listed.

The pair is synthetic and seeded: `real` is a smooth multi-scale random clip that drifts over t, with mild noise; the guess is
`real` rolled by (0, 4, 7) plus N(0, 6) noise, i.e. a volume whose patches mostly have a near copy among the keys, as a
generator's guess has.  For pm_iters in 1, 2, 4, 8, 16, from the hash start and from a warm start, plain and weighted:
the time of one search and mean d2 / the exact search's mean d2 on the same pair (weighted: mean score / exact mean score).
The warm start is the exact field of a slightly perturbed guess (guess + N(0, 2)); with --one-exact (the 65-frame run, where an
exact search takes seconds) the only exact run is the plain one of the pair itself, the warm start is the 16-iteration
PatchMatch field of the perturbed guess, and the weighted ratios are taken against the 16-iteration hash-start result.
Then one full sample of generate_patchnn.patchnn_synthesize in both modes with the program's defaults, and the coherence and
completeness that `evaluate` computes for each (evaluate.patch_score of the two exact directions).
With --compare, the `hpvg_patchnn_u8` lines of two tools/perf_patchnn.py outputs (parent commit, this tree) are copied in.
usage: python tools/perf_patchmatch.py [out.txt] [--frames T] [--reps N] [--one-exact] [--no-sample] [--append]
                                       [--compare parent_patchnn.txt tree_patchnn.txt]"""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import evaluate, generate_patchnn, ops  # noqa: E402

argv = sys.argv[1:]


def flag(name, n=0):
    if name not in argv:
        return None
    k = argv.index(name)
    vals = argv[k + 1:k + 1 + n]
    del argv[k:k + 1 + n]
    return vals if n else True


compare = flag("--compare", 2)
T = int((flag("--frames", 1) or [13])[0])
reps = int((flag("--reps", 1) or [5])[0])
one_exact, no_sample, append = flag("--one-exact"), flag("--no-sample"), flag("--append")
out_path = argv[0] if argv else None
H, W, PATCH = 144, 256, (3, 7, 7)
ITERS = (1, 2, 4, 8, 16)
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


def fmt(ms, digits=2):
    return "[" + ", ".join("%.*f" % (digits, m) for m in ms) + "]"


def clip(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    vol = torch.zeros(1, 3, T, H, W)
    for cells, amp in ((4, 50.0), (12, 30.0), (36, 14.0)):
        coarse = torch.randn(1, 3, max(T // 4, 2), cells * 9 // 16 + 2, cells + 2, generator=g)
        vol += amp * torch.nn.functional.interpolate(coarse, size=(T, H, W), mode="trilinear", align_corners=True)
    vol += 2.0 * torch.randn(vol.shape, generator=g)
    return (128 + vol).round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 3, 0).contiguous()


def noisy(vol, sigma, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (vol.float() + sigma * torch.randn(vol.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)


real_h = clip(0)
guess_h = noisy(torch.roll(real_h, (4, 7), (1, 2)), 6.0, 1)
real, guess, guess2 = real_h.to(dev), guess_h.to(dev), noisy(guess_h, 2.0, 2).to(dev)
Nq, Nr, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
NRAD = max(T - PATCH[0] + 1, H - PATCH[1] + 1, W - PATCH[2] + 1).bit_length()   # radii R, R / 2, ... 1 of the random search
say("patchmatch perf: guess %s vs real %s, patch %s dense: Nq = Nr = %d, D = %d; exhaustive: %.3e multiply-adds per search; "
    "PatchMatch: at most 6 + %d candidates of D bytes per patch and iteration = %.3e byte pairs per iteration (%.0fx fewer)"
    % ((T, H, W), (T, H, W), PATCH, Nq, D, float(Nq) * Nr * D, NRAD, float(Nq) * (6 + NRAD) * D, Nr / (6.0 + NRAD)))

I3 = ctypes.c_int * 3
pa, one = I3(*PATCH), I3(1, 1, 1)
ws = torch.empty(max(hplib.call("hpvg_patchnn_ws_bytes", T, H, W, T, H, W, pa, one, one),
                     hplib.call("hpvg_patchmatch_ws_bytes", T, H, W, T, H, W, pa)), dtype=torch.uint8, device=dev)
d2_out = torch.empty(Nq, dtype=torch.int32, device=dev)
sc_out = torch.empty(Nq, dtype=torch.float32, device=dev)
nn_out = torch.empty(Nq, dtype=torch.int32, device=dev)


def exact(q, r, w=None):
    if w is None:
        hplib.call("hpvg_patchnn_u8", hplib.ptr(q), T, H, W, hplib.ptr(r), T, H, W, pa, one, one, hplib.ptr(d2_out), hplib.ptr(nn_out),
                   hplib.ptr(ws), ws.numel(), hplib.stream())
    else:
        hplib.call("hpvg_patchnn_weighted_u8", hplib.ptr(q), T, H, W, hplib.ptr(r), T, H, W, pa, one, one, hplib.ptr(w), hplib.ptr(sc_out),
                   hplib.ptr(nn_out), hplib.ptr(ws), ws.numel(), hplib.stream())


def pm(q, r, iters, w=None, init=None, seed=0):
    hplib.call("hpvg_patchmatch_u8", hplib.ptr(q), T, H, W, hplib.ptr(r), T, H, W, pa, hplib.ptr(w), hplib.ptr(init), iters, seed,
               hplib.ptr(d2_out), hplib.ptr(nn_out), hplib.ptr(sc_out) if w is not None else None, hplib.ptr(ws), ws.numel(),
               hplib.stream())


def mean(t):
    return float(t.to(torch.float64).mean())


ex_reps = 1 if one_exact else reps
med_e, ms_e = timed(lambda: exact(guess, real), 0 if one_exact else 1, ex_reps)
exact_d2 = mean(d2_out)
say("exhaustive hpvg_patchnn_u8, one direction: median %.1f ms of %s; mean d2 %.1f" % (med_e, fmt(ms_e, 1), exact_d2))
if one_exact:
    pm(real, guess, 16)
    weights = generate_patchnn.patchnn_weights(d2_out.clone(), 0.005 * D * 255 * 255)
    pm(guess2, real, 16)
    warm = nn_out.clone()
    pm(guess, real, 16, weights)
    exact_sc, med_w = mean(sc_out), None
    say("one exact run only: the weights come from the 16-iteration PatchMatch of the reverse direction, the warm start is the "
        "16-iteration field of the perturbed guess, and the weighted ratios are against the 16-iteration hash-start score %.6f" % exact_sc)
else:
    exact(real, guess)
    weights = generate_patchnn.patchnn_weights(d2_out.clone(), 0.005 * D * 255 * 255)
    exact(guess2, real)
    warm = nn_out.clone()
    med_w, ms_w = timed(lambda: exact(guess, real, weights), 1, reps)
    exact_sc = mean(sc_out)
    say("exhaustive hpvg_patchnn_weighted_u8 (weights 1 / (m + alpha), alpha 0.005): median %.1f ms of %s; mean score %.6f"
        % (med_w, fmt(ms_w, 1), exact_sc))

say("hpvg_patchmatch_u8 (start launch + pm_iters launches); ratio = mean d2 (weighted: mean score) over the exhaustive search's:")
table = {}
for w, wname in ((None, "plain"), (weights, "weighted")):
    for init, sname in ((None, "hash start"), (warm, "warm start")):
        for it in ITERS:
            med, ms = timed(lambda: pm(guess, real, it, w, init), 1, reps)
            ratio = (mean(sc_out) / exact_sc) if w is not None else (mean(d2_out) / exact_d2)
            table[(wname, sname, it)] = (med, ratio)
            ref = med_e if w is None else med_w
            say("  %-8s %-10s pm_iters %2d: median %7.2f ms of %s  ratio %.4f%s"
                % (wname, sname, it, med, fmt(ms), ratio, "" if ref is None else "  (exhaustive / this = x%.1f)" % (ref / med)))
d = generate_patchnn.PM_ITERS
say("default pm_iters %d, warm start: plain ratio %.4f, weighted ratio %.4f (the issue's condition for keeping 4: <= 1.05 at the "
    "finest level); plain search %.2f ms (hash start) / %.2f ms (warm start) against the exhaustive %.1f ms: %s"
    % (d, table[("plain", "warm start", d)][1], table[("weighted", "warm start", d)][1], table[("plain", "hash start", d)][0],
       table[("plain", "warm start", d)][0], med_e,
       "FASTER" if max(table[("plain", "hash start", d)][0], table[("plain", "warm start", d)][0]) < med_e else "NOT FASTER"))

if not no_sample:
    sizes = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH)
    pyramid = (sizes,) + generate_patchnn.patchnn_real_levels(real, sizes)
    for search in ("exact", "patchmatch"):
        kw = {"search": search} if search == "patchmatch" else {}
        keep = []

        def sample():
            keep[:] = [generate_patchnn.patchnn_synthesize(real, None, PATCH, 0.75, 16, 10, 0.75, 0.005, 0, 1, pyramid, **kw)[0]]
        med_s, ms_s = timed(sample, 0 if one_exact else 1, 1 if one_exact else 3)
        coh = evaluate.patch_score(ops.patch_nn(keep[0], real, PATCH)[0], D)
        com = evaluate.patch_score(ops.patch_nn(real, keep[0], PATCH)[0], D)
        say("one full sample, defaults (%d levels %s ... %s, 10 steps per level, alpha 0.005), search %-10s: median %.1f ms of %s; "
            "coherence %.6f completeness %.6f" % (len(sizes), sizes[0], sizes[-1], search, med_s, fmt(ms_s, 1), coh, com))

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
    say("the existing exhaustive path (tools/perf_patchnn.py, both directions), same session:")
    say("  parent commit: " + pl)
    say("  this tree:     " + tl)
    say("  this tree's median %.1f ms %s the parent's min-max spread widened by 2 %% [%.1f, %.1f] ms"
        % (tmed, "lies within" if lo <= tmed <= hi else ("lies below (faster than)" if tmed < lo else "LIES ABOVE"), lo, hi))
if out_path:
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n")
