"""Rings (generate_patchnn --wrap) at the generator's size - guess = real = 13 x 144 x 256, patch 3 x 7 x 7 (development tool, not
a test).  HIP events around the C entry points on preallocated outputs, warm-up, median of `reps` with every repetition listed.

The pair is tools/perf_patchmatch.py's: `real` a smooth multi-scale random clip that drifts over t (it does not loop), the guess
`real` rolled by (0, 4, 7) plus N(0, 6) noise.
  1. hpvg_patch_vote_u8 against hpvg_patch_vote_wrap_u8 with rings t and thw (the field is the exact one of the padded guess).
  2. hpvg_patchmatch_u8 against hpvg_patchmatch_wrap_u8 (rings t / thw on the query's side, then on the key's side), warm
     start, pm_iters 4; the ring forms see the padded guess, i.e. more patches, and the counts are printed beside the times.
  3. One full default sample with and without --wrap t under both searches, with the coherence, completeness and
     seam_coherence (rings t) that `evaluate --wrap t` computes for each.
With --existing only the entry points that every commit has are timed (hpvg_patchmatch_u8 warm start pm_iters 4,
hpvg_patch_vote_u8, hpvg_patchnn_u8), one `name: median` line each: run it on the parent commit and on this tree in one
session, then --compare parent.txt tree.txt copies both in and says where this tree's median lies in the parent's min-max
spread widened by 2 %.
usage: python tools/perf_patchwrap.py [out.txt] [--reps N] [--existing] [--no-sample] [--append] [--compare parent.txt tree.txt]"""
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
reps = int((flag("--reps", 1) or [7])[0])
existing, no_sample, append = flag("--existing"), flag("--no-sample"), flag("--append")
out_path = argv[0] if argv else None
T, H, W, PATCH = 13, 144, 256, (3, 7, 7)
PM_ITERS = 4
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def finish():
    if out_path:
        with open(out_path, "a" if append else "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)


if compare:
    def parse(path):
        found = {}
        with open(path) as f:
            for ln in f:
                m = re.match(r"(hpvg_\w+)[^:]*: median ([0-9.]+) ms of \[(.*)\]", ln)
                if m:
                    found[m.group(1)] = (ln.strip(), float(m.group(2)), [float(v) for v in m.group(3).split(",")])
        return found
    parent, tree = parse(compare[0]), parse(compare[1])
    say("the existing entry points, parent commit and this tree in one session (tools/perf_patchwrap.py --existing):")
    for name in sorted(parent):
        (pl, _, pall), (tl, tmed, _) = parent[name], tree[name]
        lo, hi = min(pall) * 0.98, max(pall) * 1.02
        say("  parent commit: " + pl)
        say("  this tree:     " + tl)
        say("  %s: this tree's median %.3f ms %s the parent's min-max spread widened by 2 %% [%.3f, %.3f] ms"
            % (name, tmed, "lies within" if lo <= tmed <= hi else ("lies below (faster than)" if tmed < lo else "LIES ABOVE"), lo, hi))
    finish()

dev = torch.device("cuda")


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
I3 = ctypes.c_int * 3
pa, one = I3(*PATCH), I3(1, 1, 1)
D = 3 * PATCH[0] * PATCH[1] * PATCH[2]


def grid_of(shape):
    return tuple(s - p + 1 for s, p in zip(shape, PATCH))


def count(shape):
    g = grid_of(shape)
    return g[0] * g[1] * g[2]


def run_pm(q, r, init, qwrap=None, rwrap=None, outs=None):
    """One warm-started search of pm_iters 4 through the C entry point; the plain one when both flag sets are None."""
    qs, rs = tuple(q.shape[:3]), tuple(r.shape[:3])
    if outs is None:
        n = count(qs)
        ws = torch.empty(hplib.call("hpvg_patchmatch_ws_bytes", *qs, *rs, pa), dtype=torch.uint8, device=dev)
        outs = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), ws)
    d2, nn, ws = outs
    if qwrap is None and rwrap is None:
        def fn():
            hplib.call("hpvg_patchmatch_u8", hplib.ptr(q), *qs, hplib.ptr(r), *rs, pa, None, hplib.ptr(init), PM_ITERS, 0, hplib.ptr(d2),
                       hplib.ptr(nn), None, hplib.ptr(ws), ws.numel(), hplib.stream())
    else:
        qw, rw = (None if f is None else I3(*f) for f in (qwrap, rwrap))

        def fn():
            hplib.call("hpvg_patchmatch_wrap_u8", hplib.ptr(q), *qs, hplib.ptr(r), *rs, pa, qw, rw, None, hplib.ptr(init), PM_ITERS, 0,
                       hplib.ptr(d2), hplib.ptr(nn), None, hplib.ptr(ws), ws.numel(), hplib.stream())
    return fn, outs


# the warm start of every search: the exact field of a slightly perturbed guess
warm = ops.patch_nn(guess2, real, PATCH)[1].reshape(-1).contiguous()
fn_pm, _ = run_pm(guess, real, warm)
med_pm, ms_pm = timed(fn_pm, 2, reps)
nn_plain = ops.patch_nn(guess, real, PATCH)[1].reshape(-1).contiguous()
out_plain = torch.empty_like(guess)


def vote_plain():
    hplib.call("hpvg_patch_vote_u8", hplib.ptr(real), T, H, W, hplib.ptr(nn_plain), T, H, W, pa, one, one, hplib.ptr(guess),
               hplib.ptr(out_plain), hplib.stream())


med_v, ms_v = timed(vote_plain, 2, reps)

if existing:
    ws = torch.empty(hplib.call("hpvg_patchnn_ws_bytes", T, H, W, T, H, W, pa, one, one), dtype=torch.uint8, device=dev)
    d2_out, nn_out = torch.empty(count((T, H, W)), dtype=torch.int32, device=dev), torch.empty(count((T, H, W)), dtype=torch.int32, device=dev)

    def exact():
        hplib.call("hpvg_patchnn_u8", hplib.ptr(guess), T, H, W, hplib.ptr(real), T, H, W, pa, one, one, hplib.ptr(d2_out),
                   hplib.ptr(nn_out), hplib.ptr(ws), ws.numel(), hplib.stream())
    med_e, ms_e = timed(exact, 1, reps)
    say("hpvg_patchmatch_u8 (warm start, pm_iters %d, %s vs %s): median %.3f ms of %s" % (PM_ITERS, (T, H, W), (T, H, W), med_pm, fmt(ms_pm)))
    say("hpvg_patch_vote_u8 (%s from %s): median %.3f ms of %s" % ((T, H, W), (T, H, W), med_v, fmt(ms_v)))
    say("hpvg_patchnn_u8 (one direction, %s vs %s): median %.3f ms of %s" % ((T, H, W), (T, H, W), med_e, fmt(ms_e)))
    finish()

say("patchwrap perf: guess = real = %s, patch %s, D = %d; the plain grids have %d patches" % ((T, H, W), PATCH, D, count((T, H, W))))
say("1. the vote (one thread per output voxel, %d voxels):" % (T * H * W))
say("  hpvg_patch_vote_u8                  (%7d patches vote): median %.3f ms of %s" % (count((T, H, W)), med_v, fmt(ms_v)))
for axes in ("t", "thw"):
    wrap = generate_patchnn.parse_wrap_axes(axes)
    padded = generate_patchnn.patchnn_wrap_pad(guess, PATCH, wrap)
    nn_ring = ops.patch_nn(padded, real, PATCH)[1].reshape(-1).contiguous()
    out_ring, wr = torch.empty_like(guess), I3(*wrap)

    def vote_ring():
        hplib.call("hpvg_patch_vote_wrap_u8", hplib.ptr(real), T, H, W, hplib.ptr(nn_ring), T, H, W, pa, one, wr, hplib.ptr(guess),
                   hplib.ptr(out_ring), hplib.stream())
    med, ms = timed(vote_ring, 2, reps)
    say("  hpvg_patch_vote_wrap_u8 rings %-3s   (%7d patches vote): median %.3f ms of %s  (x%.2f of the plain vote; patches x%.2f)"
        % (axes, nn_ring.numel(), med, fmt(ms), med / med_v, nn_ring.numel() / count((T, H, W))))

say("2. PatchMatch, warm start (the exact field of a perturbed guess, resized onto the ring's grid), pm_iters %d:" % PM_ITERS)
say("  hpvg_patchmatch_u8                               (%7d query patches): median %.3f ms of %s" % (count((T, H, W)), med_pm, fmt(ms_pm)))
fn0, _ = run_pm(guess, real, warm, (0, 0, 0), (0, 0, 0))
med0, ms0 = timed(fn0, 2, reps)
say("  hpvg_patchmatch_wrap_u8 no ring                  (%7d query patches): median %.3f ms of %s  (x%.2f)"
    % (count((T, H, W)), med0, fmt(ms0), med0 / med_pm))
for axes in ("t", "thw"):
    wrap = generate_patchnn.parse_wrap_axes(axes)
    padded = generate_patchnn.patchnn_wrap_pad(guess, PATCH, wrap)
    pgrid, rgrid = grid_of(padded.shape[:3]), grid_of((T, H, W))
    init = generate_patchnn.patchnn_field_resize(warm, rgrid, rgrid, pgrid, rgrid).reshape(-1).contiguous()
    fn, _ = run_pm(padded, real, init, qwrap=wrap)
    med, ms = timed(fn, 2, reps)
    say("  hpvg_patchmatch_wrap_u8 query rings %-3s (forward) (%7d query patches): median %.3f ms of %s  (x%.2f; patches x%.2f)"
        % (axes, count(padded.shape[:3]), med, fmt(ms), med / med_pm, count(padded.shape[:3]) / count((T, H, W))))
    rinit = ops.patch_nn(real, padded, PATCH)[1].reshape(-1).contiguous()
    fn, _ = run_pm(real, padded, rinit, rwrap=wrap)
    med, ms = timed(fn, 2, reps)
    say("  hpvg_patchmatch_wrap_u8 key rings %-3s   (reverse) (%7d query patches): median %.3f ms of %s  (x%.2f)"
        % (axes, count((T, H, W)), med, fmt(ms), med / med_pm))

if not no_sample:
    sizes = generate_patchnn.patchnn_pyramid_sizes((T, H, W), 0.75, 16, PATCH)
    pyramid = (sizes,) + generate_patchnn.patchnn_real_levels(real, sizes)
    ring = (1, 0, 0)
    say("3. one full sample, defaults (%d levels %s ... %s, 10 steps per level, alpha 0.005); seam_coherence is evaluate --wrap t's, "
        "over the %d patches that cross the t seam.  The exact search sees (T + 2) / T = 15 / 13 = x1.154 as many guess patches "
        "with --wrap t, in both of a step's searches, so x1.15 is the cost to expect:" % (len(sizes), sizes[0], sizes[-1], 2 * 138 * 250))
    seam_idx, _ = evaluate.seam_patches((T, H, W), PATCH, (1, 1, 1), ring)
    seam_sel = torch.from_numpy(seam_idx).to(device=dev, dtype=torch.int32)
    for search in ("exact", "patchmatch"):
        base = None
        for wrap in (None, ring):
            kw = {"search": search} if search == "patchmatch" else {}
            if wrap is not None:
                kw["wrap"] = wrap
            keep = []

            def sample():
                keep[:] = [generate_patchnn.patchnn_synthesize(real, None, PATCH, 0.75, 16, 10, 0.75, 0.005, 0, 1, pyramid, **kw)[0]]
            med_s, ms_s = timed(sample, 1 if search == "patchmatch" else 0, 3 if search == "patchmatch" else 1)
            base = base or med_s
            coh = evaluate.patch_score(ops.patch_nn(keep[0], real, PATCH)[0], D)
            com = evaluate.patch_score(ops.patch_nn(real, keep[0], PATCH)[0], D)
            d2s = ops.patch_nn_subset(generate_patchnn.patchnn_wrap_pad(keep[0], PATCH, ring), real, PATCH, seam_sel, None)[0]
            seam = evaluate.patch_score(d2s.reshape(-1)[seam_sel.long()], D)
            say("  search %-10s %-9s: median %.1f ms of %s (x%.3f); coherence %.6f completeness %.6f seam_coherence %.6f"
                % (search, "--wrap t" if wrap else "no ring", med_s, fmt(ms_s, 1), med_s / base, coh, com, seam))
finish()
