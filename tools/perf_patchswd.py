"""The sliced Wasserstein patch distance (hpvg_patchproj_hist_u8 + hpvg_hist_w1_i32) at the benchmarked size - a 13 x 144 x 256
sample against a 13 x 144 x 256 real volume, patch 3 x 7 x 7, dense, P = 512 directions - against a torch baseline for the same
result over the packed fp32 patch matrix: matmul with the directions, then per-direction sort or bincount, whichever is faster
(development tool, not a test).  HIP events, two warm-ups, median of `reps`.  The HBM rate is the 8.0 TB/s of the MI355X's
specification.  usage: python tools/perf_patchswd.py [out.txt] [reps] [T H W] [P]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import evaluate, ops  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, H, W = [int(a) for a in sys.argv[3:6]] if len(sys.argv) > 5 else (13, 144, 256)
P = int(sys.argv[6]) if len(sys.argv) > 6 else 512
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


def patch_matrix(vol):
    """fp32 [N][D] patch matrix of a uint8 [T][H][W][3] volume, centred like the kernel's and in its k order (dt, dy, dx, c)."""
    v = vol.to(torch.float32) - 128.0
    p = v.unfold(0, PATCH[0], 1).unfold(1, PATCH[1], 1).unfold(2, PATCH[2], 1)   # [nT][nY][nX][3][pt][ph][pw]
    return p.permute(0, 1, 2, 4, 5, 6, 3).reshape(-1, 3 * PATCH[0] * PATCH[1] * PATCH[2]).contiguous()


torch.manual_seed(0)
sample = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
real = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
N, _, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
NB = ops.patch_proj_bins(PATCH)
dirs_np = evaluate.swd_directions(P, D, 0)
dirs = torch.from_numpy(dirs_np).to(dev)
I3 = ctypes.c_int * 3
pa, one = I3(*PATCH), I3(1, 1, 1)
ws_bytes = hplib.call("hpvg_patchproj_ws_bytes", T, H, W, pa, one, P)
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
hist_s = torch.empty(P, NB, dtype=torch.int32, device=dev)
hist_r = torch.empty(P, NB, dtype=torch.int32, device=dev)
Dp = (D + 63) // 64 * 64
say("patch SWD perf: sample %s vs real %s, patch %s dense, P = %d directions: N = %d per volume, D = %d, NB = %d bins"
    % ((T, H, W), (T, H, W), PATCH, P, N, D, NB))
say("  per volume: %.3e multiply-add ops (2 N P D), %.3e histogram increments (N P), %.1f MB of packed int8 patches, %.1f MB of histogram"
    % (2.0 * N * P * D, float(N) * P, N * Dp / 1e6, P * NB * 4 / 1e6))


def hist_into(vol, hist):
    hplib.call("hpvg_patchproj_hist_u8", hplib.ptr(vol), T, H, W, pa, one, hplib.ptr(dirs), P, hplib.ptr(hist), hplib.ptr(ws), ws_bytes,
               hplib.stream())


med_a, all_a = timed(lambda: hist_into(sample, hist_s), 2, reps)
say("(a) hpvg_patchproj_hist_u8 (patch pack + direction pack + clear + i8 MFMA projection histogram), one volume: median %.2f ms of %s"
    % (med_a, ["%.2f" % m for m in all_a]))
say("    = %.2f G increments/s; the packed patches alone at this time are %.1f GB/s = %.2f %% of the %.1f TB/s HBM rate"
    % (float(N) * P / med_a / 1e6, N * Dp / med_a / 1e6, 100.0 * N * Dp / (med_a / 1e3) / HBM_PEAK, HBM_PEAK / 1e12))
hist_into(real, hist_r)
num = [None]


def w1():
    num[0] = ops.hist_w1(hist_s, N, hist_r, N)


med_b, all_b = timed(w1, 2, reps)
say("(b) hpvg_hist_w1_i32 (%d workgroups, %.1f MB of histograms read): median %.3f ms of %s = %.1f GB/s"
    % (P, 2 * P * NB * 4 / 1e6, med_b, ["%.3f" % m for m in all_b], 2 * P * NB * 4 / med_b / 1e6))
swd = evaluate.swd_score(num[0].cpu(), N, N, dirs_np)
say("    swd of two volumes of random bytes: %.6f" % swd)

Xs, Xr = patch_matrix(sample), patch_matrix(real)
St = dirs.to(torch.float32).t().contiguous()
offs = (torch.arange(P, device=dev, dtype=torch.int64) * NB + 128 * D)[None, :]


def base_sort(X):
    return torch.matmul(X, St).t().contiguous().sort(dim=1).values


def base_bincount(X):
    return torch.bincount((torch.matmul(X, St).to(torch.int64) + offs).reshape(-1), minlength=P * NB)


med_s, all_s = timed(lambda: base_sort(Xs), 2, reps)
med_c, all_c = timed(lambda: base_bincount(Xs), 2, reps)
say("(c) torch on the packed fp32 patch matrix (%.1f MB), one volume: matmul + per-direction sort: median %.2f ms of %s"
    % (Xs.numel() * 4 / 1e6, med_s, ["%.2f" % m for m in all_s]))
say("    matmul + bincount over all directions: median %.2f ms of %s" % (med_c, ["%.2f" % m for m in all_c]))
best = min(med_s, med_c)
say("    hand-written kernel over the faster baseline (%s): x%.2f" % ("sort" if med_s <= med_c else "bincount", best / med_a))
same = torch.equal(base_bincount(Xs).reshape(P, NB), hist_s.to(torch.int64))
w1_sort = (base_sort(Xs).double() - base_sort(Xr).double()).abs().sum(1) * N   # equal counts: N^2 W1 = N sum |sorted a - sorted b|
say("agreement: histogram equal to the bincount baseline: %s; W1 numerators equal to the sort baseline: %s"
    % (same, torch.equal(w1_sort.to(torch.int64), num[0])))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
