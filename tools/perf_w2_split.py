"""Per-launch time of the two-axis Winograd conv (64 -> 64, forced with mode 5) on given shapes, with the cut hpvg_conv_w2_split
reports for them.  The cut is decided once per process: run it with HPVG_W2_SPLIT=0 and without, on the same GPU, and compare
(-> profiles/w2split_perf.txt).  Prints the median and the range of `batches` back-to-back batches of `reps` launches.
usage: python tools/perf_w2_split.py reps batches "B,T,H,W;B,T,H,W;..."  (development)"""
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hp_vae_gan_amd  # noqa: F401
from hp_vae_gan_amd import ops, lib as hplib

lib = hplib.load()
reps, batches = int(sys.argv[1]), int(sys.argv[2])


def bench(fn):
    fn(); fn(); torch.cuda.synchronize()
    times = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


print("HPVG_W2_SPLIT=%s" % os.environ.get("HPVG_W2_SPLIT", "(unset)"), flush=True)
lib.hpvg_conv_wino_config(5, -1)
for spec in sys.argv[3].split(";"):
    B, T, H, W = (int(v) for v in spec.split(","))
    x = torch.randn(B, 64, T, H, W, device="cuda")
    w = torch.randn(64, 64, 3, 3, 3, device="cuda") * 0.05
    cut = (ctypes.c_int * 4)()
    has = hasattr(lib, "hpvg_conv_w2_split") and lib.hpvg_conv_w2_split(B, 64, 64, T, H, W, 3, cut) == 0
    med, lo, hi = bench(lambda: ops.conv_fwd_raw(x, w, None))
    ntl = B * T * ((((H + 1) // 2) * ((W + 1) // 2) + 63) // 64)
    print("B=%d %dx%dx%d  tiles %d (%.2f rounds)  cut %s  %.1f us (%.1f - %.1f)  %.0f voxels/us" % (
        B, T, H, W, ntl, ntl / 256.0, list(cut) if has else "n/a", med, lo, hi, B * T * H * W / med), flush=True)
lib.hpvg_conv_wino_config(1, -1)
