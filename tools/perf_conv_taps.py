"""The tap-generic conv family (hpvg_convk_*, --ker-size 5) next to the tuned 3-tap DIRECT kernel on the same shapes, in one
process (development tool, not a test).  usage: python tools/perf_conv_taps.py [out.txt]

Per layer shape: forward, backward-data and weight gradient, HIP events around `REPS` launches after a warm-up, the median of
5 such windows; milliseconds per launch and TFLOP/s.  "alg" counts the conv's own flops, 2 B Cin Cout taps T H W; "exe" is
what the matrix cores execute for the 5-tap kernels: output channels rounded up to the 32-row MFMA tile, input channels to
the 2-deep MFMA step, positions to whole tiles (forward: TH x 36 positions per 14 x 32 outputs; time taps that fall outside
the volume are skipped and not counted).  The 3-tap yardstick is the direct implicit-GEMM kernel (hpvg_conv_wino_config(0),
hpvg_conv_bwd_weight_wino_config(0)): no Winograd form runs 5 taps, so that is the like-for-like instruction stream.
Acceptance (printed at the end): the 64 -> 64 forward at K = 5 reaches at least half the direct kernel's flop rate.

Then it/s of the last stage of a small train_video run with --ker-size 5 next to the same run with --ker-size 3: two runs per
tap side that differ in --niter only, the stage's time difference over the iteration difference (set-up and graph capture
cancel)."""
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import lib as hplib, ops, programs  # noqa: E402

DEV = "cuda"
FINEST, MID = (13, 144, 256), (5, 57, 102)
SHAPES = [(FINEST, 3, 64), (FINEST, 64, 64), (FINEST, 64, 3), (FINEST, 64, 1), (MID, 64, 64)]
B = 2
REPS = 5
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def bench(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    return statistics.median(window(fn) for _ in range(5))


def cdiv(a, b):
    return (a + b - 1) // b


def exe_fwd(K, Cin, Cout, T, H, W):
    """flops the forward kernel's MFMAs execute per sample (border time taps not subtracted)"""
    th = 512 // (32 + 2 * (K // 2))
    m = cdiv(Cout, 64) * 64 if Cout > 32 else 32
    return 2.0 * T * cdiv(H, th) * cdiv(W, 32) * 512 * m * (cdiv(Cin, 2) * 2) * K ** 3


def exe_wgrad(K, Cin, Cout, T, H, W):
    return 2.0 * T * cdiv(H, 4) * cdiv(W, 32) * 128 * (cdiv(Cout, 32) * 32) * (cdiv(Cin, 32) * 32) * K ** 3


def conv_rows():
    lib = hplib.load()
    rates = {}
    for sp, Ci, Co in SHAPES:
        T, H, W = sp
        torch.manual_seed(0)
        x = torch.rand(B, Ci, *sp, device=DEV) * 2 - 1
        dy = torch.rand(B, Co, *sp, device=DEV) * 2 - 1
        for K in (5, 3):
            w = (torch.rand(Co, Ci, K, K, K, device=DEV) * 2 - 1) * 0.05
            if K == 3:
                lib.hpvg_conv_wino_config(0, -1)
                lib.hpvg_conv_bwd_weight_wino_config(0)
            try:
                t = (bench(lambda: ops.conv_fwd_raw(x, w, None)), bench(lambda: ops.conv_fwd_raw(dy, w, None, flip=True)),
                     bench(lambda: ops.conv_bwd_weight_raw(dy, x, w.shape)))
            finally:
                if K == 3:
                    lib.hpvg_conv_wino_config(1, -1)
                    lib.hpvg_conv_bwd_weight_wino_config(1)
            alg = 2.0 * B * Ci * Co * K ** 3 * T * H * W
            exe = (B * exe_fwd(K, Ci, Co, T, H, W), B * exe_fwd(K, Co, Ci, T, H, W), B * exe_wgrad(K, Ci, Co, T, H, W)) if K == 5 else (alg,) * 3
            rates[(sp, Ci, Co, K)] = [alg / ms / 1e9 for ms in t]
            say("%-14s %3d -> %-3d K=%d %-8s fwd %8.3f ms %6.1f alg %6.1f exe | bwd-data %8.3f ms %6.1f alg %6.1f exe | wgrad %8.3f ms %6.1f alg %6.1f exe  TFLOP/s"
                % ("x".join(map(str, sp)), Ci, Co, K, "taps" if K == 5 else "direct",
                   t[0], alg / t[0] / 1e9, exe[0] / t[0] / 1e9, t[1], alg / t[1] / 1e9, exe[1] / t[1] / 1e9, t[2], alg / t[2] / 1e9,
                   exe[2] / t[2] / 1e9))
    for sp in (FINEST, MID):
        a, d = rates[(sp, 64, 64, 5)][0], rates[(sp, 64, 64, 3)][0]
        say("acceptance %s 64 -> 64 forward: K=5 %.1f TFLOP/s vs direct K=3 %.1f TFLOP/s = %.2f (needs >= 0.50): %s"
            % ("x".join(map(str, sp)), a, d, a / d, "met" if a >= 0.5 * d else "NOT met"))


def mt_rows():
    """The forward's M tiles per workgroup (hpvg_convk_fwd_mt_config): one against two against the size rule on the 64 -> 64
    layer at every level of the video pyramid, alternating in one process (median of 5 windows each)."""
    lib = hplib.load()
    levels = [(4, 18, 33), (4, 28, 51), (5, 45, 81), MID, (7, 72, 129), (7, 91, 162), (7, 114, 204), FINEST]
    for sp in levels:
        T, H, W = sp
        torch.manual_seed(0)
        x = torch.rand(B, 64, *sp, device=DEV) * 2 - 1
        w = (torch.rand(64, 64, 5, 5, 5, device=DEV) * 2 - 1) * 0.05
        tiles = B * T * cdiv(H, 14) * cdiv(W, 32)
        ms = {1: [], 2: []}
        try:
            for mode in (1, 2):
                lib.hpvg_convk_fwd_mt_config(mode)
                ops.conv_fwd_raw(x, w, None)
                ops.conv_fwd_raw(x, w, None)
            torch.cuda.synchronize()
            for _ in range(5):
                for mode in (1, 2):
                    lib.hpvg_convk_fwd_mt_config(mode)
                    ms[mode].append(window(lambda: ops.conv_fwd_raw(x, w, None)))
        finally:
            lib.hpvg_convk_fwd_mt_config(0)
        one, two = statistics.median(ms[1]), statistics.median(ms[2])
        alg = 2.0 * B * 64 * 64 * 125 * T * H * W
        say("M tiles per workgroup, 64 -> 64 K=5 fwd %-12s %5d spatial tiles: one %7.3f ms (%5.1f TFLOP/s)  two %7.3f ms (%5.1f)  size rule takes %s"
            % ("x".join(map(str, sp)), tiles, one, alg / one / 1e9, two, alg / two / 1e9, "two" if tiles > 256 else "one"))


def stage_seconds(clip, K, niter, run_dir):
    argv = ["--video-path", clip, "--run-dir", run_dir, "--niter", str(niter), "--print-interval", "1000", "--manualSeed", "3",
            "--min-size", "32", "--max-size", "64", "--img-size", "64", "--vae-levels", "1", "--ker-size", str(K), "--padd-size", str(K // 2)]
    ops._rng_states.clear()
    prog = programs.Program("video", argv)
    secs = []
    inner = prog.train_stage

    def timed(resume=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = inner(resume=resume)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        return tr
    prog.train_stage = timed
    prog.run()
    shape = tuple(prog.trainers[-1].netG.body[-1].head.conv.weight.shape)
    return secs, prog.opt.stop_scale, shape


def train_rows():
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        clip = os.path.join(d, "clip.npy")
        np.save(clip, rng.integers(0, 256, size=(24, 48, 64, 3), dtype=np.uint8))
        res = {}
        for K in (3, 5):
            lo, hi = 20, 80
            a, stop, shape = stage_seconds(clip, K, lo, os.path.join(d, "a%d" % K))
            b, _, _ = stage_seconds(clip, K, hi, os.path.join(d, "b%d" % K))
            res[K] = (hi - lo) / (b[-1] - a[-1])
            say("train_video --ker-size %d (nfc 64, 64-wide pyramid, last stage %d, head weight %s): %.1f it/s" % (K, stop, shape, res[K]))
        say("5-tap stage / 3-tap stage: %.2f x the time per iteration (125 / 27 = 4.63 of the conv flops is the expectation; the 3-tap "
            "stage runs Winograd kernels)" % (res[3] / res[5]))


if __name__ == "__main__":
    say("device: %s" % torch.cuda.get_device_name(0))
    conv_rows()
    mt_rows()
    train_rows()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(OUT) + "\n")
