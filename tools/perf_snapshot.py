"""What a snapshot costs at the default video config's real size (the shapes of `bench.py --config video`: 256x144, nfc 64,
latent 128, vae_levels 3, batch 2, ten stages) on a synthetic clip, a handful of iterations per stage.

    python tools/perf_snapshot.py [--niter 6] [--bench-line profiles/r03_final_bench_line.json] [--out DIR]

Per stage: the snapshot's bytes; the wall time of one mid-stage snapshot from the call to the renamed file (BatchNorm flush,
loss-log drain, device-to-host copies, digest, torch.save, rename), the device idle before it; the digest over the full state
as the snapshot computes it (one launch per tensor of the state, device events around the launches, best of 5) with its GB/s;
and, as the kernel's own streaming rate, the digest of the generator's flat parameter arena and of one 1 GiB buffer.  From
these: the cost per iteration at --snapshot-interval 1000 against the stage's time per iteration in the bench line.  Numbers
only, no pass mark."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hp_vae_gan_amd import ops, programs, snapshot  # noqa: E402

HBM_MEASURED_TBS = 6.29   # float4 copy on this part (8.0 TB/s is the specification)


def synthetic_clip(n=14, h=144, w=256, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 8 + 1, w // 8 + 1, 3))
    big = np.kron(base, np.ones((1, 8, 8, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def digest_ms(tensors, reps=5):
    """(best milliseconds, words) of digesting `tensors` the way ops.state_digest launches it, without the final read."""
    acc = torch.zeros(1, dtype=torch.int64, device=tensors[0].device)
    best, words = None, 0
    for rep in range(reps + 1):        # the first round warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        salt = 0
        for t in tensors:
            salt += ops.state_digest_(t, salt, acc)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if rep > 0 and (best is None or ms < best):
            best = ms
        words = salt
    return best, words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--niter", type=int, default=6)
    ap.add_argument("--bench-line", default=os.path.join(ROOT, "profiles", "r03_final_bench_line.json"))
    ap.add_argument("--out", default=None, help="run directory (default: a temporary one)")
    args = ap.parse_args()
    out = args.out or tempfile.mkdtemp(prefix="perf_snapshot_")
    os.makedirs(out, exist_ok=True)
    clip = os.path.join(out, "synthetic.npy")
    np.save(clip, synthetic_clip())
    with open(args.bench_line) as f:
        per_stage = {int(k): 1000.0 / v for k, v in json.load(f)["per_stage_it_s"].items()}   # ms per iteration
    prog = programs.Program("video", ["--video-path", clip, "--run-dir", os.path.join(out, "run"), "--niter", str(args.niter),
                                      "--manualSeed", "1", "--print-interval", "100", "--snapshot-interval", "4"])
    rows = {}
    orig = prog.write_snapshot

    def timed(trainer, log, stage_done):
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        try:
            orig(trainer, log, stage_done)
        finally:
            t2 = time.perf_counter()
        if not stage_done:
            ts = snapshot.digest_tensors(prog, trainer, False)
            ms, words = digest_ms(ts)
            arena_ms, arena_words = digest_ms([trainer.arenaG.flat])
            rows[prog.opt.scale_idx] = {"bytes": os.path.getsize(os.path.join(prog.exp_dir, snapshot.FILE)),
                                        "wait_ms": (t1 - t0) * 1e3, "snapshot_ms": (t2 - t1) * 1e3, "tensors": len(ts),
                                        "digest_ms": ms, "digest_bytes": 4 * words, "arena_ms": arena_ms,
                                        "arena_bytes": 4 * arena_words}
    prog.write_snapshot = timed
    prog.run()
    big = torch.empty(1 << 28, dtype=torch.int32, device=prog.opt.device).random_()
    big_ms, big_words = digest_ms([big])
    print("snapshot cost, default video config (256x144, nfc 64, B 2), synthetic 14-frame clip, %d iterations per stage, "
          "snapshot after iteration 4" % args.niter)
    print("%5s %12s %12s %8s %11s %11s %13s %13s %12s %14s" % ("stage", "file bytes", "snapshot ms", "tensors", "digest ms",
                                                          "digest GB/s", "arena MB", "arena GB/s", "ms/iter", "cost @1000"))
    for s in sorted(rows):
        r = rows[s]
        it = per_stage.get(s)
        print("%5d %12d %12.1f %8d %11.3f %11.1f %13.1f %13.1f %12s %14s" % (
            s, r["bytes"], r["snapshot_ms"], r["tensors"], r["digest_ms"], r["digest_bytes"] / r["digest_ms"] / 1e6,
            r["arena_bytes"] / 1e6, r["arena_bytes"] / r["arena_ms"] / 1e6, "%.2f" % it if it else "-",
            "%.4f ms = %.3f %%" % (r["snapshot_ms"] / 1000, r["snapshot_ms"] / 1000 / it * 100) if it else "-"))
    print("one 1 GiB buffer: %.3f ms = %.0f GB/s (HBM: %.2f TB/s measured float4 copy, 8.0 TB/s specification; the digest "
          "reads every byte once and writes nothing)" % (big_ms, 4 * big_words / big_ms / 1e6, HBM_MEASURED_TBS))
    print("ms/iter: %s (per_stage_it_s); cost @1000 = snapshot ms / 1000 iterations, and as a share of one iteration"
          % os.path.relpath(args.bench_line, ROOT))
    return 0


if __name__ == "__main__":
    sys.exit(main())
