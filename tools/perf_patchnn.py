"""ops.patch_nn (hpvg_patchnn_u8, i8 matrix cores) at the benchmarked size - a 13 x 144 x 256 sample against a 13 x 144 x 256
real volume, patch 3 x 7 x 7, dense, both directions - against a torch baseline for the same result: fp32 matmul + min over the
packed patch matrices, in the largest row chunks that fit (development tool, not a test).  HIP events, warm-up, median of
`reps`.  The i8 peak is 2x the ~2.5 PF dense BF16 peak of an MI355X (the i8 MFMA takes the cycles of the BF16 form at twice
the K).  usage: python tools/perf_patchnn.py [out.txt] [reps] [T H W]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import ops  # noqa: E402

I8_PEAK = 5.0e15   # multiply-add ops / s, dense
out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, H, W = [int(a) for a in sys.argv[3:6]] if len(sys.argv) > 5 else (13, 144, 256)
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
    """fp32 [N][D] patch matrix of a uint8 [T][H][W][3] volume (centred like the kernel's: the distances are the same)."""
    v = vol.to(torch.float32) - 128.0
    p = v.unfold(0, PATCH[0], 1).unfold(1, PATCH[1], 1).unfold(2, PATCH[2], 1)   # [nT][nY][nX][3][pt][ph][pw]
    return p.reshape(-1, 3 * PATCH[0] * PATCH[1] * PATCH[2]).contiguous()


def baseline(Q, R, qn, rn, chunk):
    d2 = torch.empty(Q.shape[0], dtype=torch.float32, device=dev)
    nn = torch.empty(Q.shape[0], dtype=torch.int64, device=dev)
    Rt = R.t()
    for i0 in range(0, Q.shape[0], chunk):
        dist = torch.addmm(rn[None, :], Q[i0:i0 + chunk], Rt, alpha=-2.0)
        m, j = dist.min(1)
        d2[i0:i0 + chunk] = m + qn[i0:i0 + chunk]
        nn[i0:i0 + chunk] = j
    return d2, nn


torch.manual_seed(0)
sample = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
real = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
Nq, Nr, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
macs = 2.0 * Nq * Nr * D   # both directions, multiply-adds
say("patch_nn perf: sample %s vs real %s, patch %s dense, both directions: Nq = Nr = %d, D = %d, %.3e multiply-adds"
    % ((T, H, W), (T, H, W), PATCH, Nq, D, macs))


def ours():
    a = ops.patch_nn(sample, real, PATCH)
    b = ops.patch_nn(real, sample, PATCH)
    return a, b


med, all_ms = timed(ours, 2, reps)
say("hpvg_patchnn_u8 (pack + i8 MFMA min + unpack), both directions: median %.1f ms of %s" % (med, ["%.1f" % m for m in all_ms]))
say("  = %.1f T multiply-add/s = %.1f TOP/s = %.1f %% of the i8 dense peak (%.1f POP/s)"
    % (macs / med / 1e9, 2 * macs / med / 1e9, 100.0 * 2 * macs / (med / 1e3) / I8_PEAK, I8_PEAK / 1e15))

Q, R = patch_matrix(sample), patch_matrix(real)
qn, rn = (Q * Q).sum(1), (R * R).sum(1)
free = torch.cuda.mem_get_info()[0]
chunk = max(256, min(Nq, int(free * 0.4 / (4.0 * Nr)) // 256 * 256))   # the distance chunk and min's temporaries
say("baseline: torch fp32 addmm + min over the packed fp32 patch matrices, row chunks of %d (%.1f GB per distance chunk)"
    % (chunk, chunk * Nr * 4 / 1e9))


def base():
    a = baseline(Q, R, qn, rn, chunk)
    b = baseline(R, Q, rn, qn, chunk)
    return a, b


bmed, ball = timed(base, 1, reps)
say("baseline, both directions: median %.1f ms of %s" % (bmed, ["%.1f" % m for m in ball]))
say("hand-written kernel over baseline: x%.2f" % (bmed / med))
(d2a, nna), _ = ours()
(d2b, nnb), _ = base()
torch.cuda.synchronize()
say("agreement with the fp32 baseline (which rounds: distances pass 2^24): nn equal on %.4f of the patches, max |d2 difference| %d"
    % (float((nna.reshape(-1) == nnb).float().mean()), int((d2a.reshape(-1).double() - d2b.double()).abs().max())))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
