"""The two searches of evaluate --prdc at the benchmarked size - a 13 x 144 x 256 volume against itself, patch 3 x 7 x 7, dense
(development tool, not a test): ops.patch_nn one direction (the yardstick, measured in this run), ops.patch_nn_weighted,
ops.patch_knn_self at k = 3 and k = 8, ops.patch_ball_count.  One process, the five alternating, `reps` rounds after one warm-up
round, HIP events, medians and ratios.  `resources.txt`, when given, is appended as it is: the new kernels' lines of
hipcc -Rpass-analysis=kernel-resource-usage.
usage: python tools/perf_prdc.py [out.txt] [reps] [resources.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hp_vae_gan_amd  # noqa: E402,F401
from hp_vae_gan_amd import ops  # noqa: E402

argv = sys.argv[1:]
out_path = argv[0] if len(argv) > 0 else None
reps = int(argv[1]) if len(argv) > 1 else 5
res_path = argv[2] if len(argv) > 2 else None
T, H, W = 13, 144, 256
PATCH = (3, 7, 7)
I8_PEAK = 5.0e15   # multiply-add ops / s, dense (tools/perf_patchnn.py)
dev = torch.device("cuda")
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


torch.manual_seed(0)
vol = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev)
N, _, D = ops.patch_nn_counts((T, H, W), (T, H, W), PATCH)
macs = float(N) * N * D
weights = torch.rand(N, device=dev) * 3.75 + 0.25
radius = ops.patch_knn_self(vol, PATCH, 3)[..., 2].contiguous()      # the radii evaluate --prdc 3 would use
work = [("ops.patch_nn, one direction", lambda: ops.patch_nn(vol, vol, PATCH)),
        ("ops.patch_nn_weighted", lambda: ops.patch_nn_weighted(vol, vol, weights, PATCH)),
        ("ops.patch_knn_self k = 3", lambda: ops.patch_knn_self(vol, PATCH, 3)),
        ("ops.patch_knn_self k = 8", lambda: ops.patch_knn_self(vol, PATCH, 8)),
        ("ops.patch_ball_count", lambda: ops.patch_ball_count(vol, vol, radius, PATCH))]
ms = [[] for _ in work]
for rnd in range(reps + 1):          # round 0 warms up every shape
    for i, (_, fn) in enumerate(work):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rnd:
            ms[i].append(e0.elapsed_time(e1))
med = [sorted(m)[len(m) // 2] for m in ms]
say("prdc perf: %s against itself, patch %s dense, random bytes: N = %d, D = %d, %.3e multiply-adds per search; %d alternating rounds"
    % ((T, H, W), PATCH, N, D, macs, reps))
for (name, _), m, md in zip(work, ms, med):
    say("%-28s median %8.1f ms of [%s] = %5.1f %% of the i8 dense peak; x%.3f of patch_nn"
        % (name, md, ", ".join("%.1f" % v for v in m), 100.0 * 2 * macs / (md / 1e3) / I8_PEAK, md / med[0]))
say("ball count / weighted search: x%.3f;  k-nearest k = 3: x%.3f of one patch_nn (3 passes would be x3);  k = 8: x%.3f (8 passes: x8)"
    % (med[4] / med[1], med[2] / med[0], med[3] / med[0]))
if res_path:
    with open(res_path) as f:
        lines.append("")
        lines.append("hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, the new kernels:")
        lines.extend(ln.rstrip("\n") for ln in f)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
