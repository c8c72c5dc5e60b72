"""The chunk pass of `evaluate --chunks` (hpvg_nnf_chunks_i32) beside the two searches per sample it rides on: chunk_seconds against
patchnn_seconds of the same evaluate run, 4 samples of 13 x 144 x 256 against a real clip of that size, patch 3 x 7 x 7, dense,
HIP events, one warm-up run discarded (development tool, not a test).  Three inputs: random samples (an incoherent field: about
as many chunks as patches), the real clip itself (ONE chunk: the longest union-find paths and every size on one word) and the
clip rolled along W by 32 / 64 / 96 / 128 columns (two large copied pieces and a seam).  usage: python tools/perf_nnf_chunks.py [out.txt]"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hp_vae_gan_amd import evaluate  # noqa: E402


def report(rows):
    """The lines of the profile for rows of {input, Nq, patchnn_seconds, chunk_seconds, chunks, chunk_frac, nnf_coherence}."""
    out = ["nnf chunks perf: `python tools/perf_nnf_chunks.py profiles/nnf_chunks_perf.txt`: evaluate --chunks, 4 samples (13, 144, 256) vs real (13, 144, 256), patch "
           "(3, 7, 7) dense: Nq = Nr = %d patches per sample; HIP events, one warm-up run discarded" % rows[0]["Nq"],
           "  patchnn_seconds = the 2 searches per sample, chunk_seconds = hpvg_nnf_chunks_i32 (5 launches) per sample, both summed "
           "over the 4 samples"]
    for r in rows:
        out.append("%-9s patchnn_seconds %.4f s   chunk_seconds %.6f s = %.3f ms per sample = %.3f %% of the searches   "
                   "(mean chunks %.1f, chunk_frac %.6f, nnf_coherence %.6f)"
                   % (r["input"] + ":", r["patchnn_seconds"], r["chunk_seconds"], r["chunk_seconds"] / 4 * 1e3,
                      100.0 * r["chunk_seconds"] / r["patchnn_seconds"], r["chunks"], r["chunk_frac"], r["nnf_coherence"]))
    return out


def main():
    tmp = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    real = rng.integers(0, 256, size=(13, 144, 256, 3), dtype=np.uint8)
    rand = rng.integers(0, 256, size=(4, 13, 144, 256, 3), dtype=np.uint8)
    copy = np.stack([real] * 4)
    stitched = np.stack([np.concatenate([real[:, :, k:], real[:, :, :k]], 2) for k in (32, 64, 96, 128)])
    np.save(os.path.join(tmp, "R.npy"), real)
    rows = []
    for name, S in (("warm-up", rand), ("random", rand), ("copy", copy), ("stitched", stitched)):
        np.save(os.path.join(tmp, "S.npy"), S)
        m = evaluate.evaluate(samples=os.path.join(tmp, "S.npy"), real=os.path.join(tmp, "R.npy"), out=tmp, chunks=True)
        if name != "warm-up":
            rows.append({"input": name, **{k: m[k] for k in ("Nq", "patchnn_seconds", "chunk_seconds", "chunks", "chunk_frac",
                                                           "nnf_coherence")}})
    lines = report(rows)
    print("\n".join(lines), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
