"""evaluate --chunks on the GPU (fresh child processes, each under its own timeout) on a planted instance: sample 0 is the real
clip, sample 1 is stitched from two shifted halves of it.  Every chunk metric equals chunk_metrics of the yardstick's integers
(tests/nnf_chunks_ref.py) on the brute-force nearest-neighbour field of test_patchnn.py, and a run without the flag is today's."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nnf_chunks_ref import pair_count, ref_chunks  # noqa: E402
from test_evaluate_gpu import KEYS  # noqa: E402
from test_patchnn import brute  # noqa: E402

from hp_vae_gan_amd import evaluate  # noqa: E402

pytestmark = pytest.mark.gpu
PATCH = (3, 7, 7)
GRID = (3, 18, 22)
NQ = 3 * 18 * 22
CHUNK_KEYS = {"nnf_coherence", "chunks", "largest_chunk_frac", "chunk_frac", "in_place_frac"}
PER_SAMPLE = {"coherence", "completeness", "nn_unique_frac"}


@functools.lru_cache(maxsize=None)
def _planted():
    """(real, samples [2], per sample (d2, nn) of the brute force) - built once, never modified."""
    real = np.random.default_rng(3).integers(0, 256, size=(5, 24, 28, 3), dtype=np.uint8)
    s = np.empty_like(real)
    s[:, :, :14] = real[:, :, 10:24]
    s[:, :, 14:] = real[:, :, 0:14]
    S = np.stack([real, s])
    return real, S, tuple(brute(x, real, PATCH) for x in S)


def _evaluate(tmp_path, *flags):
    real, S, _ = _planted()
    np.save(str(tmp_path / "S.npy"), S)
    np.save(str(tmp_path / "R.npy"), real)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.evaluate", "--samples", str(tmp_path / "S.npy"), "--real",
                        str(tmp_path / "R.npy")] + list(flags), cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    with open(str(tmp_path / "metrics.json")) as f:
        return json.load(f), r.stdout.strip().splitlines()


def test_chunks_of_a_copy_and_of_a_stitched_sample(tmp_path):
    m, line = _evaluate(tmp_path, "--chunks", "--save-chunks")
    _, _, fields = _planted()
    assert set(m) == KEYS | CHUNK_KEYS | {"chunk_tol", "chunk_seconds"}
    assert all(set(p) == PER_SAMPLE | CHUNK_KEYS for p in m["per_sample"])
    assert m["chunk_tol"] is None and m["chunk_seconds"] > 0 and (m["Nq"], m["Nr"]) == (NQ, NQ)
    want = [ref_chunks(nn, GRID) for _, nn in fields]
    E = pair_count(GRID)
    for p, w in zip(m["per_sample"], want):
        assert {k: p[k] for k in CHUNK_KEYS} == evaluate.chunk_metrics(w[2], NQ, E)
    p0, p1 = m["per_sample"]
    assert (p0["chunks"], p0["nnf_coherence"], p0["chunk_frac"], p0["in_place_frac"], p0["largest_chunk_frac"]) == (1, 1.0, 1.0, 1.0, 1.0)
    assert p1["in_place_frac"] == 0.0 and p1["chunks"] == 73 and p1["nnf_coherence"] == 2752 / 3048
    for k in CHUNK_KEYS:
        assert m[k] == (p0[k] + p1[k]) / 2
    z = np.load(str(tmp_path / "chunks.npz"))
    assert set(z.files) == {"labels", "sizes", "nn"}
    assert all(z[k].dtype == np.int32 and z[k].shape == (2,) + GRID for k in z.files)
    for i, (w, (_, nn)) in enumerate(zip(want, fields)):
        assert np.array_equal(z["labels"][i], w[0]) and np.array_equal(z["sizes"][i], w[1]) and np.array_equal(z["nn"][i], nn)
    big = np.sort(z["sizes"][1].reshape(-1))[::-1]
    assert big[0] >= 432 and big[1] >= 432 and (big[0], big[1]) == (648, 432)
    assert all(os.path.getsize(str(tmp_path / ("source_%04d.gif" % i))) > 0 for i in range(2))
    assert len(line) == 1
    assert " chunk_frac {:.6f} nnf_coherence {:.6f} (".format(m["chunk_frac"], m["nnf_coherence"]) in line[0]


def test_chunk_tol_zero_keeps_the_exact_copies(tmp_path):
    m, line = _evaluate(tmp_path, "--chunk-tol", "0")
    _, _, fields = _planted()
    keys = CHUNK_KEYS | {"chunk_kept_frac"}
    assert set(m) == KEYS | keys | {"chunk_tol", "chunk_seconds"} and m["chunk_tol"] == 0.0
    assert all(set(p) == PER_SAMPLE | keys for p in m["per_sample"])
    for p, (d2, nn) in zip(m["per_sample"], fields):
        w = ref_chunks(nn, GRID, d2=d2, max_d2=0)
        assert {k: p[k] for k in keys} == evaluate.chunk_metrics(w[2], NQ, pair_count(GRID), kept_frac=True)
    assert m["per_sample"][0]["chunk_kept_frac"] == 1.0
    assert m["per_sample"][1]["chunk_kept_frac"] == 864 / 1188 and m["per_sample"][1]["chunks"] == 2
    assert not os.path.exists(str(tmp_path / "chunks.npz")) and len(line) == 1 and " chunk_frac " in line[0]


def test_without_the_flag_nothing_changes(tmp_path):
    m, line = _evaluate(tmp_path)
    assert set(m) == KEYS and all(set(p) == PER_SAMPLE for p in m["per_sample"])
    assert len(line) == 1 and "chunk_frac" not in line[0] and "nnf_coherence" not in line[0]
    assert sorted(os.listdir(str(tmp_path))) == ["R.npy", "S.npy", "metrics.json"]
