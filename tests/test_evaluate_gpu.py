"""The evaluate program on the GPU, each run a fresh child process under its own timeout, one after the other (a failed child
ends the test): scores with known answers, a train_video -> generate -> evaluate chain on the small pyramid of
test_programs_gpu.py checked against the numpy brute force of test_patchnn.py, and the message when no samples exist."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_patchnn import brute  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = ["--nfc", "8", "--latent-dim", "8", "--min-size", "16", "--max-size", "40", "--img-size", "40", "--vae-levels", "2"]
KEYS = {"samples", "num_samples", "patch", "stride", "Nq", "Nr", "D", "Nq_completeness", "Nr_completeness", "per_sample",
        "patchnn_seconds", "diversity", "coherence", "completeness", "nn_unique_frac"}


def _clip(n=16, h=30, w=40, seed=0):
    """The synthetic clip of test_programs_gpu.py."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def _child(args, cwd, timeout, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _metrics(d):
    with open(os.path.join(d, "metrics.json")) as f:
        return json.load(f)


def test_crops_of_the_real_clip_are_fully_coherent(tmp_path):
    real = _clip(8)
    S = np.stack([real[0:5, 2:26, 3:35], real[3:8, 6:30, 8:40]])
    np.save(str(tmp_path / "S.npy"), S)
    np.save(str(tmp_path / "R.npy"), real)
    r = _child(["hp_vae_gan_amd.evaluate", "--samples", str(tmp_path / "S.npy"), "--real", str(tmp_path / "R.npy")], str(tmp_path), 120)
    m = _metrics(str(tmp_path))
    assert set(m) == KEYS and m["patch"] == [3, 7, 7] and m["stride"] == [1, 1, 1] and m["num_samples"] == 2
    assert (m["Nq"], m["Nr"], m["D"]) == (3 * 18 * 26, 6 * 24 * 34, 441)
    assert (m["Nq_completeness"], m["Nr_completeness"]) == (m["Nr"], m["Nq"])
    assert m["coherence"] == 0.0 and all(p["coherence"] == 0.0 for p in m["per_sample"])
    assert m["diversity"] is None   # the samples are smaller than the real frames
    for s, p in zip(S, m["per_sample"]):
        d2, nn = brute(s, real, (3, 7, 7))
        assert int(d2.sum()) == 0
        assert p["nn_unique_frac"] == len(np.unique(nn)) / min(m["Nq"], m["Nr"])
        d2r, _ = brute(real, s, (3, 7, 7))
        assert p["completeness"] == int(d2r.sum()) / (d2r.size * 441 * 255 * 255)
    assert "coherence" in r.stdout and len(r.stdout.strip().splitlines()) == 1


def test_white_against_black_scores_one(tmp_path):
    real = np.zeros((4, 12, 14, 3), np.uint8)
    np.save(str(tmp_path / "R.npy"), real)
    np.save(str(tmp_path / "S.npy"), (255 - real)[None])
    _child(["hp_vae_gan_amd.evaluate", "--samples", str(tmp_path / "S.npy"), "--real", str(tmp_path / "R.npy"), "--out",
            str(tmp_path / "o")], str(tmp_path), 120)
    m = _metrics(str(tmp_path / "o"))
    assert m["coherence"] == 1.0 and m["completeness"] == 1.0 and m["diversity"] is None
    assert m["per_sample"][0]["nn_unique_frac"] == 1 / m["Nq"]


def test_missing_samples_names_generate(tmp_path):
    os.makedirs(str(tmp_path / "exp" / "eval"))
    r = _child(["hp_vae_gan_amd.evaluate", "--exp-dir", str(tmp_path / "exp")], str(tmp_path), 120, ok=False)
    assert r.returncode != 0 and "generate" in r.stderr


def test_train_generate_evaluate(tmp_path):
    tmp = str(tmp_path)
    clip = _clip()
    np.save(os.path.join(tmp, "clip.npy"), clip)
    _child(["hp_vae_gan_amd.train_video", "--video-path", os.path.join(tmp, "clip.npy"), "--niter", "3", "--print-interval", "3",
            "--manualSeed", "1", "--checkname", "t"] + SMALL, tmp, 420)
    exp = os.path.join(tmp, "run", "clip", "t", "experiment_0")
    _child(["hp_vae_gan_amd.generate", "--exp-dir", exp, "--num-samples", "2", "--seed", "2"], tmp, 120)
    _child(["hp_vae_gan_amd.evaluate", "--exp-dir", exp], tmp, 120)
    out = os.path.join(exp, "eval", "samples")
    m = _metrics(out)
    assert set(m) == KEYS and m["num_samples"] == 2 and len(m["per_sample"]) == 2
    assert all(set(p) == {"coherence", "completeness", "nn_unique_frac"} for p in m["per_sample"])
    samples = np.load(os.path.join(out, "samples.npy"))
    real = np.load(os.path.join(out, "real.npy"))
    # the last stage of this pyramid is 30 x 40 at sampling rate 1, the size and rate of the source: the real volume is the
    # source, byte for byte (the fp32 clip maps back to its uint8 levels exactly)
    assert real.dtype == np.uint8 and real.shape == clip.shape and np.array_equal(real, clip)
    assert samples.shape == (2, 13, 30, 40, 3)
    assert (m["Nq"], m["Nr"], m["D"]) == (11 * 24 * 34, 14 * 24 * 34, 441)
    for s, p in zip(samples, m["per_sample"]):
        d2, nn = brute(s, real, (3, 7, 7))
        assert p["coherence"] == int(d2.sum()) / (d2.size * 441 * 255 * 255)
        assert p["nn_unique_frac"] == len(np.unique(nn)) / min(m["Nq"], m["Nr"])
        d2r, _ = brute(real, s, (3, 7, 7))
        assert p["completeness"] == int(d2r.sum()) / (d2r.size * 441 * 255 * 255)
    for k in ("coherence", "completeness", "nn_unique_frac"):
        assert m[k] == sum(p[k] for p in m["per_sample"]) / 2
    s = samples.astype(np.float64).mean(-1)
    r = real[:13].astype(np.float64).mean(-1)
    assert m["diversity"] == pytest.approx(s.std(0).mean() / r.std(), rel=1e-12)   # float64 sums in another order
    assert m["patchnn_seconds"] > 0
