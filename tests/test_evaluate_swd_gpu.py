"""evaluate --swd on the GPU (a fresh child process under its own timeout): the metrics gain exactly the four sliced Wasserstein
keys, every sample's score equals swd_score of the numpy brute-force numerators of test_patchswd.py, and a sample equal to the
real volume scores exactly 0.0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_evaluate_gpu import KEYS, _clip  # noqa: E402
from test_patchswd import ref_hist, ref_num  # noqa: E402

from hp_vae_gan_amd import evaluate  # noqa: E402

pytestmark = pytest.mark.gpu


def test_swd_keys_scores_and_zero_for_a_copy(tmp_path):
    real = _clip(6, 20, 24)
    other = np.random.default_rng(5).integers(0, 256, size=real.shape, dtype=np.uint8)
    S = np.stack([real, other])
    np.save(str(tmp_path / "S.npy"), S)
    np.save(str(tmp_path / "R.npy"), real)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.evaluate", "--samples", str(tmp_path / "S.npy"), "--real",
                        str(tmp_path / "R.npy"), "--swd", "16", "--swd-seed", "3"], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    with open(str(tmp_path / "metrics.json")) as f:
        m = json.load(f)
    assert set(m) == KEYS | {"swd", "swd_directions", "swd_seed", "swd_seconds"}
    assert all(set(p) == {"coherence", "completeness", "nn_unique_frac", "swd"} for p in m["per_sample"])
    assert (m["swd_directions"], m["swd_seed"]) == (16, 3) and m["swd_seconds"] > 0
    assert (m["Nq"], m["Nr"], m["D"]) == (4 * 14 * 18, 4 * 14 * 18, 441)
    dirs = evaluate.swd_directions(16, 441, 3)
    hr, Nr = ref_hist(real, (3, 7, 7), dirs)
    for s, p in zip(S, m["per_sample"]):
        hs, Ns = ref_hist(s, (3, 7, 7), dirs)
        assert p["swd"] == evaluate.swd_score(ref_num(hs, Ns, hr, Nr), Ns, Nr, dirs)
    assert m["per_sample"][0]["swd"] == 0.0 and m["per_sample"][1]["swd"] > 0.0
    assert m["swd"] == (m["per_sample"][0]["swd"] + m["per_sample"][1]["swd"]) / 2
    line = r.stdout.strip().splitlines()
    assert len(line) == 1 and " swd {:.6f} (".format(m["swd"]) in line[0]
