"""The generate_patchnn program on the GPU, each run a fresh child process under its own timeout (a failed child ends the test):
the identity without noise, seeds, retargeting, the files it writes, and `evaluate` on its output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import generate_patchnn  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (6, 40, 48)
TWO_LEVELS = ["--min-size", "30", "--iters", "2"]      # 40 x 48 -> 30 x 36 -> (23 x 27 < 30): two levels


def _real():
    return np.random.default_rng(5).integers(0, 256, size=SHAPE + (3,), dtype=np.uint8)


def _blocks(seed=0):
    """The synthetic clip of test_programs_gpu.py at this size: random 5 x 5 blocks, so patches resemble each other (in a clip of
    random bytes every patch is far from every other one and the generator can only return the clip)."""
    rng = np.random.default_rng(seed)
    n, h, w = SHAPE
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


# a clip of 40 x 48 has few patches, and at the default noise of 0.75 enough of the coarsest level survives that a sample can
# come out as the clip itself, whatever the seed; at 3 the coarsest guess is almost all noise, so samples must differ
NOISY = ["--noise", "3"]


def _child(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _generate(tmp, out, extra, clip=_real):
    path = os.path.join(tmp, "clip.npy")
    if not os.path.exists(path):
        np.save(path, clip())
    _child(["hp_vae_gan_amd.generate_patchnn", "--video-path", path, "--out", os.path.join(tmp, out)] + TWO_LEVELS + extra, tmp)
    return np.load(os.path.join(tmp, out, "samples.npy"))


def _distinct_rows(vol, patch=(3, 7, 7)):
    win = sliding_window_view(vol, patch + (3,))[:, :, :, 0]
    rows = win.reshape(-1, 3 * patch[0] * patch[1] * patch[2])
    return len(np.unique(rows, axis=0)) == len(rows)


def test_no_noise_reproduces_the_real_volume(tmp_path):
    """Without noise the coarsest guess is real level 0 and its keys are real level 0: every patch's nearest key is itself
    (distance 0, score 0; any other key is farther as long as all key patches are distinct), so the vote returns the values,
    real level 0.  One level up the guess is that result resized, which is exactly the blurred keys, and the values are real
    level 1; and so on up to the real volume."""
    tmp = str(tmp_path)
    s = _generate(tmp, "o", ["--noise", "0", "--num-samples", "2", "--save-levels"])
    real = _real()
    lv = np.load(os.path.join(tmp, "o", "levels.npz"))
    assert sorted(lv.files) == ["keys_1", "level_0", "level_1"]
    assert lv["level_0"].shape == (6, 30, 36, 3) and lv["keys_1"].shape == lv["level_1"].shape == real.shape
    assert np.array_equal(lv["level_1"], real)
    for k in lv.files:                                   # the precondition of the argument above
        assert _distinct_rows(lv[k]), k
    assert s.shape == (2,) + real.shape and s.dtype == np.uint8
    assert np.array_equal(s[0], real) and np.array_equal(s[1], real)


def test_seeds(tmp_path):
    tmp = str(tmp_path)
    a = _generate(tmp, "a", ["--seed", "3", "--num-samples", "2"] + NOISY, _blocks)
    b = _generate(tmp, "b", ["--seed", "3", "--num-samples", "2"] + NOISY, _blocks)
    c = _generate(tmp, "c", ["--seed", "5", "--num-samples", "1"] + NOISY, _blocks)
    assert np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[0])


def test_retargeting_files_and_evaluate(tmp_path):
    tmp = str(tmp_path)
    s = _generate(tmp, "r", ["--size", "6", "40", "64", "--num-samples", "2", "--seed", "1"], _blocks)     # the default noise
    real = _blocks()
    assert s.shape == (2, 6, 40, 64, 3) and s.dtype == np.uint8
    assert s.min() >= real.min() and s.max() <= real.max()
    out = os.path.join(tmp, "r")
    with open(os.path.join(out, "patchnn.json")) as f:
        info = json.load(f)
    want = generate_patchnn.patchnn_pyramid_sizes(SHAPE, 0.75, 30, (3, 7, 7))
    assert want == [(6, 30, 36), (6, 40, 48)]
    assert info["level_sizes"] == [list(v) for v in want]
    assert info["size"] == [6, 40, 64] and info["real_shape"] == list(SHAPE) and info["patch"] == [3, 7, 7]
    assert (info["num_samples"], info["seed"], info["iters"], info["min_size"], info["ratio"], info["alpha"], info["noise"]) == \
        (2, 1, 2, 30, 0.75, 0.005, 0.75)
    assert len(info["seconds_per_sample"]) == 2 and all(v > 0 for v in info["seconds_per_sample"])
    assert len(info["final_score_per_sample"]) == 2 and all(np.isfinite(v) and v >= 0 for v in info["final_score_per_sample"])
    assert sorted(n for n in os.listdir(out) if n.startswith("sample_")) == ["sample_0000.gif", "sample_0001.gif"]
    # evaluate takes the output as it is
    _child(["hp_vae_gan_amd.evaluate", "--samples", os.path.join(out, "samples.npy"), "--real", os.path.join(tmp, "clip.npy")], tmp)
    with open(os.path.join(out, "metrics.json")) as f:
        m = json.load(f)
    assert m["num_samples"] == 2 and m["patch"] == [3, 7, 7] and (m["Nq"], m["Nr"]) == (4 * 34 * 58, 4 * 34 * 42)
    assert 0.0 <= m["coherence"] < 1.0 and 0.0 <= m["completeness"] < 1.0


def test_image_input_and_alpha_inf(tmp_path):
    tmp = str(tmp_path)
    img = np.random.default_rng(6).integers(0, 256, size=(40, 48, 3), dtype=np.uint8)
    np.save(os.path.join(tmp, "img.npy"), img)
    _child(["hp_vae_gan_amd.generate_patchnn", "--image-path", os.path.join(tmp, "img.npy"), "--out", os.path.join(tmp, "i"),
            "--noise", "0", "--alpha", "inf", "--num-samples", "1"] + TWO_LEVELS, tmp)
    s = np.load(os.path.join(tmp, "i", "samples.npy"))
    assert s.shape == (1, 40, 48, 3) and np.array_equal(s[0], img)
    with open(os.path.join(tmp, "i", "patchnn.json")) as f:
        info = json.load(f)
    assert info["patch"] == [1, 7, 7] and info["alpha"] == "inf" and info["level_sizes"] == [[1, 30, 36], [1, 40, 48]]
    assert info["final_score_per_sample"] == [0.0]
    assert os.path.isfile(os.path.join(tmp, "i", "sample_0000.png"))


def test_exp_dir_uses_the_real_volume_of_evaluate(tmp_path):
    """An experiment directory reduced to the settings real_volume reads: a last stage of 36 x 48 at sampling rate 1 over a
    36 x 48 clip, so the real volume is the clip byte for byte.  Without noise the samples are that volume, they land in
    <exp-dir>/eval/samples_patchnn, and `evaluate --exp-dir ... --samples ...` scores them fully coherent and complete."""
    tmp = str(tmp_path)
    clip = np.random.default_rng(7).integers(0, 256, size=(6, 36, 48, 3), dtype=np.uint8)
    np.save(os.path.join(tmp, "clip.npy"), clip)
    exp = os.path.join(tmp, "exp")
    os.makedirs(exp)
    with open(os.path.join(exp, "opt.json"), "w") as f:
        json.dump({"dims": 3, "video_path": os.path.join(tmp, "clip.npy"), "stop_scale": 2, "stop_scale_time": 2, "scale_factor": 0.75,
                   "img_size": 48, "ar": 0.75, "sampling_rates": [4, 2, 1], "org_fps": 24.0, "fps_lcm": 4, "start_frame": 0,
                   "max_frames": None}, f)
    _child(["hp_vae_gan_amd.generate_patchnn", "--exp-dir", exp, "--noise", "0", "--num-samples", "1", "--min-size", "27", "--iters", "2"], tmp)
    out = os.path.join(exp, "eval", "samples_patchnn")
    s = np.load(os.path.join(out, "samples.npy"))
    assert s.shape == (1, 6, 36, 48, 3) and np.array_equal(s[0], clip)
    with open(os.path.join(out, "patchnn.json")) as f:
        assert json.load(f)["level_sizes"] == [[6, 27, 36], [6, 36, 48]]
    _child(["hp_vae_gan_amd.evaluate", "--exp-dir", exp, "--samples", os.path.join(out, "samples.npy")], tmp)
    with open(os.path.join(out, "metrics.json")) as f:
        m = json.load(f)
    assert m["coherence"] == 0.0 and m["completeness"] == 0.0 and m["num_samples"] == 1
    assert np.array_equal(np.load(os.path.join(out, "real.npy")), clip)
