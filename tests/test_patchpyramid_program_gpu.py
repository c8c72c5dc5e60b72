"""`generate_patchnn --antialias / --t-ratio / --min-frames` and `evaluate --scales` on the GPU, each run a fresh child process
under its own timeout (a failed child ends the test): the identity without noise on an antialiased space-time pyramid, seeds
under every search and on a ring, retargeting, --mask, the files written, and the per-scale scores against a brute force on the
numpy restatement of the resize (tests/volresize_ref.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import volresize_ref as VR  # noqa: E402
from test_patchgen_program_gpu import NOISY, SHAPE, _blocks, _distinct_rows, _real  # noqa: E402
from test_patchnn import brute  # noqa: E402

pytestmark = pytest.mark.gpu
PYRAMID = ["--antialias", "--t-ratio", "0.8", "--min-size", "23", "--iters", "2"]      # (4,23,27), (5,30,36), (6,40,48)
NEW_KEYS = ("antialias", "t_ratio", "min_frames")


def _child(args, cwd, timeout=120, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _generate(tmp, out, extra, clip=_blocks):
    path = os.path.join(tmp, "clip.npy")
    if not os.path.exists(path):
        np.save(path, clip())
    _child(["hp_vae_gan_amd.generate_patchnn", "--video-path", path, "--out", os.path.join(tmp, out)] + extra, tmp)
    return np.load(os.path.join(tmp, out, "samples.npy"))


def _info(tmp, out, name="patchnn.json"):
    with open(os.path.join(tmp, out, name)) as f:
        return json.load(f)


def test_no_noise_reproduces_the_real_volume_on_an_antialiased_space_time_pyramid(tmp_path):
    """test_patchgen_program_gpu's identity argument, level by level, with T scaled (6 -> 4 frames at level 0) and every resize
    the exact one; the saved levels are the reference's bytes."""
    tmp = str(tmp_path)
    real = _real()
    s = _generate(tmp, "o", ["--noise", "0", "--antialias", "--t-ratio", "0.6", "--min-size", "30", "--iters", "2", "--save-levels",
                             "--num-samples", "2"], _real)
    lv = np.load(os.path.join(tmp, "o", "levels.npz"))
    assert sorted(lv.files) == ["keys_1", "level_0", "level_1"]
    assert lv["level_0"].shape == (4, 30, 36, 3)
    assert np.array_equal(lv["level_0"], VR.resize(real, (4, 30, 36)))
    assert np.array_equal(lv["keys_1"], VR.resize(lv["level_0"], SHAPE))
    assert np.array_equal(lv["level_1"], real)
    for k in lv.files:                                   # the precondition of the identity argument
        assert _distinct_rows(lv[k]), k
    assert s.shape == (2,) + real.shape and np.array_equal(s[0], real) and np.array_equal(s[1], real)
    info = _info(tmp, "o")
    assert info["level_sizes"] == [[4, 30, 36], [6, 40, 48]]
    assert (info["antialias"], info["t_ratio"], info["min_frames"]) == (True, 0.6, 4)


@pytest.mark.parametrize("mode", ["exact", "patchmatch", "wrap_t", "bilinear"])
def test_seeds(tmp_path, mode):
    tmp = str(tmp_path)
    extra = {"exact": [], "patchmatch": ["--search", "patchmatch"], "wrap_t": ["--wrap", "t"], "bilinear": []}[mode]
    base = (PYRAMID[1:] if mode == "bilinear" else PYRAMID) + NOISY + extra        # --t-ratio also works without --antialias
    a = _generate(tmp, "a", base + ["--seed", "3", "--num-samples", "2"])
    b = _generate(tmp, "b", base + ["--seed", "3", "--num-samples", "2"])
    assert a.shape == (2,) + SHAPE + (3,) and np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    info = _info(tmp, "a")
    assert info["level_sizes"] == [[4, 23, 27], [5, 30, 36], [6, 40, 48]]
    assert (info.get("antialias"), info["t_ratio"], info["min_frames"]) == (None if mode == "bilinear" else True, 0.8, 4)
    if mode == "exact":
        c = _generate(tmp, "c", base + ["--seed", "5", "--num-samples", "1"])
        assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[0])


def test_retargeting_scales_the_samples_own_t(tmp_path):
    tmp = str(tmp_path)
    s = _generate(tmp, "r", PYRAMID + ["--size", "9", "40", "64", "--num-samples", "1", "--seed", "1", "--min-frames", "3"])
    real = _blocks()
    assert s.shape == (1, 9, 40, 64, 3) and s.dtype == np.uint8
    assert s.min() >= real.min() and s.max() <= real.max()
    info = _info(tmp, "r")
    assert info["size"] == [9, 40, 64] and info["level_sizes"] == [[4, 23, 27], [5, 30, 36], [6, 40, 48]]
    assert (info["antialias"], info["t_ratio"], info["min_frames"]) == (True, 0.8, 3)


def test_mask_with_antialias_keeps_every_known_voxel(tmp_path):
    tmp = str(tmp_path)
    mask = np.zeros(SHAPE, bool)
    mask[2:4, 14:24, 18:30] = True
    np.save(os.path.join(tmp, "hole.npy"), mask)
    s = _generate(tmp, "m", ["--antialias", "--mask", os.path.join(tmp, "hole.npy"), "--min-size", "16", "--iters", "2", "--num-samples", "1"])
    clip = _blocks()
    assert s.shape == (1,) + clip.shape and np.array_equal(s[0][~mask], clip[~mask])
    info = _info(tmp, "m")
    assert info["antialias"] is True and "t_ratio" not in info and "min_frames" not in info and info["hole_voxels"] == int(mask.sum())
    r = _child(["hp_vae_gan_amd.generate_patchnn", "--video-path", os.path.join(tmp, "clip.npy"), "--out", os.path.join(tmp, "x"),
                "--mask", os.path.join(tmp, "hole.npy"), "--t-ratio", "0.8"], tmp, ok=False)
    assert "--t-ratio does not combine with --mask" in r.stderr and not os.path.exists(os.path.join(tmp, "x"))


def test_files_without_the_flags_name_none_of_them(tmp_path):
    tmp = str(tmp_path)
    s = _generate(tmp, "p", ["--min-size", "30", "--iters", "1", "--num-samples", "1"])
    assert s.shape == (1,) + SHAPE + (3,) and not any(k in _info(tmp, "p") for k in NEW_KEYS)
    r = _child(["hp_vae_gan_amd.evaluate", "--real", os.path.join(tmp, "clip.npy"), "--samples", os.path.join(tmp, "p", "samples.npy")], tmp)
    m = _info(tmp, "p", "metrics.json")
    assert not any(k in m for k in ("scales", "scale_ratio", "scales_seconds")) and "scales" not in m["per_sample"][0]
    assert "coherence@" not in r.stdout


def test_evaluate_scales(tmp_path):
    tmp = str(tmp_path)
    clip = _blocks()
    np.save(os.path.join(tmp, "clip.npy"), clip)
    ev = ["hp_vae_gan_amd.evaluate", "--real", os.path.join(tmp, "clip.npy")]
    # a copy scores exactly 0.0 at every scale; a sample with its frames reversed and mirrored scores what a brute force on the
    # reference resizes gives
    other = np.ascontiguousarray(clip[::-1, :, ::-1])
    os.makedirs(os.path.join(tmp, "e"))
    np.save(os.path.join(tmp, "e", "samples.npy"), np.stack([clip, other]))
    r = _child(ev + ["--samples", os.path.join(tmp, "e", "samples.npy"), "--scales", "2"], tmp)
    m = _info(tmp, "e", "metrics.json")
    sizes = [(6, 20, 24), (6, 10, 12)]
    assert m["scale_ratio"] == 0.5 and m["scales_seconds"] > 0 and [v["scale"] for v in m["scales"]] == [1, 2]
    assert " coherence@1 " in r.stdout and " coherence@2 " in r.stdout
    D = 3 * 3 * 7 * 7
    for k, size in enumerate(sizes):
        rk, ok = VR.resize(clip, size), VR.resize(other, size)
        want = []
        for q, ref in ((ok, rk), (rk, ok)):
            d2 = brute(q, ref, (3, 7, 7))[0]
            want.append(int(d2.sum()) / (d2.size * D * 255 * 255))
        copy, shuffled = m["per_sample"][0]["scales"][k], m["per_sample"][1]["scales"][k]
        assert copy == {"scale": k + 1, "size": list(size), "coherence": 0.0, "completeness": 0.0}
        assert shuffled == {"scale": k + 1, "size": list(size), "coherence": want[0], "completeness": want[1]} and want[0] > 0
        top = m["scales"][k]
        N = (size[0] - 2) * (size[1] - 6) * (size[2] - 6)
        assert (top["Nq"], top["Nr"], top["size"]) == (N, N, list(size))
        assert top["coherence"] == (0.0 + want[0]) / 2 and top["completeness"] == (0.0 + want[1]) / 2
    assert m["per_sample"][0]["coherence"] == 0.0 and m["coherence"] == m["per_sample"][1]["coherence"] / 2      # full size: as ever
    r = _child(ev + ["--samples", os.path.join(tmp, "e", "samples.npy"), "--scales", "3"], tmp, ok=False)
    assert "--scales 3" in r.stderr and "the largest K that fits is 2" in r.stderr
