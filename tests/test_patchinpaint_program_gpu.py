"""`generate_patchnn --mask` on the GPU: the known voxels survive, seeds, the files it writes and its refusals.  Each program run
is a fresh child process under its own timeout (a failed child ends the test); the refusals and the per-level check call the
module in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import generate_patchnn  # noqa: E402

pytestmark = pytest.mark.gpu
FOUR_LEVELS = ["--min-size", "16", "--iters", "2"]       # 40 x 48 -> 30 x 36 -> 23 x 27 -> 17 x 20 -> (13 x 15 < 16)
SIZES = [(17, 20), (23, 27), (30, 36), (40, 48)]


def _texture(frames, seed=0):
    """Random 5 x 5 blocks (test_patchgen_program_gpu's clip): patches resemble each other, so a hole has several plausible
    completions; in random bytes every patch is far from every other one."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((frames, 40 // 5 + 1, 48 // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :40, :48]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def _box(frames, t0=0, t1=None):
    m = np.zeros((frames, 40, 48), bool)
    m[t0:t1, 14:24, 18:30] = True          # 10 x 12
    return m


def _child(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


# the default noise of 0.75 fills the coarsest hole (5 x 6 voxels of 17 x 20) with almost pure noise, so two seeds give two fills
def _inpaint(tmp, out, extra, image=True):
    src = os.path.join(tmp, "img.npy" if image else "clip.npy")
    hole = os.path.join(tmp, "hole_img.npy" if image else "hole_clip.npy")
    if not os.path.exists(src):
        np.save(src, _texture(1)[0] if image else _texture(6))
        np.save(hole, _box(1)[0] if image else _box(6, 2, 4))
    _child(["hp_vae_gan_amd.generate_patchnn", "--image-path" if image else "--video-path", src, "--out", os.path.join(tmp, out),
            "--mask", hole] + FOUR_LEVELS + extra, tmp)
    return np.load(os.path.join(tmp, out, "samples.npy"))


def test_image_hole_keeps_the_known_voxels_and_writes_its_files(tmp_path):
    tmp = str(tmp_path)
    a = _inpaint(tmp, "a", ["--num-samples", "2", "--seed", "3"])
    b = _inpaint(tmp, "b", ["--num-samples", "2", "--seed", "3"])
    img, mask = _texture(1)[0], _box(1)[0]
    assert a.shape == (2, 40, 48, 3) and a.dtype == np.uint8            # generate's layout for images: [N,H,W,3]
    for s in a:
        assert np.array_equal(s[~mask], img[~mask])
    assert np.array_equal(a, b)                                          # the same seed, the same bytes
    assert not np.array_equal(a[0][mask], a[1][mask])                    # two samples, two completions
    out = os.path.join(tmp, "a")
    with open(os.path.join(out, "patchnn.json")) as f:
        info = json.load(f)
    assert info["mask"] == os.path.join(tmp, "hole_img.npy") and info["hole_voxels"] == 120 and info["alpha"] == "inf"
    assert info["level_sizes"] == [[1, h, w] for h, w in SIZES] and info["patch"] == [1, 7, 7] and info["size"] == [1, 40, 48]
    total = [(h - 6) * (w - 6) for h, w in SIZES]
    assert len(info["active_patches"]) == len(info["valid_keys"]) == 4
    assert [q + k for q, k in zip(info["active_patches"], info["valid_keys"])] == total
    assert info["active_patches"][-1] == 16 * 18 and all(q > 0 and k > 0 for q, k in zip(info["active_patches"], info["valid_keys"]))
    assert len(info["seconds_per_sample"]) == 2 and len(info["final_score_per_sample"]) == 2
    assert all(np.isfinite(v) and v >= 0 for v in info["final_score_per_sample"])
    assert sorted(n for n in os.listdir(out) if n.startswith("sample_")) == ["sample_0000.png", "sample_0001.png"]


def test_video_hole_over_two_frames(tmp_path):
    tmp = str(tmp_path)
    s = _inpaint(tmp, "v", ["--num-samples", "1"], image=False)
    clip, mask = _texture(6), _box(6, 2, 4)
    assert s.shape == (1, 6, 40, 48, 3) and s.dtype == np.uint8
    assert np.array_equal(s[0][~mask], clip[~mask])
    with open(os.path.join(tmp, "v", "patchnn.json")) as f:
        info = json.load(f)
    assert info["patch"] == [3, 7, 7] and info["hole_voxels"] == 240 and info["level_sizes"][0] == [6, 17, 20]
    assert os.path.isfile(os.path.join(tmp, "v", "sample_0000.gif"))


def test_every_level_keeps_the_real_level_outside_its_mask():
    img, mask, patch = _texture(1), _box(1), (1, 7, 7)
    real, hole = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    sizes = generate_patchnn.patchnn_pyramid_sizes((1, 40, 48), 0.75, 16, patch)
    assert sizes == [(1, h, w) for h, w in SIZES]
    levels, keys = generate_patchnn.patchnn_real_levels(real, sizes)
    plan = generate_patchnn.patchnn_inpaint_plan(hole, sizes, patch)
    out, score, results = generate_patchnn.patchnn_inpaint(real, hole, patch, 0.75, 16, 2, 0.75, 3, 0, (sizes, levels, keys, plan),
                                                           return_levels=True)
    assert len(results) == 4 and results[-1] is out and score >= 0
    for l, res in enumerate(results):
        M = generate_patchnn.patchnn_mask_resize(mask, sizes[l])
        assert np.array_equal(plan[l]["mask"].cpu().numpy(), M) and M.any() and not M.all()
        assert tuple(res.shape) == sizes[l] + (3,)
        assert np.array_equal(res.cpu().numpy()[~M], levels[l].cpu().numpy()[~M])
    again = generate_patchnn.patchnn_inpaint(real, hole, patch, 0.75, 16, 2, 0.75, 3, 0)      # its own pyramid and plan
    assert torch.equal(again[0], out) and again[1] == score


def test_refusals(tmp_path):
    tmp = str(tmp_path)
    src, hole, out = os.path.join(tmp, "img.npy"), os.path.join(tmp, "hole.npy"), os.path.join(tmp, "o")
    np.save(src, _texture(1)[0])
    kw = dict(image_path=src, out=out, min_size=16, iters=2, num_samples=1)
    np.save(hole, _box(1)[0][:, :47])
    with pytest.raises(SystemExit, match=r"--mask must have the real volume's shape \(1, 40, 48\), got \(1, 40, 47\)"):
        generate_patchnn.generate_patchnn(mask=hole, **kw)
    np.save(hole, np.zeros((40, 48), np.uint8))
    with pytest.raises(SystemExit, match="--mask is empty"):
        generate_patchnn.generate_patchnn(mask=hole, **kw)
    m = np.ones((40, 48), bool)
    m[:3], m[-3:], m[:, :3], m[:, -3:] = False, False, False, False          # a border of 3 known voxels: no 7 x 7 patch avoids the hole
    np.save(hole, m)
    with pytest.raises(SystemExit, match="the hole leaves no whole patch at level 0"):
        generate_patchnn.generate_patchnn(mask=hole, **kw)
    assert not os.path.exists(os.path.join(out, "samples.npy"))


def test_an_image_mask_with_three_channels_and_the_real_size(tmp_path):
    """An [H,W,3] mask also reads as a volume (H, W, 3): --size (1, H, W), the real size, must pick the image reading and run."""
    tmp = str(tmp_path)
    src, hole, out = os.path.join(tmp, "img.npy"), os.path.join(tmp, "hole.npy"), os.path.join(tmp, "o")
    img, mask = _texture(1)[0], _box(1)[0]
    np.save(src, img)
    np.save(hole, np.stack([mask * 0, mask * 255, mask * 0], -1).astype(np.uint8))
    s = generate_patchnn.generate_patchnn(image_path=src, out=out, mask=hole, size=(1, 40, 48), min_size=30, iters=1, num_samples=1)
    assert s.shape == (1, 40, 48, 3) and np.array_equal(s[0][~mask], img[~mask])
    with open(os.path.join(out, "patchnn.json")) as f:
        assert json.load(f)["hole_voxels"] == 120
