"""Guided sampling without a GPU: the numpy restatement of ops.mask_blend (tests/guide_ref.py) against hand-worked cases, the
seeded defects it must reject, every refusal of the --guide flags of both programs in a child process with no visible device
(and no output directory left behind), and the parsers without the new flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from guide_ref import DEFECTS, far_from_hole, mask_blend_ref  # noqa: E402
from hp_vae_gan_amd import generate, generate_patchnn, programs  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from make_golden import make_opt  # noqa: E402


def _const(shape, v):
    return np.full(tuple(shape) + (3,), v, np.uint8)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_single_hole_voxel_by_hand():
    """1 x 5 x 5, hole at the centre, radius (0, 1, 1): the dilated hole is the 3 x 3 block around it, c counts its voxels in
    every voxel's clipped 3 x 3 box and n is that box."""
    c = np.array([[1, 2, 3, 2, 1], [2, 4, 6, 4, 2], [3, 6, 9, 6, 3], [2, 4, 6, 4, 2], [1, 2, 3, 2, 1]])
    n = np.array([[4, 6, 6, 6, 4], [6, 9, 9, 9, 6], [6, 9, 9, 9, 6], [6, 9, 9, 9, 6], [4, 6, 6, 6, 4]])
    mask = np.zeros((1, 5, 5), np.uint8)
    mask[0, 2, 2] = 7
    got = mask_blend_ref(_const((1, 5, 5), 255), _const((1, 5, 5), 0), mask, (0, 1, 1))
    want = (2 * c * 255 + n) // (2 * n)
    assert want[0, 0] == 64 and want[1, 1] == 113 and want[2, 2] == 255 and want[0, 2] == 128      # 63.75, 113.33, 255, 127.5 up
    for k in range(3):
        assert np.array_equal(got[0, :, :, k], want)
    # other bytes on both sides: the same weights
    a, b = _const((1, 5, 5), 200), _const((1, 5, 5), 101)
    got = mask_blend_ref(a, b, mask, (0, 1, 1))
    assert np.array_equal(got[0, :, :, 1], (2 * (c * 200 + (n - c) * 101) + n) // (2 * n))


def test_corner_hole_by_hand_exercises_the_clipped_n():
    c = np.array([[4, 4, 2], [4, 4, 2], [2, 2, 1]])
    n = np.array([[4, 6, 4], [6, 9, 6], [4, 6, 4]])
    mask = np.zeros((1, 3, 3), bool)
    mask[0, 0, 0] = True
    got = mask_blend_ref(_const((1, 3, 3), 200), _const((1, 3, 3), 100), mask, (0, 1, 1))
    want = (2 * (c * 200 + (n - c) * 100) + n) // (2 * n)
    assert want.tolist() == [[200, 167, 150], [167, 144, 133], [150, 133, 125]]
    assert np.array_equal(got[0, :, :, 0], want) and np.array_equal(got[0, :, :, 2], want)
    assert not np.array_equal(mask_blend_ref(_const((1, 3, 3), 200), _const((1, 3, 3), 100), mask, (0, 1, 1), "n_unclipped"), got)


def test_radius_zero_empty_and_full_masks():
    rng = np.random.default_rng(0)
    a, b = (rng.integers(0, 256, (2, 4, 5, 3)).astype(np.uint8) for _ in range(2))
    mask = rng.random((2, 4, 5)) < 0.4
    assert np.array_equal(mask_blend_ref(a, b, mask, (0, 0, 0)), np.where(mask[..., None], a, b))
    for r in ((0, 0, 0), (1, 2, 1)):
        assert np.array_equal(mask_blend_ref(a, b, np.zeros((2, 4, 5), bool), r), b)
        assert np.array_equal(mask_blend_ref(a, b, np.ones((2, 4, 5), bool), r), a)
    out = mask_blend_ref(a, b, mask, (1, 1, 2))
    assert np.array_equal(out[mask], a[mask])                      # a on the hole
    one = np.zeros((2, 9, 11), bool)
    one[0, 1, 2] = True
    a, b = (rng.integers(0, 256, (2, 9, 11, 3)).astype(np.uint8) for _ in range(2))
    out = mask_blend_ref(a, b, one, (0, 1, 2))
    far = far_from_hole(one, (0, 1, 2))
    assert far.sum() == 2 * 9 * 11 - 4 * 7 and not far[0, 3, 6] and far[0, 4, 6] and far[0, 3, 7] and far[1, 1, 2]
    assert np.array_equal(out[far], b[far])                        # b beyond 2 r


@pytest.mark.parametrize("defect", DEFECTS)
def test_seeded_defects_are_rejected(defect):
    rng = np.random.default_rng(3)
    a, b = (rng.integers(0, 256, (3, 5, 7, 3)).astype(np.uint8) for _ in range(2))
    mask = rng.random((3, 5, 7)) < 0.1
    mask[0, 0, 0] = True
    good = mask_blend_ref(a, b, mask, (1, 1, 2))
    assert not np.array_equal(mask_blend_ref(a, b, mask, (1, 1, 2), defect), good)


# ---------------------------------------------------------------------------------------------------------------- parsers
def test_parsers_without_the_new_flags_only_gain_the_new_defaults():
    new = {"guide": None, "guide_level": None, "guide_mask": None, "guide_feather": None}
    a = vars(generate.generate_parser().parse_args(["--exp-dir", "e"]))
    assert {k: a[k] for k in new} == new
    assert {k: v for k, v in a.items() if k not in new} == {
        "exp_dir": "e", "num_samples": 8, "batch_size": None, "seed": 0, "out": None, "size": None, "wrap": None}
    new["guide_noise"] = None
    b = vars(generate_patchnn.generate_patchnn_parser().parse_args([]))
    assert {k: b[k] for k in new} == new
    assert {k: v for k, v in b.items() if k not in new} == {
        "exp_dir": None, "video_path": None, "image_path": None, "out": None, "num_samples": 8, "seed": 0, "patch": None, "ratio": 0.75,
        "min_size": 16, "iters": 10, "alpha": 0.005, "noise": 0.75, "size": None, "save_levels": False, "mask": None,
        "search": "exact", "pm_iters": None, "pm_from_level": None, "wrap": None, "antialias": False, "t_ratio": 1.0,
        "min_frames": None}
    c = generate_patchnn.generate_patchnn_parser().parse_args(
        ["--guide", "g.npy", "--guide-level", "2", "--guide-mask", "m.npy", "--guide-feather", "0", "3", "4", "--guide-noise", "0.5"])
    assert (c.guide, c.guide_level, c.guide_mask, c.guide_feather, c.guide_noise) == ("g.npy", 2, "m.npy", [0, 3, 4], 0.5)


def test_mask_readers_moved_to_programs_keep_their_names_and_messages(tmp_path):
    assert generate_patchnn.mask_forms is programs.mask_forms and generate_patchnn.pick_mask is programs.pick_mask
    np.save(str(tmp_path / "m.npy"), np.zeros((2, 3), np.float32))
    with pytest.raises(SystemExit, match="generate_patchnn: --mask must be bool or uint8"):
        programs.mask_forms(str(tmp_path / "m.npy"))
    with pytest.raises(SystemExit, match="generate: --guide-mask must be bool or uint8"):
        programs.mask_forms(str(tmp_path / "m.npy"), "generate: --guide-mask")
    with pytest.raises(SystemExit, match=r"generate_patchnn: --mask must have the real volume's shape \(1, 2, 2\), got \(1, 2, 3\)"):
        programs.pick_mask([np.zeros((1, 2, 3), bool)], (1, 2, 2))


# --------------------------------------------------------------------------------------------------------------- refusals
def _write_host_experiment(path, dims, program=None, levels=3):
    """opt.json of a small run and a netG.pth that holds only what the host checks read (the saved scale)."""
    opt = make_opt(device="cpu", dims=dims, generator="GeneratorHPVAEGAN", start_frame=0, max_frames=1000)
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    if program:
        opt.program = program
    os.makedirs(os.path.join(path, "eval"))
    with open(os.path.join(path, "opt.json"), "w") as f:
        json.dump(programs.json_settings(opt), f, indent=1, sort_keys=True)
    torch.save({"scale": levels}, os.path.join(path, "netG.pth"))
    fine = hu.images.level_shape_3d(levels, opt) if dims == 3 else [1] + hu.images.level_shape_2d(levels, opt)
    return path, tuple(fine)


def _child(module, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-m", "hp_vae_gan_amd." + module] + args, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=120)


def _files(tmp, fine):
    """The inputs the refusals name: guides, masks."""
    T, H, W = fine
    rng = np.random.default_rng(1)
    np.save(os.path.join(tmp, "guide.npy"), rng.integers(0, 256, (14, 33, 44, 3)).astype(np.uint8))
    np.save(os.path.join(tmp, "short.npy"), rng.integers(0, 256, (5, 33, 44, 3)).astype(np.uint8))
    hole = np.zeros((T, H, W), np.uint8)
    hole[:, 3:9, 4:12] = 1
    np.save(os.path.join(tmp, "hole.npy"), hole)
    np.save(os.path.join(tmp, "hole_other.npy"), hole[:, :-1])
    np.save(os.path.join(tmp, "empty.npy"), np.zeros_like(hole))
    np.save(os.path.join(tmp, "full.npy"), np.ones_like(hole))


G = ["--guide", "guide.npy", "--guide-level", "1"]
GENERATE_REFUSALS = [
    (3, None, ["--guide-level", "1"], "--guide-level needs --guide"),
    (3, None, ["--guide-mask", "hole.npy"], "--guide-mask needs --guide"),
    (3, None, ["--guide-feather", "1", "2", "2"], "--guide-feather needs --guide"),
    (3, None, ["--guide", "guide.npy"], "--guide needs --guide-level"),
    (3, None, G + ["--guide-mask", "hole.npy", "--guide-feather", "1", "65", "2"], "each in [0, 64]"),
    (3, None, G + ["--guide-mask", "hole.npy", "--guide-feather", "-1", "2", "2"], "each in [0, 64]"),
    (3, None, G + ["--guide-feather", "1", "2", "2"], "--guide-feather needs --guide-mask"),
    (3, None, G + ["--guide-mask", "empty.npy"], "--guide-mask is empty"),
    (3, None, G + ["--guide-mask", "full.npy"], "--guide-mask is all hole"),
    (3, None, G + ["--size", "13", "30", "40"], "--guide does not combine with --size"),
    (3, "train_video_baselines", G, "not built for a train_video_baselines experiment"),
    (3, None, ["--guide", "guide.npy", "--guide-level", "3"], "--guide-level must lie in 0 .. 2"),
    (3, None, ["--guide", "guide.npy", "--guide-level", "-1"], "--guide-level must lie in 0 .. 2"),
    (3, None, ["--guide", "short.npy", "--guide-level", "1"], "needs 13"),
    (3, None, G + ["--guide-mask", "hole_other.npy"], "--guide-mask must have the finest level's shape"),
    (2, None, G + ["--guide-mask", "hole.npy", "--guide-feather", "1", "2", "2"], "of an image has RT = 0"),
]


@pytest.mark.parametrize("dims,program,flags,message", GENERATE_REFUSALS)
def test_generate_refuses_before_any_device_use(tmp_path, dims, program, flags, message):
    """A child with no visible device: were the device asked for first, the message would be gpu_device()'s."""
    tmp = str(tmp_path)
    path, fine = _write_host_experiment(os.path.join(tmp, "exp"), dims, program)
    _files(tmp, fine)
    r = _child("generate", ["--exp-dir", path, "--num-samples", "1", "--out", os.path.join(tmp, "out")] + flags, tmp)
    assert r.returncode != 0 and message in r.stderr and "Traceback" not in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(os.path.join(tmp, "out")) and os.listdir(os.path.join(path, "eval")) == []


def test_generate_with_good_guide_flags_reaches_the_device_question(tmp_path):
    """The same child with flags that pass every host check ends at gpu_device(): the refusals above are the flags' own."""
    tmp = str(tmp_path)
    path, fine = _write_host_experiment(os.path.join(tmp, "exp"), 3)
    _files(tmp, fine)
    r = _child("generate", ["--exp-dir", path, "--out", os.path.join(tmp, "out")] + G + ["--guide-mask", "hole.npy", "--wrap", "t"], tmp)
    assert r.returncode != 0 and "no GPU visible" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(tmp, "out"))


CLIP = (5, 20, 24)
P = ["--video-path", "clip.npy", "--patch", "3", "5", "5", "--min-size", "8"]
PATCHNN_REFUSALS = [
    (P + ["--guide-level", "1"], "--guide-level needs --guide"),
    (P + ["--guide-mask", "pm.npy"], "--guide-mask needs --guide"),
    (P + ["--guide-feather", "1", "2", "2"], "--guide-feather needs --guide"),
    (P + ["--guide-noise", "0.5"], "--guide-noise needs --guide"),
    (P + ["--guide", "pg.npy"], "--guide needs --guide-level"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--guide-feather", "1", "2", "2"], "--guide-feather needs --guide-mask"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--guide-mask", "pm.npy", "--guide-feather", "1", "2", "99"], "each in [0, 64]"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--guide-mask", "pempty.npy"], "--guide-mask is empty"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--guide-mask", "pfull.npy"], "--guide-mask is all hole"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--mask", "pm.npy"], "they do not combine"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--size", "5", "20", "24"], "--size (5, 20, 24) differs"),
    (P + ["--guide", "pg.npy", "--guide-level", "4"], "--guide-level must lie in 0 .. 3"),
    (P + ["--guide", "pg.npy", "--guide-level", "-1"], "--guide-level must lie in 0 .. 3"),
    (P + ["--guide", "ptiny.npy", "--guide-level", "0"], "smaller than the patch"),
    (P + ["--guide", "pg.npy", "--guide-level", "1", "--guide-mask", "pm_other.npy"], "--guide-mask must have the guide's shape"),
    (["--image-path", "img.npy", "--patch", "1", "5", "5", "--min-size", "8", "--guide", "pg.npy", "--guide-level", "1"],
     "the guide of an image run is one image"),
    (["--image-path", "img.npy", "--patch", "1", "5", "5", "--min-size", "8", "--guide", "img.npy", "--guide-level", "1", "--guide-mask",
      "im.npy", "--guide-feather", "1", "2", "2"], "of an image has RT = 0"),
]


@pytest.mark.parametrize("flags,message", PATCHNN_REFUSALS)
def test_generate_patchnn_refuses_before_any_device_use(tmp_path, flags, message):
    tmp = str(tmp_path)
    rng = np.random.default_rng(2)
    np.save(os.path.join(tmp, "clip.npy"), rng.integers(0, 256, CLIP + (3,)).astype(np.uint8))
    np.save(os.path.join(tmp, "img.npy"), rng.integers(0, 256, (20, 24, 3)).astype(np.uint8))
    np.save(os.path.join(tmp, "pg.npy"), rng.integers(0, 256, (5, 16, 30, 3)).astype(np.uint8))
    np.save(os.path.join(tmp, "ptiny.npy"), rng.integers(0, 256, (5, 9, 30, 3)).astype(np.uint8))    # level 0: 9 * 0.75^3 -> 4 < 5
    hole = np.zeros((5, 16, 30), np.uint8)
    hole[1:3, 4:9, 5:12] = 1
    np.save(os.path.join(tmp, "pm.npy"), hole)
    np.save(os.path.join(tmp, "pm_other.npy"), hole[:, :, :-2])
    np.save(os.path.join(tmp, "pempty.npy"), np.zeros_like(hole))
    np.save(os.path.join(tmp, "pfull.npy"), np.ones_like(hole))
    np.save(os.path.join(tmp, "im.npy"), hole[0])
    r = _child("generate_patchnn", flags + ["--out", os.path.join(tmp, "out")], tmp)
    assert r.returncode != 0 and message in r.stderr and "Traceback" not in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(os.path.join(tmp, "out"))


def test_generate_patchnn_with_good_guide_flags_reaches_the_device_question(tmp_path):
    tmp = str(tmp_path)
    rng = np.random.default_rng(2)
    np.save(os.path.join(tmp, "clip.npy"), rng.integers(0, 256, CLIP + (3,)).astype(np.uint8))
    np.save(os.path.join(tmp, "pg.npy"), rng.integers(0, 256, (5, 16, 30, 3)).astype(np.uint8))
    hole = np.zeros((5, 16, 30), np.uint8)
    hole[1:3, 4:9, 5:12] = 1
    np.save(os.path.join(tmp, "pm.npy"), hole)
    r = _child("generate_patchnn", P + ["--guide", "pg.npy", "--guide-level", "2", "--guide-mask", "pm.npy", "--guide-noise", "0.5",
                                        "--wrap", "t", "--search", "patchmatch", "--out", os.path.join(tmp, "out")], tmp)
    assert r.returncode != 0 and "no GPU visible" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(tmp, "out"))
