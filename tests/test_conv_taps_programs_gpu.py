"""The programs with --ker-size 5 / 7, end to end, each in a fresh child process under its own time limit: train_video
--ker-size 5 --padd-size 2 on a tiny synthetic clip (hipGraph replay from the third iteration of a stage on), generate on the
experiment it leaves, a run stopped by --snapshot-exit-after and resumed against the uninterrupted one (netG.pth equal as
bits), and train_image --ker-size 7 --padd-size 3 --no-hip-graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
SIZES = ["--nfc", "4", "--latent-dim", "4", "--min-size", "32", "--max-size", "40", "--img-size", "40", "--vae-levels", "1"]
RUN = ["--niter", "6", "--print-interval", "3", "--manualSeed", "3"]
TAPS5 = ["--ker-size", "5", "--padd-size", "2"]


def _clip(n=16, h=30, w=40, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def _child(args, cwd, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _bits_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_bits_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_bits_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("taps"))
    np.save(os.path.join(d, "clip.npy"), _clip())
    common = ["hp_vae_gan_amd.train_video", "--video-path", "clip.npy"] + RUN + SIZES + TAPS5 + ["--snapshot-interval", "4"]
    r = _child(common + ["--run-dir", "r0"], d)
    return {"dir": d, "common": common, "r0": os.path.join(d, "r0", "clip", "DEBUG", "experiment_0"), "stdout": r.stdout}


def test_train_video_runs_five_taps(work):
    from hp_vae_gan_amd import programs
    exp = work["r0"]
    opt = programs.load_opt(exp)
    assert (opt.ker_size, opt.padd_size) == (5, 2) and opt.stop_scale == 2
    ck = torch.load(os.path.join(exp, "netG.pth"), weights_only=True)
    assert ck["scale"] == 2
    sd = ck["state_dict"]
    assert tuple(sd["decoder.head.conv.weight"].shape) == (4, 4, 5, 5, 5) and tuple(sd["body.1.tail.weight"].shape) == (3, 4, 5, 5, 5)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.dtype.is_floating_point)
    netD = torch.load(os.path.join(exp, "netD_2.pth"), weights_only=True)
    assert tuple(netD["state_dict"]["tail.weight"].shape) == (1, 4, 5, 5, 5)
    with open(os.path.join(exp, "logbook.txt")) as f:
        log = f.read()
    assert log.count("Snapshot: stage") == 6


def test_generate_writes_samples_of_the_right_shape(work):
    from hp_vae_gan_amd import programs
    from hp_vae_gan_amd import utils as hu
    out = os.path.join(work["dir"], "gen")
    _child(["hp_vae_gan_amd.generate", "--exp-dir", work["r0"], "--num-samples", "3", "--seed", "7", "--out", out], work["dir"])
    got = np.load(os.path.join(out, "samples.npy"))
    opt = programs.load_opt(work["r0"])
    want = [3, hu.get_fps_td_by_index(2, opt)[1]] + list(hu.images.level_shape_3d(2, opt)[1:]) + [3]
    assert got.dtype == np.uint8 and list(got.shape) == want, (got.shape, want)
    assert got.std() > 0
    assert sorted(os.listdir(out)) == sorted(["samples.npy"] + ["sample_%04d.gif" % k for k in range(3)])


def test_stopped_and_resumed_run_is_the_same_run(work):
    d = work["dir"]
    r = _child(work["common"] + ["--run-dir", "r1", "--snapshot-exit-after", "3"], d)
    assert "Stopped after snapshot 3" in r.stdout
    exp = os.path.join(d, "r1", "clip", "DEBUG", "experiment_0")
    assert not os.path.exists(os.path.join(exp, "netD_2.pth"))
    _child(["hp_vae_gan_amd.train_video", "--resume", exp], d)
    for name in ("netG.pth", "netD_2.pth", "Noise_Amps.pth"):
        a = torch.load(os.path.join(work["r0"], name), weights_only=True)
        b = torch.load(os.path.join(exp, name), weights_only=True)
        assert _bits_equal(a, b), name + " differs between the uninterrupted and the resumed run"


def test_train_image_runs_seven_taps_without_the_graph(tmp_path):
    np.save(str(tmp_path / "img.npy"), _clip(1, seed=1))
    _child(["hp_vae_gan_amd.train_image", "--image-path", "img.npy", "--run-dir", "ri", "--ker-size", "7", "--padd-size", "3",
            "--no-hip-graph", "--niter", "4", "--print-interval", "2", "--manualSeed", "4"] + SIZES, str(tmp_path))
    exp = str(tmp_path / "ri" / "img" / "DEBUG" / "experiment_0")
    ck = torch.load(os.path.join(exp, "netG.pth"), weights_only=True)
    assert tuple(ck["state_dict"]["decoder.head.conv.weight"].shape) == (4, 4, 7, 7)
    assert all(bool(torch.isfinite(v).all()) for v in ck["state_dict"].values() if v.dtype.is_floating_point)
    _child(["hp_vae_gan_amd.generate", "--exp-dir", exp, "--num-samples", "2", "--out", str(tmp_path / "gen")], str(tmp_path))
    got = np.load(str(tmp_path / "gen" / "samples.npy"))
    assert got.dtype == np.uint8 and got.shape[0] == 2 and got.shape[-1] == 3 and got.ndim == 4
