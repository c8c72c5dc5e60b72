"""`generate --guide` and `generate_patchnn --guide` end to end: fresh child processes on an experiment directory written without
training (opt.json, a freshly initialised small generator through checkpoint's own writer, the clip beside it).  Without the
flags the programs write what they wrote; with them the shapes, directory names, json fields, determinism and - with
--guide-mask - the guide's own bytes away from the hole."""
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from guide_ref import far_from_hole  # noqa: E402
from hp_vae_gan_amd import checkpoint, generate, programs  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import networks_3d  # noqa: E402
from make_golden import make_opt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FEATHER = (1, 2, 2)


def _child(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    print("%s: %.1f s, exit %d" % (args[0], time.time() - t0, r.returncode))
    assert r.returncode == 0, (args, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _clip(shape, seed):
    rng = np.random.default_rng(seed)
    n, h, w = shape
    base = rng.integers(0, 256, (n, h // 4 + 1, w // 4 + 1, 3)).astype(np.float64)
    big = np.kron(base, np.ones((1, 4, 4, 1)))[:, :h, :w]
    return np.clip(big + rng.normal(0, 8, big.shape), 0, 255).astype(np.uint8)


def _listing(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _json(path):
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    """The experiment directory (three body levels, finest level 5 x 21 x 28; the clip 14 x 36 x 48 beside it) and two flagless
    runs of each program into directories of their own."""
    tmp = str(tmp_path_factory.mktemp("guide"))
    np.save(os.path.join(tmp, "clip.npy"), _clip((14, 36, 48), 0))
    np.save(os.path.join(tmp, "guide.npy"), _clip((14, 36, 48), 1))
    torch.manual_seed(0)
    opt = make_opt(device=DEV, dims=3, generator="GeneratorHPVAEGAN", start_frame=0, max_frames=1000,
                   video_path=os.path.join(tmp, "clip.npy"))
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    netG = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(3):
        netG.init_next_stage()
    netG.to(DEV)
    opt.scale_idx = 3
    opt.Noise_Amps = [1.0, 0.1, 0.1, 0.1]
    path = os.path.join(tmp, "exp")
    os.makedirs(os.path.join(path, "eval"))
    with open(os.path.join(path, "opt.json"), "w") as f:
        json.dump(programs.json_settings(opt), f, indent=1, sort_keys=True)
    checkpoint.save_stage(path, opt, types.SimpleNamespace(netG=netG, netD=None, optimizerG=types.SimpleNamespace(state_dict=lambda: {})))
    trained = [netG._level_size(l) for l in range(4)]
    assert trained[-1] == [5, 21, 28]
    hole = np.zeros((5, 21, 28), np.uint8)
    hole[2:4, 8:12, 10:15] = 1
    np.save(os.path.join(tmp, "hole.npy"), hole)
    for name in ("plain_a", "plain_b"):
        _child(GEN + ["--exp-dir", path, "--seed", "7", "--out", os.path.join(tmp, name)], tmp)
    assert os.listdir(os.path.join(path, "eval")) == []
    return types.SimpleNamespace(tmp=tmp, path=path, trained=trained, hole=hole != 0)


GEN = ["hp_vae_gan_amd.generate", "--num-samples", "3"]
PNN = ["hp_vae_gan_amd.generate_patchnn", "--num-samples", "2", "--patch", "3", "5", "5", "--iters", "2", "--seed", "3"]


def test_generate_without_the_flags_writes_what_it_wrote(exp):
    a, b = os.path.join(exp.tmp, "plain_a"), os.path.join(exp.tmp, "plain_b")
    assert _listing(a) == _listing(b) == ["sample_0000.gif", "sample_0001.gif", "sample_0002.gif", "samples.npy"]    # no generate.json
    assert _bytes(os.path.join(a, "samples.npy")) == _bytes(os.path.join(b, "samples.npy"))
    assert list(np.load(os.path.join(a, "samples.npy")).shape) == [3, 5, 21, 28, 3]


def test_generate_guide_shapes_directory_json_and_determinism(exp):
    flags = ["--exp-dir", exp.path, "--guide", "guide.npy", "--guide-level", "1"]
    _child(GEN + flags + ["--seed", "7"], exp.tmp)
    _child(GEN + flags + ["--seed", "7", "--out", os.path.join(exp.tmp, "guide_again")], exp.tmp)
    _child(GEN + flags + ["--seed", "8", "--guide-mask", "hole.npy", "--guide-feather"] + [str(r) for r in FEATHER]
           + ["--out", os.path.join(exp.tmp, "guide_masked")], exp.tmp)
    out = os.path.join(exp.path, "eval", "samples_guide1")
    assert _listing(out) == ["generate.json", "sample_0000.gif", "sample_0001.gif", "sample_0002.gif", "samples.npy"]
    arr = np.load(os.path.join(out, "samples.npy"))
    assert arr.dtype == np.uint8 and list(arr.shape) == [3, 5, 21, 28, 3]
    assert _bytes(os.path.join(out, "samples.npy")) == _bytes(os.path.join(exp.tmp, "guide_again", "samples.npy"))
    assert not np.array_equal(arr, np.load(os.path.join(exp.tmp, "plain_a", "samples.npy")))
    meta = _json(os.path.join(out, "generate.json"))
    assert meta["guide"] == os.path.join(exp.tmp, "guide.npy") and meta["guide_level"] == 1
    assert meta["guide_mask"] is None and meta["guide_feather"] is None
    assert meta["level_sizes"] == exp.trained and meta["size"] == [5, 21, 28] and meta["wrap"] is None
    assert meta["seed"] == 7 and meta["num_samples"] == 3 and meta["batch_size"] == 2 and meta["seconds_per_sample"] > 0
    # the masked run: another seed gives other bytes inside the hole, where the composite is the sample itself; away from the hole
    # (farther than 2 r along some axis from every hole voxel) every sample is the guide at the finest trained stage
    masked = np.load(os.path.join(exp.tmp, "guide_masked", "samples.npy"))
    meta = _json(os.path.join(exp.tmp, "guide_masked", "generate.json"))
    assert meta["guide_mask"] == os.path.join(exp.tmp, "hole.npy") and meta["guide_feather"] == list(FEATHER) and meta["seed"] == 8
    assert masked.shape == arr.shape and not np.array_equal(masked[:, exp.hole], arr[:, exp.hole])
    opt = programs.load_opt(exp.path)
    store_frames = np.load(os.path.join(exp.tmp, "guide.npy"))
    guide_u8 = generate.guide_tensors(opt, store_frames, 1, DEV, finest=3)[1].cpu().numpy()
    far = far_from_hole(exp.hole, FEATHER)
    assert 0 < far.sum() < far.size
    for s in masked:
        assert np.array_equal(s[far], guide_u8[far])
        assert not np.array_equal(s[exp.hole], guide_u8[exp.hole])


def test_generate_guide_composes_with_wrap(exp):
    _child(GEN + ["--exp-dir", exp.path, "--seed", "7", "--guide", "guide.npy", "--guide-level", "2", "--wrap", "t"], exp.tmp)
    out = os.path.join(exp.path, "eval", "samples_guide2_wrapt")
    meta = _json(os.path.join(out, "generate.json"))
    assert meta["wrap"] == "t" and meta["guide_level"] == 2
    assert list(np.load(os.path.join(out, "samples.npy")).shape) == [3, 5, 21, 28, 3]


def test_generate_patchnn_without_the_flags_writes_what_it_wrote(exp):
    for name in ("pnn_a", "pnn_b"):
        _child(PNN + ["--exp-dir", exp.path, "--out", os.path.join(exp.tmp, name)], exp.tmp)
    a, b = os.path.join(exp.tmp, "pnn_a"), os.path.join(exp.tmp, "pnn_b")
    assert _listing(a) == _listing(b) == ["patchnn.json", "sample_0000.gif", "sample_0001.gif", "samples.npy"]
    assert _bytes(os.path.join(a, "samples.npy")) == _bytes(os.path.join(b, "samples.npy"))
    info = _json(os.path.join(a, "patchnn.json"))
    assert not any(k.startswith("guide") for k in info)
    assert sorted(info) == ["alpha", "final_score", "final_score_per_sample", "input", "iters", "level_sizes", "min_size", "noise",
                            "num_samples", "patch", "ratio", "real_shape", "seconds_per_sample", "seed", "size"]
    assert info["real_shape"] == [14, 30, 40] and list(np.load(os.path.join(a, "samples.npy")).shape) == [2, 14, 30, 40, 3]


def test_generate_patchnn_guide_shapes_directory_json_and_the_mask(exp):
    """A guide of another size (retargeting) at the middle level of three, with noise, kept only inside a feathered hole."""
    guide = _clip((10, 24, 32), 5)
    np.save(os.path.join(exp.tmp, "pguide.npy"), guide)
    hole = np.zeros((10, 24, 32), bool)
    hole[3:6, 9:14, 12:19] = True
    np.save(os.path.join(exp.tmp, "phole.npy"), hole)
    flags = ["--exp-dir", exp.path, "--guide", "pguide.npy", "--guide-level", "1", "--guide-noise", "0.4", "--guide-mask", "phole.npy",
             "--guide-feather"] + [str(r) for r in FEATHER]
    _child(PNN + flags, exp.tmp)
    _child(PNN + flags + ["--out", os.path.join(exp.tmp, "pguide_again")], exp.tmp)
    out = os.path.join(exp.path, "eval", "samples_patchnn_guide1")
    assert _listing(out) == ["patchnn.json", "sample_0000.gif", "sample_0001.gif", "samples.npy"]
    arr = np.load(os.path.join(out, "samples.npy"))
    assert arr.dtype == np.uint8 and arr.shape == (2, 10, 24, 32, 3)
    assert _bytes(os.path.join(out, "samples.npy")) == _bytes(os.path.join(exp.tmp, "pguide_again", "samples.npy"))
    info = _json(os.path.join(out, "patchnn.json"))
    assert info["guide"] == os.path.join(exp.tmp, "pguide.npy") and info["guide_level"] == 1 and info["guide_noise"] == 0.4
    assert info["guide_mask"] == os.path.join(exp.tmp, "phole.npy") and info["guide_feather"] == list(FEATHER)
    assert info["size"] == [10, 24, 32] and info["real_shape"] == [14, 30, 40] and len(info["level_sizes"]) == 3
    far = far_from_hole(hole, FEATHER)
    assert 0 < far.sum() < far.size
    for s in arr:
        assert np.array_equal(s[far], guide[far])
        assert not np.array_equal(s[hole], guide[hole])
    assert not np.array_equal(arr[0], arr[1])          # sample i draws under seed + i
