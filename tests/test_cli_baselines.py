"""Host logic of hp_vae_gan_amd.train_video_baselines: no GPU.

The parser is held to tests/golden/cli_flags_baselines.json, which tests/golden/make_cli_flags_baselines.py reads from the
reference's train_video_baselines.py with `ast` (names, types, defaults, nargs, actions and `required` only).  The other
tests cover the Z_init shape rule, the critic's warm-start directory, the scalar tags and the loss-log columns."""
import json
import os
import subprocess
import sys
import types

import pytest

from hp_vae_gan_amd import programs, train_video_baselines
from hp_vae_gan_amd import train as hp_train
from hp_vae_gan_amd import utils as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXTRA = {"run_dir": "run", "no_hip_graph": False}


def _actions(parser):
    return {a.dest: a for a in parser._actions if a.dest != "help"}


def test_parser_matches_reference_flags():
    with open(os.path.join(GOLDEN, "cli_flags_baselines.json")) as f:
        ref = json.load(f)["train_video_baselines"]
    acts = _actions(train_video_baselines.build_baseline_parser())
    assert set(acts) == {e["dest"] for e in ref} | set(EXTRA)
    for e in ref:
        a = acts[e["dest"]]
        assert a.option_strings == e["names"], e
        assert a.default == e.get("default"), e
        assert a.required == e.get("required", False), e
        assert a.nargs == e.get("nargs", 0 if e.get("action") == "store_true" else None), e
        if "type" in e:
            assert a.type is {"int": int, "float": float, "str": str}[e["type"]], e
        else:
            assert a.type is None, e
        if e.get("action") == "store_true":
            assert a.const is True and a.nargs == 0, e
    for dest, default in EXTRA.items():
        assert acts[dest].default == default
    assert acts["no_hip_graph"].const is True
    # what sets it apart from train_video's parser
    assert acts["generator"].default == "GeneratorCSG"
    assert {"nc_z", "Gsteps", "Dsteps", "alpha"} <= set(acts)
    assert not {"latent_dim", "vae_levels", "enc_blocks", "rec_weight", "kl_weight", "grad_clip", "const_amp",
                "train_all"} & set(acts)


def _opt(argv=()):
    opt = train_video_baselines.build_baseline_parser().parse_args(["--video-path", "clip.npy", "--min-size", "16",
                                                                    "--max-size", "40", "--img-size", "40"] + list(argv))
    opt.noise_amp_init = opt.noise_amp
    opt.scale_factor_init = opt.scale_factor
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    opt.ar = 0.75
    opt.org_fps = 24.0
    opt.fps_lcm = 12
    return opt


def test_z_init_shape_fresh_and_resumed():
    opt = _opt(["--batch-size", "3"])
    S = opt.stop_scale
    w0 = hu.get_scales_by_index(0, opt.scale_factor, S, opt.img_size)
    # a fresh run draws it at scale 0: exactly level 0's volume
    opt.td = hu.get_fps_td_by_index(0, opt)[1]
    assert train_video_baselines.z_init_shape(opt) == [3, 3] + hu.images.level_shape_3d(0, opt)
    # a resume at the last scale draws it there: level 0's height and width, the resumed scale's time depth
    opt.td = hu.get_fps_td_by_index(S, opt)[1]
    assert opt.td != hu.images.level_shape_3d(0, opt)[0]
    assert train_video_baselines.z_init_shape(opt) == [3, 3, opt.td, int(w0 * opt.ar), w0]


def test_netD_warm_start_directory():
    fresh = types.SimpleNamespace(netG="", resumed_idx=-1, scale_idx=0)
    assert train_video_baselines.baseline_netD_dir(fresh, "exp") is None
    fresh.scale_idx = 3
    assert train_video_baselines.baseline_netD_dir(fresh, "exp") == "exp"
    resumed = types.SimpleNamespace(netG="old/netG.pth", resume_dir="old", resumed_idx=4, scale_idx=4)
    assert train_video_baselines.baseline_netD_dir(resumed, "exp") == "old"     # the resumed scale: the resume directory
    resumed.scale_idx = 5
    assert train_video_baselines.baseline_netD_dir(resumed, "exp") == "exp"     # later scales: this run's own
    resumed.resumed_idx, resumed.scale_idx = 0, 0
    assert train_video_baselines.baseline_netD_dir(resumed, "exp") is None


def test_loss_log_columns_and_tags():
    assert hp_train.baseline_loss_log_columns(0.0) == ["errD_real", "errD_fake", "gradient_penalty", "errG"]
    assert hp_train.baseline_loss_log_columns(10.0) == ["errD_real", "errD_fake", "gradient_penalty", "errG", "rec_loss"]
    tags = train_video_baselines.BASELINE_TAGS
    assert set(hp_train.baseline_loss_log_columns(1.0)) == set(tags)
    assert {tags[k] for k in ("errG", "errD_fake", "errD_real", "rec_loss")} == {"errG", "errD_fake", "errD_real", "rec_loss"}
    assert tags["gradient_penalty"] == "gradient_penalty"
    assert train_video_baselines.BaselineProgram.tags is tags and programs.Program.tags is programs.TAGS
    assert programs.TAGS["rec_loss"] == "rec loss"                 # train_video's tag is unchanged


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=120)


def test_cli_refusals(tmp_path):
    r = _run(["hp_vae_gan_amd.train_video_baselines", "--video-path", "clip.mp4"], str(tmp_path))
    assert r.returncode != 0 and "no video decoder" in r.stderr
    r = _run(["hp_vae_gan_amd.train_video_baselines", "--video-path", "clip.npy", "--no-cuda"], str(tmp_path))
    assert r.returncode != 0 and "no CPU path" in r.stderr
    r = _run(["hp_vae_gan_amd.train_video_baselines"], str(tmp_path))
    assert r.returncode == 2 and "--video-path" in r.stderr
    r = _run(["hp_vae_gan_amd.train_video_baselines", "--help"], str(tmp_path))
    assert r.returncode == 0 and "--Dsteps" in r.stdout and "--no-hip-graph" in r.stdout
    assert not os.path.exists(tmp_path / "run")


@pytest.mark.parametrize("alpha", [0.0, 10.0])
def test_noise_amp_scalar_only_with_reconstruction(alpha):
    prog = train_video_baselines.BaselineProgram.__new__(train_video_baselines.BaselineProgram)
    prog.opt = types.SimpleNamespace(alpha=alpha)
    assert prog.logs_noise_amp() == (alpha > 0)
