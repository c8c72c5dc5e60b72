"""Host logic of the programs (hp_vae_gan_amd.train_video / train_image / generate) and of the device loss log: no GPU.

The parsers are held to tests/golden/cli_flags.json, which tests/golden/make_cli_flags.py reads from the reference's two
programs with `ast` (names, types, defaults, nargs, actions and `required` only)."""
import ast
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from hp_vae_gan_amd import programs, telemetry, train_video_baselines
from hp_vae_gan_amd import train as hp_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXTRA = {"video": {"run_dir": "run", "no_hip_graph": False}, "image": {"run_dir": "run", "no_hip_graph": False}}


def _actions(parser):
    return {a.dest: a for a in parser._actions if a.dest != "help"}


@pytest.mark.parametrize("kind", ["video", "image"])
def test_parser_matches_reference_flags(kind):
    with open(os.path.join(GOLDEN, "cli_flags.json")) as f:
        ref = json.load(f)["train_" + kind]
    acts = _actions(programs.build_parser(kind))
    assert set(acts) == {e["dest"] for e in ref} | set(EXTRA[kind])
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
    for dest, default in EXTRA[kind].items():
        assert acts[dest].default == default
    assert acts["no_hip_graph"].const is True


# the flags both trainer parsers hold differ only here: the generator's default (golden) and four help texts
FORKED_HELP = {"generator", "discriminator", "mode", "visualize"}


def test_shared_flags_are_not_forked():
    video, base = _actions(programs.build_parser("video")), _actions(train_video_baselines.build_baseline_parser())
    shared = set(video) & set(base)
    assert len(shared) >= 35 and FORKED_HELP <= shared
    for dest in sorted(shared):
        a, b = video[dest], base[dest]
        assert (a.type, a.nargs) == (b.type, b.nargs), dest
        assert a.default == b.default or dest == "generator", dest
        assert (a.help == b.help) == (dest not in FORKED_HELP), dest
    assert (video["generator"].default, base["generator"].default) == ("GeneratorHPVAEGAN", "GeneratorCSG")   # the goldens'


def test_experiment_numbering(tmp_path):
    run = str(tmp_path / "run")
    dirs = [programs.experiment_dir(run, "clip", "DEBUG") for _ in range(3)]
    assert [os.path.basename(d) for d in dirs] == ["experiment_0", "experiment_1", "experiment_2"]
    assert all(os.path.isdir(os.path.join(d, "eval")) for d in dirs)
    os.makedirs(os.path.join(run, "clip", "DEBUG", "experiment_9"))
    assert os.path.basename(programs.experiment_dir(run, "clip", "DEBUG")) == "experiment_10"
    assert os.path.basename(programs.experiment_dir(run, "clip", "DEBUG")) == "experiment_11"
    assert os.path.basename(programs.experiment_dir(run, "other", "DEBUG")) == "experiment_0"


def test_clip_name(tmp_path):
    assert programs.clip_name("data/air_balloons.jpg") == "air_balloons"
    assert programs.clip_name("/x/y/clip.v2.npy") == "clip.v2"
    d = tmp_path / "frames.of.clip"
    d.mkdir()
    assert programs.clip_name(str(d)) == "frames.of.clip"
    assert programs.clip_name(str(d) + "/") == "frames.of.clip"


def test_resume_bookkeeping(tmp_path):
    exp = tmp_path / "experiment_0"
    exp.mkdir()
    torch.save({"scale": 4, "state_dict": {}, "optimizer": {}, "noise_amps": [1, 0.1, 0.2, 0.3, 0.4]}, exp / "netG.pth")
    torch.save({"data": [1, 0.1, 0.2, 0.3, 0.4]}, exp / "Noise_Amps.pth")
    scale, resume_dir = programs.resume_info(str(exp / "netG.pth"))
    assert (scale, resume_dir) == (4, str(exp))
    # a resumed run trains the saved scale again without growing, then grows at every later scale
    assert programs.stage_plan(scale, scale, 5) == [(4, False), (5, True)]
    assert programs.stage_plan(0, -1, 3) == [(0, False), (1, True), (2, True), (3, True)]
    # every trained stage appends its iteration-0 amplitude: the list grows one past the number of scales
    amps = list(torch.load(exp / "Noise_Amps.pth", weights_only=True)["data"])
    for s, _ in programs.stage_plan(scale, scale, 5):
        fake = types.SimpleNamespace(opt=types.SimpleNamespace(const_amp=True, Noise_Amps=amps, scale_idx=s))
        hp_train.StageTrainer.calibrate_noise_amp(fake, None, None)
    assert len(amps) == 5 + 1 + 1
    with pytest.raises(RuntimeError, match="no <G> checkpoint"):
        programs.resume_info(str(exp / "missing.pth"))


def test_drain_arithmetic():
    cap, K = 4, 2
    table = np.arange(cap * K, dtype=np.float32).reshape(cap, K)
    idx, rows, lost = telemetry.drain_rows(3, 0, cap, table)
    assert idx.tolist() == [0, 1, 2] and lost == 0 and np.array_equal(rows, table[:3])
    idx, rows, lost = telemetry.drain_rows(3, 3, cap, table)
    assert len(idx) == 0 and rows.shape == (0, K) and lost == 0
    idx, rows, lost = telemetry.drain_rows(7, 3, cap, table)       # exactly one ring: rows 3..6 at slots 3,0,1,2
    assert idx.tolist() == [3, 4, 5, 6] and lost == 0 and np.array_equal(rows, table[[3, 0, 1, 2]])
    idx, rows, lost = telemetry.drain_rows(13, 3, cap, table)      # 10 written, ring of 4: 6 lost, the newest 4 kept
    assert lost == 6 and idx.tolist() == [9, 10, 11, 12] and np.array_equal(rows, table[[1, 2, 3, 0]])
    with pytest.raises(RuntimeError):
        telemetry.drain_rows(2, 3, cap, table)


def test_loss_log_columns():
    assert hp_train.loss_log_columns(False) == ["rec_vae_loss", "kl_loss", "total_loss", "grad_norm"]
    assert hp_train.loss_log_columns(True) == ["rec_loss", "errG", "errD_real", "errD_fake", "gradient_penalty",
                                               "total_loss", "grad_norm"]
    assert set(hp_train.loss_log_columns(True) + hp_train.loss_log_columns(False)) <= set(programs.TAGS)
    assert {programs.TAGS[k] for k in ("rec_vae_loss", "kl_loss", "rec_loss", "errG", "errD_fake", "errD_real")} == \
        {"Rec VAE", "KLD", "rec loss", "errG", "errD_fake", "errD_real"}


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=120)


def test_cli_refusals(tmp_path):
    r = _run(["hp_vae_gan_amd.train_video", "--video-path", "clip.mp4"], str(tmp_path))
    assert r.returncode != 0 and "no video decoder" in r.stderr
    r = _run(["hp_vae_gan_amd.train_image", "--image-path", "x.png", "--no-cuda"], str(tmp_path))
    assert r.returncode != 0 and "no CPU path" in r.stderr
    r = _run(["hp_vae_gan_amd.train_video"], str(tmp_path))
    assert r.returncode == 2 and "--video-path" in r.stderr
    assert not os.path.exists(tmp_path / "run")


# module -> flags that no other program holds together (train_video and generate have no flag to themselves)
ONLY = {"train_video": ("--vae-levels", "--sampling-rates"), "train_image": ("--tag",), "train_video_baselines": ("--Dsteps",),
        "generate": ("--num-samples", "--batch-size"), "evaluate": ("--swd-seed",), "generate_patchnn": ("--save-levels",)}


@pytest.mark.parametrize("name", sorted(ONLY))
def test_every_program_module_runs_alone(name, tmp_path):
    """`python -m` loads the module as __main__ in a fresh process: it must import on its own, without another program module,
    and show its own flags."""
    r = _run(["hp_vae_gan_amd." + name, "--help"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hp_vae_gan_amd." + name + " " in r.stdout
    assert all(flag in r.stdout for flag in ONLY[name]), r.stdout
    for other, flags in ONLY.items():
        assert other == name or not all(flag in r.stdout for flag in flags), other
    with open(os.path.join(ROOT, "hp-vae-gan_amd", name + ".py")) as f:
        froms = [n for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.ImportFrom)]
    assert not ({n.module for n in froms} | {a.name for n in froms for a in n.names}) & (set(ONLY) - {name})
