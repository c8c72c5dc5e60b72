"""The host side of snapshots and resume (hp_vae_gan_amd.snapshot): flags and refusals, the recorded command line, the loader
position, scalars truncation and the file round trip.  Nothing here needs a device; the refusals are shown in children that
see no device, where asking for one would end the program with gpu_device()'s message instead."""
import os
import random
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import programs, snapshot  # noqa: E402
from hp_vae_gan_amd import train_video_baselines as tvb  # noqa: E402

SNAP_FLAGS = {"--snapshot-interval", "--snapshot-exit-after", "--resume"}
COMMON = {"--netG", "--netD", "--manualSeed", "--nc-im", "--nfc", "--ker-size", "--num-layer", "--stride", "--padd-size",
          "--scale-factor", "--noise_amp", "--min-size", "--max-size", "--niter", "--lr-g", "--lr-d", "--beta1", "--lambda-grad",
          "--disc-loss-weight", "--lr-scale", "--train-depth", "--hflip", "--img-size", "--stop-scale-time", "--data-rep",
          "--checkname", "--batch-size", "--print-interval", "--no-cuda", "--run-dir", "--no-hip-graph", "--generator",
          "--discriminator", "--mode", "--visualize", "-h", "--help"}
VIDEO = {"--video-path", "--start-frame", "--max-frames", "--sampling-rates"}
HPVAE = {"--latent-dim", "--vae-levels", "--enc-blocks", "--rec-weight", "--kl-weight", "--grad-clip", "--const-amp", "--train-all"}
BASELINE = {"--nc-z", "--Gsteps", "--Dsteps", "--alpha"}


def _flags(parser):
    return {s for a in parser._actions for s in a.option_strings}


def test_reference_parsers_hold_exactly_the_flags_they_held():
    assert _flags(programs.build_parser("video")) == COMMON | VIDEO | HPVAE
    assert _flags(programs.build_parser("image")) == COMMON | HPVAE | {"--image-path", "--tag"}
    assert _flags(tvb.build_baseline_parser()) == COMMON | VIDEO | BASELINE


def _bare(cls, kind=None):
    prog = cls.__new__(cls)
    if kind:
        prog.kind = kind
    return prog


@pytest.mark.parametrize("prog", [_bare(programs.Program, "video"), _bare(programs.Program, "image"), _bare(tvb.BaselineProgram)])
def test_program_parsers_hold_the_snapshot_flags_with_their_defaults(prog):
    p = prog.parser()
    base = tvb.build_baseline_parser() if isinstance(prog, tvb.BaselineProgram) else programs.build_parser(prog.kind)
    assert _flags(p) == _flags(base) | SNAP_FLAGS
    path = "--image-path" if getattr(prog, "kind", "video") == "image" else "--video-path"
    opt = p.parse_args([path, "x"])
    assert opt.snapshot_interval == 0 and opt.snapshot_exit_after is None and opt.resume == ""
    opt = p.parse_args([path, "x", "--snapshot-interval", "7", "--snapshot-exit-after", "2"])
    assert opt.snapshot_interval == 7 and opt.snapshot_exit_after == 2


def test_program_names():
    assert _bare(programs.Program, "video").program_name() == "train_video"
    assert _bare(programs.Program, "image").program_name() == "train_image"
    assert _bare(tvb.BaselineProgram, "video").program_name() == "train_video_baselines"
    assert set(snapshot.PROGRAMS) == {"train_video", "train_image", "train_video_baselines"}


# ---------------------------------------------------------------------------------------------------------------- refusals
def _header(program="train_video", version=snapshot.VERSION):
    return {"version": version, "program": program, "argv": ["--video-path", "clip.npy"], "snapshot_interval": 4, "stage": 0,
            "iteration": 4, "niter": 10, "stage_done": False, "scalars_bytes": 0, "digest": 1}


@pytest.mark.parametrize("flags,message", [
    (["--video-path", "clip.npy", "--snapshot-interval", "-1"], "is negative"),
    (["--video-path", "clip.npy", "--snapshot-exit-after", "2"], "needs --snapshot-interval"),
    (["--video-path", "clip.npy", "--snapshot-interval", "0", "--snapshot-exit-after", "2"], "needs --snapshot-interval"),
    (["--video-path", "clip.npy", "--snapshot-interval", "4", "--snapshot-exit-after", "0"], "1 or more"),
    (["--resume", "exp", "--niter", "5"], "takes every setting from the snapshot"),
    (["--resume", "exp", "--video-path", "clip.npy"], "takes every setting from the snapshot"),
    (["--resume", "exp", "--netG", "exp/netG.pth"], "--netG starts another run"),
    (["--resume", "nothing_here"], "no snapshot.pth in"),
    (["--resume", "other"], "was written by train_image, not by train_video"),
    (["--resume", "old"], "format version 0"),
    (["--resume", "broken"], "cannot be read")])
def test_refused_in_a_child_before_any_device_use(tmp_path, flags, message):
    for name, snap in (("exp", _header()), ("other", _header(program="train_image")), ("old", _header(version=0))):
        os.makedirs(str(tmp_path / name))
        torch.save(snap, str(tmp_path / name / "snapshot.pth"))
    os.makedirs(str(tmp_path / "broken"))
    with open(str(tmp_path / "broken" / "snapshot.pth"), "wb") as f:
        f.write(b"not a snapshot")
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.train_video"] + flags, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stderr[-2000:])
    assert "no GPU visible" not in r.stderr
    assert not os.path.exists(str(tmp_path / "run"))


@pytest.mark.parametrize("module,program", [("train_image", "train_video"), ("train_video_baselines", "train_video")])
def test_the_other_programs_refuse_a_foreign_snapshot(tmp_path, module, program):
    os.makedirs(str(tmp_path / "exp"))
    torch.save(_header(program=program), str(tmp_path / "exp" / "snapshot.pth"))
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd." + module, "--resume", "exp"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "was written by %s, not by %s" % (program, module) in r.stderr, r.stderr[-2000:]


def test_check_flags_in_process():
    ns, rest = snapshot.split_flags(["--resume", "exp", "--snapshot-exit-after", "1", "--snapshot-interval", "3"])
    assert (ns.resume, ns.snapshot_exit_after, ns.snapshot_interval, rest) == ("exp", 1, 3, [])
    snapshot.check_flags(ns, rest)
    ns, rest = snapshot.split_flags(["--resume", "exp", "--snapshot-exit-after", "1"])
    assert ns.snapshot_interval is None      # the recorded interval holds
    snapshot.check_flags(ns, rest)
    with pytest.raises(SystemExit):
        snapshot.check_flags(*snapshot.split_flags(["--resume", "exp", "--netG=x"]))


# ------------------------------------------------------------------------------------------------- recorded command line
def test_recorded_command_line():
    argv = ["--video-path", "a b.npy", "--snapshot-interval", "4", "--checkname", "c", "--snapshot-exit-after=2", "--run-dir",
            "r", "--niter", "9"]
    ns, rest = snapshot.split_flags(argv)
    assert rest == ["--video-path", "a b.npy", "--checkname", "c", "--run-dir", "r", "--niter", "9"]
    assert snapshot.recorded_command_line(rest, 1234, False) == rest + ["--manualSeed", "1234"]
    with_seed = rest + ["--manualSeed", "5"]
    assert snapshot.recorded_command_line(with_seed, 5, True) == with_seed
    # the recorded line parses to the same settings, seed included, and holds none of the three flags
    p = programs.build_parser("video")
    a = p.parse_args(snapshot.recorded_command_line(rest, 1234, False))
    assert (a.video_path, a.checkname, a.run_dir, a.niter, a.manualSeed) == ("a b.npy", "c", "r", 9, 1234)


def test_resolve_takes_everything_from_the_snapshot(tmp_path):
    exp = str(tmp_path / "exp")
    os.makedirs(exp)
    snap = _header()
    snap["argv"] = ["--video-path", "clip.npy", "--niter", "10", "--manualSeed", "77"]
    snapshot.write(exp, snap)
    assert not os.path.exists(os.path.join(exp, "snapshot.pth.tmp"))
    argv, ns, got = snapshot.resolve(["--resume", exp], "train_video")
    assert argv == snap["argv"] and ns.snapshot_interval == 4 and ns.snapshot_exit_after is None and got["iteration"] == 4
    argv, ns, got = snapshot.resolve(["--resume", exp, "--snapshot-interval", "2", "--snapshot-exit-after", "1"], "train_video")
    assert ns.snapshot_interval == 2 and ns.snapshot_exit_after == 1
    argv, ns, got = snapshot.resolve(["--video-path", "x", "--niter", "3"], "train_video")
    assert argv == ["--video-path", "x", "--niter", "3"] and ns.snapshot_interval == 0 and got is None


# --------------------------------------------------------------------------------------------------------- loader position
class _Toy(torch.utils.data.Dataset):
    def __len__(self):
        return 7

    def __getitem__(self, i):
        return torch.tensor([float(i), random.random()])


def _loader():
    return torch.utils.data.DataLoader(_Toy(), shuffle=True, drop_last=True, batch_size=2, num_workers=0)


class _Data:
    def __init__(self, loader, pos):
        self.loader, self.pos = loader, pos

    def __iter__(self):
        return snapshot.iterate(self.loader, self.pos)


def _loop(data, n, start=0, stop_at=None, pos=None):
    """train._train_loop's use of the data: next(), a new iterator when exhausted; one torch.rand draw per iteration."""
    out, saved = [], None
    iterator = iter(data)
    for k in range(start, n):
        try:
            item = next(iterator)
        except StopIteration:
            iterator = iter(data)
            item = next(iterator)
        out.append((item.clone(), torch.rand(1)))
        if stop_at is not None and k + 1 == stop_at:
            saved = (pos.state(), snapshot.host_rng_state())
    return out, saved


def test_loader_position_restores_every_stop_point_across_epoch_ends():
    N = 12     # three batches an epoch: stop points 1..9 cover every place in an epoch and three epoch ends
    random.seed(5)
    torch.manual_seed(5)
    plain, _ = _loop(_Data(_loader(), None), N)
    for stop in range(1, 10):
        random.seed(5)
        torch.manual_seed(5)
        pos = snapshot.LoaderPosition()
        full, saved = _loop(_Data(_loader(), pos), N, stop_at=stop, pos=pos)
        # counting changes nothing
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(full, plain))
        state, now = saved
        assert state["taken"] == (stop - 1) % 3 + 1
        # through a file, into a process whose generators stand elsewhere
        random.seed(999)
        torch.manual_seed(999)
        pos2 = snapshot.LoaderPosition()
        pos2.restore(state, now)
        rest, _ = _loop(_Data(_loader(), pos2), N, start=stop)
        assert len(rest) == N - stop
        for k, (a, b) in enumerate(zip(rest, full[stop:])):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (stop, stop + k)
        # the hooks that leave something out do make a difference
        # (at an epoch's end a dropped position is no defect: the next epoch starts from the same generators either way)
        for skip in ("loader", "random") if state["taken"] < 3 else ("random",):
            random.seed(999)
            torch.manual_seed(999)
            pos3 = snapshot.LoaderPosition()
            pos3.restore(state, now, skip=(skip,))
            other, _ = _loop(_Data(_loader(), pos3), N, start=stop)
            assert not all(torch.equal(a[0], b[0]) for a, b in zip(other, full[stop:])), (stop, skip)


def test_loader_state_survives_the_file(tmp_path):
    random.seed(1)
    torch.manual_seed(1)
    pos = snapshot.LoaderPosition()
    full, saved = _loop(_Data(_loader(), pos), 8, stop_at=4, pos=pos)
    snap = dict(_header(), loader=saved[0], rng=saved[1], netG={"w": torch.arange(6, dtype=torch.float32).view(2, 3)},
                Noise_Amps=[1, 0.25], noise_amp=0.25, optimizerG={"steps": 4, "m": [torch.ones(3)], "v": [torch.zeros(3)]},
                digest=(1 << 64) - 3)
    exp = str(tmp_path)
    size = snapshot.write(exp, snap)
    assert size == os.path.getsize(os.path.join(exp, "snapshot.pth"))
    got = snapshot.load(exp, "train_video")          # torch.load(weights_only=True)
    assert got["digest"] == (1 << 64) - 3 and got["Noise_Amps"] == [1, 0.25] and got["argv"] == snap["argv"]
    assert torch.equal(got["netG"]["w"], snap["netG"]["w"]) and torch.equal(got["optimizerG"]["m"][0], torch.ones(3))
    assert torch.equal(got["rng"]["torch"], saved[1]["torch"])
    assert snapshot._as_getstate(got["rng"]["python"]) == saved[1]["python"]
    random.seed(999)
    torch.manual_seed(999)
    pos2 = snapshot.LoaderPosition()
    pos2.restore(got["loader"], got["rng"])
    rest, _ = _loop(_Data(_loader(), pos2), 8, start=4)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(rest, full[4:]))


def test_set_rng_state_brings_back_the_initial_seed():
    torch.manual_seed(4242)
    st = snapshot.host_rng_state()
    torch.manual_seed(1)
    snapshot.set_host_rng_state(st)
    assert torch.initial_seed() == 4242


# ------------------------------------------------------------------------------------------------------------ scalars file
def test_scalars_truncation(tmp_path):
    path = str(tmp_path / "scalars.jsonl")
    lines = ['{"tag": "a", "step": %d, "value": 0.5}\n' % i for i in range(6)]
    with open(path, "w") as f:
        f.write("".join(lines))
    keep = len("".join(lines[:4]))
    snapshot.truncate_scalars(path, keep)
    with open(path) as f:
        assert f.read() == "".join(lines[:4])
    snapshot.truncate_scalars(path, keep)             # already that long: untouched
    assert os.path.getsize(path) == keep
    with open(path, "a") as f:                        # the resumed run appends
        f.write(lines[4])
    with open(path) as f:
        assert f.read() == "".join(lines[:5])
    with pytest.raises(SystemExit):
        snapshot.truncate_scalars(path, 10 ** 6)      # shorter than recorded: not this run's file
    with pytest.raises(SystemExit):
        snapshot.truncate_scalars(str(tmp_path / "missing.jsonl"), 5)
