"""--snapshot-interval / --snapshot-exit-after / --resume on the GPU: a run that is stopped and resumed is THE SAME run.

R0 is an uninterrupted run with --snapshot-interval 4; R1 the same command line stopped by --snapshot-exit-after and continued
by --resume.  R1 must leave what R0 leaves: every tensor of netG.pth, netD_<s>.pth, Noise_Amps.pth and Z_init.pth equal as bits,
the optimizer dicts equal, scalars.jsonl equal byte for byte, and the digest equal in the logbook line of every snapshot both
wrote.

The smallest run with every kind of stage: SMALL of tests/test_programs_gpu.py with min_size 32, so stop_scale is 2 (two VAE
stages and one GAN stage; the baselines: three critic stages), 10 iterations a stage, a snapshot every 4: snapshots 1-3 in
stage 0 (k = 4, k = 8, stage done), 4-6 in stage 1, 7-9 in stage 2.  Slices run in-process the way _program_run does: a new
Program per slice, ops._rng_states.clear(), and random / torch seeded with 999 before each resume so that nothing left over
from the slice before can help.  One case runs as child processes.

Seeded defects (snapshot.restore's skip hook) show that the comparison can fail: each leaves one part of the state as a
fresh stage has it and must end somewhere else than R0.  The loader-position defect runs on an input of two different images:
with one image every item of the dataset is the same image and the flips are drawn from python's generator in the order of
use, so a reset position provably changes nothing there."""
import json
import os
import random
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import ops, programs, snapshot  # noqa: E402
from hp_vae_gan_amd import train_video_baselines as tvb  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = ["--nfc", "8", "--min-size", "32", "--max-size", "40", "--img-size", "40"]
HPVAE = ["--latent-dim", "8", "--vae-levels", "2"]
RUN = ["--niter", "10", "--print-interval", "3", "--manualSeed", "3"]
SNAP = ["--snapshot-interval", "4"]
LINE = re.compile(r"^Snapshot: stage (\d+), iteration (\d+)/\d+( \(stage done\))?, \d+ bytes, digest ([0-9a-f]{16})$")


def _clip(n=16, h=30, w=40, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("snap"))
    np.save(os.path.join(d, "clip.npy"), _clip())
    np.save(os.path.join(d, "one.npy"), _clip(1, seed=1))
    np.save(os.path.join(d, "two.npy"), _clip(2, seed=2))
    return {"dir": d, "runs": {}, "n": 0}


def _make(kind, argv):
    if kind == "baselines":
        return tvb.BaselineProgram(argv)
    return programs.Program(kind, argv)


def _argv(work, kind, src, extra):
    work["n"] += 1
    flag = "--image-path" if kind == "image" else "--video-path"
    return [flag, os.path.join(work["dir"], src), "--run-dir", os.path.join(work["dir"], "run%d" % work["n"])] + RUN + SIZES + \
        (HPVAE if kind != "baselines" else []) + extra


def _fresh(work, kind, src, extra):
    ops._rng_states.clear()
    prog = _make(kind, _argv(work, kind, src, extra))
    assert prog.opt.stop_scale == 2
    return prog.run()


def _resume(kind, exp, extra=(), skip=(), verify=True):
    ops._rng_states.clear()
    random.seed(999)
    torch.manual_seed(999)
    prog = _make(kind, ["--resume", exp] + list(extra))
    assert prog.exp_dir == os.path.normpath(exp)
    prog.restore_skip, prog.restore_verify = skip, verify
    return prog.run()


def _copy(exp):
    """A stopped experiment is resumed in place: every continuation gets its own copy."""
    n = 0
    while os.path.exists("%s_c%d" % (exp, n)):
        n += 1
    return shutil.copytree(exp, "%s_c%d" % (exp, n))


def _cached(work, key, make):
    if key not in work["runs"]:
        t0 = time.time()
        work["runs"][key] = make()
        print("%s: %.1f s" % (key, time.time() - t0))
    return work["runs"][key]


def _r0(work, kind, src, extra):
    """exp dir of the uninterrupted run with snapshots."""
    def make():
        prog = _fresh(work, kind, src, extra + SNAP)
        assert len(prog.trainers) == 3
        if kind != "baselines":
            assert [t.netD is not None for t in prog.trainers] == [False, False, True]    # two VAE stages, one GAN stage
        assert _digests(prog.exp_dir).keys() == {(s, k, d) for s in range(3) for k, d in ((4, False), (8, False), (10, True))}
        return prog.exp_dir
    return _cached(work, ("r0", kind, src, tuple(extra)), make)


def _stopped(work, kind, src, extra, after):
    """exp dir of the same run stopped after its `after`-th snapshot (never resumed: continuations copy it)."""
    def make():
        prog = _fresh(work, kind, src, extra + SNAP + ["--snapshot-exit-after", str(after)])
        assert prog.snapshots_written == after
        with open(os.path.join(prog.exp_dir, "logbook.txt")) as f:
            assert "Stopped after snapshot %d" % after in f.read()
        return prog.exp_dir
    return _cached(work, ("stopped", kind, src, tuple(extra), after), make)


# -------------------------------------------------------------------------------------------------------------- comparison
def _bits_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_bits_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_bits_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def _digests(exp):
    out = {}
    with open(os.path.join(exp, "logbook.txt")) as f:
        for ln in f:
            m = LINE.match(ln.rstrip("\n"))
            if m:
                out[(int(m.group(1)), int(m.group(2)), m.group(3) is not None)] = m.group(4)
    return out


def _difference(a, b, digests=True):
    """None when experiment b left what experiment a left, else the first thing that differs."""
    names = sorted(n for n in os.listdir(a) if n.endswith(".pth") and n != snapshot.FILE)
    assert "netG.pth" in names and "Noise_Amps.pth" in names and "netD_2.pth" in names
    if names != sorted(n for n in os.listdir(b) if n.endswith(".pth") and n != snapshot.FILE):
        return "checkpoint files"
    for n in names:
        x = torch.load(os.path.join(a, n), weights_only=True)
        y = torch.load(os.path.join(b, n), weights_only=True)
        for k in x:
            if k not in y or not _bits_equal(x[k], y[k]):
                return "%s[%r]" % (n, k)
    with open(os.path.join(a, "scalars.jsonl"), "rb") as f, open(os.path.join(b, "scalars.jsonl"), "rb") as g:
        if f.read() != g.read():
            return "scalars.jsonl"
    if digests:
        da, db = _digests(a), _digests(b)
        common = da.keys() & db.keys()
        assert common
        for key in sorted(common):
            if da[key] != db[key]:
                return "digest of snapshot %r" % (key,)
    return None


def _header(exp):
    snap = torch.load(os.path.join(exp, snapshot.FILE), weights_only=True)
    return snap["stage"], snap["iteration"], snap["stage_done"]


# -------------------------------------------------------------------------------------------------------------------- cases
VIS = ["--visualize"]


def test_video_stopped_twice_in_the_gan_stage_equals_the_uninterrupted_run(work):
    r0 = _r0(work, "video", "clip.npy", VIS)
    exp = _copy(_stopped(work, "video", "clip.npy", VIS, 7))
    assert _header(exp) == (2, 4, False)
    mid = _resume("video", exp, ["--snapshot-exit-after", "1"])
    assert _header(exp) == (2, 8, False) and mid.snapshots_written == 1
    # resumed at k = 4: one eager iteration, the capture's warm-up, then replays
    assert mid.resumed_trainer._graph is not None and mid.resumed_trainer.iteration == 8
    last = _resume("video", exp)
    assert _header(exp) == (2, 10, True) and last.trainers[-1].iteration == 10
    assert last.trainers[-1].optimizerG.steps() == 10
    assert _difference(r0, exp) is None
    assert len(_digests(exp)) == 9
    with open(os.path.join(exp, "scalars.jsonl")) as f:
        rows = [json.loads(ln) for ln in f]
    assert sorted(r["step"] for r in rows if r["tag"] == "Video/Scale 2/errG") == list(range(10))


def test_video_resumed_from_a_finished_stage(work):
    r0 = _r0(work, "video", "clip.npy", VIS)
    exp = _copy(_stopped(work, "video", "clip.npy", VIS, 3))
    assert _header(exp) == (0, 10, True)
    last = _resume("video", exp)
    assert len(last.trainers) == 2 and last.trainers[-1]._graph is not None
    assert _difference(r0, exp) is None


def test_video_eager_with_flips(work):
    extra = ["--no-hip-graph", "--hflip"]
    r0 = _r0(work, "video", "clip.npy", extra)
    exp = _copy(_stopped(work, "video", "clip.npy", extra, 7))
    last = _resume("video", exp)
    assert getattr(last.trainers[-1], "_graph", None) is None
    assert _difference(r0, exp) is None


@pytest.mark.parametrize("src", ["one.npy", "two.npy"])
def test_image_stopped_in_the_middle_of_an_epoch(work, src):
    """--data-rep 6 and a batch of 2: three batches an epoch of one image, six of two images.  The capture's warm-up trains
    on the batch at hand, so four iterations have taken three batches: with one image the snapshot at k = 4 stands at an
    epoch's end (the resumed run must open the next epoch as the uninterrupted one does), with two in the middle of one."""
    extra = ["--hflip", "--data-rep", "6"]
    r0 = _r0(work, "image", src, extra)
    exp = _copy(_stopped(work, "image", src, extra, 7))
    snap = torch.load(os.path.join(exp, snapshot.FILE), weights_only=True)
    assert snap["loader"]["taken"] == 3 and len(torch.load(os.path.join(r0, "netG.pth"), weights_only=True)["noise_amps"]) == 3
    _resume("image", exp)
    assert _difference(r0, exp) is None


def test_baselines_with_two_critic_steps(work):
    extra = ["--Dsteps", "2"]
    r0 = _r0(work, "baselines", "clip.npy", extra)
    assert os.path.exists(os.path.join(r0, "Z_init.pth"))
    exp = _copy(_stopped(work, "baselines", "clip.npy", extra, 7))
    last = _resume("baselines", exp)
    assert last.resumed_trainer._graph is not None
    assert _difference(r0, exp) is None
    exp = _copy(_stopped(work, "baselines", "clip.npy", extra, 3))
    _resume("baselines", exp)
    assert _difference(r0, exp) is None


def test_snapshots_change_nothing(work):
    r0 = _r0(work, "video", "clip.npy", VIS)
    plain = _fresh(work, "video", "clip.npy", VIS)
    assert not os.path.exists(os.path.join(plain.exp_dir, snapshot.FILE)) and plain.loader_pos is None
    assert _difference(r0, plain.exp_dir, digests=False) is None
    with open(os.path.join(r0, "opt.json")) as f, open(os.path.join(plain.exp_dir, "opt.json")) as g:
        a, b = json.load(f), json.load(g)
    assert {k: v for k, v in a.items() if k not in ("run_dir", "experiment_dir")} == \
        {k: v for k, v in b.items() if k not in ("run_dir", "experiment_dir")}
    assert not any(k.startswith(("snapshot", "resume")) for k in a)


@pytest.mark.parametrize("kind,src,extra,skip", [
    ("video", "clip.npy", VIS, "adam"),
    ("video", "clip.npy", VIS, "rng_iter"),
    ("video", "clip.npy", VIS, "cuda_rng"),
    ("image", "two.npy", ["--hflip", "--data-rep", "6"], "loader"),
    ("video", "clip.npy", ["--no-hip-graph", "--hflip"], "random")])
def test_a_seeded_defect_ends_somewhere_else(work, kind, src, extra, skip):
    r0 = _r0(work, kind, src, extra)
    exp = _copy(_stopped(work, kind, src, extra, 7))
    last = _resume(kind, exp, skip=(skip,), verify=False)
    assert last.trainers[-1].iteration == 10
    d = _difference(r0, exp, digests=False)
    assert d is not None
    print("%s left out: first difference %s" % (skip, d))


def test_the_digest_refuses_zeroed_adam_moments(work):
    exp = _copy(_stopped(work, "video", "clip.npy", VIS, 7))
    with pytest.raises(SystemExit, match="digest"):
        _resume("video", exp, skip=("adam",), verify=True)


def test_a_flipped_byte_in_a_saved_tensor_is_refused(work):
    exp = _copy(_stopped(work, "video", "clip.npy", VIS, 7))
    path = os.path.join(exp, snapshot.FILE)
    snap = torch.load(path, weights_only=True)
    name = [k for k, v in snap["netG"].items() if v.dtype == torch.float32 and v.numel() > 8][-1]
    t = snap["netG"][name].contiguous()
    t.reshape(-1).view(torch.uint8)[5] ^= 0x10
    snap["netG"][name] = t
    torch.save(snap, path)
    with pytest.raises(SystemExit, match="digest"):
        _resume("video", exp)


def test_child_processes(work):
    env = dict(os.environ, PYTHONPATH=ROOT)
    d = work["dir"]

    def child(args):
        r = subprocess.run([sys.executable, "-m", "hp_vae_gan_amd.train_video"] + args, cwd=d, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (args, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        return r
    common = ["--video-path", "clip.npy"] + RUN + SIZES + HPVAE + SNAP
    child(common + ["--run-dir", "child_r0"])
    r = child(common + ["--run-dir", "child_r1", "--snapshot-exit-after", "7"])
    assert "Stopped after snapshot 7" in r.stdout
    exp = os.path.join(d, "child_r1", "clip", "DEBUG", "experiment_0")
    assert _header(exp) == (2, 4, False) and not os.path.exists(os.path.join(exp, "netD_2.pth"))
    child(["--resume", exp])
    assert _difference(os.path.join(d, "child_r0", "clip", "DEBUG", "experiment_0"), exp) is None
