"""The SinGAN baselines on the GPU: the box-copy kernel behind ops.ZeroPad / ops.CropBorder against torch's pad and slicing,
the baseline iteration bit for bit against its ATen pad / crop form, no ATen pad left on the path, the program's default
networks (GeneratorCSG + WDiscriminator3D) under hipGraph replay with the device loss log, and train_video_baselines /
generate end to end (each started as a fresh child process).

The end-to-end runs use the small pyramid of tests/test_programs_gpu.py (nfc 8, 40 wide, min_size 16 -> stop_scale 5) on a
synthetic 16-frame uint8 clip."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import NoiseFeed, hip_opt, load_golden  # noqa: E402
from hp_vae_gan_amd import datasets, ops, telemetry, train_video_baselines  # noqa: E402
from hp_vae_gan_amd import train as hp_train  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import _nets, networks_3d  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = ["--nfc", "8", "--min-size", "16", "--max-size", "40", "--img-size", "40"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    flat = x.view(-1)
    flat[::97] = -0.0                      # signs of zero and NaN payloads travel unchanged
    flat[5::101] = float("nan")
    return x.to(DEV)


def _pad_ref(x, p):
    return F.pad(x, (p,) * 2 * (x.dim() - 2))


def _crop_ref(y, c):
    return y[(slice(None), slice(None)) + (slice(c, -c),) * (y.dim() - 2)].contiguous()


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("p", [1, 5, 7])
@pytest.mark.parametrize("shape", [(1, 1, 3, 5, 7), (2, 3, 4, 9, 16), (1, 6, 1, 11, 13), (2, 64, 3, 10, 33), (1, 128, 2, 6, 8),
                                   (2, 3, 17, 30), (1, 128, 9, 10), (1, 1, 1, 1)])
def test_box_copy_matches_pad_and_slicing(p, shape):
    x = _rand(shape, sum(shape) * 10 + p)
    y = ops.ZeroPad.apply(x, p)                      # offset +p
    want = _pad_ref(x, p)
    assert y.shape == want.shape and torch.equal(_bits(y), _bits(want))
    back = ops.CropBorder.apply(y, p)                # offset -p (the pad's backward)
    assert torch.equal(_bits(back), _bits(x))
    big = _rand(tuple(s + 2 * p if i >= 2 else s for i, s in enumerate(shape)), p)
    crop = ops.CropBorder.apply(big, p)
    assert torch.equal(_bits(crop), _bits(_crop_ref(big, p)))
    if min(shape[2:]) > 2:                           # crop by 1 (offset -1) and its backward (offset +1)
        c1 = ops.CropBorder.apply(x, 1)
        assert torch.equal(_bits(c1), _bits(_crop_ref(x, 1)))
        assert torch.equal(_bits(ops.ZeroPad.apply(c1, 1)), _bits(_pad_ref(_crop_ref(x, 1), 1)))


def test_box_copy_rejects_empty_crops():
    with pytest.raises(RuntimeError):
        ops.CropBorder.apply(torch.zeros(1, 1, 2, 5, 5, device=DEV), 1)


def test_box_copy_stage9_volume():
    """The padded stage-9 baseline volume (B = 2, 64 channels, 13 x 144 x 256 grown by 2 * 5): both directions bit-exact; the
    rate counts the bytes read and written once."""
    x = _rand((2, 64, 13, 144, 256), 9)
    y = ops.ZeroPad.apply(x, 5)
    assert torch.equal(_bits(y), _bits(_pad_ref(x, 5)))
    assert torch.equal(_bits(ops.CropBorder.apply(y, 5)), _bits(x))
    for name, fn, nbytes in (("pad", lambda: ops.ZeroPad.apply(x, 5), 4 * (x.numel() + y.numel())),
                             ("crop", lambda: ops.CropBorder.apply(y, 5), 8 * x.numel()),
                             ("aten pad", lambda: _pad_ref(x, 5), 4 * (x.numel() + y.numel()))):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        print("%s: %.3f ms, %.2f TB/s" % (name, ms, nbytes / ms / 1e9))


@pytest.mark.parametrize("p", [1, 5])
@pytest.mark.parametrize("dims", [2, 3])
def test_pad_crop_gradients_to_second_order(p, dims):
    """First- and second-order gradients through ZeroPad and CropBorder equal those through F.pad and slicing, bit for bit."""
    shape = (2, 3, 5, 9, 12)[:2 + dims]
    big = tuple(s + 2 * p if i >= 2 else s for i, s in enumerate(shape))
    x0 = _rand(shape, 1).nan_to_num(0.0)
    a = _rand(big, 2).nan_to_num(0.0)
    v = _rand(shape, 3).nan_to_num(0.0)

    def run(pad, crop):
        x = x0.clone().requires_grad_(True)
        y = crop(pad(x, p) * a, p) * x          # x -> pad -> crop: both directions in one graph
        gx, = torch.autograd.grad(y, x, v, create_graph=True)
        gg, = torch.autograd.grad((gx * gx).sum(), x)
        return y.detach(), gx.detach(), gg

    got = run(ops.ZeroPad.apply, ops.CropBorder.apply)
    want = run(_pad_ref, _crop_ref)
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))


# ------------------------------------------------------------------------------------------------------ the whole step
def _aten_helpers(monkeypatch):
    """Put the ATen pad / crop forms of the modules back (the code before ops.ZeroPad / ops.CropBorder)."""
    def crop_border(y):
        idx = (slice(None), slice(None)) + (slice(1, -1),) * (y.dim() - 2)
        return y[idx].contiguous()

    def sg_pad(self, x):
        p = self.pad
        return F.pad(x, (p, p, p, p, p, p))

    def d_forward(self, x):
        x = F.pad(x, (self.pad,) * 6)
        return self.tail(self.body(self.head(x)))
    monkeypatch.setattr(_nets, "crop_border", crop_border)
    monkeypatch.setattr(_nets.GeneratorSG, "_zero_pad", sg_pad)
    monkeypatch.setattr(_nets.GeneratorCSG, "_zero_pad", staticmethod(lambda x, p: F.pad(x, (p,) * 6)))
    monkeypatch.setattr(_nets.WDiscriminatorBaselines, "forward", d_forward)


def _no_aten_pad(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.pad on the baselines' path")
    monkeypatch.setattr(torch.nn.functional, "pad", refuse)


def _one_step(fname, generator, critic):
    fx = load_golden(fname)
    s = fx["scale_idx"]
    opt = hip_opt(fx["opt"], 3, s, "cuda")
    ops.weights_changed()
    netG = getattr(networks_3d, generator)(opt)
    for _ in range(s):
        netG.init_next_stage()
    netG.load_state_dict(fx["G_init"])
    netG.to(DEV)
    netD = getattr(networks_3d, critic)(opt)
    netD.load_state_dict(fx["D_init"])
    netD.to(DEV)
    opt.Noise_Amps = list(fx["noise_amps_init"])
    opt.Z_init = fx["Z_init"].to(DEV)
    opt.record_grads = True
    tr = hp_train.BaselineStageTrainer(opt, netG, netD)
    rec = fx["iters"][0]
    netG.noise_source = NoiseFeed(rec["noises"], DEV)
    out = tr.step(fx["real"].to(DEV), noise_init=rec["noise_init"].to(DEV), alphas=rec["alphas"])
    torch.cuda.synchronize()
    out = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    after = {"G." + k: v.detach().clone() for k, v in netG.state_dict().items()}
    after.update({"D." + k: v.detach().clone() for k, v in netD.state_dict().items()})
    return out, after, list(opt.Noise_Amps)


@pytest.mark.parametrize("fname,generator,critic", [("baseline3d_csg_s2.pt", "GeneratorCSG", "WDiscriminator3D"),
                                                    ("baseline3d_dbl_s1.pt", "GeneratorSG", "WDiscriminatorBaselines")])
def test_baseline_step_bit_identical_to_aten_pads(fname, generator, critic, monkeypatch):
    with monkeypatch.context() as m:
        _no_aten_pad(m)
        new = _one_step(fname, generator, critic)
    with monkeypatch.context() as m:
        _aten_helpers(m)
        old = _one_step(fname, generator, critic)
    (o_new, a_new, amps_new), (o_old, a_old, amps_old) = new, old
    assert set(o_new) == set(o_old) >= {"errD_real", "errD_fake", "gradient_penalty", "errG", "rec_loss", "fake", "generated",
                                        "gradG_flat", "gradD_flat"}
    for k in o_new:
        assert torch.equal(_bits(o_new[k]), _bits(o_old[k])), k
    for k in a_new:
        assert torch.equal(a_new[k], a_old[k]), k
    assert amps_new == amps_old


@pytest.mark.parametrize("fname,generator,critic", [("baseline3d_s2.pt", "GeneratorSG", "WDiscriminator3D"),
                                                    ("baseline3d_csg_s2.pt", "GeneratorCSG", "WDiscriminatorBaselines"),
                                                    ("baseline3d_dbl_s1.pt", "GeneratorSG", "WDiscriminatorBaselines")])
def test_no_aten_pad_left(fname, generator, critic, monkeypatch):
    """GeneratorSG, GeneratorCSG (rand and rec passes) and WDiscriminatorBaselines, forward and backward, the gradient
    penalty's double backward included (fixtures' critics swapped where a state dict fits), run with F.pad refusing."""
    fx = load_golden(fname)
    s = fx["scale_idx"]
    opt = hip_opt(fx["opt"], 3, s, "cuda")
    _no_aten_pad(monkeypatch)
    netG = getattr(networks_3d, generator)(opt)
    for _ in range(s):
        netG.init_next_stage()
    netG.to(DEV)
    netD = getattr(networks_3d, critic)(opt).to(DEV)
    opt.Noise_Amps = list(fx["noise_amps_init"])
    opt.Z_init = fx["Z_init"].to(DEV)
    tr = hp_train.BaselineStageTrainer(opt, netG, netD)
    out = tr.step(fx["real"].to(DEV), alphas=fx["iters"][0]["alphas"])
    torch.cuda.synchronize()
    for k in ("errD_real", "errD_fake", "gradient_penalty", "errG", "rec_loss"):
        assert torch.isfinite(out[k]).all(), k


# ---------------------------------------------------------------------------------------------- program defaults, replay
def _clip(n=16, h=30, w=40, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def test_program_defaults_under_replay(tmp_path):
    """GeneratorCSG + WDiscriminator3D (the program's defaults) through train.train_baseline: the replayed iteration holds
    kernel nodes only, and the device loss log holds one row per iteration equal to the iteration's outputs - the eager
    ones, the capture's warm-up and every replay (the last row is the graph's own output)."""
    np.save(str(tmp_path / "clip.npy"), _clip())
    ops._rng_states.clear()
    torch.manual_seed(0)
    opt = train_video_baselines.build_baseline_parser().parse_args(["--video-path", str(tmp_path / "clip.npy")] + SMALL)
    assert (opt.generator, opt.discriminator) == ("GeneratorCSG", "WDiscriminator3D")
    opt.device, opt.dims, opt.hip_graph = DEV, 3, True
    opt.noise_amp_init, opt.scale_factor_init = opt.noise_amp, opt.scale_factor
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    opt.Noise_Amps = []
    ds = datasets.SingleVideoDataset(opt)
    netG = networks_3d.GeneratorCSG(opt).to(DEV)
    cols = hp_train.baseline_loss_log_columns(opt.alpha)
    niter = 9
    for s in range(2):
        opt.scale_idx = s
        if s > 0:
            netG.init_next_stage()
            netG.to(DEV)
        opt.fps, opt.td, opt.fps_index = hu.get_fps_td_by_index(s, opt)
        ds.generate_frames(s)
        if s == 0:
            opt.Z_init = hu.generate_noise(size=train_video_baselines.z_init_shape(opt), device=DEV)
        items = [ds[i] for i in range(opt.batch_size)]
        data = [tuple(torch.stack([it[j] for it in items]) for j in range(2))] if s > 0 else [torch.stack(items)]
        netD = networks_3d.WDiscriminator3D(opt).to(DEV)
        log = telemetry.LossLog(cols, capacity=64, device=DEV)
        rec = []

        def cb(trainer, out):
            torch.cuda.synchronize()
            rec.append([float(out[k]) for k in cols])
        tr = hp_train.train_baseline(opt, netG, data, netD=netD, niter=niter, loss_log=log, callback=cb)
        assert tr._graph is not None and tr.iteration == niter
        nodes = {k: v for k, v in tr.graph_nodes.items() if v}
        assert set(nodes) <= {"kernel", "empty", "event_record", "wait_event"}, nodes
        idx, rows, lost = log.drain()
        assert lost == 0 and idx.tolist() == list(range(niter)) and len(rec) == niter
        assert np.isfinite(rows).all()
        want = np.array(rec, dtype=np.float32)
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), (rows, want)
        last = np.array([float(tr._g_out[k]) for k in cols], dtype=np.float32)
        assert np.array_equal(rows[-1].view(np.uint32), last.view(np.uint32))
    assert len(opt.Noise_Amps) == 2


# ------------------------------------------------------------------------------------------------------------ end to end
def _child(args, cwd, timeout=420):
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print("%s: %.1f s" % (args[0], time.time() - t0))
    return r


def _scalars(exp):
    with open(os.path.join(exp, "scalars.jsonl")) as f:
        return [json.loads(ln) for ln in f]


def _check_experiment(exp, opt, scales):
    S = opt.stop_scale
    g = networks_3d.GeneratorCSG(opt)
    for _ in range(S):
        g.init_next_stage()
    keysG, keysD = set(g.state_dict()), set(networks_3d.WDiscriminator3D(opt).state_dict())
    netG = torch.load(os.path.join(exp, "netG.pth"), weights_only=True)
    assert set(netG) == {"scale", "state_dict", "optimizer", "noise_amps"} and set(netG["state_dict"]) == keysG
    amps = torch.load(os.path.join(exp, "Noise_Amps.pth"), weights_only=True)["data"]
    assert list(netG["noise_amps"]) == list(amps)
    for s in scales:
        d = torch.load(os.path.join(exp, "netD_%d.pth" % s), weights_only=True)
        assert set(d) == {"scale", "state_dict", "optimizer"} and d["scale"] == s and set(d["state_dict"]) == keysD
    z = torch.load(os.path.join(exp, "Z_init.pth"), weights_only=True)
    assert set(z) == {"data"}
    rows = _scalars(exp)
    assert all(math.isfinite(r["value"]) for r in rows)
    with open(os.path.join(exp, "logbook.txt")) as f:
        book = f.read()
    return netG, amps, z["data"], rows, book


def test_end_to_end_baselines(tmp_path):
    import types
    from PIL import Image
    t0 = time.time()
    tmp = str(tmp_path)
    np.save(os.path.join(tmp, "clip.npy"), _clip())
    niter = 5
    common = ["--video-path", os.path.join(tmp, "clip.npy"), "--niter", str(niter), "--print-interval", "2", "--manualSeed",
              "1", "--checkname", "b"] + SMALL
    _child(["hp_vae_gan_amd.train_video_baselines", "--visualize"] + common, tmp)
    exp0 = os.path.join(tmp, "run", "clip", "b", "experiment_0")
    with open(os.path.join(exp0, "opt.json")) as f:
        saved = json.load(f)
    assert saved["program"] == "train_video_baselines" and saved["generator"] == "GeneratorCSG" and saved["manualSeed"] == 1
    opt = types.SimpleNamespace(**saved)
    S = opt.stop_scale
    assert S == 5
    netG, amps, z0, rows, book = _check_experiment(exp0, opt, range(S + 1))
    assert netG["scale"] == S and len(amps) == S + 1
    assert list(z0.shape) == [2, 3] + hu.images.level_shape_3d(0, opt)
    assert book.count("hipGraph replay on") == S + 1
    for s in range(S + 1):
        tags = {"Video/Scale %d/%s" % (s, t) for t in ("errG", "errD_fake", "errD_real", "rec_loss", "noise_amp",
                                                       "gradient_penalty")}
        got = {t: sorted(r["step"] for r in rows if r["tag"] == t) for t in tags}
        assert all(v == list(range(niter)) for v in got.values()), got
        assert {r["tag"] for r in rows if r["tag"].startswith("Video/Scale %d/" % s)} == tags
        # (the run directory is relative to the working directory, as --run-dir gives it)
        assert ("warm-started from %s" % os.path.join("run", "clip", "b", "experiment_0", "netD_%d.pth" % (s - 1)) in book) \
            == (s > 0)
    prev = sorted(os.listdir(os.path.join(exp0, "previews")))
    want = ["scale%d_iter%06d_%s_%d.gif" % (s, i, n, b) for s in range(S + 1) for i in (0, 2, 4)
            for n in ("real", "generated", "fake") for b in range(2)]
    assert prev == sorted(want)
    for s in (0, S):
        td = hu.get_fps_td_by_index(s, opt)[1]
        shape = [td] + hu.images.level_shape_3d(s, opt)[1:]
        for n in ("real", "generated", "fake"):
            im = Image.open(os.path.join(exp0, "previews", "scale%d_iter000004_%s_1.gif" % (s, n)))
            assert [im.n_frames, im.size[1], im.size[0]] == shape, (n, shape)

    # resume from the last scale: scale S trained again, the critic read from experiment_0, Noise_Amps one longer
    _child(["hp_vae_gan_amd.train_video_baselines", "--netG", os.path.join(exp0, "netG.pth")] + common, tmp)
    exp1 = os.path.join(tmp, "run", "clip", "b", "experiment_1")
    netG1, amps1, z1, rows1, book1 = _check_experiment(exp1, opt, [S])
    assert netG1["scale"] == S and len(amps1) == S + 2 and amps1[:S + 1] == amps
    assert list(z1.shape) == [2, 3, hu.get_fps_td_by_index(S, opt)[1]] + hu.images.level_shape_3d(0, opt)[1:]
    assert sorted({r["tag"].split("/")[1] for r in rows1}) == ["Scale %d" % S]
    assert "Resumed scale %d" % S in book1
    assert "warm-started from %s" % os.path.join(exp0, "netD_%d.pth" % (S - 1)) in book1
    assert not os.path.exists(os.path.join(exp1, "netD_%d.pth" % (S - 1)))

    # eager only, no reconstruction term: three stages
    _child(["hp_vae_gan_amd.train_video_baselines", "--no-hip-graph", "--alpha", "0", "--video-path",
            os.path.join(tmp, "clip.npy"), "--niter", str(niter), "--print-interval", "2", "--checkname", "eager", "--nfc",
            "8", "--min-size", "32", "--max-size", "40", "--img-size", "40"], tmp)
    exp2 = os.path.join(tmp, "run", "clip", "eager", "experiment_0")
    with open(os.path.join(exp2, "opt.json")) as f:
        opt2 = types.SimpleNamespace(**json.load(f))
    _, amps2, _, rows2, book2 = _check_experiment(exp2, opt2, range(opt2.stop_scale + 1))
    assert book2.count("hipGraph replay off") == opt2.stop_scale + 1 and "hipGraph replay on" not in book2
    assert {r["tag"].split("/")[2] for r in rows2} == {"errG", "errD_fake", "errD_real", "gradient_penalty"}

    # generate on the first run: [N, T, H, W, 3] uint8 and one GIF per sample
    out = os.path.join(tmp, "gen")
    _child(["hp_vae_gan_amd.generate", "--exp-dir", exp0, "--num-samples", "3", "--seed", "4", "--out", out], tmp)
    arr = np.load(os.path.join(out, "samples.npy"))
    assert arr.dtype == np.uint8
    assert list(arr.shape) == [3, hu.get_fps_td_by_index(S, opt)[1]] + hu.images.level_shape_3d(S, opt)[1:] + [3]
    assert sorted(os.listdir(out)) == sorted(["samples.npy"] + ["sample_%04d.gif" % k for k in range(3)])
    print("baselines end to end: %.1f s" % (time.time() - t0))
