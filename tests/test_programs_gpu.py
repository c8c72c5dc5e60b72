"""The programs on the GPU: write_video's conversion kernel, the device loss log under hipGraph replay, previews that leave the
training trajectory alone, and train_video / train_image / generate end to end (each started as a fresh child process).

Small pyramid throughout: nfc 8, latent 8, 40 wide with min_size 16 and vae_levels 2 -> stop_scale 5 (stages 2-5 are GAN
stages), on a synthetic 16-frame uint8 clip (the dataset needs more than fps_lcm + 1 = 13 frames for a batch of 2)."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from hp_vae_gan_amd import datasets, ops, programs, telemetry  # noqa: E402
from hp_vae_gan_amd import train as hp_train  # noqa: E402
from hp_vae_gan_amd import utils as hu  # noqa: E402
from hp_vae_gan_amd.modules import networks_3d  # noqa: E402
from make_golden import make_opt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = ["--nfc", "8", "--latent-dim", "8", "--min-size", "16", "--max-size", "40", "--img-size", "40", "--vae-levels", "2"]


def _ref_u8(x):
    x = x.astype(np.float32)
    return np.trunc(np.clip((x + np.float32(1)) * np.float32(127.5), 0, 255)).astype(np.uint8)


def _clip(n=16, h=30, w=40, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- export
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [1, 13])
@pytest.mark.parametrize("HW", [(33, 59), (144, 256)])
def test_video_to_u8_matches_numpy(B, C, T, HW):
    H, W = HW
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + T * 10 + H)
    n = B * C * T * H * W
    x = (torch.rand(n, generator=g) * 2.4 - 1.2).numpy().astype(np.float32)
    # values within 2 ulp either side of each of the 256 level boundaries: x = k / 127.5 - 1
    lv = (np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    near = [lv]
    up, dn = lv.copy(), lv.copy()
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf))
        dn = np.nextafter(dn, np.float32(-np.inf))
        near += [up.copy(), dn.copy()]
    special = np.concatenate(near + [np.array([np.inf, -np.inf], np.float32)])
    pos = torch.randperm(n, generator=g)[:min(n, special.size)].numpy()
    x[pos] = special[:pos.size]
    xs = x.reshape(B, C, T, H, W)
    xt = torch.from_numpy(xs).to(DEV)
    got = ops.video_to_u8(xt if T > 1 else xt[:, :, 0]).cpu()
    want = torch.from_numpy(np.ascontiguousarray(_ref_u8(xs).transpose(0, 2, 3, 4, 1)))
    if T == 1:
        want = want[:, 0]
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want)


def test_video_to_u8_nan_is_zero():
    x = torch.full((1, 3, 2, 5, 7), float("nan"), device=DEV)
    x[0, 1, 1, 2, 3] = 0.5
    got = ops.video_to_u8(x).cpu()
    assert int(got[0, 1, 2, 3, 1]) == 191 and int(got.sum()) == 191


def test_video_to_u8_of_a_frames_clip():
    """A frames-kernel clip at identity size, converted back: equal to the numpy expression; levels that land one below
    their source are counted and reported (the reference's mapping has the same drop)."""
    frames = _clip(5, 33, 59, seed=3)
    store = datasets._DeviceFrames(frames, DEV)
    clip = store.clip(0, 1, 5, 33, 59, False)                      # [3][5][33][59], normalise(x / 255)
    got = ops.video_to_u8(clip[None]).cpu().numpy()[0]             # [5][33][59][3]
    want = _ref_u8(clip.cpu().numpy()).transpose(1, 2, 3, 0)
    assert np.array_equal(got, want)
    diff = got.astype(int) - frames.astype(int)
    assert diff.min() >= -1 and diff.max() <= 0
    print("levels one below the source: %d of %d" % (int((diff == -1).sum()), diff.size))


# ---------------------------------------------------------------------------------------------------- loss log and replay
def _opt(niter):
    opt = make_opt(device=DEV, dims=3, generator="GeneratorHPVAEGAN", discriminator="WDiscriminator3D", niter=niter)
    hu.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    opt.Noise_Amps = []
    opt.frames, opt.data_rep, opt.hflip, opt.max_frames, opt.start_frame = _clip(), 1, False, 16, 0
    return opt


def _run_stages(last, niter, with_log, hip_graph=True, feed_alphas=False):
    """Stages 0..last on one fixed batch; returns [(trainer, log, recorded rows)].  hip_graph False: every iteration eager.
    feed_alphas: the gradient penalty's alphas come through the trainer's alpha_source seam (helpers.AlphaFeed: the first is
    written before train(), the callback writes the next iteration's), and the callback also makes the programs' preview draw
    (Program.sample: a no_grad forward under ops.noise_stream) - the one thing between two replays that reads the packed-weight
    cache."""
    from helpers import AlphaFeed
    ops._rng_states.clear()
    torch.manual_seed(0)
    opt = _opt(niter)
    opt.hip_graph = hip_graph
    assert opt.stop_scale == 5
    ds = datasets.SingleVideoDataset(opt)
    netG = networks_3d.GeneratorHPVAEGAN(opt).to(DEV)
    res = []
    for s in range(last + 1):
        opt.scale_idx = s
        if s > 0:
            netG.init_next_stage()
            netG.to(DEV)
        opt.fps, opt.td, opt.fps_index = hu.get_fps_td_by_index(s, opt)
        ds.generate_frames(s)
        items = [ds[i] for i in range(opt.batch_size)]
        data = [tuple(torch.stack([it[j] for it in items]) for j in range(2))] if s > 0 else [torch.stack(items)]
        netD = networks_3d.WDiscriminator3D(opt).to(DEV) if opt.vae_levels < s + 1 else None
        cols = hp_train.loss_log_columns(netD is not None)
        log = telemetry.LossLog(cols, capacity=64, device=DEV) if with_log else None
        rec = []

        feed = AlphaFeed(1, niter, DEV, seed=100 + s) if feed_alphas else None
        opt.alpha_source = feed
        if feed is not None:
            feed.write(0)

        def cb(trainer, out, feed=feed, rec=rec):
            if with_log:
                torch.cuda.synchronize()
                rec.append([float(out[k]) for k in cols[:-1]] + [float(out["clip_info"][1])])
            if feed is not None:
                if trainer.iteration < niter:
                    feed.write(trainer.iteration)
                with torch.no_grad(), ops.noise_stream(DEV):
                    noise_init = hu.generate_noise(size=opt.Z_init_size, device=DEV)
                    trainer.netG(noise_init, opt.Noise_Amps, noise_init=noise_init, mode="rand")
        tr = hp_train.train(opt, netG, data, netD=netD, loss_log=log, callback=cb if with_log or feed_alphas else None)
        if feed is not None and netD is not None:
            # train() handed opt.alpha_source on: asked once per iteration that passed through python (replays do not)
            assert feed.calls == (4 if hip_graph else niter), feed.calls
        res.append((tr, log, rec))
    torch.cuda.synchronize()
    return res


def _state(tr):
    sd = {"G." + k: v.detach().cpu().clone() for k, v in tr.netG.state_dict().items()}
    if tr.netD is not None:
        sd.update({"D." + k: v.detach().cpu().clone() for k, v in tr.netD.state_dict().items()})
    return sd


def _opt_state(tr):
    out = [tr.optimizerG.state_dict()]
    if tr.netD is not None:
        out.append(tr.optimizerD.state_dict())
    return out


def _equal_nested(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_nested(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal_nested(x, y) for x, y in zip(a, b))
    return a == b


def test_loss_log_under_replay_and_changes_nothing():
    t0 = time.time()
    on = _run_stages(2, 12, True)
    off = _run_stages(2, 12, False)
    for s in (0, 2):           # a VAE stage and a GAN stage
        tr, log, rec = on[s]
        assert tr._graph is not None and tr.iteration == 12
        nodes = {k: v for k, v in tr.graph_nodes.items() if v}
        assert set(nodes) <= {"kernel", "empty", "event_record", "wait_event"}, nodes
        off_nodes = off[s][0].graph_nodes
        assert tr.graph_nodes["kernel"] == off_nodes["kernel"] + 1                    # the one append node
        assert {k: v for k, v in tr.graph_nodes.items() if k != "kernel"} == \
            {k: v for k, v in off_nodes.items() if k != "kernel"}
        idx, rows, lost = log.drain()
        assert lost == 0 and idx.tolist() == list(range(12)) and len(rec) == 12
        want = np.array(rec, dtype=np.float32)
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), (rows, want)
    for s in range(3):
        assert _equal_nested(_state(on[s][0]), _state(off[s][0])), s
        assert _equal_nested(_opt_state(on[s][0]), _opt_state(off[s][0])), s
    print("wall %.1f s" % (time.time() - t0))


def test_train_loop_with_replay_equals_eager_loop_bit_for_bit():
    """train() itself, stages 0..2 (two VAE stages and a GAN stage), opt.hip_graph True against False: the switch to replays
    after two eager iterations, the warm-up's callback, the re-capture of every stage on pinned workspaces, and each stage
    starting from the weights a graph-trained stage left.  Exact: network state, optimizer state, the callback's scalars and
    the drained loss-log rows (tests/test_graph_replay_exact.py has the per-iteration comparison of a single stage)."""
    from helpers import first_difference
    t0 = time.time()
    on = _run_stages(2, 8, True, hip_graph=True, feed_alphas=True)
    off = _run_stages(2, 8, True, hip_graph=False, feed_alphas=True)
    for s in range(3):
        (tr_on, log_on, rec_on), (tr_off, log_off, rec_off) = on[s], off[s]
        assert tr_on._graph is not None and getattr(tr_off, "_graph", None) is None and tr_on.iteration == tr_off.iteration == 8
        assert tr_on.optimizerG.steps() == tr_off.optimizerG.steps() == 8
        idx_on, rows_on, lost_on = log_on.drain()
        idx_off, rows_off, lost_off = log_off.drain()
        assert lost_on == lost_off == 0 and idx_on.tolist() == idx_off.tolist() == list(range(8))
        for i in range(8):
            assert np.array_equal(rows_on[i].view(np.uint32), rows_off[i].view(np.uint32)), \
                "stage %d: loss-log row %d (0-based) differs: replay %s, eager %s" % (s, i, rows_on[i], rows_off[i])
        assert len(rec_on) == len(rec_off) == 8
        assert np.array_equal(np.array(rec_on, np.float32).view(np.uint32), np.array(rec_off, np.float32).view(np.uint32)), s
        d = first_difference(_state(tr_on), _state(tr_off), "stage %d state" % s)
        assert d is None, d
        assert _equal_nested(_state(tr_on), _state(tr_off)), s
        d = first_difference(_opt_state(tr_on), _opt_state(tr_off), "stage %d optimizers" % s)
        assert d is None, d
        assert _equal_nested(_opt_state(tr_on), _opt_state(tr_off)), s
    print("wall %.1f s" % (time.time() - t0))


# ------------------------------------------------------------------------------------------------------------- previews
def _program_run(tmp, extra):
    ops._rng_states.clear()
    np.save(os.path.join(tmp, "clip.npy"), _clip())
    argv = ["--video-path", os.path.join(tmp, "clip.npy"), "--run-dir", os.path.join(tmp, "run"), "--niter", "5",
            "--manualSeed", "3", "--stop-scale-time", "-1"] + SMALL + extra
    prog = programs.Program("video", argv)
    return prog.run()


def _scalars(exp):
    with open(os.path.join(exp, "scalars.jsonl")) as f:
        return [json.loads(ln) for ln in f]


def test_previews_change_nothing(tmp_path):
    t0 = time.time()
    a = _program_run(str(tmp_path), ["--visualize", "--print-interval", "2"])
    b = _program_run(str(tmp_path), ["--print-interval", "2"])
    assert os.listdir(os.path.join(a.exp_dir, "previews")) and not os.path.exists(os.path.join(b.exp_dir, "previews"))
    ta, tb = a.trainers[-1], b.trainers[-1]
    sa, sb = _state(ta), _state(tb)
    bn = [k for k in sa if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert _equal_nested({k: v for k, v in sa.items() if k not in bn}, {k: v for k, v in sb.items() if k not in bn})
    assert _equal_nested(_opt_state(ta), _opt_state(tb))
    assert _scalars(a.exp_dir) == _scalars(b.exp_dir)
    assert any(not torch.equal(sa[k], sb[k]) for k in bn if k.startswith("G.") and k.endswith("running_mean"))
    # preview keys never meet training keys: at the same device iteration, a draw under noise_stream differs element-wise
    # from the draws of call indices 0..63.  Two independent fp32 normals coincide now and then (the Box-Muller outputs are
    # quantised), so a few equal elements in 16384 are chance; a shared key would make all of them equal, as the repeated
    # noise_stream draw shows.
    st = ops._rng(DEV)
    saved = st.call
    with ops.noise_stream(DEV):
        x = ops.normal_(torch.empty(1 << 14, device=DEV))
    assert st.call == saved
    with ops.noise_stream(DEV):
        assert torch.equal(ops.normal_(torch.empty(1 << 14, device=DEV)), x)
    for c in range(64):
        st.call = c
        y = ops.normal_(torch.empty(1 << 14, device=DEV))
        assert int((x == y).sum()) <= 2, c
    st.call = saved
    print("wall %.1f s" % (time.time() - t0))


# ------------------------------------------------------------------------------------------------------------ end to end
def _child(args, cwd, timeout=420):
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print("%s: %.1f s" % (args[0], time.time() - t0))
    return r


def _check_experiment(exp, ref_netG, ref_netD, gan_stages, niter):
    netG = torch.load(os.path.join(exp, "netG.pth"), weights_only=True)
    assert set(netG) == {"scale", "state_dict", "optimizer", "noise_amps"}
    assert set(netG["state_dict"]) == ref_netG
    amps = torch.load(os.path.join(exp, "Noise_Amps.pth"), weights_only=True)["data"]
    for s in gan_stages:
        d = torch.load(os.path.join(exp, "netD_%d.pth" % s), weights_only=True)
        assert set(d) == {"scale", "state_dict", "optimizer"} and d["scale"] == s and set(d["state_dict"]) == ref_netD
    rows = _scalars(exp)
    assert all(math.isfinite(r["value"]) for r in rows)
    return netG, amps, rows


def _ref_keys(opt, nets):
    g = nets.GeneratorHPVAEGAN(opt)
    for _ in range(opt.stop_scale):
        g.init_next_stage()
    return set(g.state_dict()), set(getattr(nets, opt.discriminator)(opt).state_dict())


def _tags(s, gan):
    own = ["noise_amp", "gradient_penalty", "total_loss", "grad_norm"] if gan else ["noise_amp", "total_loss", "grad_norm"]
    ref = ["rec loss", "errG", "errD_fake", "errD_real"] if gan else ["KLD", "Rec VAE"]
    return {"Video/Scale %d/%s" % (s, t) for t in own + ref}


def _end_to_end(tmp, kind, src):
    from hp_vae_gan_amd.modules import networks_2d
    t0 = time.time()
    flag = "--video-path" if kind == "video" else "--image-path"
    common = [flag, src, "--niter", "6", "--print-interval", "3", "--manualSeed", "1", "--checkname", "t"] + SMALL
    _child(["hp_vae_gan_amd.train_" + kind, "--visualize"] + common, tmp)
    clip = programs.clip_name(src)
    exp0 = os.path.join(tmp, "run", clip, "t", "experiment_0")
    with open(os.path.join(exp0, "opt.json")) as f:
        saved = json.load(f)
    import types
    opt = types.SimpleNamespace(**saved)
    nets = networks_3d if kind == "video" else networks_2d
    S = opt.stop_scale
    assert S == 5 and saved["manualSeed"] == 1
    keysG, keysD = _ref_keys(opt, nets)
    gan = list(range(opt.vae_levels, S + 1))
    netG, amps, rows = _check_experiment(exp0, keysG, keysD, gan, 6)
    assert netG["scale"] == S and len(amps) == S + 1
    for s in range(S + 1):
        tags = _tags(s, s in gan)
        got = {t: sorted(r["step"] for r in rows if r["tag"] == t) for t in tags}
        assert all(v == list(range(6)) for v in got.values()), got
        assert not {r["tag"] for r in rows if r["tag"].startswith("Video/Scale %d/" % s)} - tags
    prev = os.listdir(os.path.join(exp0, "previews"))
    from PIL import Image
    for s in range(S + 1):
        if kind == "video":
            td = hu.get_fps_td_by_index(s, opt)[1]
            shape = [td] + hu.images.level_shape_3d(s, opt)[1:]
        else:
            shape = [1] + hu.images.level_shape_2d(s, opt)
        names = [n for n in prev if n.startswith("scale%d_iter000000_fake_var_" % s)]
        assert len(names) == 3 * 2, names
        for n in names + ["scale%d_iter000003_real_0%s" % (s, ".gif" if kind == "video" else ".png")]:
            im = Image.open(os.path.join(exp0, "previews", n))
            assert [getattr(im, "n_frames", 1), im.size[1], im.size[0]] == shape, (n, shape)
    # resume from the last scale: critic warm-started from experiment_0/netD_{S-1}.pth, scale S trained again
    _child(["hp_vae_gan_amd.train_" + kind, "--netG", os.path.join(exp0, "netG.pth")] + common, tmp)
    exp1 = os.path.join(tmp, "run", clip, "t", "experiment_1")
    netG1, amps1, rows1 = _check_experiment(exp1, keysG, keysD, [S], 6)
    assert netG1["scale"] == S and len(amps1) == S + 2 and amps1[:S + 1] == amps
    assert sorted({r["tag"].split("/")[1] for r in rows1}) == ["Scale %d" % S]
    with open(os.path.join(exp1, "logbook.txt")) as f:
        assert "Resumed scale %d" % S in f.read()
    # generate: shape, determinism per seed
    outs = []
    for i, seed in enumerate((7, 7, 8)):
        out = os.path.join(tmp, "gen%d" % i)
        _child(["hp_vae_gan_amd.generate", "--exp-dir", exp0, "--num-samples", "5", "--seed", str(seed), "--out", out], tmp)
        outs.append(np.load(os.path.join(out, "samples.npy")))
        ext = ".gif" if kind == "video" else ".png"
        assert sorted(os.listdir(out)) == sorted(["samples.npy"] + ["sample_%04d%s" % (k, ext) for k in range(5)])
    if kind == "video":
        want = [5, hu.get_fps_td_by_index(S, opt)[1]] + hu.images.level_shape_3d(S, opt)[1:] + [3]
    else:
        want = [5] + hu.images.level_shape_2d(S, opt) + [3]
    assert outs[0].dtype == np.uint8 and list(outs[0].shape) == want
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    assert torch.load(os.path.join(exp0, "netG.pth"), weights_only=True)["scale"] == S
    print("%s end to end: %.1f s" % (kind, time.time() - t0))


def test_end_to_end_video(tmp_path):
    np.save(str(tmp_path / "clip.npy"), _clip())
    _end_to_end(str(tmp_path), "video", str(tmp_path / "clip.npy"))


def test_end_to_end_image(tmp_path):
    from PIL import Image
    Image.fromarray(_clip(1)[0]).save(str(tmp_path / "balloon.png"))
    _end_to_end(str(tmp_path), "image", str(tmp_path / "balloon.png"))
