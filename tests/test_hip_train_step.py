"""GPU parity of the whole train iteration (hp_vae_gan_amd.train.StageTrainer.step) against the golden stage fixtures
recorded from the reference modules (tests/golden/make_golden.py): losses, every gradient, clip norm, post-Adam
parameters, BN running stats, SN u/v and the calibrated noise amplitude."""
import pytest
import torch

from helpers import RTOL, assert_close, bn_bias_atol, flat_to_named, load_golden, run_hip_stage  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fname", ["step3d_vae_s0.pt", "step3d_vae_s1.pt", "step3d_gan_s3.pt", "step2d_gan_s2.pt", "step2d_vae_s1.pt",
                                   "step3d_gan_s3_td2.pt", "step3d_gan_s2_all.pt", "step3d_gan_s7.pt"])
def test_train_step_matches_reference(fname):
    """Tolerances are measured, not guessed: each quantity gets max(1e-3 relative (north_star), 2 x the spread the reference
    itself shows for it between its oneDNN, native-ATen, input-perturbed (2^-20) and gradient-noise evaluations;
    fx["spread"]).  Optimizer steps are judged by their UPDATE: frozen parameters must be bit-identical to the initial state,
    trained ones must make the reference's Adam step (learning rate of their group, bounded by lr) except on the sign-flip
    fraction; everything after a step is computed from the reference's post-step state (helpers.run_hip_stage, sync)."""
    from helpers import _bn_fed_bias, compare_step, compare_update
    from hp_vae_gan_amd import train as hp_train
    fx = load_golden(fname)
    prevG = {k: v.clone() for k, v in fx["G_init"].items()}
    prevD = {k: v.clone() for k, v in fx["D_init"].items()} if fx["D_init"] is not None else None
    for it, (rec, out, netG, netD, trainer) in enumerate(run_hip_stage(fx)):
        spread = fx["spread"][it] if "spread" in fx else None
        what = "%s[%d]" % (fname, it)
        assert trainer.opt.Noise_Amps == pytest.approx(rec["noise_amps"], rel=1e-4)
        got = dict(out)
        got["total_norm"] = out["clip_info"][1]
        got["gradsG"] = flat_to_named(out["gradG_flat"], trainer.arenaG, netG)
        if "gradsD" in rec:
            got["gradsD"] = flat_to_named(out["gradD_flat"], trainer.arenaD, netD)
        compare_step(what, rec, spread, got)
        # ---- post-step state, by update
        lr_by_id = {}
        for params, lr in hp_train.generator_param_groups(trainer.opt, netG):
            for p in params:
                lr_by_id[id(p)] = lr
        sdG = netG.state_dict()
        gnames = dict(netG.named_parameters())
        for k, v in rec["G_after"].items():
            if k in gnames:
                sf = 0.0
                if spread is not None:
                    lr_k = lr_by_id.get(id(gnames[k]))
                    # the reference's own sign-flip fraction is not recorded per tensor for these fixtures; its spread on the
                    # tensor (max |difference| between evaluations) tells whether ANY element flipped
                    sf = 0.05 if (lr_k and spread["G_after"].get(k, 0.0) > lr_k / 10) else 0.0
                compare_update(what + ".G." + k, prevG[k], v, sdG[k], lr_by_id.get(id(gnames[k])), sf,
                               _bn_fed_bias(k, set(gnames)), first_step=(it == 0))
            elif k.endswith("num_batches_tracked"):
                assert int(sdG[k]) == int(v), what + "." + k
            else:
                assert_close(sdG[k].float(), v.float(), RTOL, what + ".G_after." + k, atol=max(1e-6, 2 * (spread or {}).get("G_after", {}).get(k, 0.0)))
        prevG = {k: v.clone() for k, v in rec["G_after"].items()}
        if rec["D_after"] is not None:
            sdD = out["D_hip_after"]          # the critic as OUR optimizer step left it (before the reference's state replaced it)
            dnames = dict(netD.named_parameters())
            for k, v in rec["D_after"].items():
                if k in dnames:
                    sf = 0.05 if (spread is not None and spread["D_after"].get(k, 0.0) > fx["opt"]["lr_d"] / 10) else 0.0
                    compare_update(what + ".D." + k, prevD[k], v, sdD[k], fx["opt"]["lr_d"], sf, False, first_step=(it == 0))
                else:
                    # buffers (spectral-norm u / v): as they stand at the END of the iteration, like the recorded ones
                    assert_close(netD.state_dict()[k].float(), v.float(), RTOL, what + ".D_after." + k, atol=max(1e-6, 2 * (spread or {}).get("D_after", {}).get(k, 0.0)))
            prevD = {k: v.clone() for k, v in rec["D_after"].items()}


def test_sampling_path_matches_reference():
    """Generation path (forward with noise_init / sample_init, networks_3d.py:367-387) as the trainers' previews run it
    (no_grad, train-mode BatchNorm): outputs and the moved running statistics against the reference fixture."""
    from helpers import NoiseFeed, hip_opt
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden("sample3d_s3.pt")
    dev = "cuda"
    opt = hip_opt(fx["opt"], fx["dims"], fx["scale_idx"], dev)
    netG = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(fx["scale_idx"]):
        netG.init_next_stage()
    netG.load_state_dict(fx["G_init"])
    netG.to(dev)
    for call in fx["calls"]:
        netG.noise_source = NoiseFeed(call["noises"], dev)
        si = None if call["sample_start"] is None else (call["sample_start"], call["sample_tensor"].to(dev))
        with torch.no_grad():
            x, vae_out = netG(call["noise_init"].to(dev), fx["noise_amps"], noise_init=call["noise_init"].to(dev), sample_init=si,
                              mode="rand")
        assert_close(x, call["x"], RTOL, "sample.x")
        assert_close(vae_out, call["vae_out"], RTOL, "sample.vae_out")
        sd = netG.state_dict()
        for k, v in call["G_after"].items():
            assert_close(sd[k].float(), v.float(), RTOL, "sample.G_after." + k, atol=1e-6)
    with pytest.raises(AssertionError):
        netG(None, fx["noise_amps"], noise_init=fx["calls"][0]["noise_init"].to(dev), sample_init=(3, fx["calls"][1]["sample_tensor"].to(dev)))


def test_smoke_entry():
    from smoke_step import run_smoke
    run_smoke()


@pytest.mark.parametrize("fname,generator,critic", [("baseline3d_s2.pt", "GeneratorSG", "WDiscriminator3D"),
                                                    ("baseline3d_csg_s2.pt", "GeneratorCSG", "WDiscriminator3D"),
                                                    ("baseline3d_dbl_s1.pt", "GeneratorSG", "WDiscriminatorBaselines"),
                                                    ("baseline3d_sg_s7.pt", "GeneratorSG", "WDiscriminator3D")])
def test_baseline_singan_step_matches_reference(fname, generator, critic):
    """BASELINE config 5 (GeneratorSG) and the baselines script's default GeneratorCSG: BaselineStageTrainer (HIP)
    against the reference-generated fixtures."""
    from helpers import NoiseFeed, hip_opt
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden(fname)
    s = fx["scale_idx"]
    dev = "cuda"
    opt = hip_opt(fx["opt"], 3, s, dev)
    netG = getattr(networks_3d, generator)(opt)
    for _ in range(s):
        netG.init_next_stage()
    assert list(netG.state_dict().keys()) == list(fx["G_init"].keys())
    netG.load_state_dict(fx["G_init"])
    netG.to(dev)
    netD = getattr(networks_3d, critic)(opt)
    assert list(netD.state_dict().keys()) == list(fx["D_init"].keys())
    netD.load_state_dict(fx["D_init"])
    netD.to(dev)
    opt.Noise_Amps = list(fx["noise_amps_init"])
    opt.Z_init = fx["Z_init"].to(dev)
    opt.record_grads = True
    tr = hp_train.BaselineStageTrainer(opt, netG, netD)
    rec = fx["iters"][0]
    netG.noise_source = NoiseFeed(rec["noises"], dev)
    # each critic update is judged on its own and then replaced by the reference's (helpers.run_hip_stage explains why)
    hip_d_steps = []

    def hook(t, j):
        hip_d_steps.append({k: v.detach().clone() for k, v in t.netD.state_dict().items()})
        t.netD.load_state_dict(rec["D_steps"][j])
    tr.after_d_step = hook
    out = tr.step(fx["real"].to(dev), noise_init=rec["noise_init"].to(dev), alphas=rec["alphas"])
    assert opt.Noise_Amps == pytest.approx(rec["noise_amps"], rel=1e-4)
    from helpers import _bn_fed_bias, compare_step, compare_update
    spread = fx["spread"][0]
    got = dict(out)
    got["gradsG"] = flat_to_named(out["gradG_flat"], tr.arenaG, netG)
    got["gradsD"] = flat_to_named(out["gradD_flat"], tr.arenaD, netD)
    compare_step(fname, rec, spread, got)
    # post-step state by UPDATE (frozen stages bit-identical; trained blocks / head / tail at their group's learning rate)
    gnames = dict(netG.named_parameters())
    lr_of = {}
    for n, p in gnames.items():
        o, _ = tr.arenaG.range[id(p)]
        hit = [g["lr"] for g in tr.optimizerG.groups if g["lo"] <= o < g["hi"]]
        lr_of[n] = hit[0] if hit else None
    sdG, sdD = netG.state_dict(), netD.state_dict()
    for k, v in rec["G_after"].items():
        if k in gnames:
            sf = 0.05 if (lr_of[k] and spread["G_after"].get(k, 0.0) > lr_of[k] / 10) else 0.0
            compare_update("baseline.G." + k, fx["G_init"][k], v, sdG[k], lr_of[k], sf, _bn_fed_bias(k, set(gnames)),
                           first_step=(opt.Gsteps == 1))
        elif k.endswith("num_batches_tracked"):
            assert int(sdG[k]) == int(v), k
        else:
            assert_close(sdG[k].float(), v.float(), RTOL, "baseline.G_after." + k, atol=max(1e-6, 2 * spread["G_after"].get(k, 0.0)))
    dnames = dict(netD.named_parameters())
    assert len(hip_d_steps) == opt.Dsteps == len(rec["D_steps"])
    for j in range(opt.Dsteps):
        before = fx["D_init"] if j == 0 else rec["D_steps"][j - 1]
        for k, v in rec["D_steps"][j].items():
            mine = hip_d_steps[j][k]
            if k in dnames:
                sf = 0.05 if spread["D_after"].get(k, 0.0) > opt.lr_d / 10 else 0.0
                compare_update("baseline.D[%d].%s" % (j, k), before[k], v, mine, opt.lr_d, sf, _bn_fed_bias(k, set(dnames)), first_step=(j == 0))
            elif k.endswith("num_batches_tracked"):
                assert int(mine) == int(v), k
            else:
                assert_close(mine.float(), v.float(), RTOL, "baseline.D[%d].%s" % (j, k), atol=max(1e-6, 2 * spread["D_after"].get(k, 0.0)))


@pytest.mark.parametrize("fname", ["step3d_gan_s3.pt", "step3d_vae_s1.pt"])
def test_graph_replay_equals_eager(fname):
    """hipGraph capture of the iteration (StageTrainer.enable_graph): replays must produce what eager steps produce, bit for
    bit.  Noise is pinned by a cycling noise_source and a fixed noise_init, so that both runs see identical draws whatever the
    library's stream does; the gradient penalty's alphas reach both runs through alpha_source (helpers.AlphaFeed).  The same
    `real` every iteration.  (tests/test_graph_replay_exact.py: the library's own noise, changing inputs, every output.)"""
    from helpers import AlphaFeed, first_difference, hip_opt
    from hp_vae_gan_amd import ops as hp_ops
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden(fname)
    dev = "cuda"
    s = fx["scale_idx"]
    rec = fx["iters"][0]

    def build():
        hp_ops._rng_states.clear()           # both runs start the library's noise stream at iteration 0 (calibration pass draws)
        opt = hip_opt(fx["opt"], 3, s, dev)
        netG = networks_3d.GeneratorHPVAEGAN(opt)
        for _ in range(s):
            netG.init_next_stage()
        netG.load_state_dict(fx["G_init"])
        netG.to(dev)
        netD = None
        if fx["D_init"] is not None:
            netD = networks_3d.WDiscriminator3D(opt)
            netD.load_state_dict(fx["D_init"])
            netD.to(dev)
        opt.Noise_Amps = list(fx["noise_amps_init"])
        opt.alpha_source = AlphaFeed(1, 8, dev)
        tr = hp_train.StageTrainer(opt, netG, netD)
        noises = {tuple(t.shape): t.to(dev) for t in rec["noises"]}
        netG.noise_source = lambda ref: noises[tuple(ref.shape)]     # the same draw for a given shape, every time
        return tr, netG, netD

    real, rz = fx["real"].to(dev), fx["real_zero"].to(dev)
    ni = rec["noise_init"].to(dev)
    import hp_vae_gan_amd.utils as hu
    orig = hu.generate_noise
    hu.images.generate_noise  # noqa: B018
    try:
        # pin noise_init for both runs (generate_noise(size=...) is called inside step)
        import hp_vae_gan_amd.train as T
        T.utils.generate_noise = lambda ref=None, size=None, type='normal', emb_size=None, device=None: ni if size is not None else orig(ref=ref)
        a_tr, a_G, a_D = build()
        torch.manual_seed(7)
        for it in range(8):
            a_tr.alpha_source.write(it)
            a_tr.step(real, rz)
        b_tr, b_G, b_D = build()
        torch.manual_seed(7)
        b_tr.alpha_source.write(0)
        b_tr.step(real, rz)
        b_tr.alpha_source.write(1)
        b_tr.enable_graph(real, rz)          # runs one warm-up iteration (eager, side stream) + capture (no execution)
        # the graph bakes in the scratch buffer's address: a later, larger request must not free that buffer
        baked = hp_ops.workspace(1, real.device)
        grown = hp_ops.workspace(baked.numel() + (1 << 20), real.device)
        assert grown is not baked and any(b is baked for b in hp_ops._ws_pinned)
        for it in range(2, 8):
            b_tr.alpha_source.write(it)
            out = b_tr.step(real, rz)        # replays
            # a device synchronise between replays: this is what exposed hipMemsetAsync nodes being mis-ordered inside a
            # captured graph (upsample backward scattered into a buffer zeroed too late; back-to-back replays hid it)
            torch.cuda.synchronize()
            assert torch.isfinite(out["clip_info"]).all() and float(out["clip_info"][1]) < 1e4, out["clip_info"]
    finally:
        T.utils.generate_noise = orig
    # a: 8 eager iterations; b: 1 eager + 1 warm-up + 6 replays = 8 iterations on the same draws, the same alphas, kernels
    # without float atomics: the same bits
    assert b_tr.iteration == a_tr.iteration == 8
    for net_a, net_b, tag in ((a_G, b_G, "G"), (a_D, b_D, "D")):
        if net_a is None:
            continue
        sd_a, sd_b = net_a.state_dict(), net_b.state_dict()
        for k, vb in sd_b.items():
            assert torch.isfinite(vb.float()).all(), k
            assert torch.equal(vb, sd_a[k]), first_difference(sd_a[k].cpu(), vb.cpu(), "graph.%s.%s (eager vs replay)" % (tag, k))
        assert list(sd_a) == list(sd_b)


@pytest.mark.parametrize("fname,critic", [("baseline3d_s2.pt", "WDiscriminator3D"), ("baseline3d_dbl_s1.pt", "WDiscriminatorBaselines")])
def test_baseline_graph_replay_tracks_eager(fname, critic):
    """hipGraph capture of the baselines' iteration (BaselineStageTrainer.enable_graph; Dsteps = 2 in baseline3d_s2, the
    BatchNorm critic and its double backward in baseline3d_dbl_s1): the captured graph holds kernel nodes only (enable_graph
    refuses anything else), replays stay finite with a device synchronise in between, and after 8 iterations both networks -
    parameters, BatchNorm statistics and counters, spectral-norm u / v - hold the bits of an eager run fed the same noise
    (a cycling noise_source) and the same alphas (alpha_source)."""
    from helpers import AlphaFeed, first_difference, hip_opt
    from hp_vae_gan_amd import ops as hp_ops
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden(fname)
    dev = "cuda"
    s = fx["scale_idx"]
    rec = fx["iters"][0]

    def build():
        # noise_init is the one draw this test leaves to the library's stream (generate_noise(ref=opt.Z_init)): both runs
        # start that stream at iteration 0, or the second would continue where the first stopped
        hp_ops._rng_states.clear()
        opt = hip_opt(fx["opt"], 3, s, dev)
        netG = networks_3d.GeneratorSG(opt)
        for _ in range(s):
            netG.init_next_stage()
        netG.load_state_dict(fx["G_init"])
        netG.to(dev)
        netD = getattr(networks_3d, critic)(opt)
        netD.load_state_dict(fx["D_init"])
        netD.to(dev)
        opt.Noise_Amps = list(fx["noise_amps_init"])
        opt.Z_init = fx["Z_init"].to(dev)
        opt.alpha_source = AlphaFeed(opt.Dsteps, 8, dev)
        tr = hp_train.BaselineStageTrainer(opt, netG, netD)
        noises = {tuple(t.shape): t.to(dev) for t in rec["noises"]}
        netG.noise_source = lambda ref: noises[tuple(ref.shape)]     # the same draw for a given shape, every time
        return tr, netG, netD

    real = fx["real"].to(dev)
    a_tr, a_G, a_D = build()
    torch.manual_seed(7)
    for it in range(8):
        a_tr.alpha_source.write(it)
        a_tr.step(real)
    b_tr, b_G, b_D = build()
    torch.manual_seed(7)
    b_tr.alpha_source.write(0)
    b_tr.step(real)
    b_tr.alpha_source.write(1)
    b_tr.enable_graph(real)              # one warm-up iteration (eager, side stream) + capture
    assert b_tr.graph_nodes.get("kernel", 0) > 50 and not b_tr.graph_nodes.get("memset", 0) and not b_tr.graph_nodes.get("memcpy", 0)
    for it in range(2, 8):
        b_tr.alpha_source.write(it)
        out = b_tr.step(real)            # replays
        torch.cuda.synchronize()
        for k in ("errD_real", "errD_fake", "gradient_penalty", "errG", "rec_loss"):
            assert torch.isfinite(out[k]).all(), k
    assert b_tr.iteration == a_tr.iteration == 8
    for net_a, net_b, tag in ((a_G, b_G, "G"), (a_D, b_D, "D")):
        sd_a, sd_b = net_a.state_dict(), net_b.state_dict()
        assert list(sd_a) == list(sd_b)
        for k, vb in sd_b.items():
            assert torch.isfinite(vb.float()).all(), k
            assert torch.equal(vb, sd_a[k]), first_difference(sd_a[k].cpu(), vb.cpu(), "baseline.graph.%s.%s (eager vs replay)" % (tag, k))


@pytest.mark.parametrize("fname,iters", [("step3d_gan_s3.pt", 6), ("step3d_vae_s1.pt", 6)])
def test_several_iterations_track_the_oracle(fname, iters):
    """Longer horizon than the reference fixtures hold: N consecutive iterations of the same stage (optimizer moments and
    step counts, BatchNorm running statistics, spectral-norm u/v and the calibrated amplitude all carried over) on the HIP
    path and on the oracle, fed with the same fresh noise.  Adam's sign-flip chaos lets parameters
    drift apart by O(lr) per step, so the losses are compared with a tolerance that grows with the iteration."""
    from helpers import NoiseFeed, oracle_state, opt_from
    from oracle import hpvg_oracle as O
    fx = load_golden(fname)
    rec0 = fx["iters"][0]
    gan = fx["D_init"] is not None
    g = torch.Generator().manual_seed(4242)
    draws = []          # per iteration: (noise_init, [noises...], alpha)
    for it in range(iters):
        shapes = [t.shape for t in (rec0["noises"] if it == 0 else rec0["noises"][1:])]   # [1:]: no calibration pass
        draws.append((torch.randn(rec0["noise_init"].shape, generator=g), [torch.randn(s, generator=g) for s in shapes],
                      torch.rand(1, 1, generator=g) if gan else None))
    # oracle
    opt = opt_from(fx["opt"])
    O.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    PG = oracle_state(fx["G_init"])
    PD = oracle_state(fx["D_init"]) if gan else None
    amps = list(fx["noise_amps_init"])
    adam_g, adam_d, want = {}, {}, []
    for it, (z, noises, alpha) in enumerate(draws):
        feed = iter(noises)
        if it == 0:
            O.noise_amp_for_stage(PG, opt, fx["dims"], fx["scale_idx"], fx["real"], fx["real_zero"], amps, feed)
        want.append(O.train_step(PG, PD, opt, fx["dims"], fx["scale_idx"], fx["real"], fx["real_zero"], z, feed,
                                 alpha.reshape(()) if gan else None, amps, adam_g, adam_d))
    # HIP: run_hip_stage drives fx["iters"]; give it our draws
    fx2 = dict(fx)
    fx2["iters"] = [dict(noise_init=z, noises=noises, alpha=alpha) for z, noises, alpha in draws]
    keys = ("errD_real", "errD_fake", "gradient_penalty", "rec_loss", "errG") if gan else ("rec_vae_loss", "kl_loss", "total_loss")
    for it, (rec, out, netG, netD, trainer) in enumerate(run_hip_stage(fx2)):
        tol = 2e-3 * (1 + 2 * it)
        for k in keys:
            assert_close(out[k], want[it][k], tol, "%s[%d].%s" % (fname, it, k), atol=1e-5)
    sd = netG.state_dict()
    lr = fx["opt"]["lr_g"] * iters
    worst = max(float((sd[k].float().cpu() - v.detach().float()).abs().max()) for k, v in PG.items() if O.is_param(k))
    assert worst <= 3 * lr, "post-training G parameters drifted by %.3e (> 3 lr*N = %.3e)" % (worst, 3 * lr)
    assert trainer.opt.Noise_Amps == pytest.approx(amps, rel=1e-4)


def test_train_loop_captures_the_iteration_after_two_eager_steps():
    """train.train(): the reference-shaped stage loop (train_video.py:98-109 data cycling, :111-202 step) - two eager
    iterations, then hipGraph replays fed from the data iterator through the static input buffers; opt.hip_graph=False
    keeps it eager.  Both runs stay finite and keep training (the reconstruction loss of the fixed clip goes down)."""
    from helpers import hip_opt
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden("step3d_gan_s3.pt")
    dev = "cuda"
    s = fx["scale_idx"]
    real, rz = fx["real"].to(dev), fx["real_zero"].to(dev)
    data = [(real, rz), (real.flip(-1).contiguous(), rz.flip(-1).contiguous())]   # a 2-item "loader", cycled
    for use_graph in (True, False):
        opt = hip_opt(fx["opt"], 3, s, dev)
        opt.hip_graph = use_graph
        opt.niter = 12
        netG = networks_3d.GeneratorHPVAEGAN(opt)
        for _ in range(s):
            netG.init_next_stage()
        netG.load_state_dict(fx["G_init"])
        netG.to(dev)
        netD = networks_3d.WDiscriminator3D(opt)
        netD.load_state_dict(fx["D_init"])
        netD.to(dev)
        opt.Noise_Amps = list(fx["noise_amps_init"])
        torch.manual_seed(3)
        tr = hp_train.train(opt, netG, data, netD=netD, niter=1)
        first = float(tr.last["rec_loss"])
        opt.scale_idx = s
        torch.manual_seed(3)
        # a fresh trainer on the already-stepped nets would re-calibrate; run the long loop on a fresh copy instead
        netG.load_state_dict(fx["G_init"])
        netD.load_state_dict(fx["D_init"])
        opt.Noise_Amps = list(fx["noise_amps_init"])
        tr = hp_train.train(opt, netG, data, netD=netD)
        torch.cuda.synchronize()
        assert tr.iteration == 12
        assert (getattr(tr, "_graph", None) is not None) == use_graph
        last = float(tr.last["rec_loss"])
        assert last == last and last < first, (use_graph, first, last)
        for k, v in netG.state_dict().items():
            assert torch.isfinite(v.float()).all(), k
