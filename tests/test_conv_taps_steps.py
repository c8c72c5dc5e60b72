"""Whole train iterations with --ker-size 5 / 7 against the reference: the four fixtures of tests/golden/make_golden_taps.py
through the very check of tests/test_hip_train_step.py (helpers.run_hip_stage, compare_step, compare_update, its RTOL and
each fixture's own spreads), and hipGraph replay against eager iterations, bit for bit, as tests/test_graph_replay_exact.py
does it for the 3-tap stages."""
import pytest
import torch

from helpers import STEP_ORDER, AlphaFeed, assert_runs_identical, hip_opt, load_golden, run_iterations
from test_hip_train_step import test_train_step_matches_reference as _step_matches_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 6


@pytest.mark.parametrize("fname", ["taps5_3d_gan_s3.pt", "taps5_3d_vae_s1.pt", "taps5_2d_gan_s2.pt", "taps7_2d_gan_s2.pt"])
def test_train_step_matches_reference(fname):
    fx = load_golden(fname)
    assert fx["opt"]["ker_size"] in (5, 7) and "spread" in fx
    _step_matches_reference(fname)


def _sequence(x, gen):
    return [(x + 0.1 * torch.randn(x.shape, generator=gen)).clamp_(-1, 1).to(DEV) for _ in range(N)]


def _run(fname, graph_after, sync):
    from hp_vae_gan_amd import ops, telemetry
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_2d, networks_3d
    fx = load_golden(fname)
    s, dims = fx["scale_idx"], fx["dims"]
    nets = networks_3d if dims == 3 else networks_2d
    ops._rng_states.clear()
    torch.manual_seed(11)
    opt = hip_opt(fx["opt"], dims, s, DEV)
    netG = nets.GeneratorHPVAEGAN(opt)
    for _ in range(s):
        netG.init_next_stage()
    netG.load_state_dict(fx["G_init"])
    netG.to(DEV)
    netD = getattr(nets, opt.discriminator)(opt)
    netD.load_state_dict(fx["D_init"])
    netD.to(DEV)
    opt.Noise_Amps = list(fx["noise_amps_init"])
    gen = torch.Generator().manual_seed(99)
    reals = _sequence(fx["real"], gen)
    feed = AlphaFeed(1, N, DEV)
    opt.alpha_source = feed
    trainer = hp_train.StageTrainer(opt, netG, netD)
    inputs = list(zip(reals, _sequence(fx["real_zero"], gen)))
    trainer.loss_log = telemetry.LossLog(hp_train.loss_log_columns(trainer.is_gan), capacity=2 * N, device=DEV)
    run = run_iterations(trainer, inputs, feed, graph_after=graph_after, sync=sync)
    if graph_after is not None:
        assert trainer._graph is not None
        bad = {k: v for k, v in trainer.graph_nodes.items() if v and k not in ("kernel", "empty", "event_record", "wait_event")}
        assert not bad and trainer.graph_nodes["kernel"] > 50, trainer.graph_nodes
    return run


@pytest.mark.parametrize("fname", ["taps5_3d_gan_s3.pt", "taps5_2d_gan_s2.pt"])
def test_replay_equals_eager_bit_for_bit(fname):
    """N eager iterations, the same again, and 1 eager + warm-up + N - 2 replays leave identical bits everywhere."""
    a, a2 = _run(fname, None, False), _run(fname, None, False)
    assert not torch.equal(a[0][2]["params_G"], a[0][3]["params_G"])
    assert not torch.equal(a[0][2]["fake"], a[0][3]["fake"])
    assert_runs_identical("%s: eager vs eager again (not a capture fault)" % fname, a, a2, STEP_ORDER)
    b = _run(fname, 1, False)
    assert_runs_identical("%s: eager vs 1 eager + warm-up + %d replays" % (fname, N - 2), a, b, STEP_ORDER)


def test_generator_block_at_40_channels_matches_float64_torch():
    """The step fixtures stay below 1 MiB and so run 2 to 8 channels: every conv in them is one channel chunk and one M tile.
    This is the module chain at a width the fixtures cannot carry - a level's block (head 3 -> 40, two 40 -> 40 ConvBlocks
    with train-mode BatchNorm and LeakyReLU, tail 40 -> 3; 5 x 5 x 5 taps: three channel chunks, two M tiles, the 64 x 64
    weight-gradient block partly filled) - forward, and the gradients of every parameter and of the input, against the same
    stack of torch modules in float64 on the CPU, at the RTOL of the whole-step tests."""
    import types
    from collections import OrderedDict
    import torch.nn as nn
    from helpers import RTOL, assert_close, bn_bias_atol
    from hp_vae_gan_amd.modules import _nets
    K, N = 5, 40
    opt = types.SimpleNamespace(ker_size=K, num_layer=2, nc_im=3, nfc=N, padd_size=K // 2)
    torch.manual_seed(3)
    ours = _nets._seven_conv_stack(3, 3, N, opt, K // 2)

    def block(ci, co):
        return nn.Sequential(OrderedDict(conv=nn.Conv3d(ci, co, K, 1, K // 2), norm=nn.BatchNorm3d(co), act=nn.LeakyReLU(0.2)))
    ref = nn.Sequential(OrderedDict(head=block(3, N), block0=block(N, N), block1=block(N, N), tail=nn.Conv3d(N, 3, K, 1, K // 2)))
    ref.load_state_dict(ours.state_dict(), strict=True)
    ref.double().train()
    ours.to(DEV).train()
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, 4, 9, 11, generator=g) * 2 - 1
    u = torch.rand(2, 3, 4, 9, 11, generator=g) * 2 - 1
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    gr = torch.autograd.grad((yr * u.double()).sum(), [xr] + list(ref.parameters()))
    xd = x.to(DEV).requires_grad_(True)
    yd = ours(xd)
    gd = torch.autograd.grad((yd * u.to(DEV)).sum(), [xd] + list(ours.parameters()))
    assert_close(yd, yr.detach(), RTOL, "block output")
    names = ["x"] + [n for n, _ in ours.named_parameters()]
    assert names[1:] == [n for n, _ in ref.named_parameters()]
    named = dict(zip(names, gr))
    for n, a, b in zip(names, gd, gr):
        # (the bias of a conv that feeds a BatchNorm has a true gradient of exactly 0: the suite's slack for it)
        assert_close(a, b, RTOL, "d/d " + n, atol=bn_bias_atol(n, named, base=0.0))
    for (n, a), (_, b) in zip(ours.named_buffers(), ref.named_buffers()):
        if not n.endswith("num_batches_tracked"):
            assert_close(a.float(), b.float(), RTOL, "buffer " + n, atol=1e-6)
