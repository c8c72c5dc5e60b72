"""hipGraph replay == eager iterations, bit for bit.

Every stage below the finest trains as a captured hipGraph after its first eager iterations (train._train_loop ->
enable_graph -> _capture_iteration); that replay is what bench.py times and what the programs ship.  Every kernel of the
iteration is free of float atomics and fixed in summation order, so N eager iterations and the same N iterations run as
1 eager + 1 warm-up + N - 2 replays must leave identical bits everywhere: no tolerance.

Per case three runs from the same fixture state, the same torch.manual_seed and a cleared library noise stream:
  A   N eager iterations
  A'  the same again                    (A == A': the whole step is deterministic; if this fails the fault is not the capture)
  B   1 eager, enable_graph (its warm-up is iteration 1), replays up to N      (A == B: the capture changes nothing)
All noise - noise_init included - comes from the library's Philox stream (seed, device iteration counter, call index); the
gradient penalty's alphas, the one draw the library does not make, come through the trainers' `alpha_source` seam from a
device buffer written before every iteration; `real` / `real_zero` are a fresh, different tensor every iteration, so the copy
into the replay's static input buffers is exercised.  Compared: every tensor of every iteration's `out`, both parameter
arenas after every iteration, the loss-log rows, and at the end both networks' state_dict (BatchNorm statistics and counts,
spectral-norm u / v), both optimizers' state_dict (moments, step counts), clip_info and opt.Noise_Amps."""
import pytest
import torch

from helpers import (BASELINE_ORDER, STEP_ORDER, AlphaFeed, assert_runs_identical, hip_opt, load_golden, run_iterations)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 8

CASES = {
    "vae_s1": ("step3d_vae_s1.pt", "stage", None),                              # VAE stage, no critic
    "gan_s3": ("step3d_gan_s3.pt", "stage", "WDiscriminator3D"),                # merged rec / rand pass, SN critic, GP + double backward
    "baseline_s2": ("baseline3d_s2.pt", "baseline", "WDiscriminator3D"),        # Dsteps = 2: two alphas per iteration
    "baseline_dbl_s1": ("baseline3d_dbl_s1.pt", "baseline", "WDiscriminatorBaselines"),   # BatchNorm critic, its second-order backward
}


def _sequence(x, gen):
    """N different inputs derived from the fixture's tensor (device tensors, one allocation each)."""
    return [(x + 0.1 * torch.randn(x.shape, generator=gen)).clamp_(-1, 1).to(DEV) for _ in range(N)]


def _run(case, graph_after, sync):
    from hp_vae_gan_amd import ops, telemetry
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fname, kind, critic = CASES[case]
    fx = load_golden(fname)
    s = fx["scale_idx"]
    ops._rng_states.clear()
    torch.manual_seed(11)
    opt = hip_opt(fx["opt"], 3, s, DEV)
    netG = (networks_3d.GeneratorHPVAEGAN if kind == "stage" else networks_3d.GeneratorSG)(opt)
    for _ in range(s):
        netG.init_next_stage()
    netG.load_state_dict(fx["G_init"])
    netG.to(DEV)
    netD = None
    if fx["D_init"] is not None:
        netD = getattr(networks_3d, critic)(opt)
        netD.load_state_dict(fx["D_init"])
        netD.to(DEV)
    opt.Noise_Amps = list(fx["noise_amps_init"])
    gen = torch.Generator().manual_seed(99)
    reals = _sequence(fx["real"], gen)
    if kind == "stage":
        feed = AlphaFeed(1, N, DEV) if netD is not None else None
        opt.alpha_source = feed
        trainer = hp_train.StageTrainer(opt, netG, netD)
        cols = hp_train.loss_log_columns(trainer.is_gan)
        inputs = list(zip(reals, _sequence(fx["real_zero"], gen)))
    else:
        feed = AlphaFeed(opt.Dsteps, N, DEV)
        opt.alpha_source = feed
        opt.Z_init = fx["Z_init"].to(DEV)
        trainer = hp_train.BaselineStageTrainer(opt, netG, netD)
        cols = hp_train.baseline_loss_log_columns(opt.alpha)
        inputs = [(r,) for r in reals]
    trainer.loss_log = telemetry.LossLog(cols, capacity=2 * N, device=DEV)
    run = run_iterations(trainer, inputs, feed, graph_after=graph_after, sync=sync)
    if feed is not None:
        # eager iterations and the warm-up ask the seam once each, the capture once more; replays never pass through python
        assert feed.calls == (N if graph_after is None else graph_after + 2), feed.calls
    if graph_after is not None:
        assert trainer._graph is not None
        bad = {k: v for k, v in trainer.graph_nodes.items() if v and k not in ("kernel", "empty", "event_record", "wait_event")}
        assert not bad and trainer.graph_nodes["kernel"] > 50, trainer.graph_nodes
    return run


_eager = {}


def _eager_pair(case):
    """(A, A') of a case, run once and shared by its two replay forms (host copies; nothing changes them)."""
    if case not in _eager:
        _eager[case] = (_run(case, None, False), _run(case, None, False))
    return _eager[case]


@pytest.mark.parametrize("sync", [True, False], ids=["synchronised", "back_to_back"])
@pytest.mark.parametrize("case", list(CASES))
def test_replay_equals_eager_bit_for_bit(case, sync):
    """sync: a device synchronise between replays (the form that exposed mis-ordered memset nodes) or
    replays back to back (the form production runs)."""
    order = STEP_ORDER if CASES[case][1] == "stage" else BASELINE_ORDER
    a, a2 = _eager_pair(case)
    # the inputs really differ from iteration to iteration, and so do the draws: else equality below would say little
    assert not torch.equal(a[0][2]["params_G"], a[0][3]["params_G"])
    key = "fake" if "fake" in a[0][0] else "generated"
    assert not torch.equal(a[0][2][key], a[0][3][key])
    assert_runs_identical("%s: eager vs eager again (not a capture fault)" % case, a, a2, order)
    b = _run(case, 1, sync)
    assert_runs_identical("%s: eager vs 1 eager + warm-up + %d replays" % (case, N - 2), a, b, order)
