"""The critic step back-propagates nothing through the forward graph of D(x_hat).

The gradient penalty differentiates D(x_hat) w.r.t. x_hat under create_graph=True.  ops.Conv.backward then builds ConvBwdData /
LReLUMaskMul nodes whose LeakyReLU-mask operands are activations of that forward pass.  No gradient is ever returned for a mask
operand (LeakyReLU's second derivative is zero), but an operand that requires grad still gives the new node an edge to the
forward Conv that produced it, and errD_total.backward() then runs that Conv's backward - backward-data conv, weight gradient,
bias sum - on a tensor of zeros, for every conv of D(x_hat).  ops.DETACH_MASKS (default on) hands the operands over detached.

Checked on the smallest committed GAN step fixture (2-D, stage 2, batch B = 2, L = num_layer = 5 square critic layers):
  * launch counts of one eager iteration, by an ops.KernelTimer that keys every conv / weight-gradient launch:
      square (nfc -> nfc) weight gradients at batch B        3 L   D(real), D(fake), the penalty's double backward
      flipped masked square convs at batch B                 4 L   D(real), D(fake), d D(x_hat) / d x_hat, the generator's critic term
      flipped nfc -> nc_im convs at batch B                  2     d D(x_hat) / d x_hat, the generator's critic term
    (with the edges in place: 4 L, 5 L and 3);
  * two iterations with the edges cut and two with them in place, from identical state and inputs, leave identical bits in
    every output, both recorded flat gradients and both parameter arenas after each step, and in the end state."""
import pytest
import torch

from helpers import STEP_ORDER, _snapshot, _to_host, assert_runs_identical, load_golden, run_hip_stage

pytestmark = pytest.mark.gpu
FIXTURE = "step2d_gan_s2.pt"


class _Keys:
    """KernelTimer.match: a key for every launch (the timer appends the launch's (B, Cin, Cout, T, H, W))."""

    def __call__(self, desc):
        return "%s flip=%d var=%s" % (desc["op"], 1 if desc.get("flip") else 0, desc.get("var", "-"))


def _run(fx, detach, iters, count):
    """`iters` eager iterations of the product path from the fixture's state; returns ((records, final), launches) with
    launches = {(family, B, Cin, Cout, T, H, W): count} of the first iteration when `count`."""
    from hp_vae_gan_amd import ops
    ops._rng_states.clear()
    torch.manual_seed(5)
    prev = ops.DETACH_MASKS
    ops.DETACH_MASKS = detach
    launches = None
    recs, final = [], {}
    try:
        for i, (rec, out, netG, netD, trainer) in enumerate(run_hip_stage(fx, sync=False)):
            if i >= iters:
                break
            if i == 0 and count:
                torch.cuda.synchronize()
                launches = {k: n for k, (_, n) in ops._kernel_timer.summary().items()}
                ops.set_kernel_timer(None)
            out.pop("D_hip_after", None)
            recs.append(_to_host(_snapshot(trainer, out)))
            final = {"netD": _to_host(dict(netD.state_dict())), "netG": _to_host(dict(netG.state_dict())),
                     "optimizerD": _to_host(trainer.optimizerD.state_dict()), "optimizerG": _to_host(trainer.optimizerG.state_dict())}
    finally:
        ops.DETACH_MASKS = prev
        ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    return (recs, final), launches


def _counted(fx, detach):
    from hp_vae_gan_amd import ops
    ops.set_kernel_timer(ops.KernelTimer(_Keys()))
    return _run(fx, detach, 1, True)[1]


def _tally(launches, fx):
    o = fx["opt"]
    B, N, nc = int(o["batch_size"]), int(o["nfc"]), int(o["nc_im"])
    sq_wgrad = sum(n for k, n in launches.items() if k[0].startswith("wgrad") and k[1:4] == (B, N, N))
    sq_masked = sum(n for k, n in launches.items() if k[0] == "conv flip=1 var=mask" and k[1:4] == (B, N, N))
    narrow = sum(n for k, n in launches.items() if k[0].startswith("conv flip=1") and k[1:4] == (B, N, nc))
    return sq_wgrad, sq_masked, narrow


def test_one_iteration_launches_no_backward_of_the_interpolate_forward():
    fx = load_golden(FIXTURE)
    L = int(fx["opt"]["num_layer"])
    got = _tally(_counted(fx, True), fx)
    print("edges cut: square wgrad %d, flipped masked square %d, flipped nfc->nc_im %d" % got)
    assert got == (3 * L, 4 * L, 2), got


def test_with_the_edges_in_place_the_zero_pass_is_there():
    """The other form of the attribute really is the old graph: else the equality test below would compare a run with itself."""
    fx = load_golden(FIXTURE)
    L = int(fx["opt"]["num_layer"])
    got = _tally(_counted(fx, False), fx)
    print("edges in place: square wgrad %d, flipped masked square %d, flipped nfc->nc_im %d" % got)
    assert got == (4 * L, 5 * L, 3), got


def test_cutting_the_edges_changes_no_bit():
    fx = load_golden(FIXTURE)
    assert len(fx["iters"]) >= 2
    on, _ = _run(fx, True, 2, False)
    off, _ = _run(fx, False, 2, False)
    assert len(on[0]) == 2 and "gradD_flat" in on[0][0] and "gradG_flat" in on[0][0] and "params_D" in on[0][0] and "params_G" in on[0][0]
    assert not torch.equal(on[0][0]["params_D"], on[0][1]["params_D"])
    assert_runs_identical("mask operands detached vs attached", on, off, STEP_ORDER)
