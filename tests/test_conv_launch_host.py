"""Host checks (no GPU) behind tests/test_conv_launches.py: the benchmark's pyramid shapes, the kernel kind the size rules
pick for every launch of them, the float64 reference of tests/conv_ref.py against the pure-loop oracle, and the power of
its per-element error bound."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from helpers import RTOL, assert_close
from oracle import hpvg_oracle as O


@pytest.fixture(scope="module")
def lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def test_video_level_shapes():
    """BASELINE configs[2]'s ten levels: a geometry change shows up here (and moves the launch list with it)."""
    shapes = R.level_shapes()
    assert shapes["video"] == [(4, 18, 33), (4, 23, 41), (4, 28, 51), (5, 36, 65), (5, 45, 81), (5, 57, 102), (7, 72, 129),
                               (7, 91, 162), (7, 114, 204), (13, 144, 256)]
    assert shapes["video8"][-1] == shapes["video"][-1] and len(shapes["video8"]) == 8
    assert len(shapes["image"]) == 10 and all(len(s) == 2 for s in shapes["image"])
    groups = R.launch_groups()
    # 27 distinct level shapes x 4 layers + the encoder / decoder layers at the three level-0 shapes
    assert len(groups) == 27 * 4 + 3 * 2
    assert len(set((g[2], g[3]) for g in groups)) == len(groups)
    assert set(R.KINDS) == set(s for sh in shapes.values() for s in sh)


def test_kernel_kinds_of_every_launch(lib):
    """The host-only kernel queries return the committed table for every layer at every level shape and batch size."""
    bad = []
    for sp in R.KINDS:
        for B in R.BATCHES:
            for layer in R.KIND_LAYERS:
                got, want = R.kinds_of(lib, B, layer, sp), R.expected_kinds(B, layer, sp)
                if got != want:
                    bad.append("B=%d %d->%d %s: (fwd, bwd-data, wgrad, fuses_bias) %s, table %s" % (B, *layer, sp, got, want))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape,Cin,Cout", [
    ((2, 5, 6), 3, 64), ((3, 4, 5), 64, 64), ((2, 4, 3), 64, 3), ((3, 3, 4), 64, 1), ((2, 3, 4), 128, 64), ((2, 4, 3), 64, 128),
    ((6, 7), 3, 64), ((5, 6), 64, 1), ((4, 5), 128, 64), ((7, 5), 1, 3),
])
def test_float64_reference_against_pure_loop_oracle(shape, Cin, Cout):
    """conv_ref's forward, backward-data, weight gradient and bias sum against O.conv_direct (pure loops) and autograd, all
    in float64, within 1e-12 of the error scale.  conv_direct rounds its output to fp32; its float64 arithmetic is reached
    through autograd: the input gradient of conv(., w~) with the flipped, transposed weight w~ is conv(., w)."""
    nd = len(shape)
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + nd)
    B = 2
    x = torch.randn(B, Cin, *shape, generator=g)
    w = torch.randn(Cout, Cin, *([3] * nd), generator=g) / (Cin * 3 ** nd) ** 0.5
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, *shape, generator=g)
    flip = tuple(range(2, 2 + nd))

    y, A = R.conv_fwd64(x, w, b)
    z = torch.zeros(B, Cout, *shape, dtype=torch.float64, requires_grad=True)
    (y_loops,) = torch.autograd.grad(O.conv_direct(z, w.double().flip(flip).transpose(0, 1)), z, x)
    y_loops = y_loops + b.double().view(1, -1, *([1] * nd))
    assert float((y - y_loops).abs().max()) <= 1e-12 * float(A.max())
    assert bool(((O.conv_direct(x, w, b).double() - y).abs() <= 2 ** -24 * y.abs()).all())   # one fp32 rounding of y
    xa = x.abs()
    (a_loops,) = torch.autograd.grad(O.conv_direct(z, w.double().abs().flip(flip).transpose(0, 1)), z, xa)
    assert float((A.double() - a_loops - b.double().abs().view(1, -1, *([1] * nd))).abs().max()) <= 1e-6 * float(A.max())

    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    dx_l, dw_l = torch.autograd.grad(O.conv_direct(x64, w64), [x64, w64], dy)
    dx, dxA = R.conv_bwd_data64(dy, w)
    assert float((dx - dx_l).abs().max()) <= 1e-12 * float(dxA.max())
    dw, dwA = R.conv_bwd_weight64(dy, x, w.shape)
    assert float((dw - dw_l).abs().max()) <= 1e-12 * float(dwA.max())
    pre = R.conv_bwd_weight64(dy, x, w.shape, prefixes=(1, 2))
    (dw1,) = torch.autograd.grad(O.conv_direct(x64[:1], w64), [w64], dy[:1])
    assert float((pre[1][0] - dw1).abs().max()) <= 1e-12 * float(dwA.max()) and torch.equal(pre[2][0], dw)
    db, dbA = R.bias_sum64(dy)
    assert float((db - dy.double().sum(dim=[0] + list(flip))).abs().max()) <= 1e-12 * float(dbA.max())
    assert torch.equal(R.bias_sum64(dy, prefixes=(1,))[1][0], dy[:1].double().sum(dim=[0] + list(flip)))
    # the scales: autograd of the same loops on |.|
    xa64, wa64 = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    dxa_l, dwa_l = torch.autograd.grad(O.conv_direct(xa64, wa64), [xa64, wa64], dy.abs())
    assert float((dxA.double() - dxa_l).abs().max()) <= 1e-6 * float(dxA.max())
    assert float((dwA.double() - dwa_l).abs().max()) <= 1e-6 * float(dwA.max())


def test_checker_power():
    """At a stage-0 body layer (64 -> 64, 4 x 18 x 33): fp32 F.conv3d passes the per-element bound; the same conv with one
    weight element scaled by 1.01, or with one input channel's contribution dropped on a border plane, fails it - and the
    suite's global-maximum check (assert_close at RTOL) passes the 1 % weight error."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 64, 4, 18, 33, generator=g)
    w = torch.randn(64, 64, 3, 3, 3, generator=g) / (64 * 27) ** 0.5
    b = torch.randn(64, generator=g)
    ref, A = R.conv_fwd64(x, w, b)
    y = F.conv3d(x, w, b, padding=1)
    assert R.check(y, ref, A, "fp32 conv3d") <= R.TAU

    w_bad = w.clone()
    k = int(torch.argmax(w.abs()))
    w_bad.view(-1)[k] *= 1.01
    y_bad = F.conv3d(x, w_bad, b, padding=1)
    assert_close(y_bad, ref, RTOL, "1 % in one tap, global-maximum measure")        # the old measure lets it through
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(y_bad, ref, A, "1 % in one tap")
    ratio, idx = R.err_ratio(y_bad, ref, A)
    assert ratio > 8 * R.TAU and idx[1] == k // (64 * 27)                            # the worst element is in the scaled row

    x_drop = x.clone()
    x_drop[:, 5, 0] = 0
    y_drop = y.clone()
    y_drop[:, :, 0] = F.conv3d(x_drop, w, b, padding=1)[:, :, 0]                      # channel 5's taps missing on plane t = 0
    with pytest.raises(AssertionError, match=r"at \(n=\d+, c=\d+, t=0,"):
        R.check(y_drop, ref, A, "channel dropped on a border plane")
