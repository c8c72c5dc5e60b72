"""Host checks (no GPU) behind tests/test_baseline_conv_launches.py and tests/test_baseline_ew_launches.py: the launch lists
of the SinGAN-3D baselines config, the kernel kinds and BatchNorm plans the library picks for them, the tap-sum float64
conv references against conv_ref's CPU references, and the power of the per-element bounds on the faults the new shapes can
hide (W > 256, 64 resize channels, a scalar tail of S % 4 elements)."""
import collections

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import ew_ref as E
from helpers import RTOL, rel_err
from oracle import hpvg_oracle as O


@pytest.fixture(scope="module")
def lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


# ------------------------------------------------------------------------------------------------ the lists
def test_baseline_launch_list():
    """81 (layer, padded shape) pairs over the eight levels (= video8's), none of them a pyramid launch; the finest level's
    seven padded shapes on top of (13, 144, 256); the list is the union of what single train steps launch."""
    opt, shapes = R.baseline_opt()
    assert shapes == R.level_shapes()["video8"] == R.baseline_level_shapes() and len(shapes) == 8
    assert int(opt.num_layer) == 5 and int(opt.nfc) == 64 and opt.generator == "GeneratorSG"
    groups = R.baseline_launch_groups()
    pairs = [(g[2], g[3]) for g in groups]
    assert len(groups) == 81 and len(set(pairs)) == 81
    assert collections.Counter(l for l, _ in pairs) == {(3, 64): 9, (64, 64): 56, (64, 3): 8, (64, 1): 8}
    assert shapes[7] == (13, 144, 256)
    assert sorted(sp for (l, sp), g in zip(pairs, groups) if g[1] == 7 and l == (64, 64)) == [
        (15, 146, 258), (17, 148, 260), (19, 150, 262), (21, 152, 264), (23, 154, 266), (25, 156, 268), (27, 158, 270)]
    assert ((3, 64), (6, 29, 50)) in pairs                       # GeneratorCSG's head: level 0 + 2
    assert not set(pairs) & set((g[2], g[3]) for g in R.launch_groups())
    assert set(sp for _, sp in pairs) == set(R.BASELINE_KINDS)
    # the union of the steps of every stage and network pair, less the unpadded critic's pyramid launches
    steps = set()
    for gen in ("GeneratorSG", "GeneratorCSG"):
        for disc in ("WDiscriminator3D", "WDiscriminatorBaselines"):
            for s in range(len(shapes)):
                steps |= R.baseline_step_groups(gen, disc, s, opt, shapes)
    pyramid = set((g[2], g[3]) for g in R.launch_groups())
    assert steps - pyramid == set(pairs) and steps & pyramid == set((l, sp) for l in ((3, 64), (64, 64), (64, 1)) for sp in shapes)
    # every residue of W mod 4 and of S mod 4, T up to 27, widths above 256
    sps = [sp for _, sp in pairs]
    assert {sp[2] % 4 for sp in sps} == {0, 1, 2, 3} and {E.spatial(sp) % 4 for sp in sps} == {0, 1, 2, 3}
    assert max(sp[0] for sp in sps) == 27 and sum(sp[2] > 256 for sp in set(sps)) == 7
    assert all(E.spatial(R.grown(shapes[l], k)) % 2 for l in (3, 5) for k in range(2, 16, 2))


def test_baseline_kernel_kinds(lib):
    """The host-only kernel queries return the committed table at every padded shape (all four layers, B = 2), and the
    listed launches split into the kinds the GPU module's table of worst ratios is keyed by."""
    bad = []
    for sp in R.BASELINE_KINDS:
        for layer in R.LAYERS:
            got, want = R.kinds_of(lib, R.BASELINE_B, layer, sp), R.baseline_expected_kinds(layer, sp)
            if got != want:
                bad.append("%d->%d %s: (fwd, bwd-data, wgrad, fuses_bias) %s, table %s" % (*layer, sp, got, want))
    assert not bad, "\n".join(bad)
    count = collections.Counter((g[2], R.baseline_expected_kinds(g[2], g[3])) for g in R.baseline_launch_groups())
    assert count == {((3, 64), (0, 3, 4, 0)): 9, ((64, 3), (3, 0, 4, 0)): 8, ((64, 1), (3, 0, 4, 0)): 8,
                     ((64, 64), (2, 2, 3, 1)): 45, ((64, 64), (1, 1, 3, 1)): 11}
    one_axis = sorted(g[3] for g in R.baseline_launch_groups() if R.baseline_expected_kinds(g[2], g[3])[0] == 1)
    assert [sp for sp in one_axis if sp[2] <= 256] == [(6, 29, 50), (6, 36, 63), (8, 31, 52), (12, 42, 69)]
    assert len([sp for sp in one_axis if sp[2] > 256]) == 7


def test_baseline_bn_plans(lib):
    """hpvg_bn_plan returns the committed table at every shape the baselines' BatchNorms see; (0, 16, 1) is reached at
    three shapes of level 5 and by no launch of BN_PLANS; the + 14 shapes are BN2_PLANS' with the same plans."""
    cases = E.baseline_bn_shapes()
    assert len(cases) == 56 and set(sp for _, sp in cases) == set(E.BASELINE_BN_PLANS)
    assert not set(E.BASELINE_BN_PLANS) & set(E.BN_PLANS)
    bad = []
    for _, sp in cases:
        got = E.bn_plan_of(lib, R.BASELINE_B, E.spatial(sp), 1)
        if got != E.BASELINE_BN_PLANS[sp]:
            bad.append("%s: (fused, nsplit, V) %s, table %s" % (sp, got, E.BASELINE_BN_PLANS[sp]))
    assert not bad, "\n".join(bad)
    assert sorted(sp for sp, p in E.BASELINE_BN_PLANS.items() if p == (0, 16, 1)) == [(17, 99, 169), (19, 101, 171), (21, 103, 173)]
    assert (0, 16, 1) not in [p for plans in E.BN_PLANS.values() for p in plans]
    assert {p[:1] + p[2:] for p in E.BASELINE_BN_PLANS.values()} == {(f, v) for f in (0, 1) for v in (1, 2, 4)}
    for sp, plan in E.BN2_PLANS.items():
        assert E.BASELINE_BN_PLANS[sp] == plan


def test_baseline_resize_launches():
    rs = E.baseline_resize_launches()
    shapes = R.baseline_level_shapes()
    assert len(rs) == 3 * 7
    assert collections.Counter((c, noisy) for _, c, _, _, noisy in rs) == {(3, True): 7, (64, False): 7, (64, True): 7}
    for lvl, c, ins, outs, noisy in rs:
        assert ins == shapes[lvl] and all(o >= i for i, o in zip(ins, outs))
        assert outs == R.grown(shapes[lvl + 1], {(3, True): 14, (64, False): 0, (64, True): 10}[(c, noisy)])
    assert len(E.all_level_shapes()) == 27


# ------------------------------------------------------------------------------------------------ the tap-sum references
@pytest.mark.parametrize("shape,Cin,Cout", [
    ((3, 5, 7), 3, 64), ((5, 3, 9), 64, 64), ((3, 7, 5), 64, 3), ((1, 5, 7), 64, 1), ((3, 3, 5), 128, 64), ((2, 5, 3), 64, 128),
    ((7, 9), 3, 64), ((5, 11), 64, 64), ((9, 5), 64, 1), ((1, 1, 1), 64, 64), ((4, 6, 260), 8, 5),
])
def test_tap_sum_reference_against_cpu_reference(shape, Cin, Cout):
    """conv_fwd64_taps, conv_bwd_data64_taps, conv_bwd_weight64_taps and bias_sum64_on against conv_fwd64, conv_bwd_data64,
    conv_bwd_weight64 and bias_sum64 (torch's float64 CPU convs, themselves pinned to the pure-loop oracle) within 1e-12
    of the error scale, and their scales A within fp32 rounding."""
    nd = len(shape)
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + nd + sum(shape))
    B = 2
    x = torch.randn(B, Cin, *shape, generator=g)
    w = torch.randn(Cout, Cin, *([3] * nd), generator=g) / (Cin * 3 ** nd) ** 0.5
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, *shape, generator=g)
    for name, (got, gotA), (ref, refA) in (
            ("forward", R.conv_fwd64_taps(x, w, b), R.conv_fwd64(x, w, b)),
            ("forward, no bias", R.conv_fwd64_taps(x, w), R.conv_fwd64(x, w)),
            ("backward-data", R.conv_bwd_data64_taps(dy, w), R.conv_bwd_data64(dy, w)),
            ("weight gradient", R.conv_bwd_weight64_taps(dy, x), R.conv_bwd_weight64(dy, x, w.shape)),
            ("bias sum", R.bias_sum64_on(dy), R.bias_sum64(dy))):
        assert got.dtype == torch.float64 and gotA.dtype == torch.float32 and got.shape == ref.shape, name
        assert float((got - ref).abs().max()) <= 1e-12 * float(refA.max()), name
        assert float((gotA.double() - refA.double()).abs().max()) <= 1e-6 * float(refA.max()), name + " scale"


# ------------------------------------------------------------------------------------------------ checker power
def test_checker_power_wide_rows():
    """At 1 x 8 x 2 x 5 x 260 (fp32 F.conv3d as the stand-in kernel, the tap-sum reference): the bound passes the honest
    forward and weight gradient and fails (a) output columns w >= 256 computed from the input shifted by one row, (b) one of
    the 27 taps missing from the weight gradient for columns w >= 256 only.  Found: neither is subtle - the suite's
    global-maximum measure (RTOL of max |ref|) fails both as well: (a) is 0.82 of max |ref| (0.61 of A against 1.5e-7 for
    the honest conv), (b) 0.15 of the largest weight gradient (2.0e-2 of A against 6.8e-8).  What the per-element bound adds
    is the place: it names a column >= 256, or the dropped tap, and passes everything else."""
    g = torch.Generator().manual_seed(260)
    x = torch.randn(1, 8, 2, 5, 260, generator=g)
    w = torch.randn(8, 8, 3, 3, 3, generator=g) / (8 * 27) ** 0.5
    b = torch.randn(8, generator=g)
    dy = torch.randn(1, 8, 2, 5, 260, generator=g)
    ref, A = R.conv_fwd64_taps(x, w, b)
    y = F.conv3d(x, w, b, padding=1)
    assert R.check(y, ref, A, "fp32 conv3d") <= R.TAU
    y_bad = y.clone()
    y_bad[..., 256:] = F.conv3d(torch.roll(x, 1, dims=3), w, b, padding=1)[..., 256:]
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A = .* at \(n=0, c=\d+, t=\d+, h=\d+, w=2\d\d\)"):
        R.check(y_bad, ref, A, "columns >= 256 from a shifted row")
    ratio, idx = R.err_ratio(y_bad, ref, A)
    assert idx[-1] >= 256 and ratio > 1000 * R.TAU
    assert R.err_ratio(y_bad[..., :256], ref[..., :256], A[..., :256])[0] <= R.TAU
    assert rel_err(y_bad, ref) > 100 * RTOL                      # not subtle: the old measure sees it as well

    dwref, dwA = R.conv_bwd_weight64_taps(dy, x)
    dw = torch.nn.grad.conv3d_weight(x, w.shape, dy, padding=1)
    assert R.check(dw, dwref, dwA, "fp32 conv3d_weight", names=R.WEIGHT_NAMES[5]) <= R.TAU
    tail = torch.zeros_like(dy)
    tail[..., 256:] = dy[..., 256:]
    part = torch.nn.grad.conv3d_weight(x, w.shape, tail, padding=1)
    dw_bad = dw.clone()
    dw_bad[:, :, 1, 2, 0] -= part[:, :, 1, 2, 0]
    with pytest.raises(AssertionError, match=r"at \(o=\d+, i=\d+, kt=1, kh=2, kw=0\)"):
        R.check(dw_bad, dwref, dwA, "tap (1, 2, 0) without columns >= 256", names=R.WEIGHT_NAMES[5])
    assert R.err_ratio(dw_bad, dwref, dwA)[0] > 100 * R.TAU and rel_err(dw_bad, dwref) > 100 * RTOL
    keep = torch.ones(3, 3, 3, dtype=torch.bool)
    keep[1, 2, 0] = False
    assert R.err_ratio(dw_bad[:, :, keep], dwref[:, :, keep], dwA[:, :, keep])[0] <= R.TAU


def test_checker_power_resize_channels():
    """(c) A 64-channel resize (2 x 64 x 4 x 9 x 13 -> 6 x 12 x 17, the oracle's fp32-coordinate resize as the stand-in)
    passes the bound (7.0e-7 of A); with channel 63 computed from channel 62's input it fails at c = 63 (5.6 A).  Found: this
    fault is gross too - the global-maximum measure fails it as well (1.08 of max |ref|)."""
    g = torch.Generator().manual_seed(63)
    x = torch.randn(2, 64, 4, 9, 13, generator=g)
    outs = (6, 12, 17)
    y, A = E.resize64(x, outs)
    good = O.resize_linear_ac(x, outs)
    assert R.check(good, y, A, "fp32 resize, 64 channels") <= E.TAU
    bad = good.clone()
    bad[:, 63] = O.resize_linear_ac(x[:, 62:63], outs)[:, 0]
    with pytest.raises(AssertionError, match=r"at \(n=\d+, c=63,"):
        R.check(bad, y, A, "channel 63 reads channel 62")
    assert R.err_ratio(bad[:, :63], y[:, :63], A[:, :63])[0] <= E.TAU
    assert rel_err(bad, y) > 100 * RTOL


def _bn_fp32(r, gamma, beta, drop_tail=0):
    """BatchNorm + LeakyReLU applied in fp32 with statistics from float64 sums that leave out the last `drop_tail` elements
    of every sample row (what a vector loop without its scalar tail computes) -> (h, mean)."""
    B, Cn = r.shape[:2]
    x = r.double().reshape(B, Cn, -1)
    S = x.shape[-1]
    n = torch.ones(S, dtype=torch.float64)
    if drop_tail:
        n[S - drop_tail:] = 0
    N = B * S
    mean = (x * n).sum(dim=(0, 2)) / N
    var = (x * x * n).sum(dim=(0, 2)) / N - mean * mean
    invstd = 1 / (var + E.BN_EPS).sqrt()
    sc = (gamma.double() * invstd).float()
    sh = (beta.double() - mean * gamma.double() * invstd).float()
    z = r.reshape(B, Cn, -1) * sc[None, :, None] + sh[None, :, None]
    return O.leaky_relu(z).reshape(r.shape), mean.float()


@pytest.mark.parametrize("sp", [(3, 5, 7), (7, 57, 101)], ids=["3x5x7", "level3+2"])
def test_checker_power_bn_tail(sp):
    """(d) A BatchNorm whose sums leave out the last S % 4 elements of every row, at S = 105 (S % 4 = 1) and at the baselines'
    level 3 + 2 volume 7 x 57 x 101 (S = 40299, S % 4 = 3; 8 channels): the honest fp32 form passes (h 5.9e-8 of A, mean
    1.9e-8); without the tail the mean fails TAU_STAT (1.7e-2 and 8.8e-5 of A) and h fails TAU (7.2e-3 and 6.7e-5 of A: at
    the real size only 7x the bound, so the statistics' own 1e-6 is what catches a dropped tail with a margin)."""
    S = E.spatial(sp)
    assert S % 4 in (1, 3)
    g = torch.Generator().manual_seed(S)
    Cn = 8
    r = (torch.randn(2, Cn, *sp, generator=g) * (0.5 + torch.rand(1, Cn, 1, 1, 1, generator=g))
         + (torch.rand(1, Cn, 1, 1, 1, generator=g) * 2 - 1))
    gamma, beta = 1 + 0.3 * torch.randn(Cn, generator=g), 0.3 * torch.randn(Cn, generator=g)
    ref = E.bn_fwd64(r, gamma, beta, torch.zeros(Cn), torch.ones(Cn), groups=1, lrelu=True)
    h, mean = _bn_fp32(r, gamma, beta)
    assert R.check(h, *ref["h"], "fp32 BatchNorm") <= E.TAU
    assert R.check(mean.view(1, Cn), *ref["mean"], "mean", tau=E.TAU_STAT) <= E.TAU_STAT
    h_bad, mean_bad = _bn_fp32(r, gamma, beta, drop_tail=S % 4)
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(mean_bad.view(1, Cn), *ref["mean"], "mean without the tail", tau=E.TAU_STAT)
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(h_bad, *ref["h"], "h without the tail")
